"""The host side of the batch producer's three further transforms, without a GPU: `loader.draw_extra`
consumes exactly the torch calls the docstring of tests/augment_ref.py fixes (written out by hand below), nothing more is drawn
with the transforms off, the ctypes mirror of AugExtraDesc has the layout the kernels read, the taps and descriptor values are the
definition's, the refusals, and the keywords reach `get_data_loader` / `train_model`."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from interactive_unet import loader, trainer
from tests import augment_ref as ar

H, W = 300, 400


def _by_hand(gen, elastic, color_jitter, blur_or_noise):
    """The draws of one sample exactly as the definition lists them, on torch's generator API directly."""
    hflip = bool(torch.rand(1, generator=gen).item() < 0.5)
    vflip = bool(torch.rand(1, generator=gen).item() < 0.5)
    angle = torch.empty(1).uniform_(-360.0, 360.0, generator=gen).item()
    crop = loader.resized_crop_params(H, W, gen)
    extra = {}
    if elastic:
        lo, hi = torch.randint(0, 2 ** 32, (2,), generator=gen).tolist()
        extra['elastic'] = {'key': lo | hi << 32, 'alpha': 50.0}
    if color_jitter:
        first = bool(torch.rand(1, generator=gen).item() < 0.5)
        b = torch.empty(1).uniform_(0.75, 1.25, generator=gen).item()
        c = torch.empty(1).uniform_(0.5, 2.0, generator=gen).item()
        extra['color_jitter'] = {'brightness': b, 'contrast': c, 'contrast_first': first}
    if blur_or_noise:
        if torch.randint(0, 2, (1,), generator=gen).item() == 0:
            extra['blur_or_noise'] = {'kind': 'blur', 'sigma': torch.empty(1).uniform_(0.1, 2.0, generator=gen).item()}
        else:
            lo, hi = torch.randint(0, 2 ** 32, (2,), generator=gen).tolist()
            extra['blur_or_noise'] = {'kind': 'noise', 'key': lo | hi << 32, 'sigma': 0.1}
    return (hflip, vflip, angle, crop), extra


@pytest.mark.parametrize('switches', [(True, False, False), (False, True, False), (False, False, True), (True, True, True)])
def test_draw_order(switches):
    kinds = set()
    for seed in range(6):                                              # both branches of blur_or_noise occur among the seeds
        a, b = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        for _ in range(3):                                             # per sample: draw_params, then draw_extra
            got = (loader.draw_params(H, W, a), loader.draw_extra(a, *switches))
            assert got == _by_hand(b, *switches)
            assert torch.equal(a.get_state(), b.get_state())
            assert set(got[1]) == {n for n, on in zip(('elastic', 'color_jitter', 'blur_or_noise'), switches) if on}
            if switches[2]:
                kinds.add(got[1]['blur_or_noise']['kind'])
            if switches[0]:
                assert 0 <= got[1]['elastic']['key'] < 2 ** 64
            if switches[1]:
                assert 0.75 <= got[1]['color_jitter']['brightness'] <= 1.25 and 0.5 <= got[1]['color_jitter']['contrast'] <= 2.0
    assert not switches[2] or kinds == {'blur', 'noise'}


def test_nothing_more_is_drawn_with_everything_off():
    a, b = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    loader.draw_params(H, W, a)
    assert loader.draw_extra(a) == {} and loader.draw_extra(a, False, False, False) == {}
    hflip = torch.rand(1, generator=b)                                 # today's four draws and nothing else
    vflip = torch.rand(1, generator=b)
    torch.empty(1).uniform_(-360.0, 360.0, generator=b)
    loader.resized_crop_params(H, W, b)
    assert torch.equal(a.get_state(), b.get_state())
    # the parameters draw_extra takes are passed on, not drawn
    e = loader.draw_extra(a, True, False, True, elastic_alpha=400.0, noise_sigma=0.25)
    assert e['elastic']['alpha'] == 400.0 and e['blur_or_noise'].get('sigma') is not None


def test_extra_descriptor_layout_and_values():
    D = loader.AugExtraDesc
    want = {'flags': 0, 'kind': 4, 'ekey': 8, 'a2': 16, 'brightness': 20, 'contrast': 24, 'contrast_first': 28, 'w2': 32, 'nkey': 132,
            'sigma_n': 140}
    assert {n: getattr(D, n).offset for n, _ in D._fields_} == want and ctypes.sizeof(D) == 144
    from interactive_unet import _native as nv
    if os.path.isfile(nv.LIB_PATH):
        assert nv.lib().iunet_augment_extra_desc_bytes() == ctypes.sizeof(D)
        assert nv.lib().iunet_augment_desc_bytes() == ctypes.sizeof(loader.AugDesc) and ctypes.sizeof(loader.AugDesc) % 8 == 0
    # the values a descriptor carries are the definition's float32 ones
    d = D()
    use = loader._fill_extra(d, {'elastic': {'key': 0x299f31d0a4093822, 'alpha': 50.0},
                                 'color_jitter': {'brightness': 1.1, 'contrast': 0.7, 'contrast_first': True},
                                 'blur_or_noise': {'kind': 'blur', 'sigma': 0.1}})
    assert use == loader.USE_ELASTIC | loader.USE_JITTER | loader.USE_BLUR and d.flags == 3 and d.kind == 1
    assert (d.ekey[0], d.ekey[1]) == ar.key_words(0x299f31d0a4093822) and d.a2 == np.float32(50.0 / 2)
    assert d.brightness == np.float32(1.1) and d.contrast == np.float32(0.7) and d.contrast_first == 1
    k = ar.taps(0.1, 5)
    w2 = np.array(list(d.w2), np.float32).reshape(5, 5)
    assert np.array_equal(w2, k[:, None] * k[None, :]) and (w2[w2 > 0] < 2.0 ** -126).any()          # denormal weights survive the trip
    d = D()
    assert loader._fill_extra(d, {'blur_or_noise': {'kind': 'noise', 'key': (7 << 32) | 5, 'sigma': 0.1}}) == loader.USE_NOISE
    assert d.flags == 0 and d.kind == 2 and (d.nkey[0], d.nkey[1]) == (5, 7) and d.sigma_n == np.float32(0.1)
    assert loader._fill_extra(D(), {}) == 0
    with pytest.raises(ValueError):
        loader._fill_extra(D(), {'blur_or_noise': {'kind': 'sharpen'}})
    for sigma, K in ((5.0, None), (2.0, None), (0.1, None), (1.3, 5)):
        assert np.array_equal(loader.gaussian_taps(sigma, K), ar.taps(sigma, K))


def test_refusals():
    for kw in ({'elastic': True}, {'color_jitter': True}, {'blur_or_noise': True}):
        with pytest.raises(ValueError):
            loader.UNetDataset([], None, augment=False, **kw)
        with pytest.raises(ValueError):
            loader.get_data_loader(augment=False, annotations=[], **kw)
        with pytest.raises(ValueError, match='3-D'):
            trainer.train_model(dim=3, **kw)
    ds = loader.UNetDataset([], None, augment=True, elastic=True, color_jitter=True, blur_or_noise=True)
    assert (ds.elastic, ds.color_jitter, ds.blur_or_noise, ds.elastic_alpha, ds.elastic_sigma, ds.noise_sigma) == (True, True, True, 50.0, 5.0, 0.1)
    ds = loader.UNetDataset([], None, augment=True)
    assert not (ds.elastic or ds.color_jitter or ds.blur_or_noise)


def test_keywords_pass_through():
    names = ('elastic', 'color_jitter', 'blur_or_noise')
    for fn in (loader.get_data_loader, trainer.train_model, loader.UNetDataset.__init__, loader.draw_extra):
        prm = inspect.signature(fn).parameters
        assert all(prm[n].default is False for n in names), fn
    prm = inspect.signature(loader.UNetDataset.__init__).parameters
    assert (prm['elastic_alpha'].default, prm['elastic_sigma'].default, prm['noise_sigma'].default) == (50.0, 5.0, 0.1)
    assert list(inspect.signature(loader.UNetDataset.batch).parameters) == ['self', 'indices', 'params', 'extra']
    # the app calls train_model positionally: the new keywords come after every existing one
    order = list(inspect.signature(trainer.train_model).parameters)
    assert order[-3:] == list(names) and order[:5] == ['lr', 'batch_size', 'epochs', 'num_channels', 'num_classes']
    assert order.index('patches_per_epoch') == len(order) - 4
    dl = loader.get_data_loader(annotations=[], elastic=True, blur_or_noise=True)
    assert (dl.dataset.elastic, dl.dataset.color_jitter, dl.dataset.blur_or_noise) == (True, False, True)
    seen = {}

    def spy(**kw):
        seen[kw['set_type']] = kw
        return []
    orig = loader.get_data_loader
    loader.get_data_loader = spy
    try:
        trainer._loaders(2, 1, False, 2, True, False, True)
    finally:
        loader.get_data_loader = orig
    assert (seen['train']['elastic'], seen['train']['color_jitter'], seen['train']['blur_or_noise']) == (True, False, True)
    assert not any(seen['val'].get(n) for n in names) and seen['val']['augment'] is False          # validation stays unaugmented

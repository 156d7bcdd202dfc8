"""U-Net++ (architecture='U-Net++') without a GPU: parameter names and shapes, the constructor, checkpoints, the refusals, and the
CPU reference's L = 2 identity with the U-Net."""
import warnings

import pytest
import torch

from oracle import unet_ref
from tests import unetpp_ref


def _model(**kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='U-Net++', pretrained=False, **kw)


def test_param_shapes_names_and_order():
    from interactive_unet import unet
    shapes = unet.param_shapes(2, 4, 32, 1, 2, architecture='U-Net++')
    assert list(shapes) == list(unetpp_ref.param_shapes(2, 4, 32, 1, 2))
    assert shapes == unetpp_ref.param_shapes(2, 4, 32, 1, 2)
    assert [k for k in shapes if k.endswith('.up.weight')] == [f'dec{i}_{j}.up.weight' for i, j in
                                                                 ((0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (0, 3))]
    assert shapes['dec0_3.conv1.weight'] == (32, 128, 3, 3)
    assert shapes['dec1_2.up.weight'] == (128, 64, 2, 2)
    assert shapes['dec2_1.conv2.weight'] == (128, 128, 3, 3)
    s3 = unet.param_shapes(3, 5, 64, 1, 4, architecture='U-Net++')
    assert s3 == unetpp_ref.param_shapes(3, 5, 64, 1, 4)
    # the U-Net's shapes are unchanged
    assert unet.param_shapes(2, 4, 32, 1, 2) == unet_ref.param_shapes(2, 4, 32, 1, 2)


def test_parameter_count():
    from interactive_unet import unet
    count = lambda s: sum(torch.Size(v).numel() for k, v in s.items() if not unet._is_buffer(k))      # trainable parameters
    assert count(unet.param_shapes(2, 4, 32, 1, 2, architecture='U-Net++')) == 2206658
    assert count(unet.param_shapes(2, 4, 32, 1, 2)) == 1926466


def test_constructor_hparams_and_checkpoint(tmp_path):
    from interactive_unet.unet import UNet
    m = _model(lr=3e-4, num_classes=3)
    assert m.hparams['architecture'] == 'U-Net++'
    assert m.act_dtype == torch.float16 and m.infer_dtype == torch.float32
    assert list(m.named_tensors()) == list(unetpp_ref.param_shapes(2, 4, 32, 1, 3))
    m.load_named(unetpp_ref.init_params(2, 4, 32, 1, 3, seed=4, randomize_bn=True))
    path = tmp_path / 'model.ckpt'
    m.save_checkpoint(str(path))
    r = UNet.load_from_checkpoint(checkpoint_path=str(path))
    assert r.hparams['architecture'] == 'U-Net++' and r.architecture == 'U-Net++'
    for k, v in m.named_tensors().items():
        assert torch.equal(v, r.tensor(k)), k
    assert _model(infer_dtype='bf16').infer_dtype == torch.bfloat16


def test_engine_needs_the_gpu():
    with pytest.raises(RuntimeError):
        _model().engine('eval')


@pytest.mark.parametrize('kw', [dict(norm='group'), dict(weight_dtype='fp8_e4m3'), dict(act_dtype='fp32'), dict(act_dtype='fp16x2'),
                                dict(infer_dtype='fp16x2'), dict(infer_policy='x2m'), dict(levels=10)])
def test_out_of_scope_combinations_refused(kw):
    with pytest.raises(NotImplementedError, match='U-Net\\+\\+ supports'):
        _model(**kw)


def test_other_architectures_still_refused():
    from interactive_unet.unet import UNet
    for arch in ('PSPNet', 'DeepLabV3+', 'FPN'):
        with pytest.raises(NotImplementedError):
            UNet(architecture=arch, pretrained=False)


@pytest.mark.parametrize('dim,shape', [(2, (2, 1, 32, 48)), (3, (1, 1, 8, 16, 16))])
@pytest.mark.parametrize('training', [False, True])
def test_reference_at_two_levels_is_the_unet(dim, shape, training):
    p = unetpp_ref.init_params(dim, 2, 32, 1, 2, seed=3, randomize_bn=True)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
    for act in (None, torch.float16):
        a = unetpp_ref.forward_logits(p, x, dim, 2, training=training, act_dtype=act)
        b = unet_ref.forward_logits(unetpp_ref.to_unet_names(p), x, dim, 2, training=training, act_dtype=act)
        assert torch.equal(a, b)

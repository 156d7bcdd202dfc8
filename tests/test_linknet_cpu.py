"""LinkNet (architecture='LinkNet') without a GPU: parameter names, shapes and counts, the constructor, checkpoints, the refusals, and the
CPU reference held against an independent torch.nn LinkNet (eval, training and gradients)."""
import math
import warnings

import pytest
import torch
import torch.nn as nn

from oracle import unet_ref
from tests import linknet_ref


def _model(**kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='LinkNet', pretrained=False, **kw)


def test_param_shapes_names_and_order():
    from interactive_unet import unet
    shapes = unet.param_shapes(2, 4, 32, 1, 2, architecture='LinkNet')
    assert list(shapes) == list(linknet_ref.param_shapes(2, 4, 32, 1, 2))
    assert shapes == linknet_ref.param_shapes(2, 4, 32, 1, 2)
    dec = [k for k in shapes if k.startswith('dec2.')]
    assert dec == [f'dec2.{a}' for a in ('conv1.weight', 'bn1.weight', 'bn1.bias', 'bn1.running_mean', 'bn1.running_var', 'up.weight',
                                         'bn2.weight', 'bn2.bias', 'bn2.running_mean', 'bn2.running_var', 'conv2.weight', 'bn3.weight',
                                         'bn3.bias', 'bn3.running_mean', 'bn3.running_var')]
    assert [k for k in shapes if k.endswith('up.weight')] == ['dec2.up.weight', 'dec1.up.weight', 'dec0.up.weight']
    assert shapes['dec0.conv1.weight'] == (16, 64, 1, 1) and shapes['dec0.up.weight'] == (16, 16, 4, 4)
    assert shapes['dec0.conv2.weight'] == (32, 16, 1, 1) and shapes['dec0.bn3.weight'] == (32,)
    assert shapes['dec2.conv1.weight'] == (64, 256, 1, 1)
    assert list(shapes)[-2:] == ['head.weight', 'head.bias']
    assert unet.param_shapes(3, 5, 64, 2, 4, architecture='LinkNet') == linknet_ref.param_shapes(3, 5, 64, 2, 4)
    assert unet.param_shapes(2, 4, 32, 1, 2) == unet_ref.param_shapes(2, 4, 32, 1, 2)      # the U-Net's are unchanged


def test_parameter_count():
    from interactive_unet import unet
    count = lambda s: sum(torch.Size(v).numel() for k, v in s.items() if not unet._is_buffer(k))
    assert count(unet.param_shapes(2, 4, 32, 1, 2, architecture='LinkNet')) == 1291874
    assert count(unet.param_shapes(3, 4, 32, 1, 2, architecture='LinkNet')) == 3891362
    assert count(unet.param_shapes(2, 4, 32, 1, 2)) == 1926466
    assert count(unet.param_shapes(3, 4, 32, 1, 2)) == 5601154


def test_constructor_defaults_hparams_and_init():
    m = _model(lr=3e-4, num_classes=3)
    assert m.hparams['architecture'] == 'LinkNet' and m.architecture == 'LinkNet'
    assert m.act_dtype == torch.float16 and m.infer_dtype == torch.float32
    assert list(m.named_tensors()) == list(linknet_ref.param_shapes(2, 4, 32, 1, 3))
    assert _model(infer_dtype='bf16').infer_dtype == torch.bfloat16
    assert _model(act_dtype='bf16').infer_dtype == torch.float32
    t = m.named_tensors()
    for l in range(3):
        assert torch.equal(t[f'dec{l}.bn3.weight'], torch.ones_like(t[f'dec{l}.bn3.weight']))
        assert torch.equal(t[f'dec{l}.bn2.running_var'], torch.ones_like(t[f'dec{l}.bn2.running_var']))
        assert not torch.equal(t[f'dec{l}.up.weight'], torch.zeros_like(t[f'dec{l}.up.weight']))
        w = t[f'dec{l}.conv1.weight']
        assert abs(w.std().item() - math.sqrt(2.0 / w.shape[1])) < 0.3 * math.sqrt(2.0 / w.shape[1])


def test_checkpoint_round_trip(tmp_path):
    from interactive_unet.unet import UNet
    m = _model(dim=3, levels=3, num_classes=4, num_channels=2)
    m.load_named(linknet_ref.init_params(3, 3, 32, 2, 4, seed=4, randomize_bn=True))
    path = tmp_path / 'model.ckpt'
    m.save_checkpoint(str(path))
    r = UNet.load_from_checkpoint(checkpoint_path=str(path))
    assert r.architecture == 'LinkNet' and r.dim == 3 and r.levels == 3
    for k, v in m.named_tensors().items():
        assert torch.equal(v, r.tensor(k)), k


def test_engine_needs_the_gpu():
    with pytest.raises(RuntimeError):
        _model().engine('eval')


@pytest.mark.parametrize('kw', [dict(norm='group'), dict(weight_dtype='fp8_e4m3'), dict(act_dtype='fp32'), dict(act_dtype='fp16x2'),
                                dict(infer_dtype='fp16x2'), dict(infer_policy='x2m'), dict(levels=7), dict(levels=1), dict(base=48),
                                dict(num_channels=5), dict(num_classes=11)])
def test_out_of_scope_combinations_refused(kw):
    with pytest.raises(NotImplementedError, match='LinkNet supports'):
        _model(**kw)


def test_process_group_refused_before_any_gpu_work():
    from interactive_unet.train_engine_linknet import LinkNetTrainEngine
    with pytest.raises(NotImplementedError, match='process_group'):
        LinkNetTrainEngine(_model(), process_group=object())


# ---------------------------------------------------------------------------------------------- an independent torch.nn LinkNet
class _Stage(nn.Sequential):
    def __init__(self, dim, ci, co):
        Conv, BN = (nn.Conv2d, nn.BatchNorm2d) if dim == 2 else (nn.Conv3d, nn.BatchNorm3d)
        super().__init__(Conv(ci, co, 3, padding=1, bias=False), BN(co), nn.ReLU(), Conv(co, co, 3, padding=1, bias=False), BN(co), nn.ReLU())


class _Block(nn.Module):
    def __init__(self, dim, cin, cout):
        super().__init__()
        Conv, ConvT, BN = (nn.Conv2d, nn.ConvTranspose2d, nn.BatchNorm2d) if dim == 2 else (nn.Conv3d, nn.ConvTranspose3d, nn.BatchNorm3d)
        m = cin // 4
        self.c1, self.b1 = Conv(cin, m, 1, bias=False), BN(m)
        self.up, self.b2 = ConvT(m, m, kernel_size=4, stride=2, padding=1, bias=False), BN(m)
        self.c2, self.b3 = Conv(m, cout, 1, bias=False), BN(cout)

    def forward(self, d, skip):
        a = torch.relu(self.b1(self.c1(d)))
        a = torch.relu(self.b2(self.up(a)))
        return torch.relu(self.b3(self.c2(a))) + skip


class _TorchLinkNet(nn.Module):
    def __init__(self, dim, levels, base, cin, ncls):
        super().__init__()
        ch = [base * 2 ** l for l in range(levels)]
        self.enc = nn.ModuleList([_Stage(dim, cin if l == 0 else ch[l - 1], ch[l]) for l in range(levels)])
        self.dec = nn.ModuleDict({str(l): _Block(dim, ch[l + 1], ch[l]) for l in range(levels - 2, -1, -1)})
        self.head = (nn.Conv2d if dim == 2 else nn.Conv3d)(ch[0], ncls, 1)
        self.pool = nn.MaxPool2d(2) if dim == 2 else nn.MaxPool3d(2)
        self.levels = levels

    def forward(self, x):
        X = []
        for l, st in enumerate(self.enc):
            x = st(x)
            X.append(x)
            if l < self.levels - 1:
                x = self.pool(x)
        d = X[-1]
        for l in range(self.levels - 2, -1, -1):
            d = self.dec[str(l)](d, X[l])
        return self.head(d)

    def load(self, p):
        """Copy the canonical names into the modules; -> {canonical name: torch parameter}."""
        out = {}

        def put(name, t):
            with torch.no_grad():
                t.copy_(p[name].to(t.dtype))
            out[name] = t
        for l, st in enumerate(self.enc):
            for j, (ci, bi) in enumerate(((0, 1), (3, 4)), 1):
                put(f'enc{l}.conv{j}.weight', st[ci].weight)
                for k, t in (('weight', st[bi].weight), ('bias', st[bi].bias), ('running_mean', st[bi].running_mean), ('running_var', st[bi].running_var)):
                    put(f'enc{l}.bn{j}.{k}', t)
        for l, blk in self.dec.items():
            for key, conv, bn, bname in (('conv1', blk.c1, blk.b1, 'bn1'), ('up', blk.up, blk.b2, 'bn2'), ('conv2', blk.c2, blk.b3, 'bn3')):
                put(f'dec{l}.{key}.weight', conv.weight)
                for k, t in (('weight', bn.weight), ('bias', bn.bias), ('running_mean', bn.running_mean), ('running_var', bn.running_var)):
                    put(f'dec{l}.{bname}.{k}', t)
        put('head.weight', self.head.weight)
        put('head.bias', self.head.bias)
        return out


@pytest.mark.parametrize('dim,shape,levels', [(2, (2, 1, 32, 48), 4), (3, (2, 2, 8, 16, 8), 3), (2, (1, 1, 17 * 4, 4 * 3), 3)])
def test_reference_against_torch_nn(dim, shape, levels):
    cin, ncls, base = shape[1], 3, 32
    p = linknet_ref.init_params(dim, levels, base, cin, ncls, seed=7, randomize_bn=True)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    net = _TorchLinkNet(dim, levels, base, cin, ncls).double()
    named = net.load(p)
    # eval: running statistics
    net.eval()
    with torch.no_grad():
        want = net(x)
    got = linknet_ref.forward_logits(p, x, dim, levels, training=False, dtype=torch.float64)
    assert (got - want).abs().max().item() < 1e-9
    # training: batch statistics, and the gradients of every trainable tensor
    net.train()
    want = net(x)
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (want * g).sum().backward()
    pr = {k: v.clone().double().requires_grad_(not unet_ref.is_buffer(k)) for k, v in p.items()}
    stats = {}
    got = linknet_ref.forward_logits(pr, x, dim, levels, training=True, bn_stats_out=stats, dtype=torch.float64)
    assert (got - want).abs().max().item() < 1e-9
    (got * g).sum().backward()
    for name, t in named.items():
        if unet_ref.is_buffer(name):
            continue
        assert torch.allclose(pr[name].grad, t.grad, rtol=1e-7, atol=1e-9), name
    assert set(stats) == {k[:-len('.weight')] for k in p if '.bn' in k and k.endswith('.weight')}

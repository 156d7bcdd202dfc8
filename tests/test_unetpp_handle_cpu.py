"""The U-Net++ handles of the C ABI without a GPU (both are host memory until bound / loaded): iunet_train_create_nested and
iunet_net_create_nested list the tensors of unet.param_shapes(..., 'U-Net++') in order, and refuse what the Python constructors refuse."""
import ctypes
import math

import pytest

CASES = [(2, 2, 32, 1, 2), (2, 4, 32, 1, 3), (3, 3, 32, 1, 2), (3, 5, 64, 1, 4), (2, 9, 32, 2, 2)]


def _lib():
    from interactive_unet import _native as nv
    return nv.lib()


def _layout(l, kind, h):
    out = []
    for i in range(getattr(l, f'iunet_{kind}_num_tensors')(h)):
        name = ctypes.create_string_buffer(96)
        off, n = ctypes.c_longlong(), ctypes.c_longlong()
        assert getattr(l, f'iunet_{kind}_param')(h, i, name, 96, ctypes.byref(off), ctypes.byref(n)) == 0
        out.append((name.value.decode(), off.value, n.value))
    return out


def _want(cfg, with_buffers):
    from interactive_unet.unet import param_shapes
    out, off = [], 0
    for k, shp in param_shapes(*cfg, architecture='U-Net++').items():
        if not with_buffers and (k.endswith('running_mean') or k.endswith('running_var')):
            continue
        out.append((k, off, math.prod(shp)))
        off += math.prod(shp)
    return out, off


@pytest.mark.parametrize('cfg', CASES)
def test_train_handle_layout_is_the_nested_module(cfg):
    l = _lib()
    h = ctypes.c_void_p()
    assert l.iunet_train_create_nested(*cfg, 0, 6, ctypes.byref(h)) == 0, l.iunet_last_error()
    want, total = _want(cfg, False)
    assert _layout(l, 'train', h) == want
    assert l.iunet_train_num_params(h) == total
    dim, levels = cfg[0], cfg[1]
    # the BatchNorms of NestedTrainEngine.stage_names(): every encoder level and every node, two each
    assert l.iunet_train_num_bn(h) == 2 * (levels + levels * (levels - 1) // 2)
    f = 2 ** (levels - 1)
    D = f if dim == 3 else 1
    assert l.iunet_train_workspace_bytes(h, 2, D, f, 2 * f) > 0
    assert l.iunet_train_workspace_bytes(h, 2, D, f + 1, 2 * f) == 0
    l.iunet_train_destroy(h)


@pytest.mark.parametrize('cfg', CASES)
@pytest.mark.parametrize('mode', [0, 1])
def test_net_handle_layout_is_the_nested_module(cfg, mode):
    l = _lib()
    h = ctypes.c_void_p()
    assert l.iunet_net_create_nested(*cfg, mode, ctypes.byref(h)) == 0, l.iunet_last_error()
    want, total = _want(cfg, True)
    assert _layout(l, 'net', h) == want
    assert l.iunet_net_num_params(h) == total
    from interactive_unet.unet import UNet
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(architecture='U-Net++', dim=cfg[0], levels=cfg[1], base=cfg[2], num_channels=cfg[3], num_classes=cfg[4], pretrained=False)
    assert total == sum(m.tensor(n).numel() for n in m._names)
    f = 2 ** (cfg[1] - 1)
    D = f if cfg[0] == 3 else 1
    assert l.iunet_net_workspace_bytes(h, 1, D, f, f) > 0 and l.iunet_net_eval_scratch_bytes(h, 1, D, f, f) > 0
    l.iunet_net_destroy(h)


def test_constructors_refuse_what_the_module_refuses():
    l = _lib()
    h = ctypes.c_void_p()
    for levels in (1, 10):
        assert l.iunet_train_create_nested(2, levels, 32, 1, 2, 0, 6, ctypes.byref(h)) < 0 and b'levels' in l.iunet_last_error()
        assert l.iunet_net_create_nested(2, levels, 32, 1, 2, 0, ctypes.byref(h)) < 0 and b'levels' in l.iunet_last_error()
    assert l.iunet_train_create_nested(2, 4, 32, 1, 2, 2, 6, ctypes.byref(h)) < 0 and b'dtype' in l.iunet_last_error()
    for mode in (2, 3):
        assert l.iunet_net_create_nested(2, 4, 32, 1, 2, mode, ctypes.byref(h)) < 0 and b'mode' in l.iunet_last_error()
    assert l.iunet_train_create_nested(2, 4, 32, 1, 2, 0, 6, None) < 0 and l.iunet_last_error()
    assert l.iunet_net_create_nested(2, 4, 32, 1, 2, 0, None) < 0 and l.iunet_last_error()


def test_unbound_nested_handles_refuse_to_run():
    from interactive_unet import _native as nv
    l = _lib()
    h = ctypes.c_void_p()
    assert l.iunet_train_create_nested(2, 3, 32, 1, 2, 0, 6, ctypes.byref(h)) == 0
    st = nv.ll_array((1, 1, 1, 1, 1))
    assert l.iunet_train_step(h, ctypes.c_void_p(8), 2, st, ctypes.c_void_p(8), None, 1, 1, 1, 64, 64, ctypes.c_void_p(8), 1e-4, 0.9, 0.999,
                              1e-8, 1e-2, None, None) < 0
    assert b'iunet_train_bind' in l.iunet_last_error()
    l.iunet_train_destroy(h)
    assert l.iunet_net_create_nested(2, 3, 32, 1, 2, 0, ctypes.byref(h)) == 0
    assert l.iunet_net_forward_argmax(h, ctypes.c_void_p(8), ctypes.c_void_p(8), 1, 1, 64, 64, ctypes.c_void_p(8), None) < 0
    assert b'iunet_net_load' in l.iunet_last_error()
    l.iunet_net_destroy(h)

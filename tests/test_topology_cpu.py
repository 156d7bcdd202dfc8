"""interactive_unet/topology.py against unet.param_shapes, a frozen literal and the constructors' refusals; and the engines' shared
plumbing defined once (by inspect).  No GPU; only the constructor refusals need the built library."""
import importlib
import inspect
import os
import re

import pytest

from interactive_unet import topology as T
from interactive_unet import unet

PKG = os.path.dirname(os.path.abspath(T.__file__))
SWEEP = [(arch, dim, levels, base, cin)
         for arch, top in (('U-Net', 6), ('U-Net++', 5)) for dim in (2, 3) for levels in range(2, top + 1) for base in (32, 64) for cin in (1, 3)]


def _forms(arch, levels):
    if arch == 'U-Net':
        return T.stage_names(levels), T.up_convs(levels)
    return T.nested_stage_names(levels), T.nested_up_convs(levels)


def _sources_names(names):
    """The names ForwardEngine._sources collects, in order (on the CPU: its constructor would load the library; the method needs the
    device and the staging dict only)."""
    import torch
    from interactive_unet.engine import ForwardEngine
    e = object.__new__(ForwardEngine)
    e.device, e._stage = torch.device('cpu'), {}
    params = {n: torch.zeros(1) for n in names}
    src, sig = e._sources(params, names)
    assert sig == tuple(params[n].data_ptr() for n in names) and not e._stage          # fp32, contiguous, on the device: no staging copy
    return list(src)


@pytest.mark.parametrize('arch,dim,levels,base,cin', SWEEP)
def test_topology_agrees_with_param_shapes(arch, dim, levels, base, cin):
    shapes = unet.param_shapes(dim, levels, base, cin, 2, arch)
    ch = T.channels(base, levels)
    assert ch == [base * 2 ** l for l in range(levels)]
    stages, ups = _forms(arch, levels)
    for prefix in stages:
        ci, co, level = T.stage_io(prefix, cin, ch)
        w = shapes[f'{prefix}.conv1.weight']
        assert (ci, co) == (w[1], w[0]) and co == ch[level], prefix
        assert shapes[f'{prefix}.conv2.weight'][:2] == (co, co)
    assert len(ups) == len({p for p, _ in ups}) == sum(k.endswith('.up.weight') for k in shapes)
    for prefix, l in ups:
        assert shapes[f'{prefix}.up.weight'][:2] == (ch[l + 1], ch[l]) and shapes[f'{prefix}.up.bias'] == (ch[l],), prefix
    keys = [k for k in shapes if not k.endswith('num_batches_tracked')]
    names = T.param_names(stages, ups)
    assert names == keys
    assert [n for p in stages for n in T.stage_param_names(p)] == [k for k in keys if '.conv' in k or '.bn' in k]
    assert _sources_names(names) == keys
    assert T.encoder_names(levels) == stages[:levels] == [k[:-len('.conv1.weight')] for k in keys if k.startswith('enc') and k.endswith('.conv1.weight')]


def test_frozen_literal_levels4_base32_cin1():
    """Written out by hand: a change to topology.py and unet.param_shapes at once is still caught."""
    ch = T.channels(32, 4)
    assert ch == [32, 64, 128, 256]
    unet_io = [('enc0', (1, 32, 0)), ('enc1', (32, 64, 1)), ('enc2', (64, 128, 2)), ('enc3', (128, 256, 3)),
               ('dec2', (256, 128, 2)), ('dec1', (128, 64, 1)), ('dec0', (64, 32, 0))]
    assert T.stage_names(4) == [n for n, _ in unet_io]
    assert [T.stage_io(n, 1, ch) for n in T.stage_names(4)] == [io for _, io in unet_io]
    assert T.up_convs(4) == [('dec2', 2), ('dec1', 1), ('dec0', 0)]
    nested_io = [('enc0', (1, 32, 0)), ('enc1', (32, 64, 1)), ('enc2', (64, 128, 2)), ('enc3', (128, 256, 3)),
                 ('dec0_1', (64, 32, 0)), ('dec1_1', (128, 64, 1)), ('dec2_1', (256, 128, 2)),
                 ('dec0_2', (96, 32, 0)), ('dec1_2', (192, 64, 1)), ('dec0_3', (128, 32, 0))]
    assert T.nested_stage_names(4) == [n for n, _ in nested_io]
    assert [T.stage_io(n, 1, ch) for n in T.nested_stage_names(4)] == [io for _, io in nested_io]
    assert T.nested_up_convs(4) == [('dec0_1', 0), ('dec1_1', 1), ('dec2_1', 2), ('dec0_2', 0), ('dec1_2', 1), ('dec0_3', 0)]
    assert T.encoder_names(4) == ['enc0', 'enc1', 'enc2', 'enc3']
    assert T.BN_KEYS == ('weight', 'bias', 'running_mean', 'running_var')
    assert T.stage_param_names('dec1') == [
        'dec1.conv1.weight', 'dec1.bn1.weight', 'dec1.bn1.bias', 'dec1.bn1.running_mean', 'dec1.bn1.running_var',
        'dec1.conv2.weight', 'dec1.bn2.weight', 'dec1.bn2.bias', 'dec1.bn2.running_mean', 'dec1.bn2.running_var']
    assert T.param_names(T.stage_names(2), T.up_convs(2)) == (
        T.stage_param_names('enc0') + T.stage_param_names('enc1') + ['dec0.up.weight', 'dec0.up.bias'] + T.stage_param_names('dec0')
        + ['head.weight', 'head.bias'])


def test_level_dims_and_check_spatial():
    assert T.level_dims(3, 3, 16, 24, 40) == [(16, 24, 40), (8, 12, 20), (4, 6, 10)]
    assert T.level_dims(2, 3, 1, 24, 40) == [(1, 24, 40), (1, 12, 20), (1, 6, 10)]
    T.check_spatial(2, 4, 1, 24, 40)
    T.check_spatial(3, 4, 16, 16, 16)
    for dim, levels, shape in ((2, 4, (1, 20, 40)), (2, 4, (2, 16, 16)), (3, 4, (12, 16, 16))):
        with pytest.raises(ValueError, match=re.escape(f'spatial size {shape} must be divisible by 8 (and D == 1 in 2-D)')):
            T.check_spatial(dim, levels, *shape)
    from interactive_unet import engine
    assert engine.check_spatial is T.check_spatial and engine._vox is T._vox and engine.BN_EPS == 1e-5


# ---------------------------------------------------------------------------------------------- single definition
FORWARD = ('stage_names', 'stage_io', 'level_dims', 'check_shape', 'workspace', '_source', '_sources', '_graph', '_new_params',
           '_require_loaded', '_out_strides')
TRAIN = ('stage_names', 'stage_io', 'up_convs', '_flatten', '_bucket_bounds', 'p', 'g', '_prep', 'sync_weights')
# the overrides that ARE the difference between two networks: which stages there are, and behind which transposed convs
ALLOWED = {'EncoderOnly': {'stage_names'}, '_Nested': {'stage_names'},
           'EncoderTrainEngine': {'stage_names', 'up_convs'}, 'NestedTrainEngine': {'stage_names', 'up_convs'}}


def _engine_classes():
    fwd = [('engine', 'Engine'), ('engine_x2', 'EngineX2'), ('engine_f32', 'EngineF32')]
    train = [('train_engine', 'TrainEngine'), ('train_engine_f32', 'TrainEngineF32')]
    for spec in unet.NATIVE.values():
        module, f16, f32, _ = spec['engines']
        fwd += [(module, f16), (module, f32)]
        train.append(spec['train'])
    return [unet.native_class(w) for w in fwd], [unet.native_class(w) for w in train]


def test_shared_plumbing_is_defined_once():
    from interactive_unet.engine import ForwardEngine
    from interactive_unet.train_engine import TrainEngineBase
    fwd, train = _engine_classes()
    assert len(fwd) == 3 + 2 * len(unet.NATIVE) and len(train) == 2 + len(unet.NATIVE)
    for classes, base, methods in ((fwd, ForwardEngine, FORWARD), (train, TrainEngineBase, TRAIN)):
        assert all(inspect.isfunction(vars(base).get(m)) for m in methods), base
        for cls in classes:
            assert issubclass(cls, base), cls
            for klass in cls.__mro__:
                if klass in (base, object):
                    continue
                again = {m for m in methods if m in vars(klass)}
                assert again == ALLOWED.get(klass.__name__, set()) & again, (cls.__name__, klass.__name__, again)
    # the hooks a subclass answers instead
    assert all('_build_workspace' in {m for k in c.__mro__ for m in vars(k)} for c in fwd)
    assert {c.__name__ for c in fwd if c.workspaces_kept != 1} == {'Engine', 'EngineX2'} and fwd[0].workspaces_kept == fwd[1].workspaces_kept == 5
    assert {c.__name__ for c in fwd if not c.limits_cin} == {c.__name__ for c in fwd if c.__name__.endswith('F32')}


def test_no_copy_left_in_the_sources():
    text = {f: open(os.path.join(PKG, f)).read() for f in sorted(os.listdir(PKG)) if f.endswith('.py')}
    bn_keys = re.compile(r"'weight',\s*'bias',\s*'running_mean',\s*'running_var'")
    assert {f for f, t in text.items() if bn_keys.search(t)} == {'topology.py', 'unet.py'}         # (unet.param_shapes: the independent statement)
    assert [f for f, t in text.items() for _ in re.findall(r"'Loss': *o\[0\]", t)] == ['train_engine.py']
    assert [f for f, t in text.items() for _ in re.findall(r'load_eval\(\) has not been called', t) if f != 'engine_auto.py'] == ['engine.py']
    assert [f for f, t in text.items() for _ in re.findall(r'_g_dirty = False', t)] == ['engine.py']


# ---------------------------------------------------------------------------------------------- constructor refusals
_DIM = (ValueError, 'dim must be 2 or 3')
_BASE = (NotImplementedError, 'native U-Net needs base channels to be a multiple of 32')
_CIN = (NotImplementedError, 'native U-Net supports 1..4 input channels')
_NCLS = (NotImplementedError, 'native U-Net supports 2..10 classes (app.py:162)')
_NORM = (ValueError, "norm must be 'batch' or 'group'")
_GROUPS = (ValueError, '5 groups do not divide 32 channels')
_NONE = (None, None)
# recorded from the constructors before topology.check_limits existed: one fault per row
REFUSALS = [(cls, kw) + what
            for cls, rows in (
                ('Engine', [(dict(dim=4), _DIM), (dict(dim=1), _DIM), (dict(base=48), _BASE), (dict(base=16), _BASE), (dict(cin=0), _CIN),
                            (dict(cin=5), _CIN), (dict(ncls=1), _NCLS), (dict(ncls=11), _NCLS), (dict(norm='layer'), _NORM),
                            (dict(norm='group', groups=5), _GROUPS),
                            (dict(weight_dtype='int8'), (ValueError, "weight_dtype must be None (= activation dtype) or 'fp8_e4m3'")),
                            (dict(act_quant=True), (ValueError, "act_quant selects between the two fp8-weight modes: give weight_dtype='fp8_e4m3'")),
                            (dict(norm='group', weight_dtype='fp8_e4m3'),
                             (NotImplementedError, 'the fp8 operator format folds the norm into the weights: BatchNorm only'))]),
                ('EngineX2', [(dict(dim=4), _DIM), (dict(dim=1), _DIM), (dict(base=48), _BASE), (dict(base=16), _BASE), (dict(cin=0), _CIN),
                              (dict(cin=5), _CIN), (dict(ncls=1), _NCLS), (dict(ncls=11), _NCLS), (dict(norm='layer'), _NORM),
                              (dict(norm='group', groups=5), _GROUPS)]),
                ('EngineF32', [(dict(dim=4), _DIM), (dict(dim=1), _DIM), (dict(base=48), _BASE), (dict(base=16), _BASE), (dict(cin=0), _NONE),
                               (dict(cin=5), _NONE), (dict(ncls=1), _NCLS), (dict(ncls=11), _NCLS), (dict(norm='layer'), _NORM),
                               (dict(norm='group', groups=5), _GROUPS)]),
                # EngineAuto builds its forms at the first load: their constructors refuse then, its own only checks the policy
                ('EngineAuto', [(dict(policy='fastest'), (ValueError, "policy must be 'auto', 'x2m' or 'fp16x2'")), (dict(dim=4), _NONE),
                                (dict(base=48), _NONE), (dict(cin=5), _NONE), (dict(ncls=11), _NONE), (dict(norm='layer'), _NONE),
                                (dict(norm='group', groups=5), _NONE)]))
            for kw, what in rows]


@pytest.fixture(scope='module')
def built():
    from interactive_unet import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


@pytest.mark.parametrize('cls,kw,exc,message', REFUSALS, ids=[f'{r[0]}-{"-".join(f"{k}={v}" for k, v in r[1].items())}' for r in REFUSALS])
def test_constructor_refusals(built, cls, kw, exc, message):
    module = {'Engine': 'engine', 'EngineX2': 'engine_x2', 'EngineF32': 'engine_f32', 'EngineAuto': 'engine_auto'}[cls]
    ctor = getattr(importlib.import_module('interactive_unet.' + module), cls)
    if exc is None:
        e = ctor(device='cpu', **kw)
        assert all(getattr(e, k) == v for k, v in kw.items())
        return
    with pytest.raises(exc) as info:
        ctor(device='cpu', **kw)
    assert type(info.value) is exc and str(info.value) == message

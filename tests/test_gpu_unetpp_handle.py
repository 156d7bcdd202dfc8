"""The U-Net++ in the C handles on the MI355X: the C-sequenced training step (iunet_train_create_nested) and forward / validation step
(iunet_net_create_nested) against the Python sequences of train_engine_nested.py / engine_nested.py, bit for bit; the bare C ABI;
data-parallel training (one-rank RCCL group, and two processes where two GPUs are visible); trainer.train_model with a process group;
sharded prediction of a U-Net++ module."""
import ctypes
import os
import socket
import warnings

import numpy as np
import pytest
import torch

from oracle import unet_ref
from tests import unetpp_ref

pytestmark = pytest.mark.gpu


def _nv():
    from interactive_unet import _native as nv
    return nv


def _model(dim, dtype, levels=4, seed=1, ncls=2, **kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(architecture='U-Net++', lr=1e-3, num_classes=ncls, dim=dim, levels=levels, pretrained=False, act_dtype=dtype, **kw)
    m.load_named(unetpp_ref.init_params(dim, levels, 32, 1, ncls, seed=seed))
    return m.cuda()


def _batch(seed, N, shape, scale=1.0):
    rng = np.random.default_rng(seed)
    X = torch.tensor(rng.random((N, 1) + shape, dtype=np.float32)) * scale
    lab = X[:, 0] > 0.5 * scale
    y = torch.stack([~lab, lab], 1).float()
    w = torch.tensor((rng.random((N, 1) + shape) > 0.2).astype(np.float32)).expand(N, 2, *shape).contiguous()
    return X.cuda(), (y * w).to(torch.float16).cuda(), w.to(torch.float16).cuda()


def _same(te_a, te_b, tag):
    for name in ('flat', 'm', 'v', 'state'):
        a, b = getattr(te_a, name), getattr(te_b, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{tag}: {name} differs (max {float((a - b).abs().max())})'
    for n in te_a.model._names:
        if unet_ref.is_buffer(n):
            assert torch.equal(te_a.model.tensor(n).view(torch.int32), te_b.model.tensor(n).view(torch.int32)), f'{tag}: {n} differs'


# ---------------------------------------------------------------------------------------------- 1. the training step
@pytest.mark.parametrize('dim,shape,N,dtype,L', [(2, (64, 96), 2, 'fp16', 4), (2, (64, 96), 3, 'bf16', 3), (3, (16, 32, 32), 2, 'bf16', 4)])
def test_c_sequenced_nested_step_is_the_python_sequenced_step(dim, shape, N, dtype, L):
    from interactive_unet.train_engine_nested import NestedTrainEngine
    a, b = _model(dim, dtype, L), _model(dim, dtype, L)
    te_a = NestedTrainEngine(a, lr=1e-3, loss_kind='mcc_ce')
    te_b = NestedTrainEngine(b, lr=1e-3, loss_kind='mcc_ce')
    te_a.use_handle = False                                    # every step sequenced from Python
    te_b._steps_seen = 1                                       # (the handle takes over at the second step: here from the first)
    for step in range(4):
        # step 2 (fp16): a loss scale that overflows the fp16 gradient -- skipped and halved on the device by both
        batch = _batch(step, N, shape)
        if dtype == 'fp16' and step == 2:
            te_a.loss_scale = te_b.loss_scale = 2.0 ** 30
            before = te_a.flat.clone()
        ra, rb = te_a.train_step(*batch), te_b.train_step(*batch)
        assert getattr(te_b, '_h', None) is not None and getattr(te_a, '_h', None) is None
        assert ra == rb, (step, ra, rb)
        _same(te_a, te_b, f'step {step}')
        if dtype == 'fp16' and step == 2:
            assert torch.equal(before, te_a.flat) and not te_a.last_step_ok and not te_b.last_step_ok
            assert te_a.loss_scale == te_b.loss_scale == 2.0 ** 29
            te_a.loss_scale = te_b.loss_scale = 1024.0
    assert ra['Loss'] < 10.0
    # the two sequences share weights, moments and state: a Python-sequenced step behind handle steps continues them
    te_b.use_handle = False
    batch = _batch(9, N, shape)
    ra, rb = te_a.train_step(*batch), te_b.train_step(*batch)
    assert ra == rb
    _same(te_a, te_b, 'python step behind handle steps')
    x = batch[0]
    a.eval()
    b.eval()
    assert torch.equal(a(x), b(x))


@pytest.mark.parametrize('dim,shape', [(2, (64, 96)), (3, (16, 32, 32))])
def test_nested_handle_at_two_levels_is_the_unet_handle(dim, shape):
    from interactive_unet.train_engine import TrainEngine
    from interactive_unet.train_engine_nested import NestedTrainEngine
    from interactive_unet.unet import UNet
    p = unetpp_ref.init_params(dim, 2, 32, 1, 2, seed=4, randomize_bn=True)
    pu = unetpp_ref.to_unet_names(p)
    res = []
    for nested in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m = UNet(architecture='U-Net++' if nested else 'U-Net', dim=dim, levels=2, act_dtype='fp16', pretrained=False)
        m.load_named(p if nested else pu)
        m = m.cuda()
        te = (NestedTrainEngine if nested else TrainEngine)(m, lr=1e-3, loss_scale=256.0)
        te._steps_seen = 1
        rows = [te.train_step(*_batch(s, 2, shape)) for s in range(3)]
        assert te._h is not None
        torch.cuda.synchronize()
        res.append((rows, te.flat.cpu().clone(), te.m.cpu().clone(), te.v.cpu().clone(),
                    torch.cat([m.tensor(n).cpu() for n in m._names if unet_ref.is_buffer(n)])))
    assert res[0][0] == res[1][0]
    for a, b, what in zip(res[0][1:], res[1][1:], ('parameters', 'm', 'v', 'running statistics')):
        assert torch.equal(a, b), f'{what}: the nested handle at L = 2 differs from the U-Net handle'


def test_nested_training_through_the_bare_c_abi():
    """No engine: a handle, caller-owned device vectors filled from the reference initialisation, ten iunet_train_step calls on one batch."""
    nv = _nv()
    l = nv.lib()
    dim, L, shape, N = 2, 3, (64, 64), 2
    p = unetpp_ref.init_params(dim, L, 32, 1, 2, seed=2)
    h = ctypes.c_void_p()
    nv.call('iunet_train_create_nested', dim, L, 32, 1, 2, 0, 6, ctypes.byref(h))
    n = l.iunet_train_num_params(h)
    flat = torch.empty(n, device='cuda')
    for i in range(l.iunet_train_num_tensors(h)):
        name = ctypes.create_string_buffer(96)
        off, cnt = ctypes.c_longlong(), ctypes.c_longlong()
        nv.call('iunet_train_param', h, i, name, 96, ctypes.byref(off), ctypes.byref(cnt))
        flat[off.value:off.value + cnt.value] = p[name.value.decode()].reshape(-1).cuda()
    grad, m, v = (torch.zeros(n, device='cuda') for _ in range(3))
    stages = [f'enc{i}' for i in range(L)] + [f'dec{i}_{j}' for j in range(1, L) for i in range(L - j)]
    running = []
    for s in stages:
        for j in (1, 2):
            running += [p[f'{s}.bn{j}.running_mean'].clone().cuda(), p[f'{s}.bn{j}.running_var'].clone().cuda()]
    assert len(running) == 2 * l.iunet_train_num_bn(h)
    arr = (ctypes.c_void_p * len(running))(*[t.data_ptr() for t in running])
    state = torch.zeros(8, device='cuda')
    nv.call('iunet_train_state_init', nv.ptr(state), 1024.0, 1, nv.stream())
    packed = torch.empty(l.iunet_train_packed_bytes(h), dtype=torch.uint8, device='cuda')
    nv.call('iunet_train_bind', h, nv.ptr(flat), nv.ptr(grad), nv.ptr(m), nv.ptr(v), arr, nv.ptr(packed), nv.ptr(state), nv.stream())
    ws = torch.empty(l.iunet_train_workspace_bytes(h, N, 1, *shape), dtype=torch.uint8, device='cuda')
    out4 = torch.empty(4, device='cuda')
    X, y, w = _batch(0, N, shape)
    vox = shape[0] * shape[1]
    losses = []
    for _ in range(10):
        nv.call('iunet_train_step', h, nv.ptr(X), 0, nv.ll_array((vox, vox, vox, shape[1], 1)), nv.ptr(y), nv.ptr(w), 1, N, 1, shape[0], shape[1],
                nv.ptr(ws), 1e-3, 0.9, 0.999, 1e-8, 1e-2, nv.ptr(out4), nv.stream())
        losses.append(out4[0].item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert not torch.equal(running[0], p['enc0.bn1.running_mean'].cuda())
    l.iunet_train_destroy(h)


# ---------------------------------------------------------------------------------------------- 2. forward and validation
@pytest.mark.parametrize('dim,shape,N', [(2, (64, 96), 2), (3, (16, 32, 32), 1)])
@pytest.mark.parametrize('mode', [0, 1])
def test_nested_forward_handle_is_the_python_sequence(dim, shape, N, mode):
    from interactive_unet.engine_nested import NestedEngine
    T = (torch.float16, torch.bfloat16)[mode]
    p = {k: v.cuda() for k, v in unetpp_ref.init_params(dim, 4, 32, 1, 3, seed=6, randomize_bn=True).items()}
    x = torch.randint(0, 256, (N, 1) + shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    D, H, W = shape if dim == 3 else (1,) + shape
    vox = D * H * W
    outs = []
    for use_graph in (False, True):
        eng = NestedEngine(dim, 4, 32, 1, 3, T)
        eng.use_graph = use_graph
        eng.load_eval(p)
        r = []
        for _ in range(2):                       # the handle serves the second forward on these weights
            lg, pr = torch.empty((N, 3) + shape, device='cuda'), torch.empty((N, 3) + shape, device='cuda')
            cls = torch.empty((N, vox), dtype=torch.uint8, device='cuda')
            eng.infer(x, (vox, vox, H * W, W, 1), N, D, H, W, logits=lg, probs=pr, cls=cls)
            r.append((lg, pr, cls))
        assert (eng._g is not None and eng._g.loaded) == use_graph
        outs.append(r[1])
        if use_graph:
            assert all(torch.equal(a, b) for a, b in zip(r[0], r[1]))
            # predict.py:30-38 in one call
            cls2 = torch.empty((N, vox), dtype=torch.uint8, device='cuda')
            g = eng._g
            nv = _nv()
            nv.call('iunet_net_forward_argmax', g.h, nv.ptr(x), nv.ptr(cls2), N, D, H, W, nv.ptr(g.workspace(N, D, H, W)), nv.stream())
            assert torch.equal(cls2, r[1][2])
    for a, b, what in zip(outs[0], outs[1], ('logits', 'probs', 'class map')):
        assert torch.equal(a, b), f'{what}: the C-sequenced nested forward differs'


@pytest.mark.parametrize('dim,shape,N,dtype', [(2, (64, 96), 2, 'fp16'), (3, (16, 32, 32), 2, 'bf16')])
def test_nested_validation_step_handle_is_the_python_sequence(dim, shape, N, dtype, monkeypatch):
    from interactive_unet.train_engine_nested import NestedTrainEngine
    m = _model(dim, dtype)
    te = NestedTrainEngine(m, lr=1e-3, loss_kind='mcc_ce')
    for step in range(2):
        te.train_step(*_batch(step, N, shape))
    batch = _batch(7, N, shape)
    monkeypatch.setenv('IUNET_PY_EVAL', '1')
    want = te.eval_step(*batch)
    monkeypatch.delenv('IUNET_PY_EVAL')
    first = te.eval_step(*batch)
    got = te.eval_step(*batch)
    eng = te._eval_engine()
    assert eng._g is not None and eng._g.loaded
    assert want == first == got, (want, first, got)
    assert 0.0 < got['Loss'] < 10.0


def test_module_predicting_in_fp16_uses_the_nested_graph():
    m = _model(2, 'fp16', infer_dtype='fp16').eval()
    x = torch.rand((2, 1, 64, 64), generator=torch.Generator().manual_seed(0)).cuda()
    a = m(x)
    eng = m.engine('eval')
    assert eng._g is None
    b = m(x)
    assert eng._g is not None and eng._g.loaded and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 3. data parallel
def _free_port():
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


@pytest.mark.parametrize('py_dp', [False, True])
def test_nested_data_parallel_step_over_rccl_single_rank(py_dp, monkeypatch):
    import torch.distributed as dist
    from interactive_unet.train_engine_nested import NestedTrainEngine
    if dist.is_initialized():
        pytest.skip('a process group already exists in this process')
    if py_dp:
        monkeypatch.setenv('IUNET_PY_DP', '1')
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{_free_port()}', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        runs = []
        for pg in (None, dist.group.WORLD):
            m = _model(3, 'bf16', levels=3, seed=7)
            te = NestedTrainEngine(m.train(), lr=1e-3, loss_kind='mcc_ce', process_group=pg)
            losses = [te.train_step(*_batch(s, 1, (16, 32, 32)))['Loss'] for s in range(4)]
            assert (getattr(te, '_h', None) is not None) == (pg is None or not py_dp)
            runs.append((losses, te.flat.clone()))
        assert runs[0][0] == runs[1][0], runs
        assert torch.equal(runs[0][1], runs[1][1])
    finally:
        dist.destroy_process_group()


def _dp_worker(rank, port, out_dir):
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    from interactive_unet.train_engine_nested import NestedTrainEngine
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=2, device_id=torch.device('cuda', rank))
    try:
        m = _model(2, 'fp16', levels=3, seed=8 + rank)          # rank 0's weights are broadcast to every rank
        te = NestedTrainEngine(m.train(), lr=1e-3, loss_kind='mcc_ce', process_group=dist.group.WORLD)
        X, y, w = _batch(20, 4, (64, 64))
        for _ in range(2):
            te.train_step(X[2 * rank:2 * rank + 2], y[2 * rank:2 * rank + 2], w[2 * rank:2 * rank + 2])
        torch.save(te.flat.cpu(), os.path.join(out_dir, f'rank{rank}.pt'))
    finally:
        dist.destroy_process_group()


def test_nested_data_parallel_two_processes(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two visible GPUs')
    import torch.multiprocessing as mp
    from interactive_unet.train_engine_nested import NestedTrainEngine
    mp.spawn(_dp_worker, args=(_free_port(), str(tmp_path)), nprocs=2, join=True)
    f0, f1 = torch.load(tmp_path / 'rank0.pt'), torch.load(tmp_path / 'rank1.pt')
    assert torch.equal(f0, f1), 'the ranks drifted apart'
    # one process on the concatenated batch: BatchNorm statistics are per rank, so close, not equal -- AdamW moves each weight by at most
    # about lr per step whatever the gradient
    m = _model(2, 'fp16', levels=3, seed=8)
    te = NestedTrainEngine(m.train(), lr=1e-3, loss_kind='mcc_ce')
    X, y, w = _batch(20, 4, (64, 64))
    for _ in range(2):
        te.train_step(X, y, w)
    assert float((te.flat.cpu() - f0).abs().max()) <= 2 * 2.5e-3


def test_train_model_nested_with_a_process_group(tmp_path, monkeypatch):
    import torch.distributed as dist
    from interactive_unet import trainer
    if dist.is_initialized():
        pytest.skip('a process group already exists in this process')
    monkeypatch.chdir(tmp_path)
    seen = []
    make = trainer.make_train_engine

    def spy(model, **kw):
        te = make(model, **kw)
        seen.append((te, kw.get('process_group')))
        return te
    monkeypatch.setattr(trainer, 'make_train_engine', spy)
    X, y, w = _batch(3, 4, (64, 64))
    train = [(X[:2].cpu(), y[:2].cpu(), w[:2].cpu()), (X[2:].cpu(), y[2:].cpu(), w[2:].cpu())]
    val = [train[0]]
    dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{_free_port()}', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    try:
        trainer.train_model(1e-3, 2, 2, 1, 2, 'MCC + CE', 'U-Net++', 'mit_b0', False, train_loader=train, val_loader=val,
                            process_group=dist.group.WORLD)
    finally:
        dist.destroy_process_group()
    (te, pg), = seen
    assert pg is not None and te.pg is pg and type(te).__name__ == 'NestedTrainEngine'
    assert te._h is not None
    assert os.path.isfile('model/model.ckpt')


# ---------------------------------------------------------------------------------------------- 4. sharded prediction
@pytest.mark.parametrize('kw', [{}, {'infer_dtype': 'fp16'}])
def test_nested_sharded_prediction_is_byte_identical(kw):
    import threading
    from interactive_unet import predict, shard
    from tests.test_gpu_shard import ThreadComm, _Shared, _volume
    S, C, V, world = 32, 2, (56, 40, 40), 2

    def model():
        m = _model(3, None, levels=3, seed=3, **kw)
        m.load_named(unetpp_ref.init_params(3, 3, 32, 1, C, seed=3, randomize_bn=True))
        return m.eval()
    vol = torch.tensor(_volume(V, 31)).cuda()
    want = predict.predict_volume_array(model(), vol, input_size=S, num_classes=C).cpu().numpy()
    one, _ = shard.predict_volume_sharded(shard.NativeOps(model(), C, S), vol, V, S, 0.25)
    assert np.array_equal(one.cpu().numpy(), want)
    bounds, _ = shard.slab_bounds(V[0], world)
    shared = _Shared(world)
    opss = [shard.NativeOps(model(), C, S) for _ in range(world)]
    res, errs = [None] * world, []

    def run(r):
        try:
            z0, z1 = bounds[r]
            out, _ = shard.predict_volume_sharded(opss[r], vol[z0:z1].contiguous(), V, S, 0.25, rounds=2, comm=ThreadComm(shared, r))
            torch.cuda.synchronize()
            res[r] = out.cpu().numpy()
        except Exception as e:                                   # pragma: no cover
            errs.append(e)
            shared.barrier.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    got = np.concatenate(res, 0)
    assert np.array_equal(got, want), f'{(got != want).sum()} of {got.size} bytes differ'

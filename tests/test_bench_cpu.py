"""bench.py's launcher contract, checked without a GPU: `--gpus N` with no torch.distributed environment starts N ranks
under torch.distributed.run as child processes BEFORE anything touches the GPU, and a launcher/--gpus mismatch is
refused (`--gpus` was parsed and never used)."""
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_gpus_n_relaunches_under_torch_distributed_run(monkeypatch):
    bench = _bench()
    calls = []

    def fake_run(cmd, env=None, **kw):
        calls.append((cmd, env))
        return types.SimpleNamespace(returncode=7)
    monkeypatch.setattr(bench.subprocess, 'run', fake_run)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3', '--warmup', '1'])
    import torch
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a: (_ for _ in ()).throw(AssertionError('GPU touched before the relaunch')))
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                   # the children's exit code is handed back
    (cmd, env), = calls
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node=4' in cmd and '--nnodes=1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert os.path.abspath(os.path.join(ROOT, 'bench.py')) in cmd
    assert cmd[-6:] == ['--gpus', '4', '--steps', '3', '--warmup', '1']
    assert env.get('HSA_ENABLE_IPC_MODE_LEGACY') == '0'


def test_rank_count_mismatch_is_refused(monkeypatch):
    bench = _bench()
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert 'started 2 ranks' in str(e.value.code)


def test_c4_volume_is_a_function_of_the_coordinates():
    """Every rank of every world size must generate the same volume: a slab equals the same planes of a taller one."""
    import torch
    bench = _bench()
    a = bench.synth_volume_slab(0, 70, 24, 40, 'cpu')
    b = bench.synth_volume_slab(33, 61, 24, 40, 'cpu')
    assert torch.equal(a[33:61], b)
    assert a.min() >= 1 and a.float().std() > 10               # non-zero, textured data


def test_steps_must_be_at_least_one(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2                                   # argparse's usage error, before anything touches the GPU


def test_dump_outputs_whole_arrays_in_float32(tmp_path):
    import numpy as np
    import torch
    bench = _bench()
    vol = torch.arange(24, dtype=torch.uint8).reshape(2, 3, 4)
    met = torch.tensor([0.5, 0.25, 0.125, 1.0])
    bench.dump_outputs({'predict_volume': vol, 'train_metrics': met}, str(tmp_path / 'd'))
    a = np.load(tmp_path / 'd' / 'predict_volume.npy')
    b = np.load(tmp_path / 'd' / 'train_metrics.npy')
    assert a.dtype == np.float32 and a.shape == (2, 3, 4) and np.array_equal(a, vol.numpy().astype(np.float32))
    assert b.dtype == np.float32 and np.array_equal(b, met.numpy())


def test_dump_outputs_over_budget_is_a_fixed_seeded_sample(tmp_path, monkeypatch):
    """Above the budget every array keeps its share as a sample at seeded positions: the same elements in every run, within the budget."""
    import numpy as np
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4000)     # 1 000 float32 values in all
    arrays = {'big': torch.arange(30000, dtype=torch.int32).reshape(30, 1000), 'small': torch.arange(10000, dtype=torch.float32)}
    got = []
    for run in ('r1', 'r2'):
        bench.dump_outputs(arrays, str(tmp_path / run))
        got.append({k: np.load(tmp_path / run / f'{k}.npy') for k in arrays})
    assert sum(v.size for v in got[0].values()) <= 1000
    for k, t in arrays.items():
        s = got[0][k]
        assert s.dtype == np.float32 and s.ndim == 1 and s.size > 0
        assert np.array_equal(s, got[1][k])                    # same positions, same values
        assert np.all(np.diff(s) >= 0) and np.isin(s, t.numpy().reshape(-1)).all()   # arange input: sorted positions read back sorted

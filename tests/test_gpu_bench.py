"""bench.py's plain run on the device: the headline line alone (the measurements of `--full` stay out of it) and `--dump-outputs`,
what the last timed step returned, as float32 arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / 'outputs'
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + [os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2',
                                                                          '--warmup', '1', '--dump-outputs', str(out)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith('{')][-1])
    assert line['metric'] == 'voxels/sec (train step + full-volume predict) on 128^3 chunks'
    assert line['unit'] == 'voxels/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16' and line['steps'] == 2
    assert line['value'] > 0 and line['ms_per_step'] > 0
    assert abs(line['value'] - (line['config']['train_voxels_per_step'] + line['config']['predict_unique_voxels_per_step'])
               / (line['ms_per_step'] * 1e-3)) <= 1e-2 * line['value']
    assert not {'roofline', 'legs', 'parity', 'throughput_mode', 'cpu_baseline', 'c4', 'c2', 'c5'} & set(line)
    assert sorted(os.listdir(out)) == ['predict_volume.npy', 'train_metrics.npy']
    met = np.load(out / 'train_metrics.npy')
    vol = np.load(out / 'predict_volume.npy')
    assert met.dtype == np.float32 and met.shape == (4,) and np.isfinite(met).all()
    assert vol.dtype == np.float32 and vol.shape == tuple(line['config']['predict_volume']) + (2,)
    assert vol.min() >= 0 and vol.max() <= 255 and vol.max() > 0 and np.array_equal(vol, np.round(vol))

"""bench.py's built-in launcher: `python bench.py --gpus N` must start N ranks itself, rendezvous, and rank 0 prints
ONE JSON line; a world size that differs from --gpus is an error.  Driven on CPU with --selftest-cpu (gloo, no kernels);
the same launcher path with RCCL and the real kernels runs in tests/test_gpu_multi.py when two GPUs are present."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    return env


@pytest.mark.timeout(300)
def test_launcher_spawns_two_ranks():
    r = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--steps', '3', '--selftest-cpu'], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines                                     # exactly one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['rccl_world_size'] == 2 and len(d['per_rank_ms']) == 2 and d['selftest'] is True


@pytest.mark.timeout(300)
def test_world_size_mismatch_is_an_error():
    env = _env()
    env.update(WORLD_SIZE='1', RANK='0', LOCAL_RANK='0')              # "launched" as one rank but asked for two
    r = subprocess.run([sys.executable, BENCH, '--gpus', '2', '--selftest-cpu'], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=280)
    assert r.returncode != 0
    assert b'WORLD_SIZE=1' in r.stderr and not r.stdout.strip()


@pytest.mark.timeout(300)
def test_single_rank_selftest():
    r = subprocess.run([sys.executable, BENCH, '--selftest-cpu', '--steps', '2'], env=_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=280)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = json.loads(r.stdout.decode().strip())
    assert d['n_gpus'] == 1 and d['rccl_world_size'] == 1


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: small outputs are written whole (float64 kept), a larger one as the same seeded sample every time."""
    import numpy as np
    import torch
    import bench
    assert bench.parse(['--steps', '7']).steps == 7 and not bench.parse([]).full and bench.parse([]).dump_outputs is None
    small = {'mean': torch.arange(12, dtype=torch.float32).reshape(3, 4), 'std': torch.ones(3, 4, dtype=torch.float64)}
    assert bench.dump_outputs(small, str(tmp_path / 's')) == ['mean', 'std']
    m, s = np.load(tmp_path / 's' / 'mean.npy'), np.load(tmp_path / 's' / 'std.npy')
    assert m.dtype == np.float32 and m.shape == (3, 4) and np.array_equal(m, small['mean'].numpy()) and s.dtype == np.float64
    big = torch.from_numpy(np.random.default_rng(3).random((4096, 4096), dtype=np.float32))
    for k in ('a', 'b'):
        bench.dump_outputs(big, str(tmp_path / k))
    a, b = np.load(tmp_path / 'a' / 'mean.npy'), np.load(tmp_path / 'b' / 'mean.npy')
    assert a.dtype == np.float32 and 0 < a.nbytes <= bench.DUMP_MAX_BYTES and np.array_equal(a, b)

"""bench.py's OWN multi-rank worker with an engine, before the driver's first SCALE run is its first contact
(VERDICT r5 next 2): `python bench.py --gpus 2` spawns two real processes; every rank takes device 0
(MCL_BENCH_ONE_DEVICE=1 -- the boxes of this pool have one GPU) and librccl's entry points are answered by the
cross-process test double (tests/fake_nccl, LD_PRELOAD + FAKE_NCCL_SHM=1: shared-memory transport, every count / type /
peer checked).  What runs is the worker's real world > 1 path: gloo group, RCCL-id broadcast, setup_comm with its
self-test, the sharded fused step with its collectives and grouped send / receive, max-over-ranks timing, the exchange
report.  What it is NOT: RCCL's transport or a measurement (the line says `rccl_library: TEST DOUBLE`)."""
import json
import math
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
SRC = os.path.join(ROOT, 'tests', 'fake_nccl', 'fake_nccl.cpp')
LIB = os.path.join(ROOT, 'build', 'fake_nccl', 'libfake_nccl.so')


@pytest.fixture(scope='module')
def fake_nccl():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wall', '-o', LIB, SRC], check=True)
    return LIB


def _bench(lib, args, timeout=900, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'MCL_FORCE_COMM')}
    env.update(dict(dict(LD_PRELOAD=lib, FAKE_NCCL_SHM='1', FAKE_NCCL_TIMEOUT_S='20', MCL_BENCH_ONE_DEVICE='1'), **env_extra))
    t0 = time.time()
    p = subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout, universal_newlines=True)
    return p.returncode, p.stdout, p.stderr, time.time() - t0


@pytest.mark.parametrize('exchange', ['p2p', 'allgather'])
def test_two_real_ranks_of_the_bench_worker_on_one_gpu(fake_nccl, exchange):
    extra = {} if exchange == 'p2p' else {'MCL_EXCHANGE': 'allgather'}
    rc, out, err, el = _bench(fake_nccl, ['--gpus', '2', '--steps', '5', '--warmup', '2', '--full', '--only-main', '--particles', '262144'], **extra)
    assert rc == 0, err[-4000:]
    lines = [l for l in out.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out[-2000:]   # ONE JSON line, rank 0's
    d = json.loads(lines[0])
    print({k: d[k] for k in ('value', 'ms_per_step', 'rccl_ranks', 'rccl_library', 'launcher', 'particles_total')}, d['exchange'])
    assert d['n_gpus'] == 2 and d['rccl_ranks'] == 2 and d['launcher'] == 'bench.py'
    assert d['rccl_library'].startswith('TEST DOUBLE')
    assert d['particles_total'] == 2 * 262144 and d['scaling'] == 'weak'
    assert math.isfinite(d['value']) and d['value'] > 0 and math.isfinite(d['ms_per_step'])
    ex = d['exchange']
    assert ex['rank0_p2p_ops_per_exchange'] <= ex['p2p_ops_bound'] == 2
    assert ex['lost_slots_per_step_by_rank'] and len(ex['lost_slots_per_step_by_rank']) == 2
    if exchange == 'p2p':   # (the all-gather scheme keeps no such statistics: every rank receives the whole cloud)
        assert all(x > 0 for x in ex['lost_slots_per_step_by_rank'])
        assert sum(ex['bytes_sent_per_step_by_rank']) > 0   # copies did cross the rank border
    else:
        assert ex['mode'] == 'allgather' and ex['phases_ms_per_step'].get('comm', 0) > 0
    assert d['pose_rmse_m'] < 1.0   # the sharded filter tracks the truth
    assert 'roofline' in d and d['roofline']['kernel'] == 'update_mbes'


def test_eight_real_ranks_of_the_bench_worker_on_one_gpu(fake_nccl):
    """The size of the driver's last SCALE run: `python bench.py --gpus 8`, eight real processes on the one GPU (65 536
    particles each), the point-to-point exchange among eight peers.  One line, rank 0's; every rank reports lost slots."""
    rc, out, err, el = _bench(fake_nccl, ['--gpus', '8', '--steps', '5', '--warmup', '2', '--full', '--only-main', '--particles', '65536'], FAKE_NCCL_TIMEOUT_S='60')
    assert rc == 0, err[-4000:]
    lines = [l for l in out.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out[-2000:]
    d = json.loads(lines[0])
    print({k: d[k] for k in ('value', 'ms_per_step', 'rccl_ranks', 'particles_total')}, d['exchange']['lost_slots_per_step_by_rank'])
    assert d['n_gpus'] == 8 and d['rccl_ranks'] == 8 and d['particles_total'] == 8 * 65536 and d['scaling'] == 'weak'
    assert math.isfinite(d['value']) and d['value'] > 0
    ex = d['exchange']
    assert len(ex['lost_slots_per_step_by_rank']) == 8 and all(x > 0 for x in ex['lost_slots_per_step_by_rank'])
    assert ex['rank0_p2p_ops_per_exchange'] <= ex['p2p_ops_bound'] == 14   # one send + one receive per peer
    assert d['pose_rmse_m'] < 1.0


def test_external_launcher_form_with_two_real_ranks(fake_nccl):
    """the driver's form: python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2"""
    port = subprocess.check_output([sys.executable, '-c',
                                    'import socket; s = socket.socket(); s.bind(("127.0.0.1", 0)); print(s.getsockname()[1])'],
                                   universal_newlines=True).strip()
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MCL_FORCE_COMM')}
    env.update(LD_PRELOAD=fake_nccl, FAKE_NCCL_SHM='1', FAKE_NCCL_TIMEOUT_S='20', MCL_BENCH_ONE_DEVICE='1')
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', port, BENCH, '--gpus', '2', '--steps', '5', '--warmup', '2',
                        '--full', '--only-main', '--particles', '131072'],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert d['n_gpus'] == 2 and d['rccl_ranks'] == 2 and d['launcher'] == 'external' and 'exchange' in d


def test_a_rank_killed_in_the_timed_block_ends_the_job_non_zero(fake_nccl):
    rc, out, err, el = _bench(fake_nccl, ['--gpus', '2', '--steps', '5', '--warmup', '2', '--only-main', '--particles', '131072',
                                          '--test-kill-rank', '1', '--test-kill-step', '2', '--launch-timeout', '240'])
    assert rc != 0
    assert 'rank 1 exited with code' in err, err[-3000:]
    assert not [l for l in out.splitlines() if l.startswith('{')]
    assert el < 240

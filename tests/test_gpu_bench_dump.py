"""bench.py's plain run and --dump-outputs: the line carries the headline fields and nothing that needs runs of its own
(--full does), and the outputs of the last timed step come out as float64 .npy files, bit for bit the same on a repeat
with the same arguments (the inputs are seeded, the filter is deterministic: DESIGN.md section 5)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
ARGS = ['--gpus', '1', '--steps', '4', '--warmup', '2', '--particles', '65536']
NAMES = ['ancestor_indices', 'cov9', 'mean6', 'mean_history', 'particle_ids', 'particles', 'weights', 'yaw_mean']


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step_bit_for_bit_on_a_repeat(tmp_path):
    runs = []
    for tag in ('a', 'b'):
        d = str(tmp_path / tag)
        line = _bench(ARGS + ['--dump-outputs', d])
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in line, k
        assert line['steps'] == 4 and line['warmup'] == 2 and line['unit'] == 'steps/s'
        assert np.isfinite(line['ms_per_step']) and line['ms_per_step'] > 0 and line['value'] > 0
        for k in ('extra', 'cpu_baseline', 'roofline', 'kernels', 'timed'):
            assert k not in line, k   # (--full only)
        assert sorted(f[:-4] for f in os.listdir(d)) == NAMES
        runs.append({n: np.load(os.path.join(d, n + '.npy')) for n in NAMES})
    a, b = runs
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a['particles'].shape == (6, 65536) and a['mean_history'].shape == (4, 6) and a['cov9'].shape == (9,)
    for n in NAMES:
        assert a[n].dtype == np.float64, n
        assert np.array_equal(a[n], b[n], equal_nan=True), n
    assert np.all(np.isfinite(a['particles'])) and np.all(np.isfinite(a['mean6']))

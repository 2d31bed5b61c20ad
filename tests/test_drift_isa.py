"""Register / scratch / LDS budget of the kernels of the per-particle drift states (tools/isa.sh; no GPU needed):
k_drift_init, k_drift_advance, k_drift_gather (both slot-map variants), k_drift_moments (csrc/mcl_drift.h).  None may
spill to scratch; the gather and the moments keep the occupancy of a latency-bound particle stream (the bound of
tests/test_history_isa.py); the advance holds a Philox block and two fp64 Box-Muller chains, as the predict kernel does,
and keeps at least the predict kernel's four waves per SIMD."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER = ('void k_drift_gather<false>', 'void k_drift_gather<true>')
KERNELS = GATHER + ('k_drift_init', 'k_drift_advance', 'k_drift_moments')
PARTICLE_STREAMS = GATHER + ('k_drift_moments',)


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_drift'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_drift_kernels_use_no_scratch(rows):
    for k in KERNELS:
        assert k in rows, (k, sorted(r for r in rows if 'drift' in r))
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_particle_streams_keep_their_occupancy(rows):
    for k in PARTICLE_STREAMS:
        r = rows[k]
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)


def test_the_advance_keeps_the_predict_kernels_occupancy(rows):
    r = rows['k_drift_advance']
    assert r['vgpr'] <= 128 and r['occ'] >= 4, r


def test_lds_holds_only_the_moments_words(rows):
    # four waves x nine sums of 8 bytes
    assert 0 < rows['k_drift_moments']['lds'] <= 4 * 9 * 8
    for k in GATHER + ('k_drift_init', 'k_drift_advance'):
        assert rows[k]['lds'] == 0, (k, rows[k])

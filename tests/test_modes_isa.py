"""Register / scratch / LDS budget of the kernels of mcl_pose_modes (tools/isa.sh; no GPU needed): k_modes_hist,
k_modes_score, k_modes_peak_partial, k_modes_peak_final, k_modes_moments (csrc/mcl_modes.h).  None may spill to scratch;
the two kernels that stream the particles keep the occupancy of a latency-bound stream (the bound of
tests/test_recovery_isa.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('k_modes_hist', 'k_modes_score', 'k_modes_peak_partial', 'k_modes_peak_final', 'k_modes_moments')
PARTICLE_STREAMS = ('k_modes_hist', 'k_modes_moments')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_modes'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_mode_kernels_use_no_scratch(rows):
    for k in KERNELS:
        assert k in rows, (k, sorted(rows))
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_particle_streams_keep_their_occupancy(rows):
    for k in PARTICLE_STREAMS:
        r = rows[k]
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)


def test_lds_holds_only_the_reductions_words(rows):
    # the moments kernel: four waves x eight modes x eleven sums of 8 bytes, the peaks' cells and centres
    assert rows['k_modes_moments']['lds'] <= 4 * 8 * 11 * 8 + 8 * 16 + 8 * 16
    for k in ('k_modes_hist', 'k_modes_score', 'k_modes_peak_partial', 'k_modes_peak_final'):
        assert rows[k]['lds'] <= 256, (k, rows[k])

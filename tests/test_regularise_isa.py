"""Register / scratch / LDS budget of the kernels of the regularised resampling (tools/isa.sh; no GPU needed):
k_reg_moments, k_reg_factor, k_reg_apply (csrc/mcl_regularise.h), each for three and for six dimensions.  None may spill to
scratch; the moments keep the occupancy of a latency-bound particle stream (the bound of tests/test_drift_isa.py) with no
more LDS than four waves x 27 sums; the apply holds two Philox blocks and three fp64 Box-Muller chains and keeps the
predict kernel's budget: at most 128 VGPRs, at least four waves per SIMD."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTS = ('void k_reg_moments<3>', 'void k_reg_moments<6>')
FACTOR = ('void k_reg_factor<3>', 'void k_reg_factor<6>')
APPLY = ('void k_reg_apply<3, false>', 'void k_reg_apply<3, true>', 'void k_reg_apply<6, false>', 'void k_reg_apply<6, true>')
KERNELS = MOMENTS + FACTOR + APPLY


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_regularise'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_regularise_kernels_use_no_scratch(rows):
    for k in KERNELS:
        assert k in rows, (k, sorted(r for r in rows if 'k_reg' in r))
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_the_moments_keep_a_particle_streams_occupancy(rows):
    for k in MOMENTS:
        r = rows[k]
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)


def test_the_moments_lds_holds_only_their_sums(rows):
    # four waves x (D + D (D + 1) / 2) sums of 8 bytes: 9 for three dimensions, 27 for six
    assert 0 < rows['void k_reg_moments<3>']['lds'] <= 4 * 9 * 8
    assert 0 < rows['void k_reg_moments<6>']['lds'] <= 4 * 27 * 8
    for k in APPLY:
        assert rows[k]['lds'] == 0, (k, rows[k])
    # the factor's one lane keeps C and L (21 words each at most) where a loop can index them
    for k in FACTOR:
        assert rows[k]['lds'] <= 2 * 21 * 8 + 16, (k, rows[k])


def test_the_apply_keeps_the_predict_kernels_budget(rows):
    for k in APPLY:
        r = rows[k]
        assert r['vgpr'] <= 128 and r['occ'] >= 4, (k, r)

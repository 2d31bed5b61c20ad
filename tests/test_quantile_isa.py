"""Register / scratch / LDS budget of the kernels of the exact order statistics (tools/isa.sh; no GPU needed): k_quant_range,
k_quant_plan, k_quant_hist, k_quant_pick, k_quant_mass (csrc/mcl_quantile.h).  None may spill to scratch; the three that
stream particles keep the occupancy of a latency-bound particle stream (the bound of tests/test_recovery_isa.py: at most 64
VGPRs, at least seven waves per SIMD); LDS holds the round's histogram -- eight probabilities x 256 bins of 8 bytes -- in
the hist kernel and only the reductions' words elsewhere."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = ('void k_quant_range<false>', 'void k_quant_range<true>', 'void k_quant_hist<false>', 'void k_quant_hist<true>',
           'void k_quant_mass<false>', 'void k_quant_mass<true>')
SINGLE = ('k_quant_plan', 'k_quant_pick')
KERNELS = STREAMS + SINGLE
MAX_P, BINS, WAVES = 8, 256, 4          # MCL_QUANTILE_MAX, bins of a round, waves of a workgroup
LDS = {
    'void k_quant_hist<false>': MAX_P * BINS * 8,           # the histogram and nothing else
    'void k_quant_hist<true>': MAX_P * BINS * 8,
    'void k_quant_range<false>': 2 * 16 * 8,                # block_max / block_sum words: sixteen keys, sixteen doubles
    'void k_quant_range<true>': 2 * 16 * 8,
    'k_quant_plan': 2 * 16 * 8,
    'void k_quant_mass<false>': WAVES * (MAX_P + 2) * 8,    # per wave: eight masses, the total, the used count
    'void k_quant_mass<true>': WAVES * (MAX_P + 2) * 8,
    'k_quant_pick': 0,                                      # the scan stays in the wave (DPP)
}


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_quantile'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_quantile_kernels_use_no_scratch(rows):
    assert sorted(r for r in rows if 'k_quant_' in r) == sorted(KERNELS)
    for k in KERNELS:
        print(k, rows[k])
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_the_kernels_that_stream_particles_keep_a_particle_streams_occupancy(rows):
    for k in STREAMS:
        r = rows[k]
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)


def test_lds_stays_within_the_histogram_and_the_reductions_words(rows):
    for k in KERNELS:
        assert rows[k]['lds'] <= LDS[k], (k, rows[k], LDS[k])
    for k in ('void k_quant_hist<false>', 'void k_quant_hist<true>'):
        assert rows[k]['lds'] == MAX_P * BINS * 8, (k, rows[k])

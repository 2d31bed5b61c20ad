"""Register / scratch / LDS budget of the tempering kernels (tools/isa.sh; no GPU needed): k_temper_max, k_temper_sums,
k_temper_pick, k_temper_apply (csrc/mcl_temper.h).  None may spill to scratch -- the sums kernel keeps 2 x 17 64-bit
accumulators and 17 exponents in registers, the pick kernel indexes its candidates in device memory, not in a local array
-- and LDS holds only the reductions' words."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('k_temper_max', 'k_temper_sums', 'k_temper_pick', 'k_temper_apply')
# the reductions' words: four waves x (S1, S2) x 17 candidates of 8 bytes in the sums kernel; sixteen doubles and sixteen
# 64-bit counts (block_max, block_sum) in the other two
LDS_WORDS = {'k_temper_max': 2 * 16 * 8, 'k_temper_sums': 4 * 2 * 17 * 8, 'k_temper_pick': 2 * 16 * 8, 'k_temper_apply': 0}


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_temper'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_temper_kernels_use_no_scratch_and_only_the_reductions_lds(rows):
    assert sorted(r for r in rows if 'k_temper_' in r) == sorted(KERNELS)
    for k in KERNELS:
        r = rows[k]
        print(k, r)
        assert r['scratch'] == 0, (k, r)
        assert r['lds'] <= LDS_WORDS[k], (k, r)

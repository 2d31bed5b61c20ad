"""Register / scratch / LDS budget of the recovery kernels (tools/isa.sh; no GPU needed): k_uniform_state<INJECT>,
k_wstats_partial, k_wstats_final, k_count_final (csrc/mcl_recovery.h).  Streaming kernels: none may spill to scratch, and
LDS holds only the reductions' few words."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('void k_uniform_state<false>', 'void k_uniform_state<true>', 'k_wstats_partial', 'k_wstats_final', 'k_count_final')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_recovery'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_recovery_kernels_use_no_scratch_and_a_few_words_of_lds(rows):
    for k in KERNELS:
        assert k in rows, (k, sorted(rows))
        r = rows[k]
        assert r['scratch'] == 0, (k, r)
        assert r['lds'] <= 512, (k, r)          # at most three arrays of sixteen 8-byte words
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)   # latency-bound streams: the occupancy must stay high
    assert rows['void k_uniform_state<false>']['lds'] == 0

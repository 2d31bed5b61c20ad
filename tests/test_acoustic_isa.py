"""Register / scratch / LDS budget of the kernels of the delayed acoustic updates (tools/isa.sh; no GPU needed):
k_fix_update and k_beacon_update, each in its four instantiations <LAGGED, ARM> (csrc/mcl_acoustic.h).  None may spill to
scratch or use LDS; the instantiations without a lever arm -- the common case, a stream of gathered loads -- keep the
occupancy of a latency-bound stream (the bound of tests/test_history_isa.py and tests/test_recovery_isa.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ('<false, false>', '<false, true>', '<true, false>', '<true, true>')      # <LAGGED, ARM>
KERNELS = tuple('void %s%s' % (k, v) for k in ('k_fix_update', 'k_beacon_update') for v in VARIANTS)
NO_ARM = tuple(k for k in KERNELS if k.endswith(', false>'))


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_acoustic'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_every_instantiation_is_built_and_no_other(rows):
    found = sorted(r for r in rows if 'k_fix_' in r or 'k_beacon_' in r)
    assert len(KERNELS) == 8 and found == sorted(KERNELS)


def test_acoustic_kernels_use_no_scratch_and_no_lds(rows):
    for k in KERNELS:
        assert rows[k]['scratch'] == 0 and rows[k]['lds'] == 0, (k, rows[k])


def test_the_updates_without_a_lever_arm_keep_the_streaming_bound(rows):
    for k in NO_ARM:
        r = rows[k]
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)

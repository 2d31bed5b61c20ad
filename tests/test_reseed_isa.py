"""Scratch and LDS budget of the sensor resetting's kernel (tools/isa.sh; no GPU needed): k_inject_gaussian
(csrc/mcl_reseed.h) is there, spills nothing to scratch, and uses no more LDS than RESEED_LDS_BYTES, the table of 256
components and the four wave counts its header declares.  Register counts and occupancy are recorded in DESIGN 5p, not
asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = 'k_inject_gaussian'


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_reseed'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def reseed_lds_bytes():
    """RESEED_LDS_BYTES of csrc/mcl_reseed.h, from its own defines"""
    src = open(os.path.join(ROOT, 'smarc_navigation_amd', 'csrc', 'mcl_reseed.h')).read()
    assert re.search(r'#define RESEED_ROW MCL_RESEED_MAX_COMPONENTS', src)
    rows_ = int(re.search(r'#define RESEED_ROWS (\d+)', src).group(1))
    assert re.search(r'#define RESEED_TAB_BYTES \(RESEED_ROWS \* RESEED_ROW \* 8 \+ RESEED_ROW \* 4\)', src)
    extra = int(re.search(r'#define RESEED_LDS_BYTES \(RESEED_TAB_BYTES \+ (\d+)\)', src).group(1))
    comps = int(re.search(r'#define MCL_RESEED_MAX_COMPONENTS (\d+)', open(os.path.join(ROOT, 'include', 'mcl_reseed.h')).read()).group(1))
    return rows_ * comps * 8 + comps * 4 + extra


def test_the_kernel_is_there_and_uses_no_scratch(rows):
    assert [r for r in rows if KERNEL in r] == [KERNEL]
    print(KERNEL, rows[KERNEL])
    assert rows[KERNEL]['scratch'] == 0, rows[KERNEL]


def test_lds_is_no_more_than_the_header_declares(rows):
    cap = reseed_lds_bytes()
    assert cap == 9 * 256 * 8 + 256 * 4 + 16                # 19 472 bytes: eight workgroups fit a CU's 160 KiB
    assert 8 * cap <= 160 * 1024
    assert 0 < rows[KERNEL]['lds'] <= cap, (rows[KERNEL], cap)

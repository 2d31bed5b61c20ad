"""Scratch and LDS budget of the kernels of KLD-sampling (tools/isa.sh; no GPU needed): k_kld_mark, k_kld_count,
k_kld_final and both instantiations of k_transfer_gather (csrc/mcl_kld.h) are there, spill nothing to scratch, and use no
more LDS than KLD_LDS_BYTES, the constant their header names.  Register counts and occupancy are recorded in DESIGN 5q, not
asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('k_kld_mark', 'k_kld_count', 'k_kld_final', 'k_transfer_gather<false>', 'k_transfer_gather<true>')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_kld'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            if 'k_kld_' in name or 'k_transfer_' in name:
                table[name.replace('void ', '')] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def kld_lds_bytes():
    src = open(os.path.join(ROOT, 'smarc_navigation_amd', 'csrc', 'mcl_kld.h')).read()
    return int(re.search(r'#define KLD_LDS_BYTES (\d+)', src).group(1))


def test_the_kernels_are_there_and_use_no_scratch(rows):
    assert sorted(rows) == sorted(KERNELS)
    for k in KERNELS:
        print(k, rows[k])
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_lds_is_no_more_than_the_header_declares(rows):
    cap = kld_lds_bytes()
    assert cap == 128                                           # 16 reduction words of 8 bytes
    for k in KERNELS:
        assert 0 < rows[k]['lds'] <= cap, (k, rows[k], cap)

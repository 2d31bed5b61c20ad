"""Register / scratch / LDS budget of the ping information kernel (tools/isa.sh; no GPU needed): the six instantiations of
k_information (csrc/mcl_information.h) -- height grid, regular mesh, triangle records, each per beam and per pose -- are
all there, none spills to scratch, none uses LDS (the poses travel by lane reads, the sums by wave shuffles and global
integer atomics).  Their register counts and occupancies are recorded in DESIGN 5m, not asserted."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = tuple('void k_information<%d, %s>' % (m, p) for m in (0, 1, 2) for p in ('false', 'true'))


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_information'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_every_instantiation_is_there_and_uses_no_scratch(rows):
    assert sorted(r for r in rows if 'k_information' in r) == sorted(KERNELS)
    for k in KERNELS:
        print(k, rows[k])
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_no_lds(rows):
    for k in KERNELS:
        assert rows[k]['lds'] == 0, (k, rows[k])

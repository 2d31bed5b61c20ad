"""Register / scratch / LDS budget of the swath matching kernel (tools/isa.sh; no GPU needed): the six instantiations of
k_swath_match (csrc/mcl_swath.h) -- height grid, regular mesh, triangle records, each for three and four dimensions -- are
all there, none spills to scratch, and none uses more LDS than MATCH_LDS_BYTES, the rows and the control block
csrc/mcl_match.h declares for k_ping_match, whose decision it shares.  Register counts and occupancies are recorded in
DESIGN 5o, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = tuple('void k_swath_match<%d, %d>' % (m, d) for m in (0, 1, 2) for d in (3, 4))


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_swath'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def match_lds_bytes():
    """MATCH_LDS_BYTES of csrc/mcl_match.h, from its own defines"""
    src = open(os.path.join(ROOT, 'smarc_navigation_amd', 'csrc', 'mcl_match.h')).read()
    words = int(re.search(r'#define MATCH_WORDS (\d+)', src).group(1))
    block = int(re.search(r'#define MATCH_BLOCK_BYTES (\d+)', src).group(1))
    chunk = int(re.search(r'#define BEAM_CHUNK (\d+)', open(os.path.join(ROOT, 'smarc_navigation_amd', 'csrc', 'mcl_innovation.h')).read()).group(1))
    assert re.search(r'#define MATCH_LDS_BYTES \(MATCH_WAVES \* MATCH_WORDS \* 8 \+ MATCH_BLOCK_BYTES\)', src)
    return (chunk // 64) * words * 8 + block


def test_every_instantiation_is_there_and_uses_no_scratch(rows):
    assert sorted(r for r in rows if 'k_swath_match' in r) == sorted(KERNELS)
    assert not [r for r in rows if 'k_swath_match' in r and 'k_ping_match' in r]
    for k in KERNELS:
        print(k, rows[k])
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_lds_is_no_more_than_the_ping_match_declares(rows):
    cap = match_lds_bytes()
    assert cap == 4 * 19 * 8 + 600
    for k in KERNELS:
        assert 0 < rows[k]['lds'] <= cap, (k, rows[k], cap)


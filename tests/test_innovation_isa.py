"""Register / scratch / LDS budget of the ping innovation kernel (tools/isa.sh; no GPU needed): the three instantiations of
k_innovation (csrc/mcl_innovation.h) -- height grid, regular mesh, triangle records -- are all there, none spills to
scratch, none uses LDS (the pose travels by lane reads, the sums by global integer atomics), and each keeps at least four
waves per SIMD: the ray walk is latency-bound, and the default case gives every SIMD four waves."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('void k_innovation<0>', 'void k_innovation<1>', 'void k_innovation<2>')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_innovation'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_every_instantiation_is_there_and_uses_no_scratch(rows):
    assert sorted(r for r in rows if 'k_innovation' in r) == sorted(KERNELS)
    for k in KERNELS:
        print(k, rows[k])
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_no_lds_and_four_waves_per_simd(rows):
    for k in KERNELS:
        assert rows[k]['lds'] == 0 and rows[k]['occ'] >= 4 and rows[k]['vgpr'] <= 128, (k, rows[k])

"""Register / scratch / LDS budget of the kernels of the particle genealogy (tools/isa.sh; no GPU needed):
k_history_compose (both slot-map variants), k_history_record, k_history_count0, k_history_frame, k_history_ancestors,
k_history_path (csrc/mcl_history.h).  None may spill to scratch; the kernels that stream the particles keep the occupancy
of a latency-bound stream (the bound of tests/test_recovery_isa.py and tests/test_modes_isa.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSE = ('void k_history_compose<false>', 'void k_history_compose<true>')
KERNELS = COMPOSE + ('k_history_record', 'k_history_count0', 'k_history_frame', 'k_history_ancestors', 'k_history_path')
PARTICLE_STREAMS = COMPOSE + ('k_history_record', 'k_history_count0', 'k_history_frame', 'k_history_ancestors')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = str(tmp_path_factory.mktemp('isa_history'))
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    table = {}
    with open(os.path.join(out, 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            table[name] = dict(sgpr=int(sgpr), vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), occ=int(occ))
    return table


def test_history_kernels_use_no_scratch(rows):
    for k in KERNELS:
        assert k in rows, (k, sorted(r for r in rows if 'history' in r))
        assert rows[k]['scratch'] == 0, (k, rows[k])


def test_particle_streams_keep_their_occupancy(rows):
    for k in PARTICLE_STREAMS:
        r = rows[k]
        assert r['vgpr'] <= 64 and r['occ'] >= 7, (k, r)


def test_lds_holds_only_the_reductions_words_and_the_paths_slots(rows):
    # the frame kernel: four waves x eight sums of 8 bytes; the path: one u32 slot per frame of the deepest ring
    assert rows['k_history_frame']['lds'] <= 4 * 8 * 8
    assert rows['k_history_path']['lds'] <= 1024 * 4
    for k in COMPOSE + ('k_history_record', 'k_history_count0', 'k_history_ancestors'):
        assert rows[k]['lds'] == 0, (k, rows[k])

"""The shared walk of the lattice fan sweep (mcl_sweep.h: a wave whose lanes stand on the same triangle keeps the lattice
triple in scalar registers and walks on the scalar unit until its lanes part) against the per-lane loop: the same scenes
through ONE build, once with MCL_SWEEP_UNIFORM=0 (every wave takes the per-lane loop: the default) and once with =1, in fresh
child processes, log-weights BIT FOR BIT.  A switch A/B: every result is a function of the particle alone (the determinism
rule), and the shared step performs the per-lane step's floating-point operations on the same operands in the same order,
so the tolerance is zero by construction.

A third child runs MCL_SWEEP_UNIFORM=1 under MCL_DEBUG_WORK=1: the library then launches k_mbes_sweep_work, the kernel that
counts, per wave, the walk steps taken shared and the walk steps taken at all, and prints the totals -- the proof that the
shared loop really ran (fully on a collapsed cloud, partly where slices pass close to lattice nodes); its bits are compared
too.  That kernel is ANOTHER instantiation of the same template body as the production k_mbes_sweep<2|3, false, false> the
'shared' child runs (sweep_kernel<..., WORK>): the counts describe the production kernel by construction of the source, not
by measurement of it; what ties the two together here is that all three children give the same bits.

Shapes: the smallest at which the main kernel runs with full waves -- 8 192 particles (MCL_SWEEP_NSUB=1: one lane per side,
not the sub-fan kernel), a 96 x 96-node lattice mesh, both diagonals, 64 beams and 33 with invalid ranges among them.
Sorts with the other switch / build A/B files, after the reference-pinned parity tests."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import math, sys, numpy as np
sys.path.insert(0, %(root)r)
from smarc_navigation_amd import engine as eng, synth
out = {}
origin = (-48.0, -48.0)          # nodes at the integers -48 .. 47: (0, 0) is a cell corner
# 'the middle of a cell': well inside it and 0.2 m off BOTH diagonals -- the exact centre lies on either, where the nadir
# hits of a 1 cm cloud fall into two triangles and no wave passes the gate
MID = (0.8, 0.5)
z = synth.bathymetry_grid(96, 96, 1.0, origin, seed=3)
N = 8192

def cloud(n, seed, centre, sigma_xy, yaw, sigma_yaw, roll=0.0, pitch=0.0):
    rs = np.random.RandomState(seed)
    soa = rs.randn(6, n) * np.array([sigma_xy, sigma_xy, 0.01, 0.0, 0.0, sigma_yaw])[:, None]
    soa[0] += centre[0]
    soa[1] += centre[1]
    soa[2] -= 5.0
    soa[3] = roll
    soa[4] = pitch
    soa[5] += yaw
    return soa

# name, particles, centre, sigma of x and y, yaw, sigma of yaw, roll, pitch
SCENES = [
    ('collapsed', N, MID, 0.01, 0.0, 1e-3, 0.0, 0.0),
    ('yaw_atan13', N, MID, 0.01, math.atan(1.0 / 3.0), 1e-3, 0.0, 0.0),
    ('yaw_diag', N, MID, 0.01, math.pi / 4 + 0.01, 1e-3, 0.0, 0.0),
    ('corner', N, (0.0, 0.0), 0.01, 0.0, 1e-3, 0.0, 0.0),
    ('centre', N, (0.5, 0.5), 0.01, 0.0, 1e-3, 0.0, 0.0),   # (on both diagonals: the lanes of a wave start in two triangles)
    ('wide', N, MID, 1.0, 0.0, 1.0, 0.0, 0.0),
    # the + side of the fan looks out over the border y = 47: 3 m inside it the nadir's footprint margin declines the
    # particles (hand-overs); 5.5 m inside (the closest cell the margin admits) the same 1 cm cloud passes the gate, its
    # walks run and those of the + side end on the ring of NaNs inside the shared loop (the beams beyond 20 degrees
    # meet the seabed, 15 m down, further out than the border)
    ('border3', N, (MID[0], 44.0), 0.01, 0.0, 1e-3, 0.0, 0.0),
    ('border6', N, (MID[0], 41.5), 0.01, 0.0, 1e-3, 0.0, 0.0),
    ('tilted', N, MID, 0.01, 0.0, 1e-3, 0.1, 0.35),
    ('tail24', N + 24, MID, 0.01, 0.0, 1e-3, 0.0, 0.0),
]
for diag, dname in (('00-11', 'd2'), ('10-01', 'd3')):
    verts, tris = synth.mesh_from_grid(z, 1.0, origin, diagonal=diag)
    for B in (64, 33):
        ba = synth.beam_angles(B)
        for k, (name, n, centre, sxy, yaw, syaw, roll, pitch) in enumerate(SCENES):
            tag = '%%s_%%s_%%d' %% (name, dname, B)
            sys.stderr.write('@scene %%s\n' %% tag)
            sys.stderr.flush()
            e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
            e.set_map_mesh(verts, tris)
            e.set_particles(cloud(n, 10 + k, centre, sxy, yaw, syaw, roll, pitch))
            rs = np.random.RandomState(3)
            ranges = (15.0 / np.cos(ba) + 0.1 * rs.randn(B)).astype(np.float32)
            ranges[::9] = 0.0
            e.update_mbes(ranges, ba, 0.2, 100.0)
            path = e.mbes_last_path()
            assert path[0] == 1, path
            out['lw_' + tag] = e.get_log_weights()
            out['path_' + tag] = np.array(path)
            e.close()
    # six fused steps in visiting order (MCL_VISIT_MIN_N=1: what makes waves coherent in production is live at this size)
    B = 64
    ba = synth.beam_angles(B)
    stream = synth.odom_stream(6)
    sys.stderr.write('@scene steps_%%s\n' %% dname)
    sys.stderr.flush()
    e = eng.Engine(N, seed=5, init_cov=[0.5, 0.5, 0, 0, 0, 0.01], process_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5],
                   resample_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5])
    e.set_map_mesh(verts, tris)
    e.init_particles()
    rs = np.random.RandomState(11)
    for k in range(6):
        ranges = (18.0 / np.cos(ba) + 0.3 * rs.randn(B)).astype(np.float32)
        ranges[5::17] = 0.0
        e.step_mbes(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'], ranges, ba, 0.2, 100.0)
    e.sync()
    assert e.mbes_last_path()[0] == 1
    out['steps_part_' + dname] = e.get_particles()
    out['steps_hist_' + dname] = e.mean_history(6)
    out['steps_idx_' + dname] = np.asarray(e.last_indices())
    e.close()
np.savez(sys.argv[1], **out)
'''

_LINE = re.compile(r'wave walk steps shared (\d+) of (\d+)')


def _work(stderr):
    """{scene: (shared, all)} from the MCL_DEBUG_WORK lines of a child, summed over the updates of a scene"""
    res, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith('@scene '):
            cur = line.split()[1]
            res[cur] = [0, 0]
        m = _LINE.search(line)
        if m and cur:
            res[cur][0] += int(m.group(1))
            res[cur][1] += int(m.group(2))
    return res


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('sweep_uniform')
    child = str(tmp / 'child.py')
    with open(child, 'w') as f:
        f.write(_CHILD % {'root': ROOT})
    res = {}
    for name, uniform, debug in (('lane', '0', False), ('shared', '1', False), ('counted', '1', True)):
        env = dict(os.environ)
        for k in ('MCL_LIB', 'MCL_SWEEP_UNIFORM', 'MCL_DEBUG_WORK', 'MCL_SWEEP', 'MCL_VISIT'):
            env.pop(k, None)
        env['MCL_SWEEP_NSUB'] = '1'
        env['MCL_VISIT_MIN_N'] = '1'
        if uniform is not None:
            env['MCL_SWEEP_UNIFORM'] = uniform
        if debug:
            env['MCL_DEBUG_WORK'] = '1'
        out = str(tmp / (name + '.npz'))
        p = subprocess.run([sys.executable, child, out], env=env, stderr=subprocess.PIPE, universal_newlines=True)
        assert p.returncode == 0, p.stderr[-2000:]
        res[name] = (np.load(out), p.stderr)
    return res


def test_shared_walk_equals_the_per_lane_loop_bit_for_bit(runs):
    lane = runs['lane'][0]
    assert len([k for k in lane.files if k.startswith('lw_')]) == 40
    handed = 0
    for other in ('shared', 'counted'):
        got = runs[other][0]
        assert sorted(got.files) == sorted(lane.files)
        for k in lane.files:
            a, c = lane[k], got[k]
            if k.startswith('path_'):
                assert np.array_equal(a, c), (other, k, a, c)
                handed += int(a[1])
                continue
            if k.startswith('lw_'):
                assert np.isfinite(a).all(), k
            assert np.array_equal(a, c), '%s %s: %d of %d values differ' % (other, k, (a != c).sum(), a.size)
    # the clouds 3 m from the border really went through the hand-over list, those further inside only in part
    for d in ('d2', 'd3'):
        for B in (64, 33):
            assert int(lane['path_border3_%s_%d' % (d, B)][1]) > 0
            assert 0 <= int(lane['path_border6_%s_%d' % (d, B)][1]) < 8192
    assert handed > 0


def test_shared_loop_ran_where_waves_share_their_path(runs):
    work = _work(runs['counted'][1])
    lane_work = _work(runs['lane'][1])
    assert not any(v[1] for v in lane_work.values())   # (no MCL_DEBUG_WORK there: no counts)
    for d in ('d2', 'd3'):
        for B in (64, 33):
            s, n = work['collapsed_%s_%d' % (d, B)]
            print('collapsed', d, B, 'shared', s, 'of', n)
            assert n > 0 and s > 0.9 * n, (d, B, s, n)
            s, n = work['tail24_%s_%d' % (d, B)]
            assert n > 0 and s > 0.9 * n, (d, B, s, n)
            for name in ('yaw_atan13', 'yaw_diag'):
                s, n = work['%s_%s_%d' % (name, d, B)]
                print(name, d, B, 'shared', s, 'of', n)
                assert 0 < s < n, (name, d, B, s, n)
            n_collapsed = work['collapsed_%s_%d' % (d, B)][1]
            # walks that end on the ring of NaNs / over a tilted plane inside the shared loop: shared steps were taken, and
            # at the border fewer steps than over open ground (the + side's walks are cut short there)
            for name in ('border6', 'tilted'):
                s, n = work['%s_%s_%d' % (name, d, B)]
                print(name, d, B, 'shared', s, 'of', n)
                assert 0 < s <= n, (name, d, B, s, n)
            assert work['border6_%s_%d' % (d, B)][1] < n_collapsed
            for name in ('corner', 'centre', 'wide'):   # (the gate fails or the lanes part at once: nothing to assert but sanity)
                s, n = work['%s_%s_%d' % (name, d, B)]
                print(name, d, B, 'shared', s, 'of', n)
                assert n > 0 and 0 <= s <= n, (name, d, B, s, n)
        s, n = work['steps_%s' % d]
        print('steps', d, 'shared', s, 'of', n)
        assert n > 0 and 0 <= s <= n


@pytest.mark.parametrize('setting,shares', [('0', False), (None, False), ('1', True)])
def test_switch_decides_which_loop_walks(tmp_path, setting, shares):
    """under MCL_DEBUG_WORK=1: no step is taken shared with MCL_SWEEP_UNIFORM=0 or unset (the default), every one with =1"""
    child = str(tmp_path / 'child.py')
    with open(child, 'w') as f:
        f.write(r'''
import sys, numpy as np
sys.path.insert(0, %r)
from smarc_navigation_amd import engine as eng, synth
origin = (-48.0, -48.0)
z = synth.bathymetry_grid(96, 96, 1.0, origin, seed=3)
verts, tris = synth.mesh_from_grid(z, 1.0, origin)
rs = np.random.RandomState(1)
soa = rs.randn(6, 8192) * np.array([0.01, 0.01, 0.01, 0.0, 0.0, 1e-3])[:, None]
soa[0] += 0.8
soa[1] += 0.5
soa[2] -= 5.0
e = eng.Engine(8192, rng_mode=eng.RNG_REPLAY)
e.set_map_mesh(verts, tris)
e.set_particles(soa)
ba = synth.beam_angles(64)
e.update_mbes((15.0 / np.cos(ba)).astype(np.float32), ba, 0.2, 100.0)
assert e.mbes_last_path()[0] == 1
e.close()
''' % ROOT)
    env = dict(os.environ)
    env.pop('MCL_LIB', None)
    env.pop('MCL_SWEEP_UNIFORM', None)
    env.update(MCL_SWEEP_NSUB='1', MCL_DEBUG_WORK='1')
    if setting is not None:
        env['MCL_SWEEP_UNIFORM'] = setting
    p = subprocess.run([sys.executable, child], env=env, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-2000:]
    m = _LINE.search(p.stderr)
    assert m and int(m.group(2)) > 0, p.stderr[-2000:]
    assert (int(m.group(1)) > 0.9 * int(m.group(2))) if shares else int(m.group(1)) == 0, p.stderr[-2000:]


_CAP_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
from smarc_navigation_amd import engine as eng, synth
out = {}
origin = (-48.0, -48.0)
z = synth.bathymetry_grid(96, 96, 1.0, origin, seed=3)
for diag, dname in (('00-11', 'd2'), ('10-01', 'd3')):
    verts, tris = synth.mesh_from_grid(z, 1.0, origin, diagonal=diag)
    rs = np.random.RandomState(21)
    soa = rs.randn(6, 8192) * np.array([0.01, 0.01, 0.01, 0.0, 0.0, 1e-3])[:, None]
    soa[0] += 0.8
    soa[1] += 0.5
    soa[2] -= 5.0
    e = eng.Engine(8192, rng_mode=eng.RNG_REPLAY)
    e.set_map_mesh(verts, tris)
    e.set_particles(soa)
    ba = synth.beam_angles(64)
    ranges = (15.0 / np.cos(ba)).astype(np.float32)
    ranges[::9] = 0.0
    e.update_mbes(ranges, ba, 0.2, 100.0)
    path = e.mbes_last_path()
    assert path[0] == 1, path
    out['lw_' + dname] = e.get_log_weights()
    out['path_' + dname] = np.array(path)
    e.close()
np.savez(sys.argv[1], **out)
'''


def test_step_limit_inside_the_shared_loop_hands_the_particle_over(tmp_path):
    """The walk's step limit is a safety net no sane walk reaches (three steps per cell of stop distance + 16; a lattice
    walk takes at most 2.83), so MCL_SWEEP_STEP_CAP=20 lowers it: the collapsed cloud's walks (about 50 steps) run into it at
    step 21, inside the shared loop when that is on.  The per-lane loop then declines the lane and the particle goes to the
    general kernel; the shared loop must do the same -- every particle handed over, the same bits."""
    child = str(tmp_path / 'child.py')
    with open(child, 'w') as f:
        f.write(_CAP_CHILD % {'root': ROOT})
    res = {}
    for name, uniform, debug in (('lane', '0', False), ('shared', '1', False), ('counted', '1', True)):
        env = dict(os.environ)
        for k in ('MCL_LIB', 'MCL_SWEEP_UNIFORM', 'MCL_DEBUG_WORK', 'MCL_SWEEP', 'MCL_VISIT'):
            env.pop(k, None)
        env.update(MCL_SWEEP_NSUB='1', MCL_SWEEP_STEP_CAP='20', MCL_SWEEP_UNIFORM=uniform)
        if debug:
            env['MCL_DEBUG_WORK'] = '1'
        out = str(tmp_path / (name + '.npz'))
        p = subprocess.run([sys.executable, child, out], env=env, stderr=subprocess.PIPE, universal_newlines=True)
        assert p.returncode == 0, p.stderr[-2000:]
        res[name] = (np.load(out), p.stderr)
    for d in ('d2', 'd3'):
        for name in ('lane', 'shared', 'counted'):
            assert int(res[name][0]['path_' + d][1]) == 8192, (name, d, res[name][0]['path_' + d])   # all handed over
            assert np.isfinite(res[name][0]['lw_' + d]).all()
            assert np.array_equal(res[name][0]['lw_' + d], res['lane'][0]['lw_' + d]), (name, d)
    counts = [(int(a), int(b)) for a, b in _LINE.findall(res['counted'][1])]
    assert len(counts) == 2
    for s, n in counts:   # the limit was met in the shared loop: every step shared, no wave of the 256 beyond step 21
        print('step cap: shared', s, 'of', n)
        assert 0 < s == n <= 21 * 256, (s, n)

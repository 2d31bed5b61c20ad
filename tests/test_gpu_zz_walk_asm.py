"""The per-lane walk loop of the lattice fan sweep in assembly (mcl_sweep.h: sweep_walk_asm -- walk step and merge loop of
k_mbes_sweep<2 | 3, false, false> as ONE statement) against the compiler's loop: the same scenes through the default library
and through libmcl_hip_cxxmerge.so (-DSWEEP_MERGE_CXX=1: the compiler's walk and merge everywhere), in fresh child
processes, log-weights and mbes_last_path() BIT FOR BIT, every value finite.  Every floating-point instruction of the
statement is the C++ loop's on the same operands in the same order, so the tolerance is zero by construction.

No child runs under MCL_DEBUG_WORK: that switch launches k_mbes_sweep_work, whose loop is the compiler's in every build.
Every scene runs with MCL_SWEEP_NSUB=1 (one lane per side: the main kernel, not the sub-fan kernel) on a 96 x 96-node
lattice mesh with either diagonal, 4 096 - 8 192 particles (MCL_SWEEP=1: a cloud this small is swept only on request).  The switches a scene needs are read when its engine is created,
so one child per library runs all of them.  Sorts with the other build / switch A/B files, after the parity tests."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'smarc_navigation_amd', 'csrc')

_CHILD = r'''
import math, os, sys, numpy as np
sys.path.insert(0, %(root)r)
from smarc_navigation_amd import engine as eng, synth
only = set(sys.argv[2:])
out = {}
origin = (-48.0, -48.0)          # nodes at the integers -48 .. 47
MID = (0.8, 0.5)                 # well inside a cell and off both diagonals
z = synth.bathymetry_grid(96, 96, 1.0, origin, seed=3)

def cloud(n, seed, centre, sigma_xy, sigma_yaw, roll=0.0, pitch=0.0, sigma_att=0.0):
    rs = np.random.RandomState(seed)
    soa = rs.randn(6, n) * np.array([sigma_xy, sigma_xy, 0.01, sigma_att, sigma_att, sigma_yaw])[:, None]
    soa[0] += centre[0]
    soa[1] += centre[1]
    soa[2] -= 5.0
    soa[3] += roll
    soa[4] += pitch
    return soa

def fan(B):
    return synth.beam_angles(B)

ONE_SIDE = np.linspace(0.05, 1.0, 33)   # every beam on the + side: the - side has none

# name, particles, beam angles, cloud, switches
SCENES = [
    ('collapsed', 4096, fan(512), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {}),
    ('b16', 4096, fan(16), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {}),
    ('b33', 4096, fan(33), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {}),
    ('oneside', 4096, ONE_SIDE, dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {}),
    # lanes of a wave at different beams, walks of different length in one wave; many particles off the map
    ('wide', 8192, fan(512), dict(centre=MID, sigma_xy=30.0, sigma_yaw=1.0), {}),
    ('wide33', 8192, fan(33), dict(centre=MID, sigma_xy=30.0, sigma_yaw=1.0), {}),
    # hanging over the border y = 47: slices that end on the ring of NaNs, particles the footprint test declines
    ('border', 8192, fan(512), dict(centre=(MID[0], 41.0), sigma_xy=3.0, sigma_yaw=0.3), {}),
    ('attitude', 4096, fan(512), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3, roll=0.1, pitch=0.35), {}),
    ('attitude_wide', 8192, fan(301), dict(centre=MID, sigma_xy=10.0, sigma_yaw=1.0, roll=0.1, pitch=0.35), {}),
    # the step limit, met at either parity of the limit; then the wave's own bound just below the lanes' limit: the
    # walks of this cloud are about fifty steps long, every particle is handed over either way
    ('cap5', 4096, fan(512), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {'MCL_SWEEP_STEP_CAP': '5'}),
    ('cap6', 4096, fan(512), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {'MCL_SWEEP_STEP_CAP': '6'}),
    ('cap5_wide', 8192, fan(33), dict(centre=MID, sigma_xy=30.0, sigma_yaw=1.0), {'MCL_SWEEP_STEP_CAP': '5'}),
    ('wavecap', 4096, fan(512), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {'MCL_SWEEP_STEP_CAP': '5', 'MCL_SWEEP_WAVE_CAP': '7'}),
    # the shared walk hands over to the per-lane loop where the lanes of a wave part, at either parity
    ('shared_collapsed', 4096, fan(512), dict(centre=MID, sigma_xy=0.05, sigma_yaw=1e-3), {'MCL_SWEEP_UNIFORM': '1'}),
    ('shared_tight', 4096, fan(64), dict(centre=MID, sigma_xy=0.01, sigma_yaw=1e-3), {'MCL_SWEEP_UNIFORM': '1'}),
    ('shared_atan13', 4096, fan(64), dict(centre=MID, sigma_xy=0.01, sigma_yaw=1e-3, yaw=math.atan(1.0 / 3.0)), {'MCL_SWEEP_UNIFORM': '1'}),
    ('shared_diag', 4096, fan(64), dict(centre=MID, sigma_xy=0.01, sigma_yaw=1e-3, yaw=math.pi / 4 + 0.01), {'MCL_SWEEP_UNIFORM': '1'}),
    ('lane_tight', 4096, fan(64), dict(centre=MID, sigma_xy=0.01, sigma_yaw=1e-3), {}),
    ('lane_atan13', 4096, fan(64), dict(centre=MID, sigma_xy=0.01, sigma_yaw=1e-3, yaw=math.atan(1.0 / 3.0)), {}),
    ('lane_diag', 4096, fan(64), dict(centre=MID, sigma_xy=0.01, sigma_yaw=1e-3, yaw=math.pi / 4 + 0.01), {}),
]
SWITCHES = ('MCL_SWEEP_STEP_CAP', 'MCL_SWEEP_WAVE_CAP', 'MCL_SWEEP_UNIFORM')

def switch(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)

for diag, dname in (('00-11', 'd2'), ('10-01', 'd3')):
    verts, tris = synth.mesh_from_grid(z, 1.0, origin, diagonal=diag)
    for name, n, ba, cl, env in SCENES:
        if only and name not in only:
            continue
        tag = '%%s_%%s' %% (name, dname)
        sys.stderr.write('@scene %%s\n' %% tag)
        sys.stderr.flush()
        switch(env)
        cl = dict(cl)
        yaw = cl.pop('yaw', 0.0)
        soa = cloud(n, 10, **cl)   # (one seed: scenes that differ in a switch alone see the same cloud)
        soa[5] += yaw
        e = eng.Engine(n, rng_mode=eng.RNG_REPLAY)
        e.set_map_mesh(verts, tris)
        e.set_particles(soa)
        B = len(ba)
        rs = np.random.RandomState(3)
        ranges = (15.0 / np.cos(ba) + 0.1 * rs.randn(B)).astype(np.float32)
        ranges[::9] = 0.0
        e.update_mbes(ranges, ba, 0.2, 100.0)
        path = e.mbes_last_path()
        assert path[0] == 1, path
        out['lw_' + tag] = e.get_log_weights()
        out['path_' + tag] = np.array(path)
        e.close()
    # twelve fused steps: straight after a predict the library may prove that no beam meets the seabed beyond r_max and
    # the loop leaves the clamp out (r_max 100 m: proved; 44 m and 30 m: the outer beams reach further, the clamp stays)
    if only and 'steps' not in only:
        continue
    switch({})
    B = 64
    ba = synth.beam_angles(B)
    stream = synth.odom_stream(12)
    for r_max in (100.0, 44.0, 30.0):
        sys.stderr.write('@scene steps_%%s_%%g\n' %% (dname, r_max))
        sys.stderr.flush()
        e = eng.Engine(8192, seed=5, init_cov=[0.5, 0.5, 0, 0, 0, 0.01], process_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5],
                       resample_cov=[1e-3, 1e-3, 0, 0, 0, 1e-5])
        e.set_map_mesh(verts, tris)
        e.init_particles()
        rs = np.random.RandomState(11)
        for k in range(12):
            ranges = np.minimum(18.0 / np.cos(ba) + 0.3 * rs.randn(B), r_max - 0.5).astype(np.float32)
            ranges[5::17] = 0.0
            e.step_mbes(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'], ranges, ba, 0.2, r_max)
        e.sync()
        assert e.mbes_last_path()[0] == 1
        out['steps_part_%%s_%%g' %% (dname, r_max)] = e.get_particles()
        out['steps_hist_%%s_%%g' %% (dname, r_max)] = e.mean_history(12)
        e.close()
np.savez(sys.argv[1], **out)
'''

N_SCENES = 20


def _variant():
    variant = os.path.join(ROOT, 'smarc_navigation_amd', 'libmcl_hip_cxxmerge.so')   # (built by __graft_entry__.build())
    if not os.path.exists(variant):
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        if not os.path.exists(hipcc):
            pytest.skip('no prebuilt variant and no hipcc on this box')
        subprocess.check_call(['make', '-C', CSRC, '../libmcl_hip_cxxmerge.so', 'HIPCC=' + hipcc])
    return variant


def _run(tmp, name, lib, scenes=(), debug=False):
    child = str(tmp / 'child.py')
    with open(child, 'w') as f:
        f.write(_CHILD % {'root': ROOT})
    env = dict(os.environ)
    for k in ('MCL_LIB', 'MCL_SWEEP_UNIFORM', 'MCL_DEBUG_WORK', 'MCL_SWEEP', 'MCL_VISIT', 'MCL_SWEEP_STEP_CAP', 'MCL_SWEEP_WAVE_CAP'):
        env.pop(k, None)
    env['MCL_SWEEP_NSUB'] = '1'
    env['MCL_SWEEP'] = '1'   # (clouds below 8 192 particles are swept only on request)
    if lib:
        env['MCL_LIB'] = lib
    if debug:
        env['MCL_DEBUG_WORK'] = '1'
    out = str(tmp / (name + '.npz'))
    p = subprocess.run([sys.executable, child, out] + list(scenes), env=env, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(out), p.stderr


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('walk_asm')
    variant = _variant()
    return {'asm': _run(tmp, 'asm', None), 'cxx': _run(tmp, 'cxx', variant)}


def test_assembly_walk_loop_equals_the_compilers_bit_for_bit(runs):
    asm, cxx = runs['asm'][0], runs['cxx'][0]
    assert sorted(asm.files) == sorted(cxx.files)
    assert len([k for k in asm.files if k.startswith('lw_')]) == 2 * N_SCENES
    assert len([k for k in asm.files if k.startswith('steps_')]) == 12
    for k in asm.files:
        a, c = asm[k], cxx[k]
        if k.startswith('path_'):
            assert np.array_equal(a, c), (k, a, c)
            continue
        assert np.isfinite(a).all(), k
        assert np.array_equal(a, c), '%s: %d of %d values differ (max %.3e)' % (k, (a != c).sum(), a.size, np.abs(a - c).max())


def test_border_and_step_limits_hand_over_alike(runs):
    asm, cxx = runs['asm'][0], runs['cxx'][0]
    for d in ('d2', 'd3'):
        # the cloud over the border: some particles handed over, some slices ended on the ring of NaNs inside the sweep
        h = int(asm['path_border_' + d][1])
        assert 0 < h < 8192 and h == int(cxx['path_border_' + d][1]), (d, h)
        # the step limit and the wave's bound: every walk of the collapsed cloud is cut, every particle handed over
        for name in ('cap5', 'cap6', 'wavecap'):
            assert int(asm['path_%s_%s' % (name, d)][1]) == 4096 == int(cxx['path_%s_%s' % (name, d)][1]), (name, d)
            assert np.array_equal(asm['lw_%s_%s' % (name, d)], asm['lw_cap5_' + d]), (name, d)
        h = int(asm['path_cap5_wide_' + d][1])
        assert h > 0 and h == int(cxx['path_cap5_wide_' + d][1]), (d, h)
        # without the limits the same cloud is swept
        assert int(asm['path_collapsed_' + d][1]) == 0


def test_shared_walk_hands_over_to_the_assembly_loop_bit_for_bit(runs):
    asm = runs['asm'][0]
    for d in ('d2', 'd3'):
        assert np.array_equal(asm['lw_shared_collapsed_' + d], asm['lw_collapsed_' + d]), d
        assert np.array_equal(asm['path_shared_collapsed_' + d], asm['path_collapsed_' + d]), d
        for name in ('tight', 'atan13', 'diag'):
            a, c = asm['lw_shared_%s_%s' % (name, d)], asm['lw_lane_%s_%s' % (name, d)]
            assert np.array_equal(a, c), '%s %s: %d of %d log-weights differ' % (name, d, (a != c).sum(), a.size)
            assert np.array_equal(asm['path_shared_%s_%s' % (name, d)], asm['path_lane_%s_%s' % (name, d)]), (name, d)


def test_fused_steps_ran_with_and_without_the_clamp(tmp_path):
    """the host's verdict on the clamp (the same in every build) for the r_max values of the fused scenes: a child under
    MCL_DEBUG_WORK, which prints it"""
    _, err = _run(tmp_path, 'dbg', None, scenes=('steps',), debug=True)
    assert 'proved idle: skipped' in err and 'r_max kept' in err, err[-2000:]

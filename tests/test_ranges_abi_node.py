"""CPU tests of the DVL / altimeter range update's plumbing: the two C entry points are exported and bound and refuse a
null handle without a device; the node turns a smarc_msgs/DVL altitude into mcl_update_ranges + a resampling (a
recording engine stands in for the GPU, the ROS stand-ins of tests/ros_stubs plus a `smarc_msgs` injected through
sys.modules for the transport); the new kernel keeps out of scratch (tools/isa.sh, as test_isa_resources.py reads it)."""
import ctypes
import importlib
import math
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, 'tests', 'ros_stubs')
_STUB_MODS = ('rospy', 'tf', 'tf2_ros', 'geometry_msgs', 'geometry_msgs.msg', 'nav_msgs', 'nav_msgs.msg', 'sensor_msgs',
              'sensor_msgs.msg', 'std_msgs', 'std_msgs.msg', 'smarc_msgs', 'smarc_msgs.msg')


def test_symbols_exported_bound_and_null_handle_refused():
    from smarc_navigation_amd import _lib
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ('mcl_update_ranges', 'mcl_ranges_expected'):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    L = _lib.load()
    r = np.ones(1, np.float32)
    d = np.array([0.0, 0.0, -1.0], np.float32)
    out = np.zeros(1, np.float32)
    assert L.mcl_update_ranges(None, r.ctypes.data, d.ctypes.data, 1, 0.2, 60.0, None, 0) == -1
    assert L.mcl_ranges_expected(None, 0, 1, d.ctypes.data, 1, 60.0, None, out.ctypes.data) == -1


class FakeEngine(object):
    """Records the ABI-level calls the node makes."""
    calls = []

    def __init__(self, n, **kw):
        self.n = n
        FakeEngine.calls.append(('create', n, kw))

    def __getattr__(self, name):
        def f(*a, **k):
            FakeEngine.calls.append((name, a, k))
            if name == 'mean_cov':
                return np.zeros(6), 0.0, np.zeros(9)
            return None
        return f


class DVL(object):
    """smarc_msgs/DVL stand-in (header, velocity, altitude)"""

    def __init__(self, altitude=0.0):
        from smarc_navigation_amd import msgs
        self.header = msgs.Header()
        self.velocity = msgs.Vector3()
        self.altitude = altitude


@pytest.fixture
def ros(monkeypatch, tmp_path):
    """ros_node with the stand-in ROS on the path, a smarc_msgs.msg holding DVL, the recording engine, a map file"""
    monkeypatch.syspath_prepend(STUBS)
    for m in _STUB_MODS + ('smarc_navigation_amd.ros_node',):
        sys.modules.pop(m, None)
    pkg, msg = types.ModuleType('smarc_msgs'), types.ModuleType('smarc_msgs.msg')
    msg.DVL = DVL
    pkg.msg = msg
    monkeypatch.setitem(sys.modules, 'smarc_msgs', pkg)
    monkeypatch.setitem(sys.modules, 'smarc_msgs.msg', msg)
    node = importlib.import_module('smarc_navigation_amd.ros_node')
    import rospy
    import tf2_ros
    from smarc_navigation_amd import engine as eng
    monkeypatch.setattr(eng, 'Engine', FakeEngine)
    rospy.reset()
    tf2_ros.transforms.clear()
    tf2_ros.transforms[('map', 'sam/odom')] = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    path = str(tmp_path / 'map.npz')
    np.savez(path, z=np.full((32, 32), -20.0, np.float32), origin=np.array([-16.0, -16.0]), res=1.0)
    FakeEngine.calls = []
    yield node, rospy, path
    for m in _STUB_MODS + ('smarc_navigation_amd.ros_node',):
        sys.modules.pop(m, None)


def _params(path, **kw):
    p = {'particle_count': 32, 'map_grid_file': path, 'odom_topic': '/sam/dr/odom', 'odom_frame': 'sam/odom'}
    p.update(kw)
    return p


def test_node_subscribes_the_dvl_and_turns_an_altitude_into_a_range_update(ros):
    node, rospy, path = ros
    rospy.reset(_params(path, dvl_topic='/sam/core/dvl', dvl_altitude_std=0.15, dvl_range_max=45.0,
                        dvl_sensor_offset='[0.1, 0.0, -0.2, 0.0, 0.0, 0.05]'))
    rospy.Time._now = 100.0   # (the node starts its clock here)
    assert node.main() == 0
    assert rospy.subscribers['/sam/core/dvl'].typ is DVL
    cb = rospy.subscribers['/sam/core/dvl'].cb
    FakeEngine.calls = []
    cb(DVL(12.5))
    names = [c[0] for c in FakeEngine.calls]
    assert names == ['update_ranges', 'resample'], names
    a = FakeEngine.calls[0][1]
    assert a[0] == [12.5] and [list(x) for x in a[1]] == [[0.0, 0.0, -1.0]]
    assert (a[2], a[3], list(a[4])) == (0.15, 45.0, [0.1, 0.0, -0.2, 0.0, 0.0, 0.05])
    # no bottom lock: nothing happens
    FakeEngine.calls = []
    for alt in (0.0, -1.0, float('nan'), float('inf')):
        cb(DVL(alt))
    assert not FakeEngine.calls


def test_without_dvl_topic_the_subscriber_set_is_unchanged(ros):
    node, rospy, path = ros
    rospy.reset(_params(path))
    assert node.main() == 0
    assert set(rospy.subscribers) == {'/dive', '/gps', '/mbes_scan', '/sam/dr/odom'}


def test_altitude_waits_for_odometry_and_a_map():
    from smarc_navigation_amd import auv_pf, engine as eng
    orig = eng.Engine
    eng.Engine = FakeEngine
    try:
        FakeEngine.calls = []
        pf = auv_pf.auv_pf({'particle_count': 8})
        msg = DVL(10.0)
        pf.dvl_cb(msg)                              # no odometry yet, no map
        pf.start_timing(50.0)
        pf.dvl_cb(msg)                              # odometry, no map
        assert not [c for c in FakeEngine.calls if c[0] in ('update_ranges', 'resample')]
        pf.set_map_grid(np.full((8, 8), -20.0, np.float32), (0.0, 0.0), 1.0)
        pf2 = auv_pf.auv_pf({'particle_count': 8})
        pf2.set_map_grid(np.full((8, 8), -20.0, np.float32), (0.0, 0.0), 1.0)
        FakeEngine.calls = []
        pf2.dvl_cb(msg)                             # a map, but before the first odometry
        assert not FakeEngine.calls
        pf.dvl_cb(msg)                              # both
        assert [c[0] for c in FakeEngine.calls] == ['update_ranges', 'resample']
        assert FakeEngine.calls[0][1][:4] == ([10.0], [[0.0, 0.0, -1.0]], 0.2, 60.0)
        assert not math.isnan(auv_pf.DEFAULT_PARAMS['dvl_altitude_std']) and auv_pf.DEFAULT_PARAMS['dvl_topic'] == ''
    finally:
        eng.Engine = orig


def test_range_kernel_uses_no_scratch(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    subprocess.check_call([os.path.join(ROOT, 'tools', 'isa.sh'), str(tmp_path)], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    rows = {}
    with open(str(tmp_path / 'resources.tsv')) as f:
        next(f)
        for line in f:
            name, sgpr, vgpr, scratch, lds, occ = line.rstrip('\n').split('\t')
            rows[name] = dict(vgpr=int(vgpr), scratch=int(scratch), occ=int(occ))
    mine = {k: v for k, v in rows.items() if 'k_ranges_update' in k}
    assert len(mine) == 6, sorted(mine)   # three map storages x (update, expected ranges)
    assert all(v['scratch'] == 0 for v in mine.values()), mine

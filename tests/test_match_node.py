"""The node mirror (smarc_navigation_amd/auv_pf.py) and the ping matching, over a recording engine (no GPU): with
`mbes_match_every` 0 the call is never made and the call sequence is the one without the parameter; with 3 one
`match_estimate` is made behind the update of pings 0, 3 and 6, from the pose the node publishes, and nothing else changes;
the launch file passes the parameter; replay.py has --match and reports its summary keys."""
import logging
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from smarc_navigation_amd import msgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, YAW = np.array([12.5, -3.25, 1.0, 0.01, -0.02, 9.0]), 0.75        # (mean[5] is the arithmetic mean: not what is published)


class FakeMatch(object):
    def pose(self, i):
        return dict(x=12.75, y=-3.0, yaw=0.76, z=1.0, status='CONVERGED', rms=0.01, evaluations=4)


class RecordingEngine(object):
    calls = []
    forbid = False
    refuse = False

    def __init__(self, n, **kw):
        self.n = n
        RecordingEngine.calls.append(('create', (n,), kw))

    def __getattr__(self, name):
        def f(*a, **k):
            if name.startswith('match_') and RecordingEngine.forbid:
                raise AssertionError('%s called with mbes_match_every 0' % name)
            RecordingEngine.calls.append((name, a, k))
            if name == 'mean_cov':
                return MEAN.copy(), YAW, np.zeros(9)
            if name == 'resample_prepare':
                return 1
            if name == 'match_estimate':
                if RecordingEngine.refuse:
                    from smarc_navigation_amd import engine as eng
                    raise eng.MclError(-1, 'match_ping: B outside 1 ... 2048')
                return FakeMatch(), 0
            return None
        return f


@pytest.fixture
def node(monkeypatch):
    from smarc_navigation_amd import auv_pf, engine as e
    monkeypatch.setattr(e, 'Engine', RecordingEngine)
    RecordingEngine.calls = []
    RecordingEngine.forbid = RecordingEngine.refuse = False
    yield auv_pf
    RecordingEngine.forbid = RecordingEngine.refuse = False


def _drive(pf, pings=7):
    pf.start_timing(100.0)
    pf.set_map_grid(np.full((8, 8), -20.0, np.float32), (-4.0, -4.0), 1.0)
    ranges = np.array([18.0, 18.5, 19.0, 18.2], np.float32)
    scan = msgs.LaserScan(ranges, -0.3, 0.2, 60.0)
    a = -0.3 + 0.2 * np.arange(4)
    pc = msgs.pointcloud2_from_xyz(np.stack([np.zeros(4), ranges * np.sin(a), -ranges * np.cos(a)], axis=1), 'base')
    for k in range(pings):
        m = msgs.Odometry()
        m.header.stamp = msgs.Time(100.02 + 0.02 * k)
        m.twist.twist.linear.x = 1.0
        m.pose.pose.orientation = msgs.Quaternion(0.0, 0.0, 0.0, 1.0)
        pf.odom_callback(m)
        pf.mbes_cb(scan) if k % 3 < 2 else pf.mbes_pc_cb(pc)


def test_off_by_default_the_call_is_never_made_and_the_sequence_is_todays(node):
    assert node.DEFAULT_PARAMS['mbes_match_every'] == 0
    RecordingEngine.forbid = True
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    names = [c[0] for c in plain]
    assert names.count('update_mbes') == 7 and not [n for n in names if n.startswith('match')] and 'mean_cov' not in names
    assert pf.last_match is None and pf.match_calls == 0 and pf.match_log == []
    RecordingEngine.calls = []
    pf = node.auv_pf({'particle_count': 16, 'mbes_match_every': 0})
    _drive(pf)
    assert repr(RecordingEngine.calls) == repr(plain)


def test_every_third_ping_is_matched_after_its_update_from_the_published_pose(node, caplog):
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    RecordingEngine.calls = []
    with caplog.at_level(logging.INFO, logger='auv_pf'):
        pf = node.auv_pf({'particle_count': 16, 'mbes_match_every': 3})
        _drive(pf)
    on = list(RecordingEngine.calls)
    mine = ('match_estimate', 'mean_cov')
    assert repr([c for c in on if c[0] not in mine]) == repr(plain)         # everything else: today's sequence
    names = [c[0] for c in on]
    assert names.count('match_estimate') == 3 and names.count('mean_cov') == 3 and names.count('update_mbes') == 7   # pings 0, 3, 6
    ups = [i for i, c in enumerate(on) if c[0] == 'update_mbes']
    for i, c in enumerate(on):
        if c[0] != 'match_estimate':
            continue
        before = [u for u in ups if u < i]
        assert (len(before) - 1) % 3 == 0                                     # behind the update of every 3rd ping
        u = on[before[-1]]
        assert not [x for x in on[before[-1] + 1:i] if x[0] == 'update_mbes'] and on[i - 1][0] == 'mean_cov'
        # the ping of that update: its ranges, angles, sigma, r_max, sensor offset
        assert np.array_equal(c[1][0], u[1][0]) and np.array_equal(c[1][1], u[1][1]) and repr(c[1][2:]) == repr(u[1][2:])
        # the start: the pose the node publishes -- the mean with the wrapped-yaw mean, not mean[5]
        assert list(c[2]) == ['start'] and c[2]['start'] == [12.5, -3.25, 1.0, 0.01, -0.02, 0.75]
    assert pf.match_calls == 3 and len(pf.match_log) == 3
    assert pf.last_match['converged'] and pf.last_match['status'] == 'CONVERGED' and pf.last_match['x'] == 12.75
    assert pf.match_log[0][1:7] == ('CONVERGED', 12.75, -3.0, 0.76, 0.01, 4) and pf.match_log[0][7:] == (12.5, -3.25, 0.75)
    said = [r for r in caplog.records if 'ping match' in r.getMessage()]
    assert len(said) == 1                                                     # throttled: the pings are 20 ms apart


def test_a_match_the_library_refuses_is_logged_and_the_filter_goes_on(node, caplog):
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    RecordingEngine.calls = []
    RecordingEngine.refuse = True
    with caplog.at_level(logging.WARNING, logger='auv_pf'):
        pf = node.auv_pf({'particle_count': 16, 'mbes_match_every': 3})
        _drive(pf)                                                            # (no exception leaves the callbacks)
    on = [c for c in RecordingEngine.calls if c[0] not in ('match_estimate', 'mean_cov')]
    assert repr(on) == repr(plain)                                            # every update and resampling was made
    assert pf.match_errors == 3 and pf.match_calls == 0 and pf.last_match is None and pf.match_log == []
    assert len([r for r in caplog.records if 'ping match refused' in r.getMessage()]) == 3


@pytest.mark.parametrize('bad', [-1, 2.5, float('nan')])
def test_node_refuses_a_period_that_means_nothing(node, bad):
    with pytest.raises(ValueError):
        node.auv_pf({'particle_count': 8, 'mbes_match_every': bad})


def test_launch_file_passes_the_parameter():
    from smarc_navigation_amd import auv_pf
    root = ET.parse(os.path.join(ROOT, 'ros', 'auv_particle_filter_hip', 'launch', 'auv_pf.launch')).getroot()
    args = {a.get('name'): a.get('default') for a in root.iter('arg')}
    params = {p.get('name'): p for p in next(root.iter('node')).iter('param')}
    assert int(args['mbes_match_every']) == auv_pf.DEFAULT_PARAMS['mbes_match_every'] == 0
    assert params['mbes_match_every'].get('type') == 'int'
    assert params['mbes_match_every'].get('value') == '$(arg mbes_match_every)'
    from smarc_navigation_amd import ros_node
    assert 'mbes_match_every' in ros_node.__doc__


def test_replay_summary_reports_the_four_keys():
    """replay.match_summary over a node's match_log: the keys --match adds, with and without truth, with and without a
    converged fix"""
    from smarc_navigation_amd import replay
    log = [(100.0, 'CONVERGED', 1.0, 2.0, 0.1, 0.02, 4, 1.5, 2.0, 0.1), (100.1, 'MAX_ITER', 9.0, 9.0, 0.1, 0.5, 13, 1.0, 2.5, 0.1),
           (100.2, 'CONVERGED', 2.0, 2.0, 0.1, 0.04, 5, 2.0, 3.0, 0.1)]
    truth = np.array([[1.0, 2.0], [0.0, 0.0], [2.0, 2.5]])
    s = replay.match_summary(log, truth)
    assert s['match_calls'] == 3 and s['match_converged_share'] == 2.0 / 3.0
    assert abs(s['match_rms_residual_median'] - 0.03) < 1e-15
    assert abs(s['match_rmse_xy'] - np.sqrt((0.0 + 0.25) / 2)) < 1e-12 and abs(s['match_filter_rmse_xy'] - np.sqrt((0.25 + 0.25) / 2)) < 1e-12
    s = replay.match_summary(log)
    assert s['match_rmse_xy'] is None and s['match_calls'] == 3
    s = replay.match_summary([log[1]], truth[1:2])
    assert s['match_converged_share'] == 0.0 and s['match_rms_residual_median'] is None and s['match_rmse_xy'] is None
    assert replay.match_summary([])['match_calls'] == 0


def _hand_made_stream():
    from smarc_navigation_amd import replay
    st = replay.synthetic_stream(60)
    at = np.arange(9, 60, 10)
    st.update(mbes_idx=at, mbes_ranges=np.full((at.size, 4), 18.0, np.float32), mbes_angles=np.array([-0.3, -0.1, 0.1, 0.3], np.float32),
              mbes_range_max=60.0, map_z=np.full((8, 8), -20.0, np.float32), map_origin=np.array((-4.0, -4.0)), map_res=1.0)
    return st


def test_replay_with_the_node_parameter_reports_the_summary_keys(node):
    """the whole replay over the recording engine, on a stream whose six pings are made by hand (a synthetic stream asks
    the GPU for its pings): pings 0, 2, 4 are matched, and the summary says so"""
    from smarc_navigation_amd import replay
    st = _hand_made_stream()
    s = replay.replay(st, dict(replay.SYNTH_PARAMS, particle_count=16, mbes_match_every=2))['summary']
    assert s['mbes_match_every'] == 2 and s['match_calls'] == 3
    assert s['match_converged_share'] == 1.0 and s['match_rms_residual_median'] == 0.01
    assert s['match_rmse_xy'] > 0.0 and s['match_filter_rmse_xy'] > 0.0
    plain = replay.replay(st, dict(replay.SYNTH_PARAMS, particle_count=16))['summary']
    assert not [k for k in plain if k.startswith('match') or k == 'mbes_match_every']


def test_the_command_line_with_match_reports_the_four_keys(node, tmp_path, capsys):
    """replay.py STREAM --match [EVERY] through its argument parser, over the recording engine"""
    import json
    from smarc_navigation_amd import replay
    path = str(tmp_path / 'stream.npz')
    np.savez(path, **_hand_made_stream())
    replay.main([path, '--particles', '16', '--match', '2'])
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s['mbes_match_every'] == 2 and s['match_calls'] == 3                # pings 0, 2, 4 of 6
    for k in ('match_converged_share', 'match_rmse_xy', 'match_rms_residual_median', 'match_filter_rmse_xy'):
        assert k in s
    assert s['match_converged_share'] == 1.0 and s['match_rms_residual_median'] == 0.01 and s['match_rmse_xy'] > 0.0
    replay.main([path, '--particles', '16', '--match'])                        # no number: every ping
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s['mbes_match_every'] == 1 and s['match_calls'] == 6
    replay.main([path, '--particles', '16'])
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not [k for k in s if k.startswith('match') or k == 'mbes_match_every']
    for bad in (['--match', '-1'], ['--match', '--bag'], ['--match', '2', '--recover']):
        with pytest.raises(SystemExit):
            replay.main([path] + bad)
        capsys.readouterr()

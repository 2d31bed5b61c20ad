"""The node mirror (smarc_navigation_amd/auv_pf.py) and the swath matching, over a recording engine (no GPU): with
`mbes_swath_pings` 0 no call is made, no ring is kept and the call sequence is the one without the parameter; with K = 3,
E = 2 one `match_swath_estimate` is made behind the update of pings 2, 4 and 6 -- every second ping once the ring is full --
with the last three pings' ranges and the offsets `swath_offsets` gives for the recorded odometry, from the pose the node
publishes; a changed beam count restarts the ring; a refused call is counted; the launch file and the node's docstring carry
the two parameters; replay.py has --swath and reports its summary keys."""
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
            if 'swath' in name and RecordingEngine.forbid:
                raise AssertionError('%s called with mbes_swath_pings 0' % name)
            RecordingEngine.calls.append((name, a, k))
            if name == 'mean_cov':
                return MEAN.copy(), YAW, np.zeros(9)
            if name == 'resample_prepare':
                return 1
            if name == 'match_swath_estimate':
                if RecordingEngine.refuse:
                    from smarc_navigation_amd import engine as eng
                    raise eng.MclError(-1, 'match_swath: K B above 16384')
                return FakeMatch(), 0
            if name == 'match_estimate':
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


def _odometry(k):
    """the vehicle on a turning, diving track: what dead reckoning says at ping k"""
    yaw = 0.3 + 0.05 * k
    return [2.0 * k * np.cos(0.3), 2.0 * k * np.sin(0.3) + 0.1 * k * k, -2.0 - 0.1 * k, 0.01 * k, -0.02 + 0.005 * k, yaw]


def _ranges(k, B=4):
    return (18.0 + 0.25 * k + 0.5 * np.arange(B)).astype(np.float32)


def _drive(pf, pings=7, beams=lambda k: 4):
    from smarc_navigation_amd import auv_pf
    pf.start_timing(100.0)
    pf.set_map_grid(np.full((8, 8), -20.0, np.float32), (-4.0, -4.0), 1.0)
    for k in range(pings):
        B = beams(k)
        ranges = _ranges(k, B)
        a = -0.3 + 0.2 * np.arange(B)
        o = _odometry(k)
        m = msgs.Odometry()
        m.header.stamp = msgs.Time(100.02 + 0.02 * k)
        m.twist.twist.linear.x = 1.0
        m.pose.pose.position.x, m.pose.pose.position.y, m.pose.pose.position.z = o[0], o[1], o[2]
        m.pose.pose.orientation = msgs.Quaternion(*auv_pf.quaternion_from_euler(o[3], o[4], o[5]))
        pf.odom_callback(m)
        if k % 3 < 2:
            pf.mbes_cb(msgs.LaserScan(ranges, -0.3, 0.2, 60.0))
        else:
            pf.mbes_pc_cb(msgs.pointcloud2_from_xyz(np.stack([np.zeros(B), ranges * np.sin(a), -ranges * np.cos(a)], axis=1), 'base'))


def test_off_by_default_no_call_is_made_no_ring_is_kept_and_the_sequence_is_todays(node):
    assert node.DEFAULT_PARAMS['mbes_swath_pings'] == 0 and node.DEFAULT_PARAMS['mbes_swath_every'] == 1
    RecordingEngine.forbid = True
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    names = [c[0] for c in plain]
    assert names.count('update_mbes') == 7 and not [n for n in names if 'swath' in n] and 'mean_cov' not in names
    assert pf.last_swath is None and pf.swath_calls == 0 and pf.swath_errors == 0 and pf.swath_log == [] and pf._swath_ring is None
    RecordingEngine.calls = []
    pf = node.auv_pf({'particle_count': 16, 'mbes_swath_pings': 0, 'mbes_swath_every': 5})
    _drive(pf)
    assert repr(RecordingEngine.calls) == repr(plain) and pf._swath_ring is None


def test_three_pings_every_second_ping_with_the_offsets_of_the_recorded_odometry(node, caplog):
    from smarc_navigation_amd import engine as eng
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    RecordingEngine.calls = []
    with caplog.at_level(logging.INFO, logger='auv_pf'):
        pf = node.auv_pf({'particle_count': 16, 'mbes_swath_pings': 3, 'mbes_swath_every': 2})
        _drive(pf)
    on = list(RecordingEngine.calls)
    mine = ('match_swath_estimate', 'mean_cov')
    assert repr([c for c in on if c[0] not in mine]) == repr(plain)         # everything else: today's sequence
    names = [c[0] for c in on]
    assert names.count('match_swath_estimate') == 3 and names.count('mean_cov') == 3 and names.count('update_mbes') == 7
    ups = [i for i, c in enumerate(on) if c[0] == 'update_mbes']
    at = []
    for i, c in enumerate(on):
        if c[0] != 'match_swath_estimate':
            continue
        before = [u for u in ups if u < i]
        k = len(before) - 1                                                   # the ping whose update it stands behind
        at.append(k)
        assert on[i - 1][0] == 'mean_cov' and [x[0] for x in on[before[-1] + 1:i]].count('resample') == 1
        ranges, angles, offsets, sigma, r_max, so = c[1]
        assert ranges.shape == (3, 4) and ranges.dtype == np.float32
        assert np.array_equal(ranges, np.stack([_ranges(j) for j in (k - 2, k - 1, k)]))       # the last three pings, the newest last
        assert np.allclose(ranges[2], on[before[-1]][1][0], rtol=0, atol=1e-5) and np.array_equal(angles, on[before[-1]][1][1])
        assert (sigma, r_max) == on[before[-1]][1][2:4]
        want = eng.swath_offsets(np.array([_odometry(j) for j in (k - 2, k - 1, k)]).T)
        for f in want.dtype.names:
            assert np.allclose(offsets[f], want[f], rtol=0, atol=1e-9), f       # (the odometry went through a quaternion)
        assert offsets[2].tolist()[:3] == (0.0, 0.0, 0.0) and offsets[2]['dyaw'] == 0.0       # the anchor: the newest ping
        assert abs(offsets[2]['roll'] - _odometry(k)[3]) < 1e-12 and abs(offsets[0]['dyaw'] + 0.1) < 1e-9
        # the start: the pose the node publishes -- the mean with the wrapped-yaw mean, not mean[5]
        assert list(c[2]) == ['start'] and c[2]['start'] == [12.5, -3.25, 1.0, 0.01, -0.02, 0.75]
    assert at == [2, 4, 6]                                                    # pings 0, 2, 4, 6 are asked; the ring is full from ping 2
    assert pf.swath_calls == 3 and len(pf.swath_log) == 3 and pf.swath_errors == 0
    assert pf.last_swath['converged'] and pf.last_swath['status'] == 'CONVERGED' and pf.last_swath['x'] == 12.75
    assert pf.swath_log[0][1:7] == ('CONVERGED', 12.75, -3.0, 0.76, 0.01, 4) and pf.swath_log[0][7:] == (12.5, -3.25, 0.75)
    said = [r for r in caplog.records if 'swath match' in r.getMessage()]
    assert len(said) == 1                                                     # throttled: the pings are 20 ms apart


def test_every_ping_once_the_ring_is_full_by_default(node):
    pf = node.auv_pf({'particle_count': 16, 'mbes_swath_pings': 3})
    _drive(pf)
    assert pf.swath_calls == 5                                                # pings 2 ... 6


def test_a_changed_beam_count_restarts_the_ring(node):
    pf = node.auv_pf({'particle_count': 16, 'mbes_swath_pings': 3})
    _drive(pf, pings=9, beams=lambda k: 4 if k < 4 else 6)                    # pings 0 ... 3 of 4 beams, then 6
    calls = [c for c in RecordingEngine.calls if c[0] == 'match_swath_estimate']
    assert [c[1][0].shape for c in calls] == [(3, 4), (3, 4), (3, 6), (3, 6), (3, 6)]          # behind pings 2, 3, then 6, 7, 8
    assert np.array_equal(calls[2][1][0], np.stack([_ranges(j, 6) for j in (4, 5, 6)]))
    assert pf.swath_calls == 5


def test_a_swath_the_library_refuses_is_counted_and_the_filter_goes_on(node, caplog):
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    plain = list(RecordingEngine.calls)
    RecordingEngine.calls = []
    RecordingEngine.refuse = True
    with caplog.at_level(logging.WARNING, logger='auv_pf'):
        pf = node.auv_pf({'particle_count': 16, 'mbes_swath_pings': 3, 'mbes_swath_every': 2})
        _drive(pf)                                                            # (no exception leaves the callbacks)
    on = [c for c in RecordingEngine.calls if c[0] not in ('match_swath_estimate', 'mean_cov')]
    assert repr(on) == repr(plain)                                            # every update and resampling was made
    assert pf.swath_errors == 3 and pf.swath_calls == 0 and pf.last_swath is None and pf.swath_log == []
    assert len([r for r in caplog.records if 'swath match refused' in r.getMessage()]) == 3


@pytest.mark.parametrize('bad', [dict(mbes_swath_pings=-1), dict(mbes_swath_pings=2.5), dict(mbes_swath_pings=65),
                                 dict(mbes_swath_pings=float('nan')), dict(mbes_swath_pings=float('inf')),
                                 dict(mbes_swath_pings=3, mbes_swath_every=float('inf')), dict(mbes_swath_pings=3, mbes_swath_every=float('nan')),
                                 dict(mbes_swath_pings=3, mbes_swath_every=0),
                                 dict(mbes_swath_pings=3, mbes_swath_every=1.5), dict(mbes_swath_every=-2)])
def test_node_refuses_parameter_values_that_mean_nothing(node, bad):
    with pytest.raises(ValueError):
        node.auv_pf(dict(particle_count=8, **bad))


def test_launch_file_and_docstring_carry_the_two_parameters():
    from smarc_navigation_amd import auv_pf
    root = ET.parse(os.path.join(ROOT, 'ros', 'auv_particle_filter_hip', 'launch', 'auv_pf.launch')).getroot()
    args = {a.get('name'): a.get('default') for a in root.iter('arg')}
    params = {p.get('name'): p for p in next(root.iter('node')).iter('param')}
    for name in ('mbes_swath_pings', 'mbes_swath_every'):
        assert int(args[name]) == auv_pf.DEFAULT_PARAMS[name]
        assert params[name].get('type') == 'int' and params[name].get('value') == '$(arg %s)' % name
    from smarc_navigation_amd import ros_node
    assert 'mbes_swath_pings' in ros_node.__doc__ and 'mbes_swath_every' in ros_node.__doc__


def test_replay_summary_reports_the_swath_keys():
    from smarc_navigation_amd import replay
    log = [(100.0, 'CONVERGED', 1.0, 2.0, 0.1, 0.02, 4, 1.5, 2.0, 0.1), (100.1, 'MAX_ITER', 9.0, 9.0, 0.1, 0.5, 13, 1.0, 2.5, 0.1),
           (100.2, 'CONVERGED', 2.0, 2.0, 0.1, 0.04, 5, 2.0, 3.0, 0.1)]
    truth = np.array([[1.0, 2.0], [0.0, 0.0], [2.0, 2.5]])
    s = replay.swath_summary(log, truth)
    assert sorted(s) == ['swath_calls', 'swath_converged_share', 'swath_filter_rmse_xy', 'swath_rms_residual_median', 'swath_rmse_xy']
    assert s['swath_calls'] == 3 and s['swath_converged_share'] == 2.0 / 3.0 and abs(s['swath_rms_residual_median'] - 0.03) < 1e-15
    assert abs(s['swath_rmse_xy'] - np.sqrt((0.0 + 0.25) / 2)) < 1e-12 and abs(s['swath_filter_rmse_xy'] - np.sqrt((0.25 + 0.25) / 2)) < 1e-12
    assert replay.swath_summary([])['swath_calls'] == 0 and replay.swath_summary(log)['swath_rmse_xy'] is None
    m = replay.match_summary(log, truth)                                      # the ping match's keys are what they were
    assert sorted(m) == [k.replace('swath', 'match') for k in sorted(s)] and [m[k.replace('swath', 'match')] for k in sorted(s)] == [s[k] for k in sorted(s)]


def _hand_made_stream():
    from smarc_navigation_amd import replay
    st = replay.synthetic_stream(60)
    at = np.arange(9, 60, 10)
    st.update(mbes_idx=at, mbes_ranges=np.full((at.size, 4), 18.0, np.float32), mbes_angles=np.array([-0.3, -0.1, 0.1, 0.3], np.float32),
              mbes_range_max=60.0, map_z=np.full((8, 8), -20.0, np.float32), map_origin=np.array((-4.0, -4.0)), map_res=1.0)
    return st


def test_the_command_line_with_swath_reports_the_keys_and_without_it_none(node, tmp_path, capsys):
    """replay.py STREAM --swath K [EVERY] through its argument parser, over the recording engine, on a stream whose six pings
    are made by hand"""
    import json
    from smarc_navigation_amd import replay
    path = str(tmp_path / 'stream.npz')
    np.savez(path, **_hand_made_stream())
    replay.main([path, '--particles', '16', '--swath', '3', '2'])
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s['mbes_swath_pings'] == 3 and s['mbes_swath_every'] == 2 and s['swath_calls'] == 2          # pings 2, 4 of 0 ... 5
    for k in ('swath_converged_share', 'swath_rmse_xy', 'swath_rms_residual_median', 'swath_filter_rmse_xy'):
        assert k in s
    assert s['swath_converged_share'] == 1.0 and s['swath_rms_residual_median'] == 0.01 and s['swath_rmse_xy'] > 0.0
    assert not [k for k in s if k.startswith('match')]
    replay.main([path, '--particles', '16', '--swath', '2'])                  # no EVERY: every ping once the ring is full
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s['mbes_swath_pings'] == 2 and s['mbes_swath_every'] == 1 and s['swath_calls'] == 5
    replay.main([path, '--particles', '16', '--swath', '2', '--match', '2'])  # with --match: its RMSE beside the swath's
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 'match_rmse_xy' in s and 'swath_rmse_xy' in s and s['match_calls'] == 3
    replay.main([path, '--particles', '16'])
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not [k for k in s if 'swath' in k]
    for bad in (['--swath', '0'], ['--swath', '65'], ['--swath', '3', '0'], ['--swath', '3', '1', '1'], ['--swath', '3', '--bag'],
                ['--swath', '3', '--recover']):
        with pytest.raises(SystemExit):
            replay.main([path] + bad)
        capsys.readouterr()

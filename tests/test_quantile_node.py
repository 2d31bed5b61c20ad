"""The node mirror (smarc_navigation_amd/auv_pf.py) and the credible region, over a recording engine (no GPU): with
`credible_prob` 0 the call is never made; with 0.95 one `credible` is made per loc_loop, about the pose that loc_loop
publishes; the launch file passes the parameter; replay.py has --credible and --estimate median."""
import math
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from smarc_navigation_amd import msgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, YAW = np.array([12.5, -3.25, 1.0, 0.0, 0.0, 0.0]), 0.75


class RecordingEngine(object):
    """Records the engine calls the node makes; credible can be made to raise."""
    calls = []
    forbid = False

    def __init__(self, n, **kw):
        self.n = n
        RecordingEngine.calls.append(('create', (n,), kw))

    def __getattr__(self, name):
        def f(*a, **k):
            if (name.startswith('cloud_') or name == 'credible') and RecordingEngine.forbid:
                raise AssertionError('%s called with credible_prob 0' % name)
            RecordingEngine.calls.append((name, a, k))
            if name == 'mean_cov':
                return MEAN.copy(), YAW, np.zeros(9)
            if name == 'poses':
                return np.zeros((self.n, 7))
            if name == 'resample_prepare':
                return 1
            if name == 'credible':
                from smarc_navigation_amd import engine as eng
                probs, centre = a[0], a[1]
                return eng.Credible(median=centre, radius={p: 1.5 for p in probs}, yaw_halfwidth={p: 0.25 for p in probs},
                                    n_used=self.n, centre=centre)
            return None
        return f


@pytest.fixture
def node(monkeypatch):
    from smarc_navigation_amd import auv_pf, engine as eng
    monkeypatch.setattr(eng, 'Engine', RecordingEngine)
    RecordingEngine.calls = []
    RecordingEngine.forbid = False
    yield auv_pf
    RecordingEngine.forbid = False


def _odom(stamp):
    m = msgs.Odometry()
    m.header.stamp = msgs.Time(stamp)
    m.twist.twist.linear.x = 1.0
    m.pose.pose.orientation = msgs.Quaternion(0.0, 0.0, 0.0, 1.0)
    return m


def _drive(pf, loops=3):
    pf.start_timing(100.0)
    pf.dive_cb(msgs.Bool(False))
    for k in range(loops):
        pf.odom_callback(_odom(100.02 + 0.02 * k))
        pf.gps_odom_cb(msgs.Odometry())
        pf.loc_loop(None)


def test_off_by_default_and_the_call_is_never_made(node):
    assert node.DEFAULT_PARAMS['credible_prob'] == 0.0
    RecordingEngine.forbid = True
    pf = node.auv_pf({'particle_count': 16})
    _drive(pf)
    names = [c[0] for c in RecordingEngine.calls]
    assert names.count('mean_cov') == 3 and 'credible' not in names
    assert pf.credible_prob == 0.0 and pf.last_credible is None and pf.credible_calls == 0
    plain = list(RecordingEngine.calls)
    RecordingEngine.calls = []
    pf = node.auv_pf({'particle_count': 16, 'credible_prob': 0.0})
    _drive(pf)
    assert repr(RecordingEngine.calls) == repr(plain)


def test_on_one_credible_per_loc_loop_about_the_published_pose(node):
    pf = node.auv_pf({'particle_count': 16, 'credible_prob': 0.95})
    RecordingEngine.calls = calls = []
    _drive(pf)
    names = [c[0] for c in calls]
    assert names.count('credible') == names.count('mean_cov') == 3 and pf.credible_calls == 3
    for i, c in enumerate(calls):
        if c[0] == 'credible':
            assert calls[i - 1][0] == 'mean_cov', names                       # right after the pose it is about
            assert c[1] == ((0.95,), (12.5, -3.25, 0.75)) and not c[2]        # the probability, the published x, y, yaw
    published = pf.loc_pose.pose.pose.position
    assert (published.x, published.y) == (12.5, -3.25)
    assert pf.last_credible == dict(prob=0.95, radius=1.5, yaw_halfwidth=0.25, n_used=16, centre=(12.5, -3.25, 0.75))


@pytest.mark.parametrize('bad', [-0.1, 1.5, float('nan')])
def test_a_probability_outside_the_unit_interval_is_refused(node, bad):
    with pytest.raises(ValueError) as ei:
        node.auv_pf({'particle_count': 8, 'credible_prob': bad})
    assert 'credible_prob' in str(ei.value)


def test_launch_file_passes_the_parameter_the_way_temper_ess_ratio_is_passed():
    from smarc_navigation_amd import auv_pf
    root = ET.parse(os.path.join(ROOT, 'ros', 'auv_particle_filter_hip', 'launch', 'auv_pf.launch')).getroot()
    args = {a.get('name'): a.get('default') for a in root.iter('arg')}
    params = {p.get('name'): p for p in next(root.iter('node')).iter('param')}
    assert float(args['credible_prob']) == auv_pf.DEFAULT_PARAMS['credible_prob'] == 0.0
    assert params['credible_prob'].get('type') == params['temper_ess_ratio'].get('type') == 'double'
    assert params['credible_prob'].get('value') == '$(arg credible_prob)'


@pytest.mark.parametrize('argv', [['synth', '--credible', '-0.5'], ['synth', '--credible', '1.5'],
                                  ['some.bag', '--bag', '--credible', '0.95'], ['synth', '--estimate', 'mediann']])
def test_replay_refuses_flag_values_that_mean_nothing(argv):
    from smarc_navigation_amd import replay
    with pytest.raises(SystemExit) as ei:
        replay.main(argv)
    assert ei.value.code == 2


def test_replay_recover_names_median_among_its_estimates():
    from smarc_navigation_amd import replay
    with pytest.raises(ValueError) as ei:
        replay.replay_recover(dict(mbes_idx=[0], stamp=[0.0]), grid=dict(), estimate='centroid')
    assert "'median'" in str(ei.value)


def test_replay_summary_gains_the_radius_and_the_containment(node):
    from smarc_navigation_amd import replay
    st = replay.synthetic_stream(120)
    params = dict(replay.SYNTH_PARAMS, particle_count=64)
    off = replay.replay(st, params)['summary']
    assert not [k for k in off if k.startswith('credible')]
    on = replay.replay(st, dict(params, credible_prob=0.95))['summary']
    n_pub = [c[0] for c in RecordingEngine.calls].count('credible')
    assert on['credible_prob'] == 0.95 and on['credible_pings'] == n_pub > 0
    assert on['credible_radius_median'] == 1.5 and 0.0 <= on['credible_containment'] <= 1.0


def test_credible_summary_counts_the_truths_inside_the_stated_radius():
    from smarc_navigation_amd import replay
    est = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [3.0, 3.0, 0.0]])
    truth = est + np.array([[0.3, 0.4, 9.0], [3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [0.6, 0.8, 0.0]])   # 0.5, 5, 0, 1 away
    s = replay.credible_summary(0.95, [0.51, 4.9, 0.0, math.nan], est, truth)
    assert s == dict(credible_prob=0.95, credible_pings=4, credible_radius_median=0.51, credible_containment=0.5)
    assert replay.credible_summary(0.5, [1.0, 2.0], est[:2]) == dict(credible_prob=0.5, credible_pings=2)

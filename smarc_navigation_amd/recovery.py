"""Augmented MCL: how many random particles to inject, from a short-term and a long-term average of the likelihood.

Pure Python, no GPU: the engine reports the statistics of a ping's log-weights (Engine.weight_stats, include/mcl_recovery.h)
and injects (Engine.inject_uniform); this class only keeps the two averages in between.  The recursion is the standard
one (Thrun, Burgard, Fox: Probabilistic Robotics, table 8.3, Augmented_MCL),

    w_slow += alpha_slow (w_avg - w_slow)        w_fast += alpha_fast (w_avg - w_fast)        0 < alpha_slow < alpha_fast
    fraction = max(0, 1 - w_fast / w_slow)

with two choices of this build.  w_avg is the mean likelihood PER VALID BEAM, exp(log_mean_lik / n_valid): a ping's
likelihood is a product over its beams, so pings with different numbers of valid beams compare only per beam.  And the
averages are kept as logarithms (their ratio is all that is used, and likelihoods per beam of a lost filter underflow):
log w' = log w + log1p(alpha expm1(log w_avg - log w)).  Both averages start at the first observation.  After an injection w_fast is reset to
w_slow -- the usual guard: the injected particles lower the next ping's mean likelihood, which must not trigger the next
injection by itself.

SensorResetting (below) keeps that recursion and changes where the injected particles go: to the fixes of a swath match
(include/mcl_reseed.h) instead of a uniform scatter."""
import math

import numpy as np


def _mix(log_w, alpha, log_obs):
    """log((1 - alpha) w + alpha obs), relative to the larger of the two -- and exactly log_w when obs == w: a steady
    likelihood leaves both averages where they are, to the bit"""
    if log_w == log_obs:
        return log_w
    if log_w == -math.inf:
        return log_obs + math.log(alpha)
    d = log_obs - log_w
    if d <= 0.0:   # (1 - alpha) + alpha e^d = 1 + alpha (e^d - 1)
        t = alpha * math.expm1(d)
        return log_w + math.log1p(t) if t > -1.0 else -math.inf
    return log_obs + math.log(alpha + (1.0 - alpha) * math.exp(-d))


class AugmentedMCL(object):
    def __init__(self, alpha_slow=0.001, alpha_fast=0.1, max_fraction=0.1):
        if not (0.0 < alpha_slow < alpha_fast <= 1.0):
            raise ValueError('AugmentedMCL: need 0 < alpha_slow < alpha_fast <= 1')
        if not (0.0 <= max_fraction <= 1.0):
            raise ValueError('AugmentedMCL: max_fraction outside [0, 1]')
        self.alpha_slow, self.alpha_fast, self.max_fraction = float(alpha_slow), float(alpha_fast), float(max_fraction)
        self.log_w_slow = None
        self.log_w_fast = None
        self.last_log_lik_per_beam = None

    def observe(self, stats, n_valid):
        """stats: what Engine.weight_stats / merge_weight_stats return (an object or a dict with log_mean_lik), or the
        number itself; n_valid: valid beams of the ping (>= 1).  Returns the log-likelihood per beam it took in."""
        if isinstance(stats, dict):
            lml = stats['log_mean_lik']
        else:
            lml = getattr(stats, 'log_mean_lik', stats)
        lik = float(lml) / max(int(n_valid), 1)
        if math.isnan(lik) or lik == math.inf:
            raise ValueError('AugmentedMCL.observe: log_mean_lik is %r' % (lml,))
        self.last_log_lik_per_beam = lik
        if self.log_w_slow is None:
            self.log_w_slow = self.log_w_fast = lik
        else:
            self.log_w_slow = _mix(self.log_w_slow, self.alpha_slow, lik)
            self.log_w_fast = _mix(self.log_w_fast, self.alpha_fast, lik)
        return lik

    def fraction(self):
        """min(max_fraction, max(0, 1 - w_fast / w_slow)); 0 before the first observation"""
        if self.log_w_slow is None or self.log_w_slow == -math.inf:
            return 0.0
        ratio = math.exp(self.log_w_fast - self.log_w_slow) if self.log_w_fast > -math.inf else 0.0
        return min(self.max_fraction, max(0.0, 1.0 - ratio))

    def injected(self):
        """to be called after an injection: w_fast := w_slow"""
        self.log_w_fast = self.log_w_slow


class SensorResetting(object):
    """Sensor resetting (Lenser and Veloso 2000) on top of AugmentedMCL: WHEN and HOW MANY particles to inject stays the
    recursion's; WHERE comes from the measurement -- the converged fixes of a swath match started on a lattice over the
    map (include/mcl_reseed.h), instead of a uniform scatter over the footprint.

    Pure policy over an engine-shaped object (reseed_starts, pose_modes, match_swath, inject_gaussian, inject_uniform):
    no GPU of its own.  The caller feeds every ping to push() -- its ranges and the dead-reckoned pose (x, y, z, roll,
    pitch, yaw in the coordinates the state is stored in; only differences between the poses of the ring enter) -- and
    calls step() where it would have called inject_uniform: after the resample.

    step(), when aug.fraction() > 0 and the ring holds `pings` pings:
        starts = up to `modes` peaks of pose_modes + the lattice reseed_starts(box, pitch, yaw interval, n_yaw)
                 (yaw_window, standing for a compass: +- that many radians about the newest dead-reckoned heading; None:
                 the full circle)
        match  = match_swath(starts, the ring, offsets by swath_offsets with the newest ping as the anchor)
        comps  = reseed_select(match, select_cfg)
        inject_gaussian(fraction (1 - uniform_share), comps), then with uniform_share > 0 inject_uniform(fraction
        uniform_share) over the box and the same yaw interval; aug.injected().
    With no component selected, or while the ring is not yet full, it is inject_uniform(fraction) over the box and the yaw
    interval followed by aug.injected(): today's behaviour.  While the fraction is 0 nothing is called at all.

    Defaults (pitch 8 m, n_yaw 4: with a yaw_window of 0.4 rad the yaw cells are 0.2 rad wide and a start is at most 0.1 rad
    off): the row "pitch 8 m, yaw offset 0.1 rad" of the basin table of tools/reseed_timing.py, where 89 % of
    the starts within one pitch of the truth end within 0.5 m of it -- and about three lattice nodes lie that close.  Pitch
    4 m (99 %) costs four times the starts; over the full circle the same yaw spacing takes n_yaw = 32.  Peaks of pose_modes
    that would take the starts above the 65 536 one match call takes are left out."""

    def __init__(self, aug, select_cfg=None, pitch=8.0, n_yaw=4, yaw_window=None, uniform_share=0.0, modes=4, pings=4,
                 box=None, mode_cell=2.0, mode_n_yaw=36, match_kw=None):
        if not (0.0 <= uniform_share <= 1.0):
            raise ValueError('SensorResetting: uniform_share outside [0, 1]')
        if int(pings) < 1 or int(n_yaw) < 1 or not pitch > 0.0 or int(modes) < 0:
            raise ValueError('SensorResetting: pings and n_yaw >= 1, pitch > 0, modes >= 0')
        if yaw_window is not None and not (0.0 < yaw_window <= math.pi):
            raise ValueError('SensorResetting: yaw_window outside (0, pi]')
        self.aug, self.select_cfg = aug, select_cfg
        self.pitch, self.n_yaw, self.yaw_window = float(pitch), int(n_yaw), yaw_window
        self.uniform_share, self.modes, self.pings, self.box = float(uniform_share), int(modes), int(pings), box
        self.mode_cell, self.mode_n_yaw, self.match_kw = float(mode_cell), int(mode_n_yaw), dict(match_kw or {})
        self._ranges, self._poses = [], []
        self.last = None
        self.calls = self.fallbacks = self.components = self.injected = 0

    def push(self, ranges, pose6):
        """one ping: its ranges (B) and the dead-reckoned pose at it; the ring keeps the newest `pings`"""
        self._ranges.append(list(ranges))
        self._poses.append([float(v) for v in pose6])
        del self._ranges[:-self.pings], self._poses[:-self.pings]

    def ring_full(self):
        return len(self._ranges) == self.pings

    def _yaw_interval(self):
        if self.yaw_window is None or not self._poses:
            return (-math.pi, math.pi)
        h = self._poses[-1][5]
        return (h - self.yaw_window, h + self.yaw_window)

    def step(self, engine, beam_angles, sigma, r_max, sensor_offset=None):
        """to be called after the resample; returns the number of particles injected (0 while the fraction is 0)"""
        from . import engine as _engine   # (device-free helpers: swath_offsets, reseed_select)
        frac = self.aug.fraction()
        if not frac > 0.0:
            return 0
        self.calls += 1
        yaw = self._yaw_interval()
        last = dict(fraction=frac, yaw=yaw, fallback=True, starts=0, components=0, injected=0, match=None, indices=None)
        comps = ()
        if self.ring_full():
            p = self._poses[-1]
            starts = np.asarray(engine.reseed_starts(self.box, self.pitch, yaw, self.n_yaw, z=p[2], roll=p[3], pitch_angle=p[4]),
                                np.float64).reshape(6, -1)
            if self.modes > 0:   # the peaks first: the lattice's columns keep their order behind them
                peaks = [np.asarray(m.mean, np.float64).reshape(6, 1)
                         for m in engine.pose_modes(self.mode_cell, self.mode_n_yaw, self.modes)[0]]
                starts = np.concatenate(peaks[:max(0, _engine.RESEED_MAX_STARTS - starts.shape[1])] + [starts], axis=1)
            offsets = _engine.swath_offsets(np.asarray(self._poses, np.float64).T, -1)
            match = engine.match_swath(starts, np.asarray(self._ranges, np.float32), beam_angles, offsets, sigma, r_max,
                                       sensor_offset, **self.match_kw)
            comps, idx = _engine.reseed_select(match, cfg=self.select_cfg)
            last.update(starts=starts.shape[1], components=len(comps), match=match, indices=idx)
        if len(comps):
            k = engine.inject_gaussian(frac * (1.0 - self.uniform_share), comps)
            if self.uniform_share > 0.0:
                k += engine.inject_uniform(frac * self.uniform_share, self.box, frame='odom', yaw=yaw)
            last['fallback'] = False
            self.components += len(comps)
        else:
            k = engine.inject_uniform(frac, self.box, frame='odom', yaw=yaw)
            self.fallbacks += 1
        self.aug.injected()
        last['injected'] = k
        self.injected += k
        self.last = last
        return k

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
injection by itself."""
import math


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

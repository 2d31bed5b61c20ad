"""KLD-sampling across handles (include/mcl_kld.h): the cloud gets the size the spread of the posterior calls for by MOVING
between engines of different, fixed sizes.

KldLadder is the policy (pure Python, no device, no library): which of a ladder of sizes the number k of occupied cells
asks for, up at once and down only after a run of calls that all asked for less.  AdaptiveCloud ties it to the engines:
after every resample it counts k on the active engine (Engine.kld_bins), asks the ladder, and when the rung changes draws
the target engine's particles from the just-resampled cloud (Engine.resample_into).

Memory: every engine owns its own copy of the map and its own buffers, sized by its own particle count -- a ladder costs
the map once per rung plus the sum of the rungs' states (dominated by the largest), not the largest alone.  Sharing one
map between handles is not part of this."""
import math

KLD_Z_99 = 2.3263478740408408     # the upper 0.99 quantile of the standard normal (delta = 0.01)


def kld_bound(k, epsilon=0.05, z=KLD_Z_99, n_min=1, n_max=2 ** 31):
    """mcl_kld_bound in Python doubles, with exactly its operation order (include/mcl_kld.h): the same integer"""
    k, n_min, n_max = int(k), int(n_min), int(n_max)
    epsilon, z = float(epsilon), float(z)
    if (k < 0 or not math.isfinite(epsilon) or not epsilon > 0.0 or not math.isfinite(z) or z < 0.0 or
            not 1 <= n_min <= n_max <= 2 ** 31):
        raise ValueError('kld_bound: k >= 0, epsilon > 0, z >= 0, 1 <= n_min <= n_max <= 2^31')
    if k <= 1:
        return n_min
    km1 = float(k - 1)
    a = 2.0 / (9.0 * km1)
    t = (1.0 - a) + math.sqrt(a) * z
    v = km1 / (2.0 * epsilon)
    v = v * t
    v = v * t
    v = v * t
    if not math.isfinite(v):
        return n_max
    c = math.ceil(v)
    return n_max if c >= n_max else (n_min if c <= n_min else int(c))


class KldLadder(object):
    """Which rung of `sizes` (ascending particle counts) the cloud should stand on.  want(k): the smallest size >=
    headroom * kld_bound(k, epsilon, z), the top one if there is none.  decide(k) goes UP at once; it goes DOWN only after
    `patience` consecutive calls that wanted a lower rung, and then to the highest rung wanted during that streak.  The
    ladder starts on its top rung.  Deterministic: a function of the sequence of k alone."""

    def __init__(self, sizes, epsilon=0.05, z=KLD_Z_99, headroom=2.0, patience=5):
        self.sizes = [int(s) for s in sizes]
        if not self.sizes or any(s < 1 for s in self.sizes) or any(b <= a for a, b in zip(self.sizes, self.sizes[1:])):
            raise ValueError('KldLadder: sizes must be positive and strictly ascending')
        if not (float(headroom) >= 1.0 and math.isfinite(float(headroom))) or int(patience) < 1:
            raise ValueError('KldLadder: headroom >= 1 and patience >= 1')
        kld_bound(2, epsilon, z)   # (refuses a bad epsilon or z here, not at the first decide)
        self.epsilon, self.z, self.headroom, self.patience = float(epsilon), float(z), float(headroom), int(patience)
        self.top = len(self.sizes) - 1
        self.reset()

    def reset(self, rung=None):
        """stand on `rung` (the top one when None) with no streak"""
        self.rung = self.top if rung is None else int(rung)
        self.streak, self.streak_high = 0, 0

    def bound(self, k):
        return kld_bound(k, self.epsilon, self.z)

    def want(self, k):
        need = self.headroom * self.bound(k)
        for i, s in enumerate(self.sizes):
            if s >= need:
                return i
        return self.top

    def decide(self, k):
        w = self.want(k)
        if w < self.rung:
            self.streak_high = w if self.streak == 0 else max(self.streak_high, w)
            self.streak += 1
            if self.streak >= self.patience:
                self.rung, self.streak = self.streak_high, 0
        else:
            self.rung, self.streak = w, 0
        return self.rung


class AdaptiveCloud(object):
    """One filter over a ladder of engines.  engines: ascending particle counts, the sizes of `ladder`, each with the
    same map (set_map_grid / set_map_mesh here give it to all of them: every handle owns its own copy, see the module's
    note on memory) and the same noise settings.  `.active` is the engine in use: drive it as usual (attributes this class
    does not have are the active engine's), but resample through .resample().  cell, n_yaw, box: the lattice of kld_bins
    (the rules of Engine.pose_modes; box=None needs the map)."""

    def __init__(self, engines, ladder, cell=0.5, n_yaw=36, box=None):
        self.engines = list(engines)
        if [e.n for e in self.engines] != ladder.sizes:
            raise ValueError('AdaptiveCloud: the engines must have the sizes of the ladder, ascending')
        self.ladder, self.cell, self.n_yaw, self.box = ladder, float(cell), int(n_yaw), box
        self.grid = None
        self.trace = []          # (ping, k, bound, size after the decision) per resample
        self.moves = 0
        self._pings = 0

    @property
    def active(self):
        return self.engines[self.ladder.rung]

    def __getattr__(self, name):   # (only what this class lacks: the active engine's)
        if name in ('engines', 'ladder'):
            raise AttributeError(name)
        return getattr(self.active, name)

    def set_map_grid(self, z, origin, res):
        for e in self.engines:
            e.set_map_grid(z, origin, res)

    def set_map_mesh(self, verts, tris, **kw):
        for e in self.engines:
            e.set_map_mesh(verts, tris, **kw)

    def _move(self, rung):
        src = self.active
        src.resample_into(self.engines[rung])
        self.ladder.rung = rung
        self.moves += 1

    def resample(self, uniforms=None, normals=None, ping=None):
        """active.resample(), then k = active.kld_bins(...) and the ladder's decision; when the rung changes the target
        engine's particles are drawn from the just-resampled cloud (equal weights there: a thinning or a duplication, and
        the next predict's process noise separates the duplicates).  Returns the size in use afterwards."""
        src = self.active
        here = self.ladder.rung
        src.resample(uniforms, normals)
        if self.grid is None:
            self.grid = src.kld_grid(self.cell, self.n_yaw, self.box)
        k, _ = src.kld_bins(grid=self.grid)
        rung = self.ladder.decide(k)
        if rung != here:
            self.ladder.rung = here   # (the move is made from the engine that holds the cloud)
            self._move(rung)
        self.trace.append((self._pings if ping is None else ping, k, self.ladder.bound(k), self.active.n))
        self._pings += 1
        return self.active.n

    def to_top(self):
        """the whole ladder's room at once: for a caller whose AugmentedMCL.fraction() has turned positive (the filter may
        be lost, and an injection needs particles to replace).  True when the cloud moved."""
        if self.ladder.rung == self.ladder.top:
            self.ladder.reset(self.ladder.top)
            return False
        self._move(self.ladder.top)
        self.ladder.reset(self.ladder.top)
        return True

    def close(self):
        for e in self.engines:
            e.close()

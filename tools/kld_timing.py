#!/usr/bin/env python3
"""tools/kld_timing.py -- what KLD-sampling across handles (include/mcl_kld.h) costs on the GPU, and what it buys.

  * bins_*: Engine.kld_bins at 2^20 particles on a collapsed cloud (one cell), a decimetre-wide one and a uniform one, on
    lattices of 2^20, 2^24 and 2^27 cells over the same 192 m square; Engine.pose_modes (k = 1) on its largest lattice
    (2^24 cells) on the same clouds in the same run.  `device_us`: the library's own events around the launches
    (mcl_timing_get, slot MCL_K_MEAN_COV: mark + count + final, or the histogram, score, peaks and moments), `call_us`: the
    host's wall time of the whole call (launches, the copy back of the result and its one synchronisation); medians of
    --reps after --warmup calls.
  * transfer_*: the whole call Engine.resample_into (host wall time: it synchronises both streams) for 2^20 -> 2^14,
    2^14 -> 2^20 and 2^20 -> 2^20 with log-likelihoods pending on src, beside `device_us` of its launches (slot
    MCL_K_RESAMPLE of dst) and, in the same run, Engine.resample on 2^20 and 2^14 (wall time up to a synchronisation, and
    the sum of its slots normalise + scan + resample).
  * step_*: one tracking step predict -> update_mbes -> resample -> kld_bins per rung of the ladder (2^11 ... 2^20) on
    the 192 x 192 grid of the closed-loop tests, 64 beams: host wall time per step, median of --step-reps.
  * loop_*: the global localisation of tests/test_gpu_kld.py (AdaptiveCloud over 2^20, 2^17, 2^14, 2^11; cell 0.5 m, 36
    yaw bins; the ladder's defaults) and the same scene with 2^20 particles throughout, same seed: the per-ping trace
    (k, bound, size, error) and both final errors.
Appends one JSON line per figure to profiles/kld_timing.jsonl (and prints it); every number carries its source.  Nothing is
asserted about the numbers.  Run it under `timeout` on the GPU box:  timeout -k 10 500 python3 tools/kld_timing.py"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1 << 20
SPAN, X0 = 192.0, -96.0
LATTICES = (('2^20', 256, 256, 16), ('2^24', 1024, 1024, 16), ('2^27', 4096, 4096, 8))
SIGMA, R_MAX, BEAMS = 1.5, 80.0, 64
GRID_ORIGIN = (-96.0, -96.0)
LOOP_SIZES = (1 << 11, 1 << 14, 1 << 17, 1 << 20)
LOOP_COV = dict(process_cov=[0.01, 0.01, 0, 0, 0, 1e-4], resample_cov=[0.09, 0.09, 0, 0, 0, 2.5e-3])


def _median(vals):
    v = np.array(vals)
    return round(float(np.median(v)), 1), round(float(np.quantile(v, 0.1)), 1), round(float(np.quantile(v, 0.9)), 1)


def _cloud(kind, n, seed=1):
    rs = np.random.RandomState(seed)
    s = np.zeros((6, n))
    if kind == 'collapsed':
        s[0], s[1], s[5] = 10.01 + 0.01 * rs.rand(n), -20.01 + 0.01 * rs.rand(n), 0.501 + 0.001 * rs.rand(n)
    elif kind == 'decimetre':
        s[0], s[1], s[5] = 10.0 + 0.1 * rs.randn(n), -20.0 + 0.1 * rs.randn(n), 0.5 + 0.02 * rs.randn(n)
    else:
        s[0], s[1], s[5] = rs.uniform(X0, X0 + SPAN, n), rs.uniform(X0, X0 + SPAN, n), rs.uniform(-np.pi, np.pi, n)
    return s


def _emit(lines, **rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def _timed(e, call, slots, warmup, reps):
    dev, wall = [], []
    for k in range(warmup + reps):
        e.timing_get()                           # (reading the slots empties them)
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e6
        t = e.timing_get()
        if k >= warmup:
            dev.append(1e3 * sum(t[s][0] for s in slots))
            wall.append(dt)
    return _median(dev), _median(wall)


def bins_cases(a, engine, lines):
    src = ('measured: device_us = mcl_timing_get (events around the launches, MCL_K_MEAN_COV); call_us = host clock around the '
           'whole call, which ends in a stream synchronisation; medians of %d after %d warm-up calls' % (a.reps, a.warmup))
    e = engine.Engine(N, seed=5)
    e.timing_enable(True)
    for kind in ('collapsed', 'decimetre', 'uniform'):
        e.set_particles(_cloud(kind, N))
        for name, nx, ny, nw in LATTICES:
            g = engine.make_mode_grid(X0, X0, SPAN / nx, nx, ny, nw)
            k, n_out = e.kld_bins(grid=g)
            (du, d10, d90), (cu, c10, c90) = _timed(e, lambda g=g: e.kld_bins(grid=g), ('mean_cov',), a.warmup, a.reps)
            _emit(lines, figure='bins_%s_%s' % (kind, name), particles=N, cells=nx * ny * nw, k=k, n_outside=n_out, device_us=du,
                  device_p10_us=d10, device_p90_us=d90, call_us=cu, call_p10_us=c10, call_p90_us=c90, source=src)
        name, nx, ny, nw = LATTICES[1]
        g = engine.make_mode_grid(X0, X0, SPAN / nx, nx, ny, nw)
        (du, d10, d90), (cu, c10, c90) = _timed(e, lambda g=g: e.pose_modes(None, k=1, grid=g), ('mean_cov',), a.warmup, a.reps)
        _emit(lines, figure='pose_modes_%s_%s' % (kind, name), particles=N, cells=nx * ny * nw, k_max=1, device_us=du,
              device_p10_us=d10, device_p90_us=d90, call_us=cu, call_p10_us=c10, call_p90_us=c90, source=src)
    e.close()


def transfer_cases(a, engine, lines):
    src = ('measured: call_us = host clock around the whole call (resample_into synchronises both streams; resample is followed '
           'by sync()); device_us = mcl_timing_get of the handle the launches are queued on (resample_into: MCL_K_RESAMPLE of dst; '
           'resample: normalise + scan + resample); medians of %d after %d warm-up calls' % (a.reps, a.warmup))
    rs = np.random.RandomState(2)
    made = {}

    def handle(n, tag):
        if (n, tag) not in made:
            e = engine.Engine(n, seed=5 + len(made), resample_cov=[0.01, 0.01, 0, 0, 0, 1e-4])
            e.set_particles(_cloud('decimetre', n))
            e.timing_enable(True)
            made[(n, tag)] = e
        return made[(n, tag)]
    for ns, nd in ((1 << 20, 1 << 14), (1 << 14, 1 << 20), (1 << 20, 1 << 20)):
        s, d = handle(ns, 'src'), handle(nd, 'dst')
        s.set_log_weights(-0.5 * (3.0 * rs.randn(ns)) ** 2)
        (du, d10, d90), (cu, c10, c90) = _timed(d, lambda: s.resample_into(d), ('resample',), a.warmup, a.reps)
        _emit(lines, figure='transfer_%d_to_%d' % (ns, nd), n_src=ns, n_dst=nd, device_us=du, device_p10_us=d10, device_p90_us=d90,
              call_us=cu, call_p10_us=c10, call_p90_us=c90, source=src)
    for n in (1 << 20, 1 << 14):
        s = handle(n, 'src')
        lw = -0.5 * (3.0 * rs.randn(n)) ** 2

        def call():
            s.resample()
            s.sync()
        dev, wall = [], []
        for k in range(a.warmup + a.reps):
            s.set_log_weights(lw)
            s.timing_get()
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e6
            t = s.timing_get()
            if k >= a.warmup:
                dev.append(1e3 * sum(t[x][0] for x in ('normalise', 'scan', 'resample')))
                wall.append(dt)
        (du, d10, d90), (cu, c10, c90) = _median(dev), _median(wall)
        _emit(lines, figure='resample_%d' % n, particles=n, device_us=du, device_p10_us=d10, device_p90_us=d90, call_us=cu,
              call_p10_us=c10, call_p90_us=c90, source=src)
    for e in made.values():
        e.close()


def loop_scene(engine, synth, pings, x0=-40.0, y0=-30.0, yaw0=0.5):
    z = synth.bathymetry_grid(192, 192, 1.0, GRID_ORIGIN, seed=2, swell=2.0, fbm_amp=3.0)
    ba = synth.beam_angles(BEAMS)
    st = synth.odom_stream(n_steps=pings, dt=1.0, x0=x0, y0=y0, yaw0=yaw0)
    t = engine.Engine(64)
    t.set_map_grid(z, GRID_ORIGIN, 1.0)
    ranges = []
    for k in range(pings):
        t.set_particles(np.repeat(st['truth'][k][:, None], 64, axis=1))
        ranges.append(t.mbes_expected(0, 1, ba, R_MAX)[0].copy())
    t.close()
    return z, ba, st, ranges


def step_cases(a, engine, synth, lines):
    src = ('measured: host clock around predict + update_mbes + resample + kld_bins (cell 0.5 m, 36 yaw bins; the call ends in a '
           'stream synchronisation), a tracking cloud of sigma 0.3 m; median of %d steps after 5' % a.step_reps)
    z, ba, st, ranges = loop_scene(engine, synth, 5 + a.step_reps)
    for n in LOOP_SIZES:
        e = engine.Engine(n, seed=17, **LOOP_COV)
        e.set_map_grid(z, GRID_ORIGIN, 1.0)
        rs = np.random.RandomState(1)
        s = np.zeros((6, n))
        s[0], s[1], s[5] = -40.0 + 0.3 * rs.randn(n), -30.0 + 0.3 * rs.randn(n), 0.5 + 0.03 * rs.randn(n)
        s[2] = st['truth'][0][2]
        e.set_particles(s)
        g = e.kld_grid(0.5, 36)
        wall, bins_only = [], []
        for k in range(len(ranges)):
            e.sync()
            t0 = time.perf_counter()
            e.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], 1.0)
            e.update_mbes(ranges[k], ba, SIGMA, R_MAX)
            e.resample()
            e.sync()
            t1 = time.perf_counter()
            kk = e.kld_bins(grid=g)[0]
            t2 = time.perf_counter()
            if k >= 5:
                wall.append((t2 - t0) * 1e6)
                bins_only.append((t2 - t1) * 1e6)
        (su, s10, s90), (bu, b10, b90) = _median(wall), _median(bins_only)
        _emit(lines, figure='step_%d' % n, particles=n, beams=BEAMS, step_us=su, step_p10_us=s10, step_p90_us=s90, kld_bins_call_us=bu,
              kld_bins_call_p10_us=b10, kld_bins_call_p90_us=b90, k_last=kk, source=src)
        e.close()


def loop_cases(a, engine, synth, lines):
    from smarc_navigation_amd.adaptive import AdaptiveCloud, KldLadder
    src = 'measured: the closed loop of tests/test_gpu_kld.py, seed 17; error = |mean pose - truth| in the plane after each ping'
    pings = 60
    z, ba, st, ranges = loop_scene(engine, synth, pings)

    def run(cloud, resample):
        err = []
        t0 = time.perf_counter()
        for k in range(pings):
            cloud.predict(st['v'][k], st['wz'][k], st['q'][k], st['z'][k], 1.0)
            cloud.update_mbes(ranges[k], ba, SIGMA, R_MAX)
            resample(k)
            mean = cloud.mean_cov()[0]
            err.append(round(float(np.hypot(mean[0] - st['truth'][k][0], mean[1] - st['truth'][k][1])), 3))
        return err, time.perf_counter() - t0
    cloud = AdaptiveCloud([engine.Engine(n, seed=17, **LOOP_COV) for n in LOOP_SIZES], KldLadder(LOOP_SIZES, 0.05), 0.5, 36)
    cloud.set_map_grid(z, GRID_ORIGIN, 1.0)
    cloud.active.init_particles_uniform()
    err, wall = run(cloud, lambda k: cloud.resample(ping=k))
    _emit(lines, figure='loop_adaptive', sizes=list(LOOP_SIZES), epsilon=0.05, headroom=cloud.ladder.headroom, patience=cloud.ladder.patience,
          cell=0.5, n_yaw=36, trace=[[int(p), int(k), int(b), int(s), e_] for (p, k, b, s), e_ in zip(cloud.trace, err)],
          final_error_m=err[-1], final_size=int(cloud.active.n), moves=int(cloud.moves), wall_s=round(wall, 3), source=src)
    cloud.close()
    fixed = engine.Engine(1 << 20, seed=17, **LOOP_COV)
    fixed.set_map_grid(z, GRID_ORIGIN, 1.0)
    fixed.init_particles_uniform()
    err, wall = run(fixed, lambda k: fixed.resample())
    _emit(lines, figure='loop_fixed_2^20', error_per_ping=err, final_error_m=err[-1], wall_s=round(wall, 3), source=src)
    fixed.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step-reps', type=int, default=30)
    ap.add_argument('--only', choices=('bins', 'transfer', 'step', 'loop'), default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kld_timing.jsonl'))
    a = ap.parse_args()
    from smarc_navigation_amd import engine, synth
    lines = []
    if a.only in (None, 'bins'):
        bins_cases(a, engine, lines)
    if a.only in (None, 'transfer'):
        transfer_cases(a, engine, lines)
    if a.only in (None, 'step'):
        step_cases(a, engine, synth, lines)
    if a.only in (None, 'loop'):
        loop_cases(a, engine, synth, lines)
    with open(a.out, 'a') as f:
        for line in lines:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

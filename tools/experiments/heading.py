#!/usr/bin/env python3
"""The headline workload of bench.py (1 048 576 particles x 512 beams, lattice mesh) on a track at a constant heading that is
NOT a lattice axis: tools/experiments/heading.py [yaw, default 0.5 rad] [steps] [warmup].  bench.py's own track runs along x;
the shared walk of the fan sweep (mcl_sweep.h) pays while the lanes of a wave cross the same lattice edges, which at an
arbitrary heading ends where a slice passes a lattice node.  MCL_DEBUG_WORK=1 prints the shared / all walk steps per update
(do not time such a run); MCL_SWEEP_UNIFORM=1 turns the shared walk on (default: the per-lane loop)."""
import json
import math
import os
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
import bench  # noqa: E402
from smarc_navigation_amd import engine, synth  # noqa: E402

yaw = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
P, B = 1048576, 512
m = bench.build_map('mesh')
stream = synth.odom_stream(warmup + steps, yaw0=yaw)
ba = synth.beam_angles(B)
e = engine.Engine(P, seed=5, **bench.COV)
bench.attach_map(e, m)
ranges = bench.make_ranges(engine, m, stream['truth'], ba, bench.SIGMA, bench.R_MAX, device=0)
e.init_particles()


def run(k0, k1):
    for k in range(k0, k1):
        e.step_mbes(stream['v'][k], stream['wz'][k], stream['q'][k], stream['z'][k], stream['dt'], ranges[k], ba, bench.SIGMA, bench.R_MAX)


run(0, warmup)
e.sync()
t0 = time.perf_counter()
run(warmup, warmup + steps)
e.sync()
ms = 1e3 * (time.perf_counter() - t0) / steps
assert e.mbes_last_path()[0] == 1
print(json.dumps({'yaw': yaw, 'steps': steps, 'ms_per_step': ms, 'yaw_end': float(stream['rpy'][warmup + steps - 1][2])}))

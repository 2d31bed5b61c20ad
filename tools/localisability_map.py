#!/usr/bin/env python3
"""tools/localisability_map.py -- where on a map can a vehicle localise with its multibeam?

A map file in -- an .npz with a height grid (z[nx, ny], origin, res: what replay.py --map-grid takes) or a mesh (verts,
tris) --, an .npz of rasters out: over a lattice of poses `--cell` metres apart at depth `--z`, for each heading of
`--yaws`, the one-ping Cramer-Rao bounds along the direction the terrain fixes best (crlb_strong) and worst (crlb_weak,
inf where the terrain fixes one coordinate only), that worst direction (weak_axis, radians in [0, pi), map frame) and the
share of usable rays (hit_share); with several headings a cell reports the one with the worst crlb_weak
(smarc_navigation_amd.engine.localisability_map, include/mcl_information.h).  Needs the GPU; no particles are involved.

    python3 tools/localisability_map.py map.npz out.npz --cell 5 --z -2 --yaws 0 45 90 135 --beams 256 --sigma 0.2"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('map', help='.npz: z, origin, res (height grid) or verts, tris (mesh)')
    ap.add_argument('out', help='.npz to write: crlb_strong, crlb_weak, weak_axis, hit_share (ny x nx), x, y')
    ap.add_argument('--cell', type=float, default=5.0, help='lattice spacing, metres')
    ap.add_argument('--z', type=float, default=-2.0, help='the vehicle\'s height in the map frame, metres')
    ap.add_argument('--yaws', type=float, nargs='+', default=[0.0, 45.0, 90.0, 135.0], help='headings, degrees')
    ap.add_argument('--beams', type=int, default=256)
    ap.add_argument('--half-swath', type=float, default=60.0, help='degrees')
    ap.add_argument('--sigma', type=float, default=0.2, help='range noise of a beam, metres (the node\'s mbes_std)')
    ap.add_argument('--r-max', type=float, default=100.0)
    ap.add_argument('--delta-xy', type=float, default=0.5)
    ap.add_argument('--delta-yaw', type=float, default=0.01)
    ap.add_argument('--jump-max', type=float, default=None, help='metres; default min(r_max, 2048)')
    ap.add_argument('--margin', type=float, default=0.0, help='run the lattice this far past the map\'s edge, metres')
    a = ap.parse_args()
    from smarc_navigation_amd import engine, synth
    m = dict(np.load(a.map))
    e = engine.Engine(1)
    if 'z' in m:
        e.set_map_grid(m['z'], tuple(float(v) for v in m['origin']), float(m['res']))
    elif 'verts' in m and 'tris' in m:
        e.set_map_mesh(m['verts'], m['tris'])
    else:
        ap.error('the map file holds neither z / origin / res nor verts / tris')
    r = engine.localisability_map(e, a.cell, a.z, np.radians(a.yaws), synth.beam_angles(a.beams, math.radians(a.half_swath)),
                                  a.sigma, a.r_max, delta_xy=a.delta_xy, delta_yaw=a.delta_yaw, jump_max=a.jump_max,
                                  margin=a.margin)
    e.close()
    np.savez_compressed(a.out, **r)
    weak = r['crlb_weak']
    fixed = np.isfinite(weak)
    print(json.dumps(dict(cells=int(weak.size), shape=list(weak.shape), localisable_share=float(fixed.mean()),
                          crlb_weak_median=float(np.median(weak[fixed])) if fixed.any() else None,
                          crlb_strong_median=float(np.median(r['crlb_strong'][np.isfinite(r['crlb_strong'])]))
                          if np.isfinite(r['crlb_strong']).any() else None,
                          hit_share_mean=float(r['hit_share'].mean()))))
    return 0


if __name__ == '__main__':
    sys.exit(main())

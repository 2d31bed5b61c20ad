#!/usr/bin/env python3
"""Recorded answers of the reference's own Munkres (oracle/_ref/libref_munkres.so, built by oracle/Makefile where the
reference lies) on the correspondence tables of tests/test_oracle_assign.py: for every case the table and the
reference's row_of_col, so that the test runs where oracle/_ref is not built.  Data only: tables in, assignments out.
Re-run:  python oracle/ref_harness/gen_golden_munkres.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.dont_write_bytecode = True
import manifest  # noqa: E402  (this directory: where to write, and the fixture hashes)
from oracle import oracle as orc  # noqa: E402
import test_oracle_assign as t  # noqa: E402  (the cases, exactly as the test builds them)

NAME = 'munkres_ref.npz'


def main():
    out = {}

    def put(key, table):
        row_of_col = orc.ref_munkres(table)
        if row_of_col is None:
            sys.exit('oracle/_ref/libref_munkres.so is not built: run make -C oracle where the reference lies')
        out[key + '_table'] = np.ascontiguousarray(table, dtype=np.float64)
        out[key + '_row_of_col'] = np.ascontiguousarray(row_of_col, dtype=np.int32)

    for key, _, _, _, table in t.dense_cases():
        put(key, table)
    for seed in t.MAHA_SEEDS:
        soa, m2o, off, lm, cov, Q6, det = t._maha_scene(seed)
        put('maha_%d' % seed, t.maha_table(soa, m2o, off, lm, cov, Q6, det, 11.345, 9.0)[1])
    d = manifest.golden_dir()
    np.savez_compressed(os.path.join(d, NAME), **out)
    manifest.record(d, [NAME], 'oracle/ref_harness/gen_golden_munkres.py', needs_reference=True)
    print('%s: %d cases' % (NAME, len(out) // 2))


if __name__ == '__main__':
    main()

"""Generate tests/golden/ref_sweep.npz: the reference's outputs on the seeded sweep of tests/test_oracle_vs_ref.py.

Runs ONLY where oracle/_ref/libelo_ref.so has been built (oracle/build_ref.sh, from the reference checkout): it executes
the REFERENCE's grouping kernel bodies on the sweep's inputs and stores their four outputs per case and op, keyed
"<seed>/<random|select>/<output>".  The fixture is data; no reference source is stored.

    python tests/golden/make_ref_sweep.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
from oracle import grouping as G  # noqa: E402
from test_oracle_vs_ref import OPS, SWEEP, sweep_case  # noqa: E402


def main():
    if not G.have_ref():
        raise SystemExit("oracle/_ref/libelo_ref.so is not built (oracle/build_ref.sh needs the reference checkout)")
    out = {}
    for seed in range(40):
        args = sweep_case(seed)
        for op, fn in OPS:
            for j, x in enumerate(fn(*args, impl="ref")):
                out["%d/%s/%d" % (seed, op, j)] = x
    np.savez_compressed(SWEEP, **out)
    print("wrote %s: %d arrays, %d bytes" % (SWEEP, len(out), os.path.getsize(SWEEP)))


if __name__ == "__main__":
    main()

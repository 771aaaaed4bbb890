"""Generate tests/golden/grouping_forms_ref.npz: the reference's outputs on the case table of tests/grouping_forms_cases.py.

Runs ONLY where oracle/_ref/libelo_ref.so has been built (oracle/build_ref.sh, from the reference checkout): it executes the
REFERENCE's grouping kernel bodies on every case that is not a refusal and stores, keyed "<case name>/<output>", `sel`, `mask`
and the two prefix masks as their lengths (`n_valid`, `n_indis`: conftest.expand_prefix rebuilds them, as for
grouping_cases.npz).  The inputs are rebuilt from the case names, so the fixture is outputs only; no reference source is stored.

Every case is taken by the reference build, K > KT included: its per-thread arrays hold 5000 entries initialised to "far"
whatever the window, so rounds beyond the window read initialised entries.  The two "kmax" cases take their K from the
library (elo_fused_conv_random_k_dense_fits), which therefore has to be built as well.

    python tests/golden/make_grouping_forms_ref.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
from oracle import grouping as G  # noqa: E402
import grouping_forms_cases as T  # noqa: E402
from conftest import load_pkg  # noqa: E402

OUT = os.path.join(HERE, "grouping_forms_ref.npz")


def main():
    if not G.have_ref():
        raise SystemExit("oracle/_ref/libelo_ref.so is not built (oracle/build_ref.sh needs the reference checkout)")
    fits = load_pkg("_lib").lib().elo_fused_conv_random_k_dense_fits
    out = {}
    for case in T.CASES:
        if case["refuse"] is not None:
            continue
        fn = G.fused_conv_random_k if case["op"] == "random" else G.fused_conv_select_k
        sel, valid, indis, mask = fn(*T.oracle_args(case, T.resolve_K(case, fits)), impl="ref")
        for counts in (valid, indis):                          # prefix masks: ones, then zeros
            assert np.array_equal(counts[..., 0], np.arange(counts.shape[2]) < counts[..., 0].sum(-1, keepdims=True))
        name = case["name"]
        out[name + "/sel"], out[name + "/mask"] = sel, mask[..., 0].astype(np.uint8)
        out[name + "/n_valid"] = valid[..., 0].sum(-1).astype(np.int32)
        out[name + "/n_indis"] = indis[..., 0].sum(-1).astype(np.int32)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

"""CPU: the C restatement against the reference's own kernel bodies built for the host (oracle/_ref, see
oracle/build_ref.sh), on a seeded random sweep that includes heavy exact-tie inputs.  The sweep's reference outputs are
stored in tests/golden/ref_sweep.npz (tests/golden/make_ref_sweep.py), so the restatement is checked against them
everywhere, and against the live build too where oracle/_ref has been built (it cannot be built without the reference
checkout).  The tests of the contracted build need oracle/_ref and are skipped without it."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import grouping as G

SWEEP = os.path.join(GOLDEN, "ref_sweep.npz")
OPS = (("random", G.fused_conv_random_k), ("select", G.fused_conv_select_k))


def sweep_case(seed):
    """The arguments (after the op) of sweep case `seed`."""
    rng = np.random.default_rng(seed)
    B = int(rng.integers(1, 3))
    H, W = int(rng.integers(1, 12)), int(rng.integers(6, 40))
    sh, sw = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    H2, W2 = math.ceil(H / sh), math.ceil(W / sw)
    kH = int(rng.integers(1, 8))
    kW = int(rng.integers(1, min(2 * W2, 13)))
    K = int(rng.integers(1, 20))
    lattice = seed % 2 == 0
    def cloud(h, w):
        x = rng.normal(0, 2.0, (B, h, w, 3))
        if lattice:
            x = np.round(x)          # integer lattice: many equal distances and (0,0,0) points
        x[rng.random((B, h, w)) < 0.15] = 0
        return x.astype(np.float32)
    xyz1, xyz2 = cloud(H, W), cloud(H2, W2)
    N = int(rng.integers(1, 30))
    idx = np.stack([rng.integers(0, H, (B, N)), rng.integers(0, W, (B, N))], -1).astype(np.int32)
    perm = rng.permutation(kH * kW).astype(np.int32)
    dist = float(rng.choice([0.5, 2.0, 5.0, 1000.0]))
    fc = int(rng.integers(0, 2))
    return xyz1, xyz2, idx, perm, H, W, N, kH, kW, K, fc, dist, sh, sw


@pytest.mark.parametrize("seed", range(40))
def test_restatement_equals_reference_build(seed):
    args = sweep_case(seed)
    stored = np.load(SWEEP)
    for op, fn in OPS:
        a = fn(*args, impl="oracle")
        for j, x in enumerate(a):
            assert np.array_equal(x, stored["%d/%s/%d" % (seed, op, j)]), (op, j)
        if G.have_ref():
            b = fn(*args, impl="ref")
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


@pytest.mark.skipif(not G.have_ref_fma(), reason="oracle/_ref/libelo_ref_fma.so not built")
def test_contracted_reference_build_gives_the_same_outputs(golden_cases):
    """The reference is built by nvcc, which contracts a*b+c into fma by default (fused_conv.sh:2); the oracle and the
    HIP kernels use un-contracted arithmetic.  The reference bodies rebuilt WITH contraction (-ffp-contract=fast -mfma)
    reproduce every golden case and the seeded sweep bit for bit: on these inputs the neighbour decisions do not depend
    on the contraction (a distance would have to sit within one rounding of the radius or of another distance)."""
    from test_oracle_golden import _call
    meta, blobs = golden_cases
    for c in meta:
        a, b = _call(c, blobs, impl="ref"), _call(c, blobs, impl="ref_fma")
        for x, y in zip(a, b):
            assert np.array_equal(x, y), c["name"]
    differing = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        B, H, W = 1, int(rng.integers(2, 12)), int(rng.integers(8, 40))
        xyz = rng.normal(0, 2.0, (B, H, W, 3)).astype(np.float32)
        xyz[rng.random((B, H, W)) < 0.1] = 0
        N = 20
        idx = np.stack([rng.integers(0, H, (B, N)), rng.integers(0, W, (B, N))], -1).astype(np.int32)
        perm = rng.permutation(15).astype(np.int32)
        for fn in (G.fused_conv_random_k, G.fused_conv_select_k):
            a = fn(xyz, xyz, idx, perm, H, W, N, 3, 5, 4, 0, 2.0, 1, 1, impl="ref")
            b = fn(xyz, xyz, idx, perm, H, W, N, 3, 5, 4, 0, 2.0, 1, 1, impl="ref_fma")
            differing += not all(np.array_equal(x, y) for x, y in zip(a, b))
    assert differing == 0


@pytest.mark.skipif(not G.have_ref_fma(), reason="oracle/_ref/libelo_ref_fma.so not built")
def test_contraction_at_full_size_touches_only_last_ulp_ties():
    """At 64x1800 the contracted and un-contracted reference builds are NOT identical everywhere: select-k over 115 200
    centres x 75 candidates meets a few pairs of candidates whose squared distances differ in the last ulp, and fma
    rounding can order such a pair the other way (measured here: 2 of 11 059 200 index entries, i.e. one swapped pair;
    random-k: none).  Bit-equivalence of this build is therefore stated against the UN-contracted arithmetic; the
    masks and the neighbour SETS agree."""
    from conftest import load_pkg
    synth = load_pkg("synth")
    f1, f2 = synth.frame_pair(1, 64, 1800, seed=3)
    idx = synth.hw_index(1, 64, 1800)
    for fn, win, K, d in ((G.fused_conv_random_k, (9, 15), 16, 0.5), (G.fused_conv_select_k, (5, 15), 32, 1000.0)):
        perm = np.random.default_rng(1).permutation(win[0] * win[1]).astype(np.int32)
        a = fn(f1, f2, idx, perm, 64, 1800, idx.shape[1], win[0], win[1], K, 0, d, 1, 1, impl="ref")
        b = fn(f1, f2, idx, perm, 64, 1800, idx.shape[1], win[0], win[1], K, 0, d, 1, 1, impl="ref_fma")
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        moved = (a[0] != b[0]).any(-1)                                  # (B, N, K) slots whose index changed
        assert moved.sum() <= 8, moved.sum()
        for bi, n in zip(*np.nonzero(moved.any(-1))):                   # ... and only as a permutation within the centre
            assert sorted(map(tuple, a[0][bi, n])) == sorted(map(tuple, b[0][bi, n]))

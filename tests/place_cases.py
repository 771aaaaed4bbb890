"""The seeded inputs of tests/test_place_cpu.py and tests/test_place_gpu.py, and their float64 results by tests/place_reference.py
(computed once per process).  The CPU file vets the table -- every discrete result the GPU file compares EXACTLY is decided in the
reference by a gap of at least GAP, except where a tie is planted on purpose --; the GPU file then skips nothing."""
import functools
import math

import numpy as np

import place_reference as R
from conftest import load_pkg

GAP = 1e-9
LEVELS = load_pkg("sensor").ScanContext.LEVELS           # the value under test states the levels; the reference restates them
assert LEVELS == R.LEVELS == 4095

# ---- descriptor ------------------------------------------------------------------------------------------------------------------
# (n, H, W), (sectors, rings)
DESCRIPTOR_SHAPES = (((1, 2, 8), (8, 1)), ((2, 5, 67), (8, 3)), ((1, 4, 64), (60, 20)), ((3, 16, 128), (60, 20)),
                     ((1, 3, 128), (128, 32)), ((1, 1, 1), (1, 1)))


def context(sectors, rings, **kw):
    """The keywords of a sensor.ScanContext (validated by it), as the reference takes them."""
    kw = dict(dict(rings=rings, sectors=sectors, max_range=35.0, min_range=0.0, z_min=-3.0, z_step=0.005), **kw)
    load_pkg("sensor").ScanContext(**kw)
    return kw


@functools.lru_cache(maxsize=None)
def cloud(i):
    """(xyz (n,H,W,3) float32, context kwargs) of DESCRIPTOR_SHAPES[i]: points anywhere in a square that reaches beyond max_range
    (the sector is the COLUMN's, whatever the point's azimuth), heights beyond both clamps, a tenth of the cells all zero, a
    twentieth with a NaN or an infinity, some on the z axis (r2 = 0).  No point is removed: the rule is a sequence of single IEEE
    operations on the float32 inputs, so the kernel and the restatement see the same numbers at every boundary."""
    (n, H, W), (sectors, rings) = DESCRIPTOR_SHAPES[i]
    rng = np.random.default_rng(700 + i)
    xyz = np.stack([rng.uniform(-30.0, 30.0, (n, H, W)), rng.uniform(-30.0, 30.0, (n, H, W)), rng.uniform(-5.0, 20.0, (n, H, W))], -1)
    xyz = xyz.astype(np.float32)
    u = rng.random((n, H, W))
    xyz[u < 0.10] = 0.0
    bad = (u >= 0.10) & (u < 0.15)
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    axis = (u >= 0.15) & (u < 0.18)
    xyz[axis, :2] = 0.0
    return xyz, context(sectors, rings, min_range=2.0 if i % 2 else 0.0)


@functools.lru_cache(maxsize=None)
def cloud_descriptor(i):
    xyz, ctx = cloud(i)
    return R.descriptor(xyz, **ctx)


PLACED_CONTEXT = dict(rings=4, sectors=3, max_range=32.0, min_range=2.0, z_min=-3.0, z_step=0.5)       # edges 8, 16, 24, 32


def placed():
    """(xyz (1,2,7,3) float32, PLACED_CONTEXT, the descriptor worked out BY HAND (1,3,4)).  W = 7, sectors = 3: the sectors of the
    columns are 0 0 0 1 1 2 2 ((w * 3) / 7)."""
    x = np.zeros((1, 2, 7, 3), np.float32)
    want = np.zeros((1, 3, 4), np.uint16)
    # sector 0 (columns 0, 1, 2): r2 == edge2[1] = 64 exactly -> the ring ABOVE, ring 1; z = -2.5 is exactly the boundary of level 2
    x[0, 0, 0] = (8.0, 0.0, -2.5)
    # ... a second point in the same bin (|p_xy| = 10), lower: the bin holds the larger level; z just below the boundary -> level 1
    x[0, 1, 1] = (6.0, -8.0, np.nextafter(np.float32(-2.5), np.float32(-3.0)))
    want[0, 0, 1] = 2
    # ... r2 == edge2[rings] = 1024: left out; below min_range (r2 = 3.99.. < 4): left out; exactly min_range (r2 = 4): kept, ring 0
    x[0, 0, 1] = (0.0, 32.0, 5.0)
    x[0, 0, 2] = (np.nextafter(np.float32(2.0), np.float32(0.0)), 0.0, 5.0)
    x[0, 1, 2] = (0.0, -2.0, 0.0)                                                        # (0 + 3) / 0.5 = 6 -> level 7
    want[0, 0, 0] = 7
    # sector 1 (columns 3, 4): the clamps -- far below z_min -> level 1 (ring 2: r = 20); far above -> level 4095 (ring 3: r = 25)
    x[0, 0, 3] = (-20.0, 0.0, -1000.0)
    x[0, 1, 4] = (15.0, 20.0, 1.0e6)
    want[0, 1, 2], want[0, 1, 3] = 1, LEVELS
    # ... a cell with a NaN and one with an infinity: left out, like the all-zero cells
    x[0, 1, 3] = (np.nan, 3.0, 1.0)
    x[0, 0, 4] = (3.0, 3.0, np.inf)
    # sector 2 (columns 5, 6): the last level below the clamp, (2044 - (-3)) / 0.5 = 4094 -> level 4095 without clamping; 2043.5 ->
    # level 4094 in another ring
    x[0, 0, 5] = (3.0, 0.0, 2044.0)
    x[0, 1, 6] = (9.0, 0.0, 2043.5)
    want[0, 2, 0], want[0, 2, 1] = LEVELS, LEVELS - 1
    return x, dict(PLACED_CONTEXT), want


# ---- search ----------------------------------------------------------------------------------------------------------------------
# name: (sectors, rings, n, m, k, rows db holds beyond m, tie) -- tie: rings == 1 makes every term exactly 0.0 (d / sqrt(a b) =
# q v / (q v) = 1), so every dist is 0.0 or +inf: ties by construction, decided by the smaller shift and the smaller index alike
# in the kernel and the reference (the values are exact on both sides).
SEARCH = {
    "m0": (60, 20, 1, 0, 1, 2, False),
    "m0_n3_k8": (60, 20, 3, 0, 8, 0, False),
    "m1_k8_pads": (60, 20, 1, 1, 8, 0, False),
    "m2_s8": (8, 20, 3, 2, 8, 3, False),
    "m63_s60": (60, 20, 3, 63, 8, 0, False),
    "m64_s63": (63, 20, 1, 64, 1, 1, False),
    "m65_s64_r32": (64, 32, 3, 65, 8, 0, False),
    "m65_s65": (65, 20, 1, 65, 8, 2, False),
    "m257_s128_r32": (128, 32, 3, 257, 8, 0, False),
    "m64_s128_r1": (128, 1, 1, 64, 8, 0, True),
    "m63_s1": (1, 20, 3, 63, 8, 0, False),
    "m2_s1_r1": (1, 1, 1, 2, 1, 1, True),
    "m257_s60": (60, 20, 1, 257, 1, 3, False),
    "m257_s8_r32": (8, 32, 1, 257, 8, 0, False),
    "m2_s65_r32": (65, 32, 3, 2, 1, 0, False),
    "m65_s63_r1": (63, 1, 3, 65, 8, 0, True),
    "m63_s64": (64, 20, 1, 63, 1, 0, False),
}


def random_descriptors(rng, rows, sectors, rings):
    """Levels 1 .. 4095 in seven bins of ten, a tenth of the columns empty -- but never a whole descriptor."""
    d = rng.integers(1, LEVELS + 1, (rows, sectors, rings))
    d[rng.random((rows, sectors, rings)) < 0.3] = 0
    d[rng.random((rows, sectors)) < 0.1] = 0
    d[:, 0, 0] = rng.integers(1, LEVELS + 1, rows)
    return d.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def search_case(name):
    """(query (n,S,R), db (m + extra,S,R), m, k, tie, context kwargs, the reference's result)."""
    sectors, rings, n, m, k, extra, tie = SEARCH[name]
    rng = np.random.default_rng(9000 + sorted(SEARCH).index(name))
    query = random_descriptors(rng, n, sectors, rings)
    db = random_descriptors(rng, m + extra, sectors, rings)
    return query, db, m, k, tie, context(sectors, rings), R.search(query, db, m, k)


def smallest_gaps(ref, m, k):
    """(over shifts, over entries): the smallest difference between a winner and the next candidate in a reference result -- for
    every (query, entry) the two smallest dists of the shift profile, for every query the neighbours among the first k + 1 entries
    of the ranking.  A pair of infinities is no decision (infinities are compared for equality) and is left out."""
    over_shifts, over_entries = math.inf, math.inf
    profile = np.sort(ref["profile"], axis=2)
    if profile.shape[2] > 1 and m:
        two = profile[:, :, :2]
        decided = np.isfinite(two[..., 0])
        if decided.any():
            over_shifts = float((two[..., 1] - two[..., 0])[decided].min())
    for q in range(ref["best_dist"].shape[0]):
        d = np.sort(ref["best_dist"][q])[:k + 1]
        d = d[np.isfinite(d)]
        if len(d) > 1:
            over_entries = min(over_entries, float(np.diff(d).min()))
    return over_shifts, over_entries


# ---- end to end: six keyframes along a line, a query turned by seven sectors -------------------------------------------------------
E2E_H, E2E_W = 16, 128
E2E_CONTEXT = dict(rings=8, sectors=32, max_range=35.0, min_range=0.0, z_min=-3.0, z_step=0.005)         # a sector is 4 columns
E2E_TURN = 7                # sectors
E2E_KEY = 3
E2E_MOVE = (0.08, -0.06, 0.0)                                                           # 0.1 m


def e2e_position(i):
    """Off the origin: the synthetic wall 20 + 5 sin(3 az) is three-fold symmetric about it."""
    return np.array([3.0 + 1.5 * i, 2.0, 0.0])


def turned_scan(position, yaw, seed):
    """The scan of a sensor at `position` whose heading is turned by `yaw` about z: synth.range_image looks along the turned
    columns (yaw=) from the moved sensor (shift=) and returns the points in the UNTURNED frame; R_z(-yaw) takes them into the
    sensor's.  Its world pose is [R_z(yaw) | position]."""
    synth = load_pkg("synth")
    x = synth.range_image(E2E_H, E2E_W, seed=seed, yaw=yaw, shift=tuple(position), dtype=np.float64)
    hit = (x != 0).any(-1)
    c, s = math.cos(yaw), math.sin(yaw)
    out = np.stack([c * x[..., 0] + s * x[..., 1], -s * x[..., 0] + c * x[..., 1], x[..., 2]], -1)
    out[~hit] = 0.0
    return out.astype(np.float32)


def pose_of(position, yaw):
    return np.array([math.cos(0.5 * yaw), 0.0, 0.0, math.sin(0.5 * yaw), *position], np.float64)


@functools.lru_cache(maxsize=None)
def e2e():
    """dict: keys (6,H,W,3) and their world poses (6,7); query (1,H,W,3), its true pose, the shift the search must return; far
    (1,H,W,3): the scan from 100 m away; the reference's descriptors and searches of both."""
    yaw = E2E_TURN * 2.0 * math.pi / E2E_CONTEXT["sectors"]
    keys = np.stack([turned_scan(e2e_position(i), 0.0, 40 + i) for i in range(6)])
    poses = np.stack([pose_of(e2e_position(i), 0.0) for i in range(6)])
    at = e2e_position(E2E_KEY) + np.array(E2E_MOVE)
    query = turned_scan(at, yaw, 77)[None]
    far = turned_scan(e2e_position(E2E_KEY) + np.array([100.0, 0.0, 0.0]), 0.0, 78)[None]
    db = R.descriptor(keys, **E2E_CONTEXT)
    out = dict(keys=keys, poses=poses, query=query, truth=pose_of(at, yaw), yaw=yaw, far=far, db=db,
               shift=(E2E_CONTEXT["sectors"] - E2E_TURN) % E2E_CONTEXT["sectors"])
    out["query_search"] = R.search(R.descriptor(query, **E2E_CONTEXT), db, 6, 4)
    out["far_search"] = R.search(R.descriptor(far, **E2E_CONTEXT), db, 6, 4)
    return out

"""A numpy float64 / uint64 restatement of elo_map_insert and elo_map_extract (include/elo.h): the per-point rule, the key, the home
slot, and the content of a map -- the set of keys, each with {count, sx, sy, sz} -- as a function of the points put in.  Every step
after the ONE rounding of the carried point to float32 is a single IEEE operation, so numpy reproduces it bit for bit, and the
tests compare EXACTLY: keys, counts, sums, the stats words, the bits of the float32 centroids.

AMBIGUOUS points.  The device's double arithmetic may contract multiply-adds, which can move that one rounding by an ulp where the
double lies on a rounding midpoint of float32.  A point is ambiguous when rounding p' - 8 and p' + 8 double ulps gives different
floats.  The case generators REMOVE such points from the input (the cell becomes zeros: empty), and points within GATE_REL relative
of a range gate likewise; nothing is excluded from a comparison.  They assert that they removed at most REMOVED_CAP of the points.
"""
import functools
import math

import numpy as np

HALF = 1 << 20
MAX_PROBE = 128
GATE_REL = 1e-3
REMOVED_CAP = 1e-3
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
STATS = ("inserted", "filtered", "rejected", "dropped_full", "occupied")


def rotation(pose7):
    """(R (3,3), t (3)) of a [q | t] double row, q normalised, R written as the kernels write it; None: the quaternion has no
    direction (zero or non-finite norm) and its scan is skipped."""
    p = np.asarray(pose7, np.float64)
    q0, q1, q2, q3 = p[:4]
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3)
    if not (n > 0 and np.isfinite(n)):
        return None
    q0, q1, q2, q3 = q0 / n, q1 / n, q2 / n, q3 / n
    R = np.array([[1.0 - 2.0 * (q2 * q2 + q3 * q3), 2.0 * (q1 * q2 - q0 * q3), 2.0 * (q1 * q3 + q0 * q2)],
                  [2.0 * (q1 * q2 + q0 * q3), 1.0 - 2.0 * (q1 * q1 + q3 * q3), 2.0 * (q2 * q3 - q0 * q1)],
                  [2.0 * (q1 * q3 - q0 * q2), 2.0 * (q2 * q3 + q0 * q1), 1.0 - 2.0 * (q1 * q1 + q2 * q2)]])
    return R, p[4:].copy()


def carry(points32, pose7):
    """p' = R p + t in float64 from float32 points (N,3), summed in the kernel's order -> (N,3) float64, NOT yet rounded."""
    R, t = rotation(pose7)
    p = np.asarray(points32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((R[i, 0] * p[:, 0] + R[i, 1] * p[:, 1]) + R[i, 2] * p[:, 2]) + t[i] for i in range(3)], -1)


def ambiguous(p64):
    """(N,) bool: rounding p' - 8 and p' + 8 double ulps to float32 differs in some component."""
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.abs(p64))
        lo, hi = (p64 - 8.0 * ulp).astype(np.float32), (p64 + 8.0 * ulp).astype(np.float32)
    return ((lo != hi) & np.isfinite(p64)).any(-1)


def source_range(points32):
    """rf = sqrtf(x*x + y*y + z*z) in float32, summed left to right."""
    p = np.asarray(points32, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def axis_index(c32, voxel):
    """One axis of the rounded p' (float32 array): (i float64 = floor(u), g uint64, in_range bool), u = (double)c / (double)voxel."""
    u = np.asarray(c32, np.float32).astype(np.float64) / np.float64(np.float32(voxel))
    i = np.floor(u)
    ok = (i >= -float(HALF)) & (i < float(HALF))
    f = np.floor((u - i) * 65536.0)
    g = np.minimum(np.where(ok, f, 0.0).astype(np.uint64), np.uint64(65535))
    return i, g, ok


def pack(ix, iy, iz):
    """key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20), uint64; indices are integers in [-2^20, 2^20)."""
    f = [(np.asarray(v, np.int64) + HALF).astype(np.uint64) for v in (ix, iy, iz)]
    return f[0] << np.uint64(42) | f[1] << np.uint64(21) | f[2]


def unpack(key):
    k = np.asarray(key).astype(np.uint64)
    m = np.uint64(0x1FFFFF)
    return [((k >> np.uint64(s)) & m).astype(np.int64) - HALF for s in (42, 21, 0)]


def home(key, log2_capacity):
    """The splitmix64 finaliser of the key, & (C - 1)."""
    return mix(key) & np.uint64((1 << log2_capacity) - 1)


def mix(key):
    """The splitmix64 finaliser, uint64 array."""
    h = np.atleast_1d(np.asarray(key, dtype=np.uint64))
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint64(30))
        h = h * np.uint64(0xBF58476D1CE4E5B9)
        h = h ^ (h >> np.uint64(27))
        h = h * np.uint64(0x94D049BB133111EB)
        h = h ^ (h >> np.uint64(31))
    return h


def classify(xyz, pose, voxel=0.5, min_range=0.0, max_range=math.inf):
    """The per-point rule over xyz (B,H,W,3) float32 at pose (B,7) float64 -> dict of flat arrays over the B*H*W cells: kind (0
    nothing -- an empty cell or a skipped scan --, 1 filtered, 2 rejected, 3 a point), key uint64 and g (N,3) uint64 where kind == 3,
    p64 (N,3) the unrounded carried point (NaN where none was carried)."""
    xyz = np.asarray(xyz, np.float32)
    B = xyz.shape[0]
    pts = xyz.reshape(B, -1, 3)
    N = pts.shape[1]
    kind = np.zeros((B, N), np.int64)
    key = np.zeros((B, N), np.uint64)
    g = np.zeros((B, N, 3), np.uint64)
    p64 = np.full((B, N, 3), np.nan)
    lo, hi = np.float32(min_range), np.float32(max_range)
    for b in range(B):
        if rotation(pose[b]) is None:
            continue
        full = (pts[b] != 0).any(-1) | np.isnan(pts[b]).any(-1)            # exactly (0,0,0) is empty; -0.0 == 0
        rf = source_range(pts[b])
        with np.errstate(invalid="ignore"):
            gated = full & ((rf < lo) | (rf > hi))
        go = full & ~gated
        p = carry(pts[b], pose[b])
        p64[b][go] = p[go]
        with np.errstate(invalid="ignore", over="ignore"):
            p32 = p.astype(np.float32)
        finite = np.isfinite(p32).all(-1)
        idx, ok = [], finite.copy()
        for a in range(3):
            with np.errstate(invalid="ignore", over="ignore"):
                i, ga, oka = axis_index(np.where(finite, p32[:, a], np.float32(0)), voxel)
            idx.append(np.where(oka, i, 0.0).astype(np.int64))
            g[b, :, a] = ga
            ok &= oka
        kind[b] = np.where(gated, 1, np.where(go & ~ok, 2, np.where(go, 3, 0)))
        key[b] = pack(*idx)
    flat = kind.reshape(-1)
    return {"kind": flat, "key": key.reshape(-1), "g": g.reshape(-1, 3), "p64": p64.reshape(-1, 3)}


def content(xyz, pose, voxel=0.5, min_range=0.0, max_range=math.inf):
    """The map after inserting xyz at pose into an empty table large enough to drop nothing -> dict: key (m,) int64 SORTED, acc (m,4)
    int64 {count, sx, sy, sz} in that order, stats {name: int}, xyz (m,3) float32 centroids."""
    c = classify(xyz, pose, voxel, min_range, max_range)
    return content_of(c, voxel)


def content_of(c, voxel):
    point = c["kind"] == 3
    keys, inv = np.unique(c["key"][point], return_inverse=True)
    acc = np.zeros((len(keys), 4), np.int64)
    np.add.at(acc[:, 0], inv, 1)
    for a in range(3):
        np.add.at(acc[:, 1 + a], inv, c["g"][point][:, a].astype(np.int64))
    stats = {"inserted": int(point.sum()), "filtered": int((c["kind"] == 1).sum()), "rejected": int((c["kind"] == 2).sum()),
             "dropped_full": 0, "occupied": len(keys)}
    return {"key": keys.astype(np.int64), "acc": acc, "stats": stats, "xyz": centroids(keys, acc, voxel)}


def merged(contents, voxel):
    """The content of one map that took several inserts: `contents` a list of content() results."""
    key = np.concatenate([c["key"] for c in contents])
    acc = np.concatenate([c["acc"] for c in contents])
    keys, inv = np.unique(key, return_inverse=True)
    out = np.zeros((len(keys), 4), np.int64)
    np.add.at(out, inv, acc)
    stats = {n: sum(c["stats"][n] for c in contents) for n in STATS}
    stats["occupied"] = len(keys)
    return {"key": keys, "acc": out, "stats": stats, "xyz": centroids(keys, out, voxel)}


def centroids(key, acc, voxel):
    """c = ((double)i + ((double)s / (double)count + 0.5) / 65536.0) * (double)voxel per axis, rounded to float32 once."""
    idx = unpack(key)
    count = np.asarray(acc)[:, 0].astype(np.float64)
    v = np.float64(np.float32(voxel))
    cols = [((idx[a].astype(np.float64) + (np.asarray(acc)[:, 1 + a].astype(np.float64) / count + 0.5) / 65536.0) * v).astype(np.float32)
            for a in range(3)]
    return np.stack(cols, -1) if len(count) else np.zeros((0, 3), np.float32)


# ---- the cases of tests/test_world_map_gpu.py, vetted on the CPU by tests/test_world_map_cpu.py -----------------------------------
SHAPES = ((1, 3, 5), (1, 4, 64), (2, 5, 67), (3, 16, 128))         # (batch, H, W)
VOXELS = (0.1, 0.5)
GATES = (1.0, 20.0)                                                # the accounting case's min_range / max_range


def random_pose(rng, reach=100.0):
    """[q | t] float64: a random rotation, its quaternion scaled away from unit length; a translation of up to `reach` metres per
    axis, beyond half of it along one axis and beyond minus half of it along another (so a scan has coordinates of both signs)."""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    signs = rng.permutation([-1.0, 1.0, rng.choice([-1.0, 1.0])])
    return np.concatenate([q * rng.uniform(0.3, 3.0), signs * rng.uniform(0.5 * reach, reach, 3)])


def surface(rng, B, H, W, holes=0.2):
    """(B,H,W,3) float32: every row a random walk (steps of ~6 cm) from a random start within +-40 m of the sensor -- neighbouring cells
    often share a voxel, as those of a range image do --, negative and positive coordinates, `holes` of the cells empty."""
    start = rng.uniform(-40.0, 40.0, (B, H, 1, 3)) * (1.0, 1.0, 0.1)
    xyz = (start + np.cumsum(rng.normal(0.0, 0.06, (B, H, W, 3)), 2)).astype(np.float32)
    xyz[rng.random((B, H, W)) < holes] = 0.0
    return xyz


def vetted(xyz, pose, min_range=0.0, max_range=math.inf):
    """xyz with the ambiguous points and those within GATE_REL of a finite, positive gate REMOVED (zeros) -> (xyz, removed share of
    the non-empty cells).  Asserts the share stays within REMOVED_CAP."""
    xyz = np.array(xyz, np.float32)
    B = xyz.shape[0]
    flat = xyz.reshape(B, -1, 3)
    points = removed = 0
    for b in range(B):
        full = (flat[b] != 0).any(-1)
        points += int(full.sum())
        if rotation(pose[b]) is None:
            continue
        bad = ambiguous(carry(flat[b], pose[b]))
        rf = source_range(flat[b]).astype(np.float64)
        for gate in (min_range, max_range):
            if gate > 0 and math.isfinite(gate):
                bad |= np.abs(rf - gate) < GATE_REL * gate
        bad &= full
        removed += int(bad.sum())
        flat[b][bad] = 0.0
    share = removed / max(points, 1)
    assert share <= REMOVED_CAP, "the generator removed %d of %d points" % (removed, points)
    return xyz, share


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """(xyz (B,H,W,3) float32, pose (B,7) float64, removed share) of shape SHAPES[i]: surfaces at random poses, vetted."""
    B, H, W = SHAPES[i]
    rng = np.random.default_rng(400 + i)
    pose = np.stack([random_pose(rng) for _ in range(B)])
    xyz, share = vetted(surface(rng, B, H, W), pose)
    return xyz, pose, share


@functools.lru_cache(maxsize=None)
def exact_content(i, voxel):
    xyz, pose, _share = exact_case(i)
    return content(xyz, pose, voxel)


@functools.lru_cache(maxsize=None)
def accounting_case():
    """(xyz (4,16,128,3), pose (4,7), removed share): four scans about the sensor out to ~100 m behind the gates GATES; scan 2 has a
    zero quaternion (skipped whole); scan 0 holds a NaN and a 1e30 coordinate (rejected with max_range = inf, see the test) and
    scan 1 a point beyond 2^20 voxels of 0.5 m."""
    rng = np.random.default_rng(470)
    B, H, W = 4, 16, 128
    d = rng.normal(size=(B, H, W, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    xyz = (d * rng.uniform(0.2, 100.0, (B, H, W, 1))).astype(np.float32)
    xyz[rng.random((B, H, W)) < 0.25] = 0.0
    pose = np.stack([random_pose(rng, 50.0) for _ in range(B)])
    pose[2, :4] = 0.0
    xyz, share = vetted(xyz, pose, *GATES)
    xyz[0, 3, 7] = (np.nan, 1.0, 2.0)
    xyz[0, 5, 9] = (1e30, 0.0, 0.0)
    xyz[1, 2, 2] = (3.0e6, 5.0, 5.0)                                # finite; whatever the rotation, an axis lies beyond 2^20 * 0.5 m
    return xyz, pose, share


@functools.lru_cache(maxsize=None)
def order_case():
    """(xyz (6,8,64,3), pose (6,7), removed share): six overlapping scans of one place a small motion apart, so most voxels are hit
    by several scans."""
    rng = np.random.default_rng(480)
    base = surface(rng, 1, 8, 64, holes=0.1)[0]
    xyz = np.stack([np.where((base != 0).any(-1, keepdims=True), base + rng.normal(0.0, 0.02, base.shape), 0.0) for _ in range(6)])
    pose = np.stack([np.concatenate([[1.0, 0.0, 0.0, 0.002 * k], rng.uniform(-0.05, 0.05, 3)]) for k in range(6)])
    xyz, share = vetted(xyz.astype(np.float32), pose)
    return xyz, pose, share


def all_shares():
    """The removed share of every generated case."""
    return [exact_case(i)[2] for i in range(len(SHAPES))] + [accounting_case()[2], order_case()[2]]

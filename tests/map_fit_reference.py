"""A float64 numpy statement of elo_map_fit (include/elo.h): one evaluation of the scan-to-map point-to-plane sums at a world pose,
the Gauss-Newton update about the sensor's position and its iteration.  Built on tests/world_map_reference.py (the table: classify,
content, centroids, pack, home) and on pose_fit_reference.normals (the normal of a range-image cell).

Besides every sum it returns the sums of the absolute values of its terms (the scale of a float32 summation bound), the per-cell
`match` (key of the target voxel, -1 none) and the margin of every discrete decision a cell's evaluation took:

  jump     as pose_fit_reference: how far the normal's range test is from its threshold (relative)
  orient   the cosine that decides which way the normal points
  gate     | gate - |p - c| |, metres
  tie      (second-smallest d2 - smallest d2) / smallest d2 over the candidates

A margin a cell never met is +inf.  vetted() removes the scan points whose decisions could flip under last-bit differences."""
import functools
import math

import numpy as np

import pose_fit_reference as P
import world_map_reference as M

MARGIN = P.MARGIN          # of each margin's own scale
TIE_REL = 1e-9
DROP_CAP = 0.02
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]       # ascending key order


def table_of(scans, poses, voxel, min_range=0.0, max_range=math.inf):
    """The map's content after inserting scans (n,H,W,3) at poses (n,7): world_map_reference.content -- key sorted, acc, xyz."""
    return M.content(np.asarray(scans, np.float32), np.asarray(poses, np.float64), voxel, min_range, max_range)


def live_pose(pose7):
    """(R, t) of a [q | t] double row, or None: a quaternion without direction or a non-finite t gives no terms."""
    rot = M.rotation(pose7)
    if rot is None or not np.isfinite(rot[1]).all():
        return None
    return rot


def evaluate(x, pose7, table, voxel, gate=None, huber=0.1, jump_rel=0.1, min_points=1):
    """One evaluation of one scan x (H,W,3) float32 at pose7 against `table` (content()).  dict: A (6,6), b (6), cost, sw, count;
    absA, absb, abscost; match (H,W) int64; r, J of the terms (in cell order) and their cells `cell`; safe (H,W) bool: non-empty
    cells whose every margin is >= its threshold and whose carried point is not ambiguous; margins: dict of (H,W) arrays."""
    x32 = np.asarray(x, np.float32)
    H, W, _ = x32.shape
    gate = float(np.float32(voxel if gate is None else gate))
    v = np.float64(np.float32(voxel))
    full = x32.any(-1)
    inf = np.full((H, W), np.inf)
    out = {"A": np.zeros((6, 6)), "b": np.zeros(6), "cost": 0.0, "sw": 0.0, "count": 0, "absA": np.zeros((6, 6)), "absb": np.zeros(6),
           "abscost": 0.0, "match": np.full((H, W), -1, np.int64), "r": np.zeros(0), "J": np.zeros((0, 6)), "cell": np.zeros(0, np.int64),
           "safe": full.copy(), "margins": {"jump": inf, "orient": inf, "gate": inf.copy(), "tie": inf.copy()}}
    rot = live_pose(pose7)
    if rot is None:
        return out
    R, t = rot
    ns, nvalid, jump_m, orient_m = P.normals(x32, jump_rel)
    p64 = M.carry(x32.reshape(-1, 3), pose7)
    with np.errstate(invalid="ignore", over="ignore"):
        p32 = p64.astype(np.float32)
    ok = nvalid.reshape(-1) & np.isfinite(p32).all(-1)
    idx = []
    for a in range(3):
        i, _g, oka = M.axis_index(np.where(ok, p32[:, a], np.float32(0)), voxel)
        idx.append(np.where(oka, i, 0.0).astype(np.int64))
        ok &= oka
    cells = np.flatnonzero(ok)
    p = p64[cells]
    keys = np.asarray(table["key"]).astype(np.int64)
    count = np.asarray(table["acc"])[:, 0] if len(keys) else np.zeros(0, np.int64)
    cen = np.asarray(table["xyz"], np.float32).astype(np.float64).reshape(-1, 3)
    best = np.full(len(cells), np.inf)
    second = np.full(len(cells), np.inf)
    bkey = np.full(len(cells), -1, np.int64)
    bc = np.zeros((len(cells), 3))
    for dx, dy, dz in OFFSETS:
        ci = [idx[0][cells] + dx, idx[1][cells] + dy, idx[2][cells] + dz]
        inr = np.ones(len(cells), bool)
        for c in ci:
            inr &= (c >= -M.HALF) & (c < M.HALF)
        key = M.pack(*[np.where(inr, c, 0) for c in ci]).astype(np.int64)
        if len(keys):
            j = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
            found = inr & (keys[j] == key) & (count[j] >= min_points)
            c3 = cen[j]
        else:
            found, c3 = np.zeros(len(cells), bool), np.zeros((len(cells), 3))
        e = p - c3
        d2 = np.where(found, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], np.inf)
        better = d2 < best                                              # ascending keys: a tie stays with the smaller key
        second = np.where(better, best, np.minimum(second, d2))
        best = np.where(better, d2, best)
        bkey = np.where(better, key, bkey)
        bc = np.where(better[:, None], c3, bc)
    dist = np.sqrt(best)
    use = dist <= gate
    met = np.isfinite(best)
    gate_m, tie_m = inf.copy().reshape(-1), inf.copy().reshape(-1)
    gate_m[cells] = np.where(met, np.abs(gate - dist), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        tie_m[cells] = np.where(met & np.isfinite(second), (second - best) / np.maximum(best, 1e-300), np.inf)
    margins = {"jump": jump_m, "orient": orient_m, "gate": gate_m.reshape(H, W), "tie": tie_m.reshape(H, W)}
    carried = full.reshape(-1) & nvalid.reshape(-1)                     # (a cell without a normal carries nothing)
    safe = full & (jump_m >= MARGIN) & (orient_m >= MARGIN) & (margins["gate"] >= MARGIN * gate) & (margins["tie"] >= TIE_REL)
    safe &= ~(carried & M.ambiguous(p64)).reshape(H, W)
    cells, p, c, key = cells[use], p[use], bc[use], bkey[use]
    n = ns.reshape(-1, 3)[cells] @ R.T
    r = (n * (p - c)).sum(-1)
    J = np.concatenate([np.cross(c - t, n), n], -1)
    w = np.where(np.abs(r) <= huber, 1.0, huber / np.maximum(np.abs(r), 1e-300))
    JJ = w[:, None, None] * J[:, :, None] * J[:, None, :]
    Jr = w[:, None] * J * r[:, None]
    match = np.full(H * W, -1, np.int64)
    match[cells] = key
    out.update({"A": JJ.sum(0), "b": Jr.sum(0), "cost": float((w * r * r).sum()), "sw": float(w.sum()), "count": int(len(cells)),
                "absA": np.abs(JJ).sum(0), "absb": np.abs(Jr).sum(0), "abscost": float((w * r * r).sum()), "match": match.reshape(H, W),
                "r": r, "J": J, "cell": cells, "safe": safe, "margins": margins})
    return out


def retract(pose7, d):
    """The pose a perturbation d = (omega, v) about the SENSOR's position carries pose7 to: q <- dq(omega) (x) q, t <- t + v."""
    p = np.asarray(pose7, np.float64)
    q = p[:4] / np.linalg.norm(p[:4])
    d = np.asarray(d, np.float64)
    th = np.linalg.norm(d[:3])
    dq = np.concatenate([[math.cos(th / 2)], (math.sin(th / 2) / th if th > 1e-8 else 0.5) * d[:3]])
    nq = P.qmul(dq, q)
    return np.concatenate([nq / np.linalg.norm(nq), p[4:] + d[3:]])


def step(pose7, ev, damping=0.0, min_count=50):
    """The solve: the new pose (7) float64, or None where the image is flagged."""
    if ev["count"] < min_count:
        return None
    Mx = ev["A"] + damping * np.diag(np.diag(ev["A"]))
    try:
        Lc = np.linalg.cholesky(Mx)
    except np.linalg.LinAlgError:
        return None
    d = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, ev["b"]))
    return retract(pose7, d) if np.isfinite(d).all() else None


def iterate(x, pose7, table, voxel, iters, damping=0.0, min_count=50, **kw):
    """The poses after 0 .. iters steps (iters + 1 rows of float64: the kernel keeps doubles between steps).  A flagged step ends the
    list with the input pose repeated."""
    poses = [np.asarray(pose7, np.float64)]
    for _ in range(iters):
        new = step(poses[-1], evaluate(x, poses[-1], table, voxel, **kw), damping, min_count)
        if new is None:
            return poses + [poses[0]] * (iters + 1 - len(poses))
        poses.append(new)
    return poses


def vetted(x, pose7, table, voxel, **kw):
    """(x with every point removed whose decisions at pose7 are not safe, share of the non-empty points removed).  Removing a point
    takes its neighbours' normals away -- an exact decision -- and leaves every other cell's decisions as they were."""
    x = np.array(x, np.float32)
    ev = evaluate(x, pose7, table, voxel, **kw)
    full = x.any(-1)
    drop = full & ~ev["safe"]
    x[drop] = 0.0
    return x, float(drop.sum()) / max(int(full.sum()), 1)


def compose(world, rel):
    """W o T in float64, as world_map.compose."""
    qw, Rw, tw = P.split_pose(world)
    qt, _Rt, tt = P.split_pose(rel)
    q = P.qmul(qw, qt)
    return np.concatenate([q / np.linalg.norm(q), Rw @ tt + tw])


# ---- the cases of tests/test_map_fit_gpu.py, vetted on the CPU by tests/test_map_fit_cpu.py ---------------------------------------
# The synthetic scene at these shapes has its points 0.3 .. 1 m apart at the wall (20 m, 128 or 256 columns): voxels of 2 m hold
# several points each, and a gate of 1 m reaches the centroids from most cells.  jump_rel as pose_fit_reference.FIT.
VOXEL = 2.0
FIT = dict(gate=1.0, huber=0.1, jump_rel=0.2)
SHAPES = ((2, 16, 128, False), (3, 32, 256, True), (1, 8, 64, False), (2, 5, 67, False))      # (B, H, W, last image starved)
LOG2 = 14
SPREAD = 300.0             # metres between the places of a batch's images: one table holds them all
MIN_COUNT = 30            # the (2,5,67) case has three rows of normals: ~50 terms an image


def place(b):
    """The world pose of image b's map scan (frame 2 of the pair): a general rotation (a coordinate that an axis-aligned pose only
    shifts by a round number lands on float32 rounding midpoints: ambiguous points by the hundred), SPREAD metres apart, negative
    and positive coordinates."""
    q = np.array([math.cos(0.15 * b + 0.05), 0.013 * (b + 1), -0.021, math.sin(0.15 * b + 0.05)])
    return np.concatenate([q / np.linalg.norm(q), [SPREAD * b - 250.0 + math.pi / 10, 120.0 - SPREAD * b + math.e / 10, 3.0 * b - 2.0 + math.sqrt(2) / 10]])


@functools.lru_cache(maxsize=None)
def case(i):
    """(map scans (B,H,W,3), map poses (B,7), table, scans (B,H,W,3) vetted, guesses (B,7) float64, [share dropped per image]) of
    SHAPES[i]: the pair of pose_fit_reference.scene -- frame 2 is the map, inserted at place(b); frame 1 is the scan, its guess
    place(b) o (a start pose near the pair's ego-motion)."""
    B, H, W, starved = SHAPES[i]
    f1, f2 = P.scene(B, H, W, starved=starved)
    if starved:                                                         # (the MAP of the starved image stays whole)
        f2 = P.scene(B, H, W, starved=False)[1]
    poses = np.stack([place(b) for b in range(B)])
    f2, _share = M.vetted(f2, poses)
    table = table_of(f2, poses, VOXEL)
    start = P.start_poses(B).astype(np.float64)
    guess = np.stack([compose(poses[b], start[b]) for b in range(B)])
    scans, dropped = np.array(f1, np.float32), []
    for b in range(B):
        scans[b], share = vetted(f1[b], guess[b], table, VOXEL, **FIT)
        dropped.append(share)
    return f2, poses, table, scans, guess, dropped


POLISH_K = 2


@functools.lru_cache(maxsize=None)
def polish_case(b=0):
    """(scan, table, fixed point, start (7) float64, [reference's error to the fixed point after 0 .. POLISH_K steps]) on image b
    of the 32 x 256 case: the fixed point is the reference iterated from the guess until two successive poses are within 1e-7 (or
    60 steps); the start lies 0.1 m and 0.4 degrees off it."""
    _f2, _poses, table, scans, guess, _d = case(1)
    x, fixed = scans[b], guess[b]
    for _ in range(60):
        new = iterate(x, fixed, table, VOXEL, 1, **FIT)[-1]
        done = pose_error(new, fixed) < 1e-7
        fixed = new
        if done:
            break
    start = retract(fixed, np.array([0.0, 0.0, np.deg2rad(0.4), 0.1, 0.0, 0.0]))
    poses = iterate(x, start, table, VOXEL, POLISH_K, **FIT)
    return x, table, fixed, start, [pose_error(p, fixed) for p in poses]


def pose_error(pose7, fixed, lever=20.0):
    """pose_fit_reference.pose_error: |dt| + lever * angle, metres."""
    return P.pose_error(pose7, fixed, lever)


# ---- a small synthetic drive: the same place seen from poses a known motion apart ------------------------------------------------
DRIVE_N, DRIVE_H, DRIVE_W = 5, 32, 256
DRIVE_BIAS = np.array([0.0, 0.0, 0.004, 0.06, 0.03, 0.0])            # planted on every relative pose: yaw and a slide


@functools.lru_cache(maxsize=None)
def drive():
    """(scans (N,H,W,3) float32, true relative poses (N,7), biased relative poses (N,7) float32, true world poses (N,7)): scan n is
    synth.range_image of its ONE scene (the wall and the ground do not depend on the seed; noise and holes do) from the sensor
    position (0.8 n, 0, 0) without rotation -- range_image subtracts `shift` from the scene's points --, so scan n -> scan n-1 is
    the translation (0.8, 0, 0) (scan 0: the identity) and the true world pose of scan n is the translation (0.8 n, 0, 0)."""
    from conftest import load_pkg
    synth = load_pkg("synth")
    stepd = (2.0 + 24.8) / (DRIVE_H - 1)
    gen = load_pkg("sensor").Sensor(fov_up_deg=2.0 + 1.5 * stepd, fov_down_deg=-24.8 + 1.5 * stepd)
    eye = np.array([1.0, 0, 0, 0, 0, 0, 0])
    rel_true = np.stack([eye] + [np.array([1.0, 0, 0, 0, 0.8, 0, 0])] * (DRIVE_N - 1))
    scans = np.stack([synth.range_image(DRIVE_H, DRIVE_W, seed=40 + n, shift=(0.8 * n, 0.0, 0.0), sensor=gen) for n in range(DRIVE_N)])
    biased = np.stack([rel_true[0]] + [retract(r, DRIVE_BIAS) for r in rel_true[1:]]).astype(np.float32)
    worlds = np.stack([np.array([1.0, 0, 0, 0, 0.8 * n, 0, 0]) for n in range(DRIVE_N)])
    return scans.astype(np.float32), rel_true, biased, worlds


def track(scans, rels, voxel=VOXEL, iters=2, **kw):
    """The reference's WorldMap(fit=).add: compose, fit against the map as it stands, insert at the fitted pose (a flagged scan at
    its guess) -> (tracked world poses (N,7), dead-reckoned world poses (N,7))."""
    world = dead = np.array([1.0, 0, 0, 0, 0, 0, 0])
    contents, tracked, reckoned = [], [], []
    for n in range(len(scans)):
        dead = compose(dead, rels[n])
        guess = compose(world, rels[n])
        if contents:
            table = M.merged(contents, voxel)
            poses = iterate(scans[n], guess, table, voxel, iters, **kw)
            world = poses[-1]
        else:
            world = guess
        contents.append(M.content(scans[n][None], world[None], voxel))
        tracked.append(world)
        reckoned.append(dead)
    return np.stack(tracked), np.stack(reckoned)

"""A float64 numpy statement of elo_pose_fit (include/elo.h): the normals of frame 2, both row rules, one evaluation of the
point-to-plane sums at a pose, the Gauss-Newton update and its iteration.  Besides every sum it returns the sum of the absolute
values of its terms (the scale of a float32 summation bound) and, per frame-1 point, the margin of every discrete decision the
evaluation took for it -- so that a test can keep to points whose decisions float32 and float64 cannot take differently:

  border   distance of the projected column / row coordinate to the nearest cell border, in cell widths
  gate     | gate - |p - p2| |, metres
  jump     min over the four neighbours of | |r_nb - r| - jump_rel r | / r   (relative)
  orient   |n . p2| / |p2|   (the cosine that decides which way the normal points)

A margin a point never met (it was dropped before that decision) is +inf."""
import math

import numpy as np

MARGIN = 1e-3          # of each margin's own scale


def constants(H, W, fov_up_deg=2.0, fov_down_deg=-24.8):
    """(az_res, vert_res, vert_off) as the float32 values the kernel is given (sensor.projection_constants, cast by ctypes)."""
    d2r = math.pi / 180
    az = (360.0 / W) * d2r
    down, up = fov_down_deg * d2r, fov_up_deg * d2r
    vres = (up - down) / (H - 1)
    return tuple(float(np.float32(v)) for v in (az, vres, -down / vres))


def rotation(q):
    q0, q1, q2, q3 = q
    return np.array([[1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), 1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 1 - 2 * (q1 * q1 + q2 * q2)]])


def split_pose(pose7):
    p = np.asarray(pose7, np.float64)
    q = p[:4] / np.linalg.norm(p[:4])
    return q, rotation(q), p[4:]


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def normals(x2, jump_rel):
    """(n (H,W,3), valid (H,W), jump margin (H,W), orient margin (H,W)) of a frame-2 image."""
    x = np.asarray(x2, np.float64)
    H, W, _ = x.shape
    full = x.any(-1)
    left, right = np.roll(x, 1, 1), np.roll(x, -1, 1)               # columns wrap: the cylinder's seam
    up, down = np.roll(x, 1, 0), np.roll(x, -1, 0)
    inner = np.zeros((H, W), bool)
    inner[1:H - 1] = True
    have = inner & full & left.any(-1) & right.any(-1) & up.any(-1) & down.any(-1)
    r = np.linalg.norm(x, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        excess = np.stack([np.abs(np.linalg.norm(nb, axis=-1) - r) - jump_rel * r for nb in (left, right, up, down)], 0)
        jump_margin = np.where(have, np.abs(excess).min(0) / r, np.inf)
        smooth = have & (excess <= 0).all(0)
        n = np.cross(right - left, down - up)
        length = np.linalg.norm(n, axis=-1)
        valid = smooth & (length > 0)
        n = n / length[..., None]
        dot = (n * x).sum(-1)
        n = np.where((dot > 0)[..., None], -n, n)                   # towards the sensor: n . x <= 0
        orient_margin = np.where(valid, np.abs(dot) / r, np.inf)
    n[~valid] = 0.0
    return n, valid, jump_margin, orient_margin


def cells(p, H, W, consts, beam_elev=None):
    """(row, col, border margin) of points p (N,3) by the uniform formula, or by the beam table (radians, float32 values)."""
    az_res, vert_res, vert_off = consts
    r = np.linalg.norm(p, axis=-1)
    c = (math.pi - np.arctan2(p[:, 1], p[:, 0])) / az_res
    col = np.clip(np.trunc(c).astype(np.int64), 0, W - 1)
    margin = np.abs(c - np.round(c))
    s = p[:, 2] / r
    if beam_elev is None:
        v = np.arcsin(s) / vert_res + vert_off
        row = np.clip(H - np.trunc(v).astype(np.int64), 0, H - 1)
        margin = np.minimum(margin, np.abs(v - np.round(v)))
    else:
        e = np.asarray(beam_elev, np.float32).astype(np.float64)
        mid = 0.5 * (e[:-1] + e[1:])                                # the row = the number of midpoints above the point
        row = np.clip((np.sin(mid)[None, :] > s[:, None]).sum(1), 0, H - 1)
        spacing = np.abs(np.diff(e)).min()
        margin = np.minimum(margin, np.abs(np.arcsin(s)[:, None] - mid[None, :]).min(1) / spacing)
    return row, col, margin


def evaluate(x1, x2, pose7, consts, gate=1.0, huber=0.1, jump_rel=0.1, beam_elev=None):
    """One evaluation for one image pair.  dict: A (6,6), b (6), cost, sw, count; absA, absb, abscost (sums of |terms|);
    term (H,W) bool: the frame-1 cells that gave a term; safe (H,W) bool: non-empty cells whose every margin is >= MARGIN of its
    scale; margins: dict of (H,W) arrays."""
    x1 = np.asarray(x1, np.float64)
    H, W, _ = x1.shape
    _q, R, t = split_pose(pose7)
    n2, nvalid, jump_m, orient_m = normals(x2, jump_rel)
    x2 = np.asarray(x2, np.float64)
    src = np.flatnonzero(x1.any(-1).reshape(-1))
    p = x1.reshape(-1, 3)[src] @ R.T + t
    row, col, border = cells(p, H, W, consts, beam_elev)
    p2, n = x2[row, col], n2[row, col]
    dist = np.linalg.norm(p - p2, axis=-1)
    met_normal = p2.any(-1)                                          # (an empty p2 ends the decisions; the edge rows have no normal)
    jm = np.where(met_normal, jump_m[row, col], np.inf)
    om = np.where(met_normal, orient_m[row, col], np.inf)
    ok = nvalid[row, col]
    gm = np.where(ok, np.abs(gate - dist), np.inf)
    use = ok & (dist <= gate)
    p, p2, n = p[use], p2[use], n[use]
    r = (n * (p - p2)).sum(-1)
    J = np.concatenate([np.cross(p, n), n], -1)
    w = np.where(np.abs(r) <= huber, 1.0, huber / np.maximum(np.abs(r), 1e-300))
    JJ = w[:, None, None] * J[:, :, None] * J[:, None, :]
    Jr = w[:, None] * J * r[:, None]
    def spread(v, fill):
        out = np.full(H * W, fill, dtype=v.dtype)
        out[src] = v
        return out.reshape(H, W)

    margins = {"border": spread(border, np.inf), "gate": spread(gm, np.inf), "jump": spread(jm, np.inf), "orient": spread(om, np.inf)}
    safe = spread(np.ones(len(src), bool), False)
    for m in margins.values():
        safe &= m >= MARGIN
    return {"A": JJ.sum(0), "b": Jr.sum(0), "cost": float((w * r * r).sum()), "sw": float(w.sum()), "count": int(use.sum()),
            "absA": np.abs(JJ).sum(0), "absb": np.abs(Jr).sum(0), "abscost": float((w * r * r).sum()),
            "term": spread(use, False), "safe": safe, "margins": margins}


def filtered(x1, x2, pose7, consts, **kw):
    """(x1 with every point whose decisions are not safe removed, fraction of the non-empty points removed)."""
    ev = evaluate(x1, x2, pose7, consts, **kw)
    full = np.asarray(x1).any(-1)
    drop = full & ~ev["safe"]
    out = np.array(x1, copy=True)
    out[drop] = 0.0
    return out, drop.sum() / max(full.sum(), 1)


def step(pose7, ev, damping=0.0, min_count=50):
    """The solve: (new pose (7) float64 or None where the image is flagged)."""
    if ev["count"] < min_count:
        return None
    M = ev["A"] + damping * np.diag(np.diag(ev["A"]))
    try:
        Lc = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None
    d = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, ev["b"]))
    q, _R, t = split_pose(pose7)
    th = np.linalg.norm(d[:3])
    dq = np.concatenate([[math.cos(th / 2)], (math.sin(th / 2) / th if th > 1e-8 else 0.5) * d[:3]])
    nq = qmul(dq, q)
    return np.concatenate([nq / np.linalg.norm(nq), rotation(dq) @ t + d[3:]])


def iterate(x1, x2, pose7, consts, iters, damping=0.0, min_count=50, as_float32=True, **kw):
    """The poses after 0 .. iters steps (a list of iters + 1 rows).  as_float32: the pose is stored in float32 between the steps,
    as the kernel stores it.  A flagged step ends the list with the input pose repeated."""
    poses = [np.asarray(pose7, np.float64)]
    for _ in range(iters):
        new = step(poses[-1], evaluate(x1, x2, poses[-1], consts, **kw), damping, min_count)
        if new is None:
            return poses + [poses[0]] * (iters + 1 - len(poses))
        poses.append(new.astype(np.float32).astype(np.float64) if as_float32 else new)
    return poses


def pose_error(pose7, fixed, lever=20.0):
    """One number for how far a pose is from another: |dt| + lever * angle, metres -- the displacement of a point at `lever`
    metres (the range of the synthetic scene's wall), so that rotation and translation errors are counted in one unit."""
    qa, _Ra, ta = split_pose(pose7)
    qb, _Rb, tb = split_pose(fixed)
    ang = 2.0 * math.acos(min(1.0, abs(float(qa @ qb))))
    return float(np.linalg.norm(ta - tb)) + lever * ang


def scene(B, H, W, seed=4, starved=False, fov_up_deg=2.0, fov_down_deg=-24.8, **kw):
    """synth.frame_pair for a pose fit: the two (B,H,W,3) float32 images of a sensor whose beam h looks through the MIDDLE of row h
    of the projection at (fov_up_deg, fov_down_deg) -- the uniform row formula row = H - int(beta / vert_res + vert_off) puts its
    borders exactly at evenly spread beams, where rounding alone would decide a point's row; a real image holds in cell (h,w) a
    point that projects into (h,w), and so do these.  Row h of the formula is centred at fov_up + (1.5 - h) rows."""
    from conftest import load_pkg
    step = (fov_up_deg - fov_down_deg) / (H - 1)
    gen = load_pkg("sensor").Sensor(fov_up_deg=fov_up_deg + 1.5 * step, fov_down_deg=fov_down_deg + 1.5 * step)
    return load_pkg("synth").frame_pair(B, H, W, seed=seed, starved=starved, sensor=gen, **kw)


GUESS = np.array([math.cos(0.005), 0.0, 0.0, -math.sin(0.005), -0.8, 0.0, 0.0], np.float32)    # frame_pair's ego-motion, roughly


def retract(pose7, d):
    """The pose a left perturbation d = (omega, v) carries pose7 to -- step()'s update: q <- dq(omega) (x) q, t <- R(dq) t + v."""
    q, _R, t = split_pose(pose7)
    th = np.linalg.norm(d[:3])
    dq = np.concatenate([[math.cos(th / 2)], (math.sin(th / 2) / th if th > 1e-8 else 0.5) * np.asarray(d[:3], np.float64)])
    nq = qmul(dq, q)
    return np.concatenate([nq / np.linalg.norm(nq), rotation(dq) @ t + np.asarray(d[3:], np.float64)])


# ---- the scenes of tests/test_pose_fit_gpu.py, checked on the CPU by tests/test_pose_fit_cpu.py ---------------------------------
# jump_rel = 0.2: the synthetic ground is a family of rings whose range ratio from row to row is the same all the way round, and
# at these row spacings one ring pair sits within the noise of 0.1 -- a whole row of normals on the threshold, more than the 2 %
# the filter may drop.  0.2 is clear of every ring pair at all three shapes.
FIT = dict(gate=1.0, huber=0.1, jump_rel=0.2)
SHAPES = ((2, 16, 128, False), (3, 32, 256, True), (1, 8, 64, False))      # (B, H, W, last image starved to a 2 x 3 patch)
DROP_CAP = 0.02


def start_poses(B):
    """One pose per image near frame_pair's ego-motion, each a little different (float32 rows)."""
    out = np.tile(GUESS, (B, 1)).astype(np.float64)
    for b in range(B):
        out[b] = retract(out[b], 0.002 * np.array([b + 1, -b, 0.5 * b, 3 * b, -2.0 * b, b + 1.0]))
    return out.astype(np.float32)


def filtered_case(B, H, W, starved, beam_deg=None):
    """(x1 filtered, x2, poses (B,7) float32, consts, beam table in radians or None, [fraction dropped per image]) of one GPU case:
    scene() -- or, with a beam table (degrees), frame_pair of that sensor: its beams sit mid-row by the table's own rule -- with
    every frame-1 point removed whose decisions at its pose are not safe."""
    if beam_deg is None:
        f1, f2 = scene(B, H, W, starved=starved)
        beam = None
    else:
        from conftest import load_pkg
        f1, f2 = load_pkg("synth").frame_pair(B, H, W, seed=4, starved=starved, sensor=load_pkg("sensor").Sensor(beam_elevations_deg=beam_deg))
        beam = (np.asarray(beam_deg, np.float64) * (math.pi / 180)).astype(np.float32)
    consts = constants(H, W) if beam_deg is None else constants(H, W, beam_deg[0], beam_deg[-1])
    poses = start_poses(B)
    x1, dropped = np.array(f1, copy=True), []
    for b in range(B):
        x1[b], frac = filtered(f1[b], f2[b], poses[b], consts, beam_elev=beam, **FIT)
        dropped.append(float(frac))
    return x1, f2, poses, consts, beam, dropped


BEAMS_DEG = tuple(float(v) for v in 2.0 - 26.8 * (np.arange(16) / 15.0) ** 1.3)      # 16 unevenly spread beams, +2 .. -24.8 degrees

POLISH_K = 2


def polish_case(b=0, H=32, W=256):
    """(fixed point, start (7) float32, [reference's error to the fixed point after 0 .. POLISH_K steps]) of image b of the
    32 x 256 scene: the fixed point is the reference iterated from GUESS until two successive poses are within 1e-6 (or 40 steps);
    the start lies 0.1 m and 0.76 degrees off it."""
    f1, f2 = scene(3, H, W)
    c = constants(H, W)
    fixed = np.asarray(GUESS, np.float64)
    for _ in range(40):
        new = iterate(f1[b], f2[b], fixed, c, 1, **FIT)[-1]
        done = pose_error(new, fixed) < 1e-6
        fixed = new
        if done:
            break
    ang = np.deg2rad(0.76)
    start = np.concatenate([qmul(np.array([math.cos(ang / 2), 0, 0, math.sin(ang / 2)]), fixed[:4]), fixed[4:] + [0.1, 0, 0]]).astype(np.float32)
    poses = iterate(f1[b], f2[b], start, c, POLISH_K, **FIT)
    return fixed, start, [pose_error(p, fixed) for p in poses]

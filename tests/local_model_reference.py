"""A float64 numpy statement of elo_model_render (include/elo.h): K range images, each carried by its pose into one frame, rendered
into one range image by nearest range.  Per target cell it returns the winner and whether the cell is AMBIGUOUS -- a cell on
which float32 and float64 may decide differently, so that a test keeps to the others:

  border   a contributing point lies within MARGIN (in cell widths) of a cell border: the cell it is in AND the cell across that
           border are marked (both, where it is near a row and a column border: the diagonal one too);
  range    the best two ranges of the cell differ by less than RANGE_REL relative without having the same float32 bits (the same
           bits are no ambiguity: the lower source index wins, by the rule).

Also the static BOX scene of the tracker tests: ground and four walls ray-cast from a moving sensor, beams mid-row, half of the
cells empty, independently per scan."""
import functools
import math

import numpy as np

import pose_fit_reference as R

MARGIN = R.MARGIN      # 1e-3 of a cell
RANGE_REL = 1e-5
DROP_CAP = 0.02


def carry(points, pose7):
    """R(q) p + t in float64, q normalised, summed in the kernel's order -> (N,3); None where the quaternion has no direction."""
    p = np.asarray(pose7, np.float64)
    n = np.linalg.norm(p[:4])
    if not (n > 0 and np.isfinite(n)):
        return None
    _q, Rm, t = R.split_pose(p)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([Rm[i, 0] * x + Rm[i, 1] * y + Rm[i, 2] * z + t[i] for i in range(3)], -1)


def _other_cells(p, row, col, H, W, consts, beam_elev):
    """Per point: (near a column border, the column across it, near a row border, the row across it)."""
    az_res, vert_res, vert_off = consts
    c = (math.pi - np.arctan2(p[:, 1], p[:, 0])) / az_res
    near_c = np.abs(c - np.round(c)) < MARGIN
    other_c = np.mod((2 * np.round(c) - 1 - np.trunc(c)).astype(np.int64), W)              # the seam: columns 0 and W-1 are neighbours
    s = p[:, 2] / np.linalg.norm(p, axis=-1)
    if beam_elev is None:
        v = np.arcsin(s) / vert_res + vert_off
        near_r = np.abs(v - np.round(v)) < MARGIN
        other_r = np.clip(H - (2 * np.round(v) - 1 - np.trunc(v)).astype(np.int64), 0, H - 1)
    else:
        e = np.asarray(beam_elev, np.float32).astype(np.float64)
        mid = 0.5 * (e[:-1] + e[1:])
        d = np.abs(np.arcsin(s)[:, None] - mid[None, :])
        j = d.argmin(1)                                                                    # midpoint j parts rows j and j + 1
        near_r = d.min(1) / np.abs(np.diff(e)).min() < MARGIN
        other_r = np.clip(np.where(row == j + 1, j, j + 1), 0, H - 1)
    return near_c, other_c, near_r, other_r


def render(src, pose, consts, beam_elev=None):
    """One batch element: src (K,H,W,3) float32, pose (K,7) float32 -> dict: src_idx (H,W) int64 (the winner's (k*H + h)*W + w, -1:
    empty), xyz (H,W,3) float64 (the winner's unrounded p', zeros where empty), ambiguous (H,W) bool, points (how many points
    contributed)."""
    src = np.asarray(src, np.float32)
    K, H, W, _ = src.shape
    cells = H * W
    idx_l, p_l = [], []
    for k in range(K):
        pts = src[k].reshape(-1, 3)
        full = np.flatnonzero((pts != 0).any(-1))
        p = carry(pts[full].astype(np.float64), pose[k])
        if p is None:
            continue
        idx_l.append(k * cells + full)
        p_l.append(p)
    idx = np.concatenate(idx_l) if idx_l else np.zeros(0, np.int64)
    p = np.concatenate(p_l) if p_l else np.zeros((0, 3))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p32 = p.astype(np.float32)
        rf = np.sqrt(p32[:, 0] * p32[:, 0] + p32[:, 1] * p32[:, 1] + p32[:, 2] * p32[:, 2])   # float32, the kernel's sequence
        keep = np.isfinite(p32).all(-1) & (p32 != 0).any(-1) & (rf > 0) & np.isfinite(rf)
    idx, p, rf = idx[keep], p[keep], rf[keep]
    out_idx = np.full(cells, -1, np.int64)
    out_xyz = np.zeros((cells, 3))
    amb = np.zeros((H, W), bool)
    if len(idx):
        row, col, _m = R.cells(p, H, W, consts, beam_elev)
        near_c, other_c, near_r, other_r = _other_cells(p, row, col, H, W, consts, beam_elev)
        amb[row[near_c | near_r], col[near_c | near_r]] = True
        amb[row[near_c], other_c[near_c]] = True
        amb[other_r[near_r], col[near_r]] = True
        both = near_c & near_r
        amb[other_r[both], other_c[both]] = True
        cell = row * W + col
        order = np.lexsort((idx, rf, cell))                       # by cell, then range bits (rf > 0: its value orders them), then index
        cs, rs = cell[order], rf[order].astype(np.float64)
        first = np.ones(len(order), bool)
        first[1:] = cs[1:] != cs[:-1]
        win = order[first]
        out_idx[cell[win]] = idx[win]
        out_xyz[cell[win]] = p[win]
        second = np.flatnonzero(~first & np.concatenate([[False], first[:-1]]))             # the runner-up of its cell
        r64 = np.linalg.norm(p, axis=-1)[order]
        close = (np.abs(r64[second] - r64[second - 1]) < RANGE_REL * r64[second]) & (rs[second] != rs[second - 1])
        amb.reshape(-1)[cs[second[close]]] = True
    return {"src_idx": out_idx.reshape(H, W), "xyz": out_xyz.reshape(H, W, 3), "ambiguous": amb, "points": int(len(idx))}


def ulp_of_largest(xyz64):
    """(..., 1) float64: one float32 ulp at the largest component of each point (the bound on a component of the kernel's p')."""
    big = np.abs(xyz64).max(-1, keepdims=True).astype(np.float32)
    return np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64)


# ---- the render cases of tests/test_local_model_gpu.py, vetted on the CPU by tests/test_local_model_cpu.py -----------------------
CASES = ((2, 3, 16, 128, False), (1, 1, 8, 64, False), (1, 5, 32, 256, False), (2, 3, 16, 128, True))   # (B, K, H, W, beam table)


def yaw_pose(angle, t):
    return np.array([math.cos(angle / 2), 0.0, 0.0, math.sin(angle / 2), t[0], t[1], t[2]])


def render_case(i):
    """(src (B,K,H,W,3) float32, pose (B,K,7) float32, consts, beam table (radians, float32) or None) of case i: render_inputs at
    CASES[i], with pose_fit_reference.BEAMS_DEG where the case has a beam table."""
    B, K, H, W, beams = CASES[i]
    return render_inputs(B, K, H, W, R.BEAMS_DEG if beams else None, i)


def render_inputs(B, K, H, W, beam_deg, i):
    """(src (B,K,H,W,3) float32, pose (B,K,7) float32, consts, beam table (radians, float32) or None); i numbers the draw: every
    source an R.scene image (with beam_deg, a table in degrees: a frame of that beam-table sensor) of its own seed, carried by a
    small motion (<= 1 m, <= 3 degrees, about a tilted axis); the LAST source of every batch element is turned by about 180
    degrees, so its points cross the seam.
    The sources are SPARSE, about 1.5 / K of their cells filled (the scans a local model is for): every contributing point within
    MARGIN of a border marks two cells, 4 MARGIN of the points are that near, so the ambiguous share is about 0.8 % per point that
    reaches a cell -- 1.5 points per cell keep it under DROP_CAP, and still most filled cells are contested by two sources."""
    from conftest import load_pkg
    holes = max(0.05, 1.0 - 1.5 / K)
    rng = np.random.default_rng(100 + i)
    src = np.zeros((B, K, H, W, 3), np.float32)
    pose = np.zeros((B, K, 7), np.float32)
    for b in range(B):
        for k in range(K):
            seed = 7 + 10 * i + 2 * (b * K + k)
            if beam_deg is not None:
                f1, _f2 = load_pkg("synth").frame_pair(1, H, W, seed=seed, hole_rate=holes,
                                                       sensor=load_pkg("sensor").Sensor(beam_elevations_deg=beam_deg))
            else:
                f1, _f2 = R.scene(1, H, W, seed=seed, hole_rate=holes)
            src[b, k] = f1[0]
            axis = rng.normal(size=3) * (0.2, 0.2, 1.0)
            axis /= np.linalg.norm(axis)
            ang = np.deg2rad(rng.uniform(-3.0, 3.0))
            t = rng.uniform(-1.0, 1.0, 3) * (0.55, 0.55, 0.1)
            q = np.concatenate([[math.cos(ang / 2)], math.sin(ang / 2) * axis])
            if k == K - 1 and K > 1:
                q = R.qmul(yaw_pose(math.pi - 0.01 * (b + 1), (0, 0, 0))[:4], q)
            pose[b, k] = np.concatenate([q * rng.uniform(0.5, 2.0), t])         # (the kernel normalises q)
    if beam_deg is None:
        return src, pose, R.constants(H, W), None
    return src, pose, R.constants(H, W, beam_deg[0], beam_deg[-1]), (np.asarray(beam_deg, np.float64) * (math.pi / 180)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rendered_case(i):
    """render_case(i) and the reference's render of each of its batch elements, computed once per process."""
    src, pose, consts, beam = render_case(i)
    return src, pose, consts, beam, [render(src[b], pose[b], consts, beam) for b in range(len(src))]


# ---- the box scene ---------------------------------------------------------------------------------------------------------------
BOX_H, BOX_W, BOX_SCANS = 16, 128, 6
BOX_STEP = (0.8, 0.01)                       # metres forward and radians of yaw per scan
GROUND_Z, WALL_X, WALL_Y = -1.73, 20.0, 15.0


def box_world_pose(i):
    """[q | t] of scan i's sensor in the world: it drives along x and turns about z."""
    return yaw_pose(BOX_STEP[1] * i, (BOX_STEP[0] * i, 0.0, 0.0))


def box_scan(i, H=BOX_H, W=BOX_W, hole_rate=0.5, seed=900):
    """(H,W,3) float32: scan i of the box -- the ground z = -1.73 and the walls x = +-20, y = +-15, ray-cast from box_world_pose(i)
    by beams through the MIDDLE of every row and column of the projection (R.scene's placement); each cell is empty with
    probability hole_rate, independently per scan."""
    _q, Rw, tw = R.split_pose(box_world_pose(i))
    step = 26.8 / (H - 1)
    el = np.deg2rad(2.0 + 1.5 * step - np.arange(H) * step)[:, None] * np.ones((1, W))
    az = (math.pi - (np.arange(W) + 0.5) * (2 * math.pi / W))[None, :] * np.ones((H, 1))
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    dw = d @ Rw.T
    best = np.full((H, W), np.inf)
    for axis, value in ((2, GROUND_Z), (0, WALL_X), (0, -WALL_X), (1, WALL_Y), (1, -WALL_Y)):
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (value - tw[axis]) / dw[..., axis]
        best = np.where((s > 0) & (s < best), s, best)
    img = d * best[..., None]
    img[np.random.default_rng(seed + i).random((H, W)) < hole_rate] = 0.0
    return img.astype(np.float32)


def relative_pose(a, b):
    """[q | t] float64 carrying the frame of world pose a into the frame of world pose b: p_b = R p_a + t."""
    qa, Ra, ta = R.split_pose(a)
    qb, Rb, tb = R.split_pose(b)
    q = R.qmul(qb * (1, -1, -1, -1), qa)
    return np.concatenate([q / np.linalg.norm(q), Rb.T @ (ta - tb)])


def box_pairs():
    """[(xyz1, xyz2, pose7 float32)] of the drive: pair n = (scan n, scan n-1) and the true pose from frame 1 to frame 2 rounded to
    float32, n = 1 .. BOX_SCANS - 1."""
    scans = [box_scan(i) for i in range(BOX_SCANS)]
    return [(scans[n], scans[n - 1], relative_pose(box_world_pose(n), box_world_pose(n - 1)).astype(np.float32))
            for n in range(1, BOX_SCANS)]


def rebase(poses64, T):
    """numpy float64: every row P_j becomes T^-1 o P_j (local_model.rebase's statement)."""
    q, Rm, t = R.split_pose(T)
    out = np.array(poses64, np.float64)
    for j in range(len(out)):
        qj = out[j, :4] / np.linalg.norm(out[j, :4])
        qn = R.qmul(q * (1, -1, -1, -1), qj)
        out[j] = np.concatenate([qn / np.linalg.norm(qn), Rm.T @ (out[j, 4:] - t)])
    return out


def track_counts(pairs, scans, consts):
    """The reference's tracker at the pairs' own poses (no polish): per step (terms of the fit against the model, scans held,
    share of ambiguous cells of the render)."""
    H, W, _ = pairs[0][0].shape
    ring = np.zeros((scans, H, W, 3), np.float32)
    poses = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (scans, 1))
    entered, out = 0, []

    def enter(x):
        nonlocal entered
        ring[entered % scans] = x
        poses[entered % scans] = (1.0, 0, 0, 0, 0, 0, 0)
        entered += 1

    for x1, x2, pose7 in pairs:
        if entered == 0:
            enter(x2)
        got = render(ring, poses.astype(np.float32), consts)
        ev = R.evaluate(x1, got["xyz"], pose7, consts, **R.FIT)
        out.append((ev["count"], min(entered, scans), float(got["ambiguous"].mean())))
        poses[:] = rebase(poses, pose7)
        enter(x1)
    return out

"""float64 restatement of elo_input_stage_deskew (include/elo.h) for tests/test_deskew_gpu.py: the correction
    a = s - phase_ref;   p' = Rot(u, a theta) p + a t
its inverse (which the tests use to BUILD a raw cloud from the de-skewed cloud they want), the input stage's point half and its
projection -- winner of minimum range per cell, duplicates summed, zero points blanking their cell -- and the scene generators."""
import math

import numpy as np

D2R = math.pi / 180
TABLE8 = (1.5, -0.5, -2.5, -4.5, -9.5, -14.0, -19.0, -23.5)            # two blocks: 2 degree and ~4.5-5 degree spacing
TABLE128 = tuple([10.0 - 0.3 * i for i in range(64)] + [-9.2 - 0.5 * i for i in range(64)])      # 0.3 and 0.5 degree blocks, H > 64


def rotation(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def inverse_row(row):
    """The row of the inverse rigid transform, (q^-1, -R(q)^T t), float64."""
    row = np.asarray(row, np.float64)
    q = row[:4] / np.linalg.norm(row[:4])
    return np.concatenate([q * (1, -1, -1, -1), -(rotation(q).T @ row[4:])])


def axis_angle(row, invert=False):
    """(u, theta, t) of a motion row as the entry defines them: q normalised, negated where q0 < 0, the transform inverted first
    where `invert`."""
    row = inverse_row(row) if invert else np.asarray(row, np.float64)
    q = row[:4] / np.linalg.norm(row[:4])
    if q[0] < 0:
        q = -q
    vn = np.linalg.norm(q[1:])
    return (q[1:] / vn if vn > 0 else np.zeros(3)), 2 * math.atan2(vn, q[0]), row[4:].copy()


def _rot(u, ang, p):
    """Rodrigues: rotation of the rows of p (M,3) about the unit vector u by ang (M)."""
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    return p * c + np.cross(u[None, :], p) * s + u[None, :] * (p @ u)[:, None] * (1 - c)


def deskew(p, s, row, phase_ref, invert=False):
    """p (M,3), s (M) float64 -> p' (M,3); zero points are left alone."""
    u, theta, t = axis_angle(row, invert)
    a = s - phase_ref
    out = _rot(u, a * theta, p) + a[:, None] * t[None, :]
    zero = (p == 0).all(-1)
    out[zero] = p[zero]
    return out


def skew(target, s, row, phase_ref):
    """The raw points whose correction is `target`: p = Rot(u, -a theta) (p' - a t)."""
    u, theta, t = axis_angle(row)
    a = s - phase_ref
    return _rot(u, -a * theta, target - a[:, None] * t[None, :])


def azimuth_phase(p):
    return (np.pi - np.arctan2(p[:, 1], p[:, 0])) / (2 * np.pi)


def point_half(p, crop, T=None):
    """The input stage's point half in float64 on de-skewed points: crop, optional (4,4) T_trans, validity re-mask."""
    valid = (p != 0).any(-1)
    p4 = np.concatenate([p, np.ones((len(p), 1))], 1)
    p4[np.hypot(p[:, 0], p[:, 1]) > crop] = 0
    if T is not None:
        p4 = p4 @ np.asarray(T, np.float64).T
    return p4[:, :3] * valid[:, None]


def zero_cell(H, W, az_res):
    """The cell of a (+0, +0, +0) point: row H-1, column int((pi - atan2(+0, +0)) / az_res) as the kernels evaluate it, in fp32."""
    return (H - 1) * W + min(int(np.float32(np.pi) / np.float32(az_res)), W - 1)


def zero_cells(pts, H, W, az_res):
    """The cells the zero points among pts (M,3) fall in: row H-1 (by the formula's NaN -> 0 conversion, and by the beam table's
    clamp), the column by atan2 of their signed zeros -- +-0: zero_cell's; pi (x = -0, y = +0): column 0; -pi: column W-1."""
    dead = pts[(pts == 0).all(-1)]
    at = np.arctan2(dead[:, 1], dead[:, 0])
    col = np.where(at > 1.0, 0, np.where(at < -1.0, W - 1, zero_cell(H, W, az_res) - (H - 1) * W))
    return np.unique((H - 1) * W + col)


def project(pts, H, W, az_res, row_of):
    """float64 (M,3) points of ONE image -> (image (H,W,3) = the sum of the points of minimum range per cell, how many were summed
    (H,W)).  Zero points win their cell (zero_cells: by their signs) and blank it."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    r = np.sqrt(x * x + y * y + z * z)
    live = r > 0
    col = np.clip(np.trunc((np.pi - np.arctan2(y, x)) / az_res), 0, W - 1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        row = np.clip(row_of(np.arcsin(z / r)), 0, H - 1).astype(np.int64)
    cell = row * W + col
    best = np.full(H * W, np.inf)
    np.minimum.at(best, cell[live], r[live])
    win = live & (r == best[cell])
    img, count = np.zeros((H * W, 3)), np.zeros(H * W, np.int64)
    np.add.at(img, cell[win], pts[win])
    np.add.at(count, cell[win], 1)
    if not live.all():
        blank = zero_cells(pts, H, W, az_res)
        img[blank], count[blank] = 0.0, 0
    return img.reshape(H, W, 3), count.reshape(H, W)


def formula_rows(H, vres, voff):
    return lambda beta: H - np.trunc(beta / vres + voff)


def nearest_beam(table_rad):
    mids = 0.5 * (np.asarray(table_rad, np.float64)[:-1] + np.asarray(table_rad, np.float64)[1:])
    return lambda beta: (beta[:, None] < mids[None, :]).sum(1)         # the number of midpoints above beta


def xyz(beta, az, r):
    return np.stack([r * np.cos(beta) * np.cos(az), r * np.cos(beta) * np.sin(az), r * np.sin(beta)], -1)


def target_cloud(rng, B, N, H, W, consts, table_deg=None):
    """(B, 2N, 3) float64, the cloud the de-skewed scan should BE: every point 0.3 cells or more from every cell border (formula
    rows at `consts`) or within 0.1 degree of a beam of `table_deg`, ranges distinct on a 5 mm grid within an image, nobody within
    0.5 m of the 35 m crop (which bites)."""
    az_res, vres, voff = consts
    az = np.pi - (rng.integers(0, W, (B, 2 * N)) + rng.uniform(0.3, 0.7, (B, 2 * N))) * az_res
    if table_deg is None:
        beta = (rng.integers(1, H, (B, 2 * N)) + rng.uniform(0.3, 0.7, (B, 2 * N)) - voff) * vres
    else:
        beta = (np.asarray(table_deg)[rng.integers(0, H, (B, 2 * N))] + rng.uniform(-0.1, 0.1, (B, 2 * N))) * D2R
    if B * 2 * N <= 16000:                                              # 3 .. 63 m over the whole batch
        r = 3.0 + 0.005 * rng.permutation(B * 2 * N).reshape(B, 2 * N)
    else:                                                               # 3 .. 3 + N / 200 m in every image
        r = 3.0 + 0.005 * np.stack([np.concatenate([rng.permutation(N), rng.permutation(N)]) for _ in range(B)])
    r = np.where(np.abs(r * np.cos(beta) - 35.0) < 0.5, r + 2.0025, r)
    return xyz(beta, az, r)


def motion_row(rng, q0_negative=False, scale=1.0):
    """[q | t]: 5 .. 15 degrees about a random axis, 1 .. 3 m in a random direction; `scale`: q is not normalised."""
    axis, direction = rng.normal(size=3), rng.normal(size=3)
    half = 0.5 * rng.uniform(5.0, 15.0) * D2R
    q = np.concatenate([[math.cos(half)], math.sin(half) * axis / np.linalg.norm(axis)]) * scale
    return np.concatenate([-q if q0_negative else q, rng.uniform(1.0, 3.0) * direction / np.linalg.norm(direction)]).astype(np.float32)


def raw_scan(rng, target, motion, motion2, phase_ref):
    """The fp32 stride-4 raw cloud (B, 2N, 4) -- phase in channel 3 -- whose correction is `target`, with exact duplicates inside
    every frame (made in `target` too, in place) and 5 % zero padding."""
    B, N2, _ = target.shape
    N = N2 // 2
    cloud = np.zeros((B, N2, 4), np.float32)
    cloud[..., 3] = rng.uniform(0.0, 1.0, (B, N2))
    for b in range(B):
        for f in range(2):
            sl = slice(f * N, (f + 1) * N)
            row = (motion2 if f and motion2 is not None else motion)[b]
            cloud[b, sl, :3] = skew(target[b, sl], cloud[b, sl, 3].astype(np.float64), row, phase_ref)
            src, dst = rng.integers(0, N, N // 20) + f * N, rng.integers(0, N, N // 20) + f * N
            cloud[b, dst], target[b, dst] = cloud[b, src], target[b, src]          # point and phase: summed
    cloud[rng.random((B, N2)) < 0.05, :3] = 0.0
    return cloud


def raw_scan_azimuth(rng, target, motion, phase_ref):
    """The fp32 raw cloud (B, 2N, 3) of a sensor whose phase IS its azimuth: p = skew(target, s) with s = azimuth_phase(p), by
    fixed-point iteration (a contraction wherever the motion is small against the range); the few points it does not settle for --
    near the seam of the sweep -- become zero padding, as do 5 % of the others; exact duplicates (made in `target` too, in place)."""
    B, N2, _ = target.shape
    N = N2 // 2
    cloud = np.zeros((B, N2, 3), np.float32)
    for b in range(B):
        tgt = target[b]
        s = azimuth_phase(tgt)
        for _ in range(60):
            raw = skew(tgt, s, motion[b], phase_ref)
            s_next = azimuth_phase(raw)
            settled = np.abs(s_next - s) < 1e-13
            s = s_next
        raw[~settled] = 0.0
        assert settled.mean() > 0.9
        cloud[b] = raw
        for f in range(2):
            src, dst = rng.integers(0, N, N // 20) + f * N, rng.integers(0, N, N // 20) + f * N
            cloud[b, dst], target[b, dst] = cloud[b, src], target[b, src]
    cloud[rng.random((B, N2)) < 0.05] = 0.0
    return cloud


def stack_frames(x):
    """(B, 2N, ...) by batch element -> (2B, N, ...) stacked as the entry's outputs are: frame 1 of every element first."""
    N = x.shape[1] // 2
    return np.concatenate([x[:, :N], x[:, N:]], 0)


def restack(points, B):
    """The entry's stacked (2B,N,3) `points` as a (B,2N,3) cloud."""
    return np.concatenate([points[:B], points[B:]], 1)

"""The pose tail's operators in float64 numpy, on the inputs AS STORED (an fp16 tensor converts to float64 exactly, so fp16 storage
has no error of its own here): the masked softmax-weighted mean over the valid points with its (maximum, denominator) statistics
(model_util.py:319-343), the pose head's two linear layers, normalise_q with its two 1e-10 terms (pwclo_model.py:203), the composition
with the coarse pose (pwclo_model.py:262-280 as csrc/elo_features.hip pose_head_kernel cites it), the warp (pwclo_model.py:213-227) and
the projection's cell rule and winner rule (model_util.py:229-273).  tests/test_pose_tail_cpu.py pins the pooled vector to
oracle/ops_np.py: softmax_valid at one shape."""
import numpy as np

D = np.float64
EPS = D(np.float32(1e-10))                               # the kernels' 1e-10f


def valid(xyz):
    """(B,N) bool: a point is valid unless all three components are zero (-0.0 == 0.0)."""
    return ~np.all(np.asarray(xyz) == 0, -1)


def softmax_valid(feature, weight, xyz):
    """pooled (B,C), stats (B,2,C) = [maximum | denominator] of the masked softmax; no valid point: pooled 0, maximum -inf, denominator 0."""
    f, w, ok = np.asarray(feature, D), np.asarray(weight, D), valid(xyz)
    B, N, C = f.shape
    pooled, stats = np.zeros((B, C), D), np.zeros((B, 2, C), D)
    for b in range(B):
        if not ok[b].any():
            stats[b, 0] = -np.inf
            continue
        l, v = w[b][ok[b]], f[b][ok[b]]
        m = l.max(0)
        e = np.exp(l - m)
        stats[b, 0], stats[b, 1] = m, e.sum(0)
        pooled[b] = (e * v).sum(0) / e.sum(0)
    return pooled, stats


def merge_triples(mx, den, acc):
    """pooled (B,C) of (B,parts,C) partial sums (maximum, denominator, weighted sum); slices with denominator 0 do not count."""
    mx, den, acc = (np.asarray(x, D) for x in (mx, den, acc))
    live = den != 0
    m = np.where(live, mx, -np.inf).max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        sc = np.where(live, np.exp(np.where(live, mx - m, 0.0)), 0.0)
    dd, aa = (den * sc).sum(1), (np.where(live, acc, 0.0) * sc).sum(1)
    return np.where(dd > 0, aa / np.where(dd > 0, dd, 1.0), 0.0)


def head(pooled, W_big, b_big, W_q, b_q, W_t, b_t):
    """raw (B,7) = [q_raw | t_det] and big (B,hidden): two linear layers, no activation (pwclo_model.py:197-201)."""
    big = np.asarray(pooled, D) @ np.asarray(W_big, D) + np.asarray(b_big, D)
    raw = np.concatenate([big @ np.asarray(W_q, D) + np.asarray(b_q, D), big @ np.asarray(W_t, D) + np.asarray(b_t, D)], -1)
    return raw, big


def normalise_q(q):
    return q / (np.sqrt((q * q).sum(-1, keepdims=True) + EPS) + EPS)


def hamilton(a, b):
    r0 = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    r1 = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    r2 = a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1]
    r3 = a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]
    return np.stack([r0, r1, r2, r3], -1)


def inv_q(q):
    return np.concatenate([q[..., :1], -q[..., 1:]], -1) / ((q * q).sum(-1, keepdims=True) + EPS)


def compose(raw, q_coarse=None, t_coarse=None):
    """(q (B,4), t (B,3), q_norm (B,4)) from the head's raw (B,7) and the coarse pose (None at the coarsest level)."""
    raw = np.asarray(raw, D)
    q_det, t_det = normalise_q(raw[:, :4]), raw[:, 4:]
    if q_coarse is None:
        q, t = q_det, t_det
    else:
        qc, tc = np.asarray(q_coarse, D).reshape(-1, 4), np.asarray(t_coarse, D).reshape(-1, 3)
        tq = np.concatenate([np.zeros((len(tc), 1)), tc], -1)
        q = hamilton(q_det, qc)
        t = hamilton(hamilton(q_det, tq), inv_q(q_det))[:, 1:] + t_det
    return q, t, normalise_q(q)


def pose(feature, weight, xyz, W_big, b_big, W_q, b_q, W_t, b_t, q_coarse=None, t_coarse=None):
    pooled, _ = softmax_valid(feature, weight, xyz)
    return compose(head(pooled, W_big, b_big, W_q, b_q, W_t, b_t)[0], q_coarse, t_coarse)


def warp(xyz, q, t):
    """(B,N,3): p' = (q (x) [0,p] (x) q^-1)[1:] + t for valid points, 0 for the others."""
    p = np.asarray(xyz, D)
    q, t = np.asarray(q, D).reshape(-1, 1, 4), np.asarray(t, D).reshape(-1, 1, 3)
    pq = np.concatenate([np.zeros(p.shape[:2] + (1,)), p], -1)
    w = hamilton(hamilton(q, pq), inv_q(q))[..., 1:] + t
    return w * valid(xyz)[..., None]


def warp32(xyz, q, t):
    """The warp in float32, operation by operation in warp_cell_point's order (no contraction): where the RESULT'S BITS are the
    statement -- a valid point the pose maps exactly onto the origin, which float64 puts 1e-10 beside it (the 1e-10 of the inverse)."""
    F = np.float32
    p, q, t = np.asarray(xyz, F), np.asarray(q, F).reshape(-1, 1, 4), np.asarray(t, F).reshape(-1, 1, 3)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    q0, q1, q2, q3 = (q[..., i] for i in range(4))
    zero = F(0.0)
    v0 = q0 * zero - q1 * x - q2 * y - q3 * z
    v1 = q0 * x + q1 * zero + q2 * z - q3 * y
    v2 = q0 * y - q1 * z + q2 * zero + q3 * x
    v3 = q0 * z + q1 * y - q2 * x + q3 * zero
    n2 = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3 + F(1e-10)
    i0, i1, i2, i3 = q0 / n2, -q1 / n2, -q2 / n2, -q3 / n2
    w1 = v0 * i1 + v1 * i0 + v2 * i3 - v3 * i2
    w2 = v0 * i2 - v1 * i3 + v2 * i0 + v3 * i1
    w3 = v0 * i3 + v1 * i2 - v2 * i1 + v3 * i0
    k = valid(xyz).astype(F)
    out = np.stack([(w1 + t[..., 0]) * k, (w2 + t[..., 1]) * k, (w3 + t[..., 2]) * k], -1)
    assert out.dtype == F
    return out


def projection_constants(H, W):
    """model_util.py:189-200: python doubles rounded to the float32 constants every implementation uses."""
    d2r = np.pi / 180
    vres = (2.0 * d2r + 24.8 * d2r) / (H - 1)
    return D(np.float32(360.0 / W * d2r)), D(np.float32(vres)), D(np.float32(24.8 * d2r / vres))


def cell_coordinates(points, H, W):
    """Continuous (col, tmp) per point (..., 3) with iCol = int(col), iRow = H - int(tmp); NaN for a point of range 0."""
    az, vres, voff = projection_constants(H, W)
    p = np.asarray(points, D)
    r = np.sqrt((p * p).sum(-1))
    with np.errstate(all="ignore"):
        col = (D(np.float32(np.pi)) - np.arctan2(p[..., 1], p[..., 0])) / az
        tmp = np.arcsin(p[..., 2] / r) / vres + voff
    return col, tmp, r


def cells(points, H, W):
    """The cell rule: (..,) cell ids; NaN -> 0 before the clamps (a point of range 0 lands in row H-1)."""
    col, tmp, _ = cell_coordinates(points, H, W)
    to_int = lambda v: np.trunc(np.nan_to_num(v, nan=0.0)).astype(np.int64)
    return np.clip(H - to_int(tmp), 0, H - 1) * W + np.clip(to_int(col), 0, W - 1)


def project(points32, feat, cell, H, W):
    """The winner rule on ONE image: per cell the point(s) of minimum float32 range are SUMMED (ties add, model_util.py:255-273).
    points32: (N,3) float32 as stored (ranges compare as the float32 the kernel computes); returns out_xyz (H,W,3), out_feat."""
    p = np.asarray(points32, np.float32)
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).astype(np.float32) + p[:, 2] * p[:, 2]).astype(np.float32)
    min_r = np.full(H * W, np.inf, np.float32)
    np.minimum.at(min_r, cell, r)
    won = r == min_r[cell]
    out = np.zeros((H * W, 3), D)
    np.add.at(out, cell[won], p[won].astype(D))
    of = None
    if feat is not None:
        of = np.zeros((H * W, feat.shape[-1]), D)
        np.add.at(of, cell[won], np.asarray(feat, D)[won])
        of = of.reshape(H, W, -1)
    return out.reshape(H, W, 3), of, won

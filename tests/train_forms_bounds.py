"""TEST INFRASTRUCTURE of the training-form tests: the float64 references of the row kernels of csrc/elo_train.hip, their error bounds
DERIVED from operation counts (never from what a kernel produced) and stated in float64 quantities of the reference, and float32 numpy
restatements of each kernel's order of operations -- tests/test_train_forms_cpu.py requires the restatements to stay within HALF of the
bounds, and deliberately wrong restatements (MUTANTS) to miss them by 5 bounds, before tests/test_train_forms_gpu.py trusts them.

u = 2^-24 is the unit roundoff of fp32.  A value that passes n roundings is off by at most gam(n) = n u / (1 - n u) relative (Higham,
Accuracy and Stability of Numerical Algorithms, lemma 3.1).  Contraction into fused multiply-adds only removes roundings.
THE BUDGET OF AN ELEMENTWISE ROUNDING IS ONE ULP, e = 2u, not u.  A bound made of a handful of roundings is ATTAINED by a correct kernel
(a single rounding reaches u), and the CPU test demands that a correct float32 restatement stays within HALF of every bound: headroom
that only a budget of twice the attainable error has.  The long chains keep gam(n): their worst case needs every rounding of the
chain to go the same way, and a restatement stays far below it.  Below, `e` marks the roundings budgeted this way.

THE TWO REDUCTIONS (bn_stats_kernel, bn_bwd_reduce_kernel).  With rpb = 1024 / C rows per block iteration and parts =
elo_bn_parts(M, C) blocks, a thread adds its per = ceil(ceil(M / rpb) / parts) rows one after the other, and the rpb threads of a
channel quad are then added one after the other through LDS: a term passes at most n = per + rpb additions.  The blocks' partial rows
are added in double (at most 512 + 6 additions of 2^-53 each: DBL = 2^-43 relative covers them).
    |d sum| <= (gam(n) + DBL) sum|z|           |d sumsq| <= (gam(n + 1) + DBL) sum z^2            (the square is one more rounding)
    mean  = fl(sum / M):           d sum / M + e |mean|                                (M < 2^24: exact as a float; the division is double)
    var   = sumsq / M - mean^2:    dvar = d sumsq / M + 2 |mean| d sum / M + (d sum / M)^2            (clamping at 0 moves it towards var)
    invstd = fl((var + eps)^-1/2): invstd * (dvar / 2 * (var + eps)^1/2 / (var + eps - dvar)^3/2 + e)        (mean value theorem)
    moving averages, group after group: r <- fl((1 - momentum) r + momentum m): the error is (1 - momentum) times the one before, plus
      momentum * (d sum / M  |  dvar * M / (M - 1)), plus e of the new value.
    sum g: as sum z, and e for the result's rounding to fp32.   sum g xhat: xhat = fl(fl(z - mean) * invstd) and the product are three
      roundings more: gam(n + 3), and e for the result.
ELO_BN_APPLY, y = fl(fl(fl(fl(z - m) s) g) + b): with t = (z - m) s g and pre = t + b, |y - pre| <= e (1 + 4u) (3 |t| + |pre|).  ReLU is
1-Lipschitz.  At a placed tie t = pre = 0: the bound is 0, y must be 0.  bn_inputs keeps every other pre-activation 4 bounds from zero.
DZ = fl(fl(g s) * fl(fl(gr - k1) - fl(xhat k2))), k = fl(sums * fl(1 / M)) (two roundings), gr = dy or 0:
    inner <= E1 / M + |xhat| E2 / M + e (2 |gr| + 4 |k1| + 6 |xhat k2|)       (E: the bounds of the two sums; xhat k2: 2 + 2 + 1 roundings
    and the two subtractions' (|gr| + |k1|) and (|gr| + |k1| + |xhat k2|))
    |d dz| <= (|g s| inner + 2e |dz|) (1 + 16u)
DW: the fp32 MFMA is a k-ordered fmaf chain, one rounding per product-and-add and no wider accumulator, so an element of a slice's
partial block passes 4 * per_slice roundings (per_slice groups of 4 rows); slices_combine_kernel adds every 16th slice in a thread
(ceil(slices / 16) additions) and the 16 threads' sums in order: n = 4 per_slice + ceil(slices / 16) + 16, bound gam(n) * (|x|^T |g|).
DB: a lane adds its row of every group (per_slice additions), two butterfly additions, the same combine:
n = per_slice + 2 + ceil(slices / 16) + 16, bound gam(n) * sum|g|.

The references and bounds below take numpy arrays or torch tensors (the two cases beyond the elementwise kernels' block cap are made
and checked on the device); the restatements are numpy."""
import numpy as np

import train_forms_cases as table

U = 2.0 ** -24
E = 2 * U
DBL = 2.0 ** -43
_F = np.float32


def gam(n):
    return n * U / (1 - n * U)


def _d(a):
    return a.double() if hasattr(a, "double") else np.asarray(a, np.float64)


def _grouped(G, *tensors):
    """(G * M, C) -> (G, M, C) and (G, C) -> (G, 1, C), in float64."""
    return [_d(a).reshape(G, -1, a.shape[-1]) for a in tensors]


def _stack(a, b):
    if isinstance(a, np.ndarray):
        return np.stack([a, b], 1)
    import torch
    return torch.stack([a, b], 1)


def reduction_terms(M, C):
    """n of the module docstring: the additions a term of a batch-norm reduction passes at most."""
    return table.bn_per(M, C) + 1024 // C


# ------------------------------------------------------------------------------------------------------------------------ references
def preactivation(z, mean, invstd, gamma, beta, G):
    """float64: the pre-activation ((z - mean) invstd) gamma + beta and the bound of its fp32 evaluation, both (G * M, C)."""
    z3, m, s = _grouped(G, z, mean, invstd)
    t = (z3 - m) * s * _d(gamma)
    pre = t + _d(beta)
    return pre.reshape(z.shape), (E * (1 + 4 * U) * (3 * abs(t) + abs(pre))).reshape(z.shape)


def apply_reference(z, mean, invstd, gamma, beta, relu, G):
    """elo_bn_apply: (y, bound), float64."""
    pre, bound = preactivation(z, mean, invstd, gamma, beta, G)
    return (pre * (pre > 0) if relu else pre), bound


def stats_reference(z, G, eps, momentum, rm=None, rv=None):
    """elo_bn_stats on numpy float32 z (G * M, C): dict of (value, bound) pairs -- mean, invstd (G, C); rm, rv (C) where given."""
    C, M = z.shape[1], z.shape[0] // G
    assert M < 2 ** 24                                              # (float)M is exact
    z3 = np.asarray(z, np.float64).reshape(G, M, C)
    n = reduction_terms(M, C)
    mean = z3.sum(1) / M
    var = ((z3 - mean[:, None, :]) ** 2).sum(1) / M
    eps, momentum = float(eps), float(momentum)
    dsum = (gam(n) + DBL) * np.abs(z3).sum(1) / M
    dvar = (gam(n + 1) + DBL) * (z3 * z3).sum(1) / M + 2 * np.abs(mean) * dsum + dsum ** 2
    assert (dvar < (var + eps) / 2).all()                           # the bound of invstd is meaningful
    invstd = (var + eps) ** -0.5
    out = {"mean": (mean, dsum + E * (np.abs(mean) + dsum)),
           "invstd": (invstd, invstd * (dvar / 2 * (var + eps) ** 0.5 / (var + eps - dvar) ** 1.5 + E) * (1 + 4 * U))}
    if rm is not None:
        a, b = np.asarray(rm, np.float64), np.asarray(rv, np.float64)
        ea, eb = np.zeros(C), np.zeros(C)
        unb = M / (M - 1.0) if M > 1 else 1.0
        for g in range(G):
            a = (1 - momentum) * a + momentum * mean[g]
            b = (1 - momentum) * b + momentum * var[g] * unb
            ea = (1 - momentum) * ea + momentum * dsum[g]
            eb = (1 - momentum) * eb + momentum * dvar[g] * unb
            ea, eb = ea + E * (np.abs(a) + ea), eb + E * (np.abs(b) + eb)
        out["rm"], out["rv"] = (a, ea), (b, eb)
    return out


def backward_reference(dy, z, mean, invstd, gamma, beta, relu, G):
    """elo_bn_backward: dict of (value, bound) pairs -- sums (G, 2, C) = [sum g | sum g xhat] and dz (G * M, C); float64."""
    C, M = z.shape[-1], z.shape[0] // G
    assert M < 2 ** 24
    dy3, z3, m, s = _grouped(G, dy, z, mean, invstd)
    gamma, beta = _d(gamma), _d(beta)
    xh = (z3 - m) * s
    g = dy3 * (xh * gamma + beta > 0) if relu else dy3
    n = reduction_terms(M, C)
    s1, s2 = g.sum(1), (g * xh).sum(1)
    e1 = (gam(n) + DBL) * abs(g).sum(1)
    e2 = (gam(n + 3) + DBL) * abs(g * xh).sum(1)
    b1, b2 = e1 + E * (abs(s1) + e1), e2 + E * (abs(s2) + e2)
    k1, k2 = s1[:, None, :] / M, s2[:, None, :] / M
    dz = gamma * s * (g - k1 - xh * k2)
    inner = b1[:, None, :] / M + abs(xh) * b2[:, None, :] / M + E * (2 * abs(g) + 4 * abs(k1) + 6 * abs(xh * k2))
    bdz = (abs(gamma * s) * inner + 2 * E * abs(dz)) * (1 + 16 * U)
    return {"sums": (_stack(s1, s2), _stack(b1, b2)), "dz": (dz.reshape(z.shape), bdz.reshape(z.shape))}


def wgrad_terms(rows, cin, cout):
    """(n of dW, n of db) of the module docstring."""
    p = table.wgrad_plan(rows, cin, cout)
    tail = (p["slices"] + 15) // 16 + 16
    return 4 * p["per_slice"] + tail, p["per_slice"] + 2 + tail


def wgrad_reference(x, g):
    """elo_dense_weight_grad on float32 x (rows, cin), g (rows, cout): dict of (value, bound) pairs -- dW (cin, cout), db (cout)."""
    x, g = _d(x), _d(g)
    nw, nb = wgrad_terms(x.shape[0], x.shape[1], g.shape[1])
    return {"dW": (x.T @ g, gam(nw) * (abs(x).T @ abs(g))), "db": (g.sum(0), gam(nb) * abs(g).sum(0))}


def share(got, want, bound):
    """(the largest |got - want| / bound, where): 0 / 0 counts as 0, anything over a zero bound -- and a NaN -- as inf."""
    err = abs(_d(got) - want)
    if hasattr(err, "cpu"):                                            # torch, on the device
        import torch
        inf = torch.full_like(err, float("inf"))
        r = torch.where(err == 0, torch.zeros_like(err), torch.where((bound > 0) & ~torch.isnan(err), err / bound, inf))
        at = int(r.argmax())
        return float(r.reshape(-1)[at]), tuple(int(i) for i in np.unravel_index(at, tuple(r.shape)))
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    if r.size == 0:
        return 0.0, ()
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[at]), tuple(int(i) for i in at)


# The companions (elo_pose_compose, elo_pose_loss, elo_adam_flat at more batch elements / parameters than one block or one trip):
# the tolerances tests/test_train_kernels_gpu.py uses for these operators at its one size, relative to the scale of the compared tensor.
POSE_VALUE_REL, POSE_GRAD_REL, LOSS_VALUE_REL = 2e-6, 1e-5, 2e-6
ADAM_PARAM_REL, ADAM_MOMENT_REL = 2e-6, 1e-6


# ------------------------------------------------------------------------------------- float32 restatements (numpy, CPU), with mutants
MUTANTS = ("biased_moving_variance", "momentum_on_the_wrong_term", "last_group_only", "mask_from_z", "ge_at_ties", "xhat_term_dropped",
           "m_minus_1", "last_partial_group_dropped", "tile_order", "db_per_block")


def _block_sums(terms, C):
    """The two-stage fp32 sum of (M, C) terms as bn_stats_kernel / bn_bwd_reduce_kernel form it, then the partial rows in double."""
    M = terms.shape[0]
    rpb, parts, per = 1024 // C, table.bn_parts(M, C), table.bn_per(M, C)
    pad = np.zeros((parts * per * rpb, C), _F)                        # (rows past M or past a block's share are zeros: x + 0 = x)
    pad[:M] = terms
    a = pad.reshape(parts, per, rpb, C)
    s = np.zeros((parts, rpb, C), _F)
    for k in range(per):                                              # a thread's rows, one after the other
        s = s + a[:, k]
    t = np.zeros((parts, C), _F)
    for i in range(rpb):                                              # the threads of a channel quad through LDS, in order
        t = t + s[:, i]
    return t.astype(np.float64).sum(0)


def stats_f32(z, G, eps, momentum, rm=None, rv=None, mutant=None):
    """elo_bn_stats restated: mean, invstd (G, C) and the moving averages, float32."""
    C, M = z.shape[1], z.shape[0] // G
    mean, invstd = np.zeros((G, C), _F), np.zeros((G, C), _F)
    a = None if rm is None else np.asarray(rm, np.float64)
    b = None if rv is None else np.asarray(rv, np.float64)
    a0, b0 = a, b
    mom = float(momentum)
    for g in range(G):
        zg = z[g * M:(g + 1) * M]
        s, ss = _block_sums(zg, C), _block_sums(zg * zg, C)
        m = s / M
        var = np.maximum(ss / M - m * m, 0.0)
        mean[g], invstd[g] = m.astype(_F), (1.0 / np.sqrt(var + float(eps))).astype(_F)
        if a is not None:
            unbiased = var * M / (M - 1) if M > 1 and mutant != "biased_moving_variance" else var
            if mutant == "last_group_only":
                a, b = a0, b0
            w_old, w_new = (mom, 1.0 - mom) if mutant == "momentum_on_the_wrong_term" else (1.0 - mom, mom)
            a = (w_old * a + w_new * m).astype(_F).astype(np.float64)
            b = (w_old * b + w_new * unbiased).astype(_F).astype(np.float64)
    return mean, invstd, (None if a is None else a.astype(_F)), (None if b is None else b.astype(_F))


def apply_f32(z, mean, invstd, gamma, beta, relu, G):
    C = z.shape[1]
    z3 = z.reshape(G, -1, C)
    y = (z3 - mean[:, None, :]) * invstd[:, None, :] * gamma + beta
    return (np.maximum(y, _F(0)) if relu else y).reshape(z.shape)


def backward_f32(dy, z, mean, invstd, gamma, beta, relu, G, mutant=None):
    """elo_bn_backward restated: sums (G, 2, C) and dz, float32."""
    C, M = z.shape[1], z.shape[0] // G
    dy3, z3 = dy.reshape(G, M, C), z.reshape(G, M, C)
    xh = (z3 - mean[:, None, :]) * invstd[:, None, :]
    pre = xh * gamma + beta
    keep = (z3 > 0) if mutant == "mask_from_z" else (pre >= 0) if mutant == "ge_at_ties" else (pre > 0)
    g = np.where(keep, dy3, _F(0)) if relu else dy3
    sums = np.zeros((G, 2, C), _F)
    for i in range(G):
        sums[i, 0], sums[i, 1] = _block_sums(g[i], C).astype(_F), _block_sums(g[i] * xh[i], C).astype(_F)
    inv_m = _F(1.0) / _F(M - 1 if mutant == "m_minus_1" and M > 1 else M)
    k1, k2 = (sums[:, 0] * inv_m)[:, None, :], (sums[:, 1] * inv_m)[:, None, :]
    inner = g - k1 if mutant == "xhat_term_dropped" else g - k1 - xh * k2
    return sums, ((gamma * invstd[:, None, :]) * inner).reshape(z.shape)


def _fma(a, b, c):
    """fl(a * b + c) on float32 arrays: the product of two floats is exact in double, the sum is rounded to double first (a double
    rounding in rare cases, far below what the bounds count)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_F)


def _combine_slices(part):
    """slices_combine_kernel: part (slices, ...) -> (...)"""
    slices = part.shape[0]
    rows = []
    for sr in range(16):
        v = np.zeros(part.shape[1:], _F)
        for s in range(sr, slices, 16):
            v = v + part[s]
        rows.append(v)
    t = np.zeros(part.shape[1:], _F)
    for v in rows:
        t = t + v
    return t


def wgrad_f32(x, g, plan, mutant=None):
    """elo_dense_weight_grad restated on (a channel subset of) x (rows, cin'), g (rows, cout'); plan = wgrad_plan of the FULL shape."""
    rows = x.shape[0]
    if mutant == "last_partial_group_dropped":
        rows -= rows % 4
    slices, R = plan["slices"], plan["per_slice"] * 4
    xp, gp = np.zeros((slices * R, x.shape[1]), _F), np.zeros((slices * R, g.shape[1]), _F)
    xp[:rows], gp[:rows] = x[:rows], g[:rows]
    xs, gs = xp.reshape(slices, R, -1), gp.reshape(slices, R, -1)
    acc = np.zeros((slices, x.shape[1], g.shape[1]), _F)
    for r in range(R):                                               # the k-ordered fmaf chain of the MFMAs of a slice
        acc = _fma(xs[:, r, :, None], gs[:, r, None, :], acc)
    lanes = [np.zeros((slices, g.shape[1]), _F) for _ in range(4)]   # db: lane group k adds row k of every group of 4 ...
    for r in range(R):
        lanes[r % 4] = lanes[r % 4] + gs[:, r]
    bsum = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3])             # ... and the butterfly adds the four
    dW, db = _combine_slices(acc), _combine_slices(bsum)
    if mutant == "db_per_block":
        db = db * _F(plan["gy"])
    if mutant == "tile_order" and plan["xv"]:
        CI, out = plan["CI"], dW.copy()
        for ci0 in range(0, dW.shape[0], 16 * CI):
            for a in range(CI):
                for i in range(16):
                    out[ci0 + 16 * a + i] = dW[ci0 + CI * i + a]      # tile a holds the channels ci0 + CI i + a: left where they are
        dW = out
    return dW, db

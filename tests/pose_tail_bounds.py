"""Per-element error bounds of the pose tail (csrc/elo_features.hip: softmax_valid_partial_kernel, softmax_valid_merge_kernel,
pose_head_kernel; csrc/elo_fused.hip: mlp_sv_kernel) against the float64 statements of tests/pose_tail_reference.py, derived from
the kernels' summation structure -- not from what the kernels return.

HOW.  The structure is written ONCE, below, as functions over an arithmetic `ar`:
  partial_sums   a slice of the points per workgroup: four waves stride over it, 16 rows in flight per wave and trip -- the batch's
                 own softmax (16 exponentials on the batch maximum, 16-term sums), ONE rescale of the running triple per batch --
                 then the 4-wave combine on the slice maximum;
  ride_sums      mlp_sv_kernel: a row tile per workgroup, its rows 16 at a time with the same batch step, no waves;
  merge_seq      sv_merge (softmax_valid_merge_kernel and the head's channels 64..): the slices one after the other on their
                 maximum, then the division;
  merge_head     pose_head_kernel's merge of channels 0..63: four threads per channel, thread g over slices g, g + 4, ... as a
                 running online softmax (loaded in trips of 16 or 32 slices: `mine`), the four merged on their maximum, the division.
Two arithmetics run them.  F32 computes in float32, operation by operation in the kernel's order (no contraction: the library is
built with -ffp-contract=off): the emulation tests/test_pose_tail_cpu.py holds within HALF the bound.  BND carries (value in
float64, absolute error bound) pairs -- a running error analysis: with u = 2^-24, |fl(a op b) - (a op b)| <= u |a op b|, so
  add:  e = ea + eb + u (|v| + ea + eb)            mul:  e = |a| eb + |b| ea + ea eb + u (|v| + that)
  div:  e = (ea + |v| eb) / (|b| - eb) + u (|v| + that)
each plus TINY = 2^-126 for a result the hardware may flush.  Maxima are maxima of stored inputs: exact in both arithmetics, so
every branch (a batch without a valid row, the skipped empty slices, which of the two rescale forms) is taken alike.
  exp_acc(a - b), a, b exact:  e = v (3 |x| + 2) u, x = a - b: the term tests/fused_shapes_bounds.py established for exp_acc -- the
       subtraction rounds (|x| u in the exponent), x log2(e) is carried in two pieces whose product and correction round again
       (2 |x| u together), v_exp_f32 is good to 1 ulp (2 u) -- and exp_acc clamps x at -104, where e^x < 2^-150 <= TINY.
  expf(a - b) (sv_merge):      e = v (|x| + 2) u: the subtraction's |x| u, and the 1 ulp = 2 u the HIP math library documents for
       expf (its argument reduction is carried in extended precision, so no further |x| term).
BND's VALUE is the same operator in float64 by another route; the CPU test also holds it to the reference within 1e-12.

THE HEAD.  y = b + sum_k x_k w_k accumulated in sequence passes every term through at most n = K + 1 roundings (its product, then
the adds): |fl(y) - y| <= gamma_n (|b| + sum |x_k| |w_k|), gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, 3.1); an
input error ex adds |ex| |W| (1 + gamma_n).  big: K = C.  The 7 head sums: a thread's own ceil(hidden / 256) terms, 6 levels of the
wave's butterfly, 4 wave sums and the bias: n = ceil(hidden / 256) + 11.  The composition: the head's error through the float64
Jacobian of reference.compose at that input (central differences, step 1e-6, 1 % slack for the differences), plus the
composition's own float32 roundings in units of u: normalise_q is 4 products, 4 adds, a square root, an add and a division = 11
roundings on a vector of norm <= 1; a Hamilton product is 4 products and 3 adds per component = 7; the inverse 10.  q (normalise +
Hamilton): OWN_Q = 18 units of (1 + |q_c|_1); q_norm: that again through 1 / |q| (|q| >= 1/2: a unit q_c) plus its own 11:
OWN_QN = 2 * 18 + 11 = 47; t (two Hamilton products over normalise and the inverse, one add): OWN_T = 7 + 7 + 11 + 10 + 1 = 36
units of (|t_c|_1 + |t|_inf + 1)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
F = np.float32
D = np.float64
OWN_Q, OWN_QN, OWN_T = 18, 47, 36
JACOBIAN_SLACK = 1.01


def gamma(n):
    return n * U / (1.0 - n * U)


# ----------------------------------------------------------------------------------------------------------- the two arithmetics
def exp_acc32(x):
    """csrc/elo_common.h exp_acc in float32: the fused multiply-adds evaluated in float64 (exact products) and rounded once."""
    L2E_HI, L2E_LO, LN2 = D(F(1.44269502162933349609375)), D(F(1.925963033500011e-8)), D(F(0.693147180559945))
    x = np.maximum(np.asarray(x, F), F(-104.0)).astype(D)
    t = (x * L2E_HI).astype(F).astype(D)
    r = (x * L2E_LO + (x * L2E_HI - t).astype(F).astype(D)).astype(F).astype(D)
    return (np.exp2(t).astype(F) * (r * LN2 + 1.0).astype(F)).astype(F)


class F32:
    """float32, one rounding per operation"""
    @staticmethod
    def lift(x): return np.asarray(x, F)
    @staticmethod
    def zeros(shape): return np.zeros(shape, F)
    @staticmethod
    def add(a, b): return (a + b).astype(F)
    @staticmethod
    def mul(a, b): return (a * b).astype(F)
    @staticmethod
    def div(a, b):
        with np.errstate(all="ignore"):
            return (a / b).astype(F)
    @staticmethod
    def expdiff(a, b, libm=False):
        with np.errstate(invalid="ignore"):
            x = (np.asarray(a, F) - np.asarray(b, F)).astype(F)
        x = np.where(np.isnan(x), F(-np.inf), x)                                   # (-inf) - (-inf): lanes no branch selects
        return np.exp(x.astype(D)).astype(F) if libm else exp_acc32(x)
    @staticmethod
    def where(c, a, b): return np.where(c, a, b)
    @staticmethod
    def value(a): return np.asarray(a, D)
    @staticmethod
    def take(a, fn): return fn(a)


class BND:
    """(float64 value, absolute error bound) pairs"""
    @staticmethod
    def lift(x): return (np.asarray(x, D), np.zeros(np.shape(x), D))
    @staticmethod
    def zeros(shape): return (np.zeros(shape, D), np.zeros(shape, D))
    @staticmethod
    def _round(v, e): return (v, e + U * (np.abs(v) + e) + TINY)
    @staticmethod
    def add(a, b): return BND._round(a[0] + b[0], a[1] + b[1])
    @staticmethod
    def mul(a, b): return BND._round(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])
    @staticmethod
    def div(a, b):
        with np.errstate(all="ignore"):
            v = a[0] / b[0]
            e = (a[1] + np.abs(v) * b[1]) / (np.abs(b[0]) - b[1])
        return BND._round(v, e)
    @staticmethod
    def expdiff(a, b, libm=False):
        with np.errstate(invalid="ignore"):
            x = np.asarray(a, D) - np.asarray(b, D)
        x = np.where(np.isnan(x), -np.inf, x)
        v = np.exp(x)
        ax = np.where(np.isfinite(x), np.abs(x), 0.0)
        return (v, v * ((1.0 if libm else 3.0) * ax + 2.0) * U + TINY)
    @staticmethod
    def where(c, a, b): return (np.where(c, a[0], b[0]), np.where(c, a[1], b[1]))
    @staticmethod
    def value(a): return a[0]
    @staticmethod
    def take(a, fn): return (fn(a[0]), fn(a[1]))


# --------------------------------------------------------------------------------------------------------------- the structure
def _quiet(fn):
    """(lanes no branch selects compute inf - inf and the like, as the kernels' predicated-off lanes do)"""
    def run(*args, **kwargs):
        with np.errstate(all="ignore"):
            return fn(*args, **kwargs)
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


def _batch_step(ar, run, rows):
    """One 16-row batch into the running triple run = (M, D, A).  rows: 16 x (logit, value, ok), logit / value float64 arrays of
    the stored inputs and ok a bool array, all of one shape.  The batch's own softmax, then ONE rescale (skipped where no row is ok)."""
    M, Dn, An = run
    bm = np.full(rows[0][0].shape, -np.inf)
    for l, _v, ok in rows:
        bm = np.where(ok, np.maximum(bm, l), bm)
    d16, a16 = ar.zeros(bm.shape), ar.zeros(bm.shape)
    for l, v, ok in rows:
        e = ar.where(ok, ar.expdiff(l, bm), ar.zeros(bm.shape))
        d16 = ar.add(d16, e)
        a16 = ar.add(a16, ar.mul(e, ar.lift(v)))
    m2 = np.maximum(M, bm)
    s0, s1 = ar.expdiff(M, m2), ar.expdiff(bm, m2)
    some = bm > -np.inf
    Dn = ar.where(some, ar.add(ar.mul(Dn, s0), ar.mul(d16, s1)), Dn)
    An = ar.where(some, ar.add(ar.mul(An, s0), ar.mul(a16, s1)), An)
    return np.where(some, m2, M), Dn, An


def _on_maximum(ar, triples, libm):
    """Triples (M, D, A) summed on their common maximum, skipping those with D == 0 (sv_merge; the 4-wave and the 4-thread combine)."""
    Mx = triples[0][0]
    for M, _d, _a in triples[1:]:
        Mx = np.maximum(Mx, M)
    DD, AA = ar.zeros(Mx.shape), ar.zeros(Mx.shape)
    for M, Dn, An in triples:
        live = ar.value(Dn) != 0
        sc = ar.expdiff(M, Mx, libm)
        DD = ar.where(live, ar.add(DD, ar.mul(Dn, sc)), DD)
        AA = ar.where(live, ar.add(AA, ar.mul(An, sc)), AA)
    return Mx, DD, AA


def _pooled(ar, DD, AA):
    some = ar.value(DD) > 0
    return ar.where(some, ar.div(AA, DD), ar.zeros(some.shape))


@_quiet
def partial_sums(ar, logits, values, ok, parts):
    """softmax_valid_partial_kernel: (M, D, A), each (B, parts, C); logits / values (B,N,C) as stored, ok (B,N) bool."""
    l, v = np.asarray(logits, D), np.asarray(values, D)
    B, N, C = l.shape
    per = -(-N // parts)
    lo = np.arange(parts) * per
    hi = np.minimum(N, lo + per)
    waves = []
    for w in range(4):
        run = (np.full((B, parts, C), -np.inf), ar.zeros((B, parts, C)), ar.zeros((B, parts, C)))
        for n0 in range(w, per, 64):                                # this wave's trips: rows lo + n0 + 4 u
            rows = []
            for u in range(16):
                n = lo + n0 + 4 * u
                nn = np.minimum(n, hi - 1)                          # the clamped load
                rows.append((l[:, nn], v[:, nn], ((n < hi)[None, :] & ok[:, nn])[..., None] & np.ones(C, bool)))
            run = _batch_step(ar, run, rows)
        waves.append(run)
    return _on_maximum(ar, waves, libm=False)


@_quiet
def ride_sums(ar, logits, values, ok, tile):
    """mlp_sv_kernel's reduction: one triple per `tile` rows (the last tile of a batch element may be ragged)."""
    l, v = np.asarray(logits, D), np.asarray(values, D)
    B, N, C = l.shape
    tiles = -(-N // tile)
    first = np.arange(tiles) * tile
    run = (np.full((B, tiles, C), -np.inf), ar.zeros((B, tiles, C)), ar.zeros((B, tiles, C)))
    for r0 in range(0, tile, 16):
        rows = []
        for r in range(16):
            n = first + r0 + r
            nn = np.minimum(n, N - 1)
            rows.append((l[:, nn], v[:, nn], ((n < N)[None, :] & ok[:, nn])[..., None] & np.ones(C, bool)))
        run = _batch_step(ar, run, rows)
    return run


def _slice(ar, triple, i):
    M, Dn, An = triple
    return M[:, i], ar.take(Dn, lambda x: x[:, i]), ar.take(An, lambda x: x[:, i])


@_quiet
def merge_seq(ar, triple, parts):
    """sv_merge: pooled (B,C) and the statistics (maximum, denominator)."""
    Mx, DD, AA = _on_maximum(ar, [_slice(ar, triple, i) for i in range(parts)], libm=True)
    return _pooled(ar, DD, AA), Mx, DD


@_quiet
def merge_head(ar, triple, parts, mine=None, stride=None, combine_libm=False):
    """pose_head_kernel's merge (C <= 64 channels): thread group g over slices g, g + 4, ..., loaded `mine` per trip (16 up to 64
    slices, 32 above), a trip every 4 * mine slices; `stride` and `combine_libm` (expf in the 4-to-1 combine) restate two mutations for the CPU test."""
    mine = mine or (16 if parts <= 64 else 32)
    stride = stride or 4 * mine
    shape = triple[0][:, 0].shape
    groups = []
    for g in range(4):
        M, Dn, An = np.full(shape, -np.inf), ar.zeros(shape), ar.zeros(shape)
        for i0 in range(g, parts, stride):
            for u in range(mine):
                i = i0 + 4 * u
                if i >= parts:                                      # (the clamped load: denominator 0, skipped)
                    continue
                m, d, a = _slice(ar, triple, i)
                live = ar.value(d) != 0
                up = m > M
                sc = ar.where(up, ar.expdiff(M, m), ar.expdiff(m, M))
                Dn = ar.where(live, ar.where(up, ar.add(ar.mul(Dn, sc), d), ar.add(Dn, ar.mul(d, sc))), Dn)
                An = ar.where(live, ar.where(up, ar.add(ar.mul(An, sc), a), ar.add(An, ar.mul(a, sc))), An)
                M = np.where(live & up, m, M)
        groups.append((M, Dn, An))
    _Mx, DD, AA = _on_maximum(ar, groups, libm=combine_libm)
    return _pooled(ar, DD, AA)


@_quiet
def head_pool(ar, triple, parts, C):
    """The pooled (B,C) vector as pose_head_kernel forms it: merge_head for channels 0..63, sv_merge behind them."""
    channels = lambda sl: (triple[0][..., sl], ar.take(triple[1], lambda y: y[..., sl]), ar.take(triple[2], lambda y: y[..., sl]))
    out = merge_head(ar, channels(slice(0, 64)), parts)
    if C <= 64:
        return out
    tail = merge_seq(ar, channels(slice(64, None)), parts)[0]
    if ar is F32:
        return np.concatenate([out, tail], -1)
    return (np.concatenate([out[0], tail[0]], -1), np.concatenate([out[1], tail[1]], -1))


def merged_exactly(triple):
    """A BND triple merged WITHOUT further rounding (what a float64 merge of the kernel's stored triples is compared with): pooled
    value and bound (B,C).  pooled = sum A_i s_i / sum D_i s_i, s_i = e^(M_i - M) exact and >= 0, so the triples' bounds carry over
    as (sum eA_i s_i + |pooled| sum eD_i s_i) / (sum D_i s_i - sum eD_i s_i)."""
    M, (dv, de), (av, ae) = triple
    with np.errstate(all="ignore"):
        Mx = M.max(1, keepdims=True)
        s = np.where(dv != 0, np.exp(np.where(np.isfinite(M), M - Mx, -np.inf)), 0.0)
        dd, aa = (dv * s).sum(1), (av * s).sum(1)
        pooled = np.where(dd > 0, aa / np.where(dd > 0, dd, 1.0), 0.0)
        e = ((ae * s).sum(1) + np.abs(pooled) * (de * s).sum(1)) / np.where(dd > 0, dd - (de * s).sum(1), 1.0)
    return pooled, np.where(dd > 0, e, 0.0)


def lift_triple(ar, mx, den, acc):
    """Hand-made partial sums (exact float32 inputs) as the arithmetic's triple."""
    return np.asarray(mx, D), ar.lift(den), ar.lift(acc)


# ------------------------------------------------------------------------------------------------------------------- the head
def dense_bound(x, ex, W, b, n):
    ax, aW = np.abs(np.asarray(x, D)), np.abs(np.asarray(W, D))
    return (ex @ aW) * (1.0 + gamma(n)) + gamma(n) * (np.abs(np.asarray(b, D)) + ax @ aW)


def head_bound(pooled, e_pooled, W_big, b_big, W_q, b_q, W_t, b_t):
    """Bound (B,7) of the head's raw output given the pooled vector's (value, bound)."""
    C, hidden = np.shape(W_big)
    big = np.asarray(pooled, D) @ np.asarray(W_big, D) + np.asarray(b_big, D)
    e_big = dense_bound(pooled, e_pooled, W_big, b_big, C + 1)
    n = -(-hidden // 256) + 11
    return np.concatenate([dense_bound(big, e_big, W_q, b_q, n), dense_bound(big, e_big, W_t, b_t, n)], -1)


def pose_bound(R, raw, e_raw, q_coarse, t_coarse):
    """Bounds of (q, t, q_norm) from the raw head's bound: |Jacobian| e_raw plus the composition's own roundings."""
    raw = np.asarray(raw, D)
    B = raw.shape[0]
    flat = lambda r: np.concatenate(R.compose(r, q_coarse, t_coarse), -1)           # (B,11)
    J = np.zeros((B, 11, 7))
    h = 1e-6
    for k in range(7):
        d = np.zeros(7)
        d[k] = h
        J[:, :, k] = (flat(raw + d) - flat(raw - d)) / (2 * h)
    through = np.einsum("bok,bk->bo", np.abs(J), e_raw) * JACOBIAN_SLACK
    q, t, _qn = R.compose(raw, q_coarse, t_coarse)
    qc1 = 0.0 if q_coarse is None else np.abs(np.asarray(q_coarse, D)).reshape(B, -1).sum(-1, keepdims=True)
    tc1 = 0.0 if t_coarse is None else np.abs(np.asarray(t_coarse, D)).reshape(B, -1).sum(-1, keepdims=True)
    own_q = OWN_Q * U * (1.0 + qc1) * np.ones((B, 4))
    own_t = OWN_T * U * (tc1 + np.abs(t).max(-1, keepdims=True) + 1.0) * np.ones((B, 3))
    own_qn = OWN_QN * U * (1.0 + qc1) * np.ones((B, 4))
    return through[:, :4] + own_q, through[:, 4:7] + own_t, through[:, 7:] + own_qn

"""TEST INFRASTRUCTURE of the forward-form tests: the error bounds of the forward kernels of csrc/elo_features.hip, DERIVED from
their operation counts (never from what a kernel produced), the float64 reference quantities the bounds are stated in, and float32
numpy restatements of each pool form's arithmetic -- tests/test_forward_forms_cpu.py runs the restatements against float64 and
requires them to stay within HALF of the constants below before tests/test_forward_forms_gpu.py trusts them.

u = 2^-24 is the unit roundoff of fp32 (half an ulp, relative).

THE NORM COLUMN of the encode kernels, sqrtf(d0*d0 + d1*d1 + d2*d2 + 1e-20f) with d = fl(g*m - p): each d carries u (a correctly
rounded subtraction of the exact g*m and p: 2u on its square), each product u, and a term passes at most three additions (u each):
6u on the sum, halved by the root, plus the root's own rounding: 4u relative.  Stored as fp16, one more rounding to half: 2^-11
relative, and 2^-25 absolute (half of the smallest subnormal, 2^-24) where the result is subnormal or flushes to 0 (d = 0 gives 1e-10).

THE SOFTMAX POOL, out = sum_k e_k v_k / sum_k e_k with e_k = exp(x_k), x_k = l_k - max_k l <= 0.  If term k enters the numerator
with relative error epsA_k and the denominator with epsD_k, then to first order
    |out' - out| <= sum_k w_k (|v_k| epsA_k + |out| epsD_k) + u |out|          (w = the exact softmax weights; u |out|: the division)
and with eps_k <= (a + b |x_k|) u this is at most (max(a, b) + 1) * UNIT, where
    UNIT = u * sum_k w_k (|v_k| + |out|) (1 + |x_k|)                            (computed in float64: pool_reference below).
What a and b are, form by form:
  * x_k = fl(l_k - max) is off by u |x_k|, which moves e_k by u |x_k| relative.  The exp2 forms compute exp2(fl(x_k * fl(log2 e))):
    the constant's rounding (< u) and the product's (u) move the argument by 2u |x_k| log2 e more, e_k by 2u |x_k|: b = 3 for the
    exp2 forms, b = 1 for the scalar form's expf.
  * the exponential itself: 1 ulp = 2u (v_exp_f32, and expf's documented bound); the product e_k v_k: u (numerator only).
  * scalar form (two passes, K sequential additions): the first term passes K - 1 roundings.  a = 2 + 1 + (K - 1) = K + 2;
    constant K + 3.
  * wave form (two passes; a lane group adds its J = 1 / 2 / 4 / 8 rows, the first into an exact 0, then two butterfly additions
    across the four lane groups): a = 2 + 1 + (J - 1) + 2 = J + 4; constant J + 5 (b = 3 is never the larger).
  * quarter-wave ("vec") form (ONE pass, online softmax): whenever a later logit exceeds the running maximum, the accumulated sums
    are multiplied by sc = exp2(fl((old max - new max) * fl(log2 e))).  The arguments of term k's own exponential and of all its later
    rescales have one sign and add up to x_k exactly, so b = 3 as above; every later step costs the term at most one exponential
    (2u), one product (u) and one addition (u), 4u, or a single addition where the maximum stays.  a = 2 + 1 + 4 (K - 1) = 4K - 1;
    constant 4K.
  * exponentials below the normal range (the x40 points reach x = -300) may be flushed: each e_k is then off by at most 2^-126
    ABSOLUTE against a denominator >= 1: K * 2^-126 * (max|v| + |out|), added as an absolute term (POOL_ABS per unit of |v|).
  * fp16 storage (fp32 arithmetic on fp16-representable inputs, the result rounded to half): plus 2^-11 |out| + 2^-25.
An all-masked point has x = 0 and w = 1 / K: the plain mean of its K values, to the same bound."""
import numpy as np
import torch

import twins_torch as twin

U32 = 2.0 ** -24
NORM_REL = 4 * U32
HALF_REL, HALF_ABS = 2.0 ** -11, 2.0 ** -25
POOL_ABS = 2.0 ** -126


def pool_constant(form, K):
    """The constant in front of UNIT (module docstring) for a form name of the elo_masked_softmax_pool_form query."""
    if form == "scalar":
        return K + 3
    if form.startswith("wave"):
        return int(form[4:]) + 5
    assert form in ("vec4", "vec6"), form
    return 4 * K


def pool_reference(logits, values, mask):
    """float64 tensors (B,N,K,C), (B,N,K,C), (B,N,K) -> (out, UNIT, max|v| + |out|), each (B,N,C): tests/twins_torch.py's pool and the
    unit its error is measured in."""
    out = twin.masked_softmax_pool(logits, values, mask)
    l = torch.where(mask.unsqueeze(-1) == 1.0, logits, torch.full_like(logits, -1e10))
    x = l - l.amax(2, keepdim=True)
    w = torch.softmax(l, dim=2)                                          # (exp(-1e10) = 0 exactly: a masked slot beside a valid one weighs nothing)
    xa = torch.where(w > 0, x.abs(), torch.zeros_like(x))
    unit = U32 * (w * (values.abs() + out.abs().unsqueeze(2)) * (1 + xa)).sum(2)
    return out, unit, values.abs().amax(2) + out.abs()


def pool_bound(form, K, unit, scale, f16, out):
    b = pool_constant(form, K) * unit + K * POOL_ABS * scale
    return b + (HALF_REL * out.abs() + HALF_ABS if f16 else 0)


def norm_bound(ref, f16):
    b = NORM_REL * ref.abs()
    return b + (HALF_REL * ref.abs() + HALF_ABS if f16 else 0)


# ---------------------------------------------------------------------------- float32 restatements of the pool forms (numpy, CPU)
_F = np.float32
_LOG2E = _F(1.44269504088896)


def _exp2_form(x):
    return np.exp2(x * _LOG2E, dtype=_F)


def _logit(lg, m, k):
    return np.where(m[..., k, None] == 1, lg[..., k, :], _F(-1e10)).astype(_F)


def pool_scalar_f32(lg, v, m):
    """softmax_pool_kernel: the maximum over K, then K sequential additions of expf(l - max) and of its product with the value."""
    K = lg.shape[2]
    with np.errstate(under="ignore"):
        mx = np.full(lg.shape[:2] + lg.shape[3:], -np.inf, _F)
        for k in range(K):
            mx = np.maximum(mx, _logit(lg, m, k))
        den, acc = np.zeros_like(mx), np.zeros_like(mx)
        for k in range(K):
            e = np.exp(_logit(lg, m, k) - mx, dtype=_F)
            den = den + e
            acc = acc + e * v[..., k, :]
    return acc / den


def pool_wave_f32(lg, v, m):
    """softmax_pool_wave_kernel: lane group g of four adds the rows k = g, g + 4, ...; the groups meet as (g0 + g1) + (g2 + g3)."""
    K = lg.shape[2]
    with np.errstate(under="ignore"):
        mx = np.full(lg.shape[:2] + lg.shape[3:], -np.inf, _F)
        for k in range(K):
            mx = np.maximum(mx, _logit(lg, m, k))
        den, acc = [np.zeros_like(mx) for _ in range(4)], [np.zeros_like(mx) for _ in range(4)]
        for g in range(4):
            for k in range(g, K, 4):
                e = _exp2_form(_logit(lg, m, k) - mx)
                den[g] = den[g] + e
                acc[g] = acc[g] + e * v[..., k, :]
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) / ((den[0] + den[1]) + (den[2] + den[3]))


def pool_vec_f32(lg, v, m):
    """softmax_pool_vec_kernel: one pass over K; a logit above the running maximum rescales the sums."""
    K = lg.shape[2]
    with np.errstate(under="ignore", invalid="ignore"):
        mx = np.full(lg.shape[:2] + lg.shape[3:], -np.inf, _F)
        den, acc = np.zeros_like(mx), np.zeros_like(mx)
        for k in range(K):
            l, vv = _logit(lg, m, k), v[..., k, :]
            up = l > mx
            sc = _exp2_form(np.where(up, mx - l, _F(0)))                 # (-inf - l = -inf: exp2 gives 0, and 0 * 0 + 1 = 1)
            e = _exp2_form(np.where(up, _F(0), l - mx))
            den = np.where(up, den * sc + _F(1), den + e)
            acc = np.where(up, acc * sc + vv, acc + e * vv)
            mx = np.where(up, l, mx)
    return acc / den


def pool_restatement(form):
    return pool_scalar_f32 if form == "scalar" else pool_wave_f32 if form.startswith("wave") else pool_vec_f32

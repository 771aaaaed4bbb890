"""TEST INFRASTRUCTURE of the fused-shape tests: the error bound of the tile kernels of csrc/elo_fused.hip against the float64
statements of tests/fused_shapes_reference.py, DERIVED from the arithmetic include/elo.h documents and carried PER ELEMENT through the
layers and the pooling of a case.  No constant below comes from a measurement; before the GPU test trusts them,
tests/test_fused_shapes_cpu.py holds a float32 emulation of the arithmetic -- a k-block summed as the bound models a matrix
instruction -- within the bound with every rounding unit HALVED (half the bound for split products; for half products the fp16
rounding flips stay whole steps), and a plain sequential float32 accumulation within the full bound, where it uses up to 0.8 of it
for half products: u_half has that much room and no more, and rests on the instruction summing no worse than the model below.

U = 2^-24 is the unit roundoff of fp32, H = 2^-11 that of fp16.

ONE LAYER  y = act(x @ W + b), the kernel's input x' within e_x of the statement's x (element-wise):

    |dy| <= e_x @ |W| + u * (|x| @ |W| + |b|) + floor                                                          (1)

SPLIT products (ELO_PRODUCTS_SPLIT; the CHECKED instances compute the same numbers), u = u_split(Kp) = (28 + 5 + 3 * steps) U:
  * the activation is split into fp16 hi + lo by two round-toward-zero conversions (pack_quad / act_put): |x - hi| < 2^-10 |x|,
    |lo - rtz(lo)| < 2^-10 |lo|, so x = hi + lo to 2^-20 |x| = 16 U |x| -- or to 2^-23 where lo (or a tiny x itself) falls below
    the fp16 normal range, whose spacing is 2^-24 (twice: hi and lo of an |x| < 2^-14).  An fp16 input (fp16 storage) is exact;
  * a weight is split by two round-to-nearest conversions (fused.PackedDense): w = hi + lo to 2^-22 |w| = 4 U |w|, or to 2^-25
    (half a subnormal spacing);
  * the three products hi*hi + lo*hi + hi*lo drop lo*lo: |x_lo| |w_lo| <= 2^-10 |x| * 2^-11 |w| = 8 U |x| |w|;
  * every fp16 x fp16 product is exact in fp32.  A matrix instruction adds the products of its k-block (32 k, or 16 k for the
    tail) to the accumulator, which starts as the bias.  The instruction's internal summation is modelled as a binary tree in
    fp32 or better: 5 levels for 32 terms, each rounding relative to the magnitudes below it -- and since the blocks partition
    the terms, 5 U * sum|terms| over the whole layer -- plus ONE rounding of the updated accumulator, whose magnitude is at
    most sum|terms| + |b|.  Only the hi*hi instruction carries terms large enough for its tree to matter (the other two
    are 2^-10 of it: their tree is inside the roundings already counted), all three round the accumulator: with
    steps = ceil(Kp / 32) k-blocks, (5 + 3 * steps) U.  The vendor does not document the tree: if a measured error ever exceeds
    the bound with everything else in order, this line of the derivation is what it says something about.
  floor = FLOOR_X * colsum|W| + 2^-25 * rowsum|x| restates the two subnormal floors; FLOOR_X = 2^-23 only where |x| < 2^-3,
  i.e. it is applied as max(16 U |x|, 2^-23) per element.
HALF products (ELO_PRODUCTS_HALF), u = u_half(Kp) = (5 + steps) U: the statement rounds the operands itself; what is left is the
  one product's accumulation.  But the kernel rounds ITS input x' to fp16, and x' is not the statement's x: by monotonicity of
  rounding |rn16(x') - rn16(x)| <= max(rn16(x + e_x) - rn16(x), rn16(x) - rn16(x - e_x)) -- zero where no rounding boundary lies
  within e_x of x, one fp16 spacing where one does.  That quantity replaces e_x in (1) (flip_bound below).
Both stay below what tests/test_ops_gpu.py asserts of one layer (1e-5 resp. 2e-6 of sum|terms|) up to Kp = 256: asserted on the CPU.
Second-order terms (e_x times the relative errors above) are covered by the factor (1 + 2^-9) on the e_x term.

ReLU and the masked maximum are 1-Lipschitz and monotone: a bound passes through them unchanged (the maximum of K bounded values
is bounded by the largest of their bounds).

THE MASKED SOFTMAX POOL  out = sum_k w_k v_k, w = softmax over the K slots of l_k (the masked constant where a slot is clear):
  * the kernel's values are off by dv_k, its logits by dl_k (clear slots: dl = 0, the constant is exact).  A weight moves by the
    factor exp(dl_k - dl_ref) - 1, and the normalisation divides the common part out: to first order
        sum_k w_k |dv_k| + 2 max|dl| * sum_k w_k |v_k - out|,
    multiplied by (1 + 4 max|dl|) for the second order while max|dl| < 1/8; a point whose logits are less certain than that gets the
    trivial bound of a convex combination, max_k |v_k - out| + max_k |dv_k|.  max|dl| runs over the slots that can carry weight
    at all: those within 87 of the maximum after the bounds are applied (below that an fp32 exponential is under 2^-125; such
    slots cost at most K * 2^-125 * (max|v| + |out|), added as an absolute term);
  * the hardware exponential exp2(x * log2 e) of x = fl(l_k - max): the subtraction moves the argument by U |x|, the
    instruction is good to 1 ulp = 2 U: (|x| + 2) U relative per weight; the rounded constant log2 e and the rounded product
    move the argument by another 2 U |x| log2 e, the weight by 2 U |x|: in all (3 |x| + 2) U per weight, times |v_k - out|;
  * the sums: a term's product e_k v_k rounds once, a chunk of 8 slots adds sequentially (at most min(K, 8) roundings), every
    chunk merge multiplies and adds (2 per chunk, ceil(K / 8) chunks; the two rescaling exponentials multiply numerator and
    denominator alike and cancel), the division rounds once: n_pool(K) = min(K, 8) + 2 ceil(K / 8) + 2 roundings, each relative
    to sum_k w_k (|v_k| + |out|).
STORAGE: the stored value is the kernel's fp32 value rounded once more: + 2^-11 (|want| + bound) + 2^-25 for fp16 (the last
term: half the subnormal spacing), + 2^-24 (|want| + bound) for fp32 (the accumulator IS the stored value; kept for the
statement's own float64 -> float32 conversion in the comparison)."""
import contextlib
import math

import numpy as np

from fused_shapes_reference import D, r16

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -9
ASSERTED_SPLIT, ASSERTED_HALF = 1e-5, 2e-6               # tests/test_ops_gpu.py, per layer, of sum|terms|


_SCALE = [1.0]


@contextlib.contextmanager
def units_scaled(factor):
    """`with units_scaled(0.5):` -- the bounds below with EVERY rounding unit of the kernel's arithmetic (fp32 roundings, the split's
    2^-20 and 2^-22, the subnormal floors, the exponential's ulp) multiplied by `factor`.  For split products that is the bound
    times the factor; for half products the fp16 rounding flips stay whole steps (a flip is discrete) but fewer values are within
    reach of one.  The CPU test holds the float32 emulation within the bound at factor 1/2."""
    _SCALE.append(float(factor))
    try:
        yield
    finally:
        _SCALE.pop()


def _s():
    return _SCALE[-1]


def steps_of(K):
    return math.ceil(((K + 15) // 16 * 16) / 32)


def u_split(K):
    return (16 + 4 + 8 + 5 + 3 * steps_of(K)) * U


def u_half(K):
    return (5 + steps_of(K)) * U


def flip_bound(x, e):
    """|rn16(x') - rn16(x)| for any x' within e of x (monotone rounding): element-wise, float64"""
    c = r16(x)
    return np.maximum(r16(x + e) - c, c - r16(x - e))


def split_error(ax):
    """|x - (hi + lo)| of an activation of magnitude ax split toward zero into two fp16 values"""
    return _s() * np.maximum(16 * U * ax, 2.0 ** -23)


def layer_bound(step, e_x, mode, exact_input=False):
    """Bound (1) on one layer's output.  exact_input: True, or a boolean per input column, where the kernel's operand is an fp16
    value read from fp16 storage (no split).  step: (operand input, operand W, b, relu) as tests/fused_shapes_reference.chain records it
    (half: the ROUNDED operands); e_x: the bound on the kernel's own input against the statement's PRE-rounding input, which for
    mode "half" must already have gone through flip_bound (chain_bound does that)."""
    x, W, b, _relu = step
    ax, aW = np.abs(x), np.abs(W)
    terms = ax @ aW + np.abs(b)
    if mode == "half":
        return SECOND_ORDER * (e_x @ aW) + _s() * u_half(x.shape[-1]) * terms
    K = x.shape[-1]
    split_x = np.where(np.logical_or(exact_input, ax == 0), 0.0, split_error(ax))   # (an exact 0 is stored as a zero quad)
    u_rest = _s() * (4 + 8 + 5 + 3 * steps_of(K)) * U
    return SECOND_ORDER * (e_x @ aW) + split_x @ aW + u_rest * terms + _s() * 2.0 ** -25 * ax.sum(-1, keepdims=True)


def chain_bound(steps, pre_inputs, e_in, mode, exact_input=False):
    """Carry a bound through the layers of one chain.  steps: the chain's records; pre_inputs[l]: layer l's input BEFORE the
    statement rounded it (mode half: needed for the flip bound; the chain's own x and the previous layers' outputs);
    e_in: bound on the kernel's first input.  Returns the bound on the chain's output."""
    e = e_in
    for l, step in enumerate(steps):
        if mode == "half":
            e = flip_bound(pre_inputs[l], e)
        e = layer_bound(step, e, mode, exact_input if l == 0 else False)
    return e


def _chain(steps, first_input, e_in, mode, exact_input=False):
    return chain_bound(steps, [first_input] + outputs_of(steps)[:-1], e_in, mode, exact_input)


# ---------------------------------------------------------------------------- a case's statement and its bound, together
def _mode(products):
    return "half" if products == "half" else "split"     # (checked: the split arithmetic)


def mlp_expect(R, inp, products, storage, first_stage=None, stored=True):
    """(want, bound) of a row-wise MLP's `out` (stored=False: of the kernel's fp32 value, before the storage rounding), or -- first_stage: the product's own stored `out`, float64 -- of its `out2`:
    the second stage is checked on what the first one left in HBM (in fp16 storage the tile continues with the stored halves;
    in fp32 storage the stored value IS the accumulator the tile continues with)."""
    half, f16 = products == "half", storage == "f16"
    if first_stage is None:
        ref = R.mlp(inp["sources"], inp["layers"], half)
    else:
        ref = R.mlp_stage2(first_stage, inp.get("before"), inp.get("after"), inp["layers2"], half)
    bound = _chain(ref["steps"], ref["input"], np.zeros_like(ref["input"]), _mode(products), f16)
    return ref["out"], storage_bound(ref["out"], bound, f16) if stored else bound


def _geometry_error(geo):
    """the kernel's own rounding of the 10 geometry columns [p | g*m | g*m - p | norm]: copies, one subtraction, 4 U on the norm
    (tests/forward_forms_bounds.py derives the 4)"""
    e = np.zeros_like(geo)
    e[..., 6:9] = _s() * U * np.abs(geo[..., 6:9])
    e[..., 9] = _s() * 4 * U * np.abs(geo[..., 9])
    return e


def setconv_expect(R, inp, centre, idx, mask, products, storage, stored=True):
    """(want, bound) of a set-conv's pooled output on the given slots"""
    half, f16 = products == "half", storage == "f16"
    ref = R.setconv(centre, inp["src_xyz"], inp["src_feat"], idx, mask, inp["layers"], half)
    x = ref["input"]
    e_in = np.zeros_like(x)
    e_in[..., :3] = _s() * U * np.abs(x[..., :3])                # x*m - c: one rounded subtraction
    exact = np.arange(x.shape[-1]) >= 3 if f16 else False
    rows = _chain(ref["steps"], x, e_in, _mode(products), exact)
    bound = (rows * np.asarray(mask, D)[..., None]).max(axis=2)       # a clear slot contributes an exact 0
    return ref["out"], storage_bound(ref["out"], bound, f16) if stored else bound


def _values_error(values_pre, e, products, stored_exact):
    """the pool reads its values from an operand-format region: hi + lo (split), or the rounded half"""
    if products == "half":
        return flip_bound(values_pre, e)
    return e + (0.0 if stored_exact else np.where(values_pre == 0, 0.0, split_error(np.abs(values_pre))))


def _pool_expect(ref, mask, e_logits, e_values, f16, stored):
    bound = softmax_pool_bound(ref["w"], ref["shifted"], ref["values"], ref["out"], mask, e_logits, e_values)
    weighing = ref["shifted"] >= -87.0
    return ref["out"], storage_bound(ref["out"], bound, f16) if stored else bound, float(np.abs(np.where(weighing, ref["shifted"], 0.0)).max())


def cv1_expect(R, inp, products, storage, stored=True):
    """(want, bound, max |l - max| over the slots that carry weight) of cost-volume stage 1"""
    half, f16, mode = products == "half", storage == "f16", _mode(products)
    ref = R.cv_stage1(inp["xyz1"], inp["feat1"], inp["xyz2"], inp["feat2"], inp["idx"], inp["mask"], inp["layers"], half)
    e_geo = _geometry_error(ref["geo"])
    e_cat = np.concatenate([e_geo, np.zeros(ref["cat"].shape[:-1] + (ref["cat"].shape[-1] - 10,))], -1)
    exact = np.arange(ref["cat"].shape[-1]) >= 10 if f16 else False
    e_x = _chain(ref["steps_x"], ref["cat"], e_cat, mode, exact)
    e_enc = _chain(ref["steps_e"], ref["geo"], e_geo, mode)
    both = np.concatenate([ref["enc"], ref["x"]], -1)
    e_logits = _chain(ref["steps_l"], both, np.concatenate([e_enc, e_x], -1), mode)
    return _pool_expect(ref, inp["mask"], e_logits, _values_error(ref["x"], e_x, products, False), f16, stored)


def cv2_expect(R, inp, products, storage, stored=True):
    """(want, bound, max |l - max| over the slots that carry weight) of cost-volume stage 2"""
    half, f16, mode = products == "half", storage == "f16", _mode(products)
    ref = R.cv_stage2(inp["xyz1"], inp["feat1"], inp["cost"], inp["idx"], inp["mask"], inp["layers"], half)
    e_geo = _geometry_error(ref["geo"])
    e_enc = _chain(ref["steps_e"], ref["geo"], e_geo, mode)
    both = ref["both"]
    e_both = np.concatenate([e_enc, np.zeros(both.shape[:-1] + (both.shape[-1] - 64,))], -1)
    exact = np.arange(both.shape[-1]) >= 64 if f16 else False
    e_logits = _chain(ref["steps_l"], both, e_both, mode, exact)
    grouped = both[..., -64:]
    return _pool_expect(ref, inp["mask"], e_logits, _values_error(grouped, np.zeros_like(grouped), products, f16), f16, stored)


def outputs_of(steps):
    """the (post-activation, unrounded) output of every layer of a chain, recomputed from its records"""
    outs = []
    for x, W, b, relu in steps:
        y = x @ W + b
        outs.append(np.maximum(y, 0.0) if relu else y)
    return outs


def n_pool(K):
    return min(K, 8) + 2 * math.ceil(K / 8) + 2


def softmax_pool_bound(ref_w, shifted, values, out, mask, e_logits, e_values):
    """Bound on the pooled output.  ref_w, shifted, values: (B,n,K,64) weights, l - max and values of the statement; out (B,n,64);
    mask (B,n,K); e_logits / e_values: the bounds on the kernel's logits and values."""
    live_mask = (np.asarray(mask)[..., None] == 1.0)
    dl = np.where(live_mask, e_logits, 0.0)
    # slots that can carry weight in the kernel: within 87 of the maximum once both are moved by their bounds
    dl_at_max = np.where(shifted == 0.0, dl, 0.0).max(axis=2, keepdims=True)
    can = shifted + dl + dl_at_max >= -87.0
    dlmax = np.where(can, dl, 0.0).max(axis=2)                                   # (B,n,64)
    spread = np.abs(values - out[:, :, None, :])
    first = (ref_w * e_values).sum(2) + 2 * dlmax * (ref_w * spread).sum(2)
    first = first * (1 + 4 * dlmax)
    trivial = spread.max(axis=2) + e_values.max(axis=2)
    soft = np.where(dlmax < 0.125, np.minimum(first, trivial), trivial)
    ax = np.where(can, np.abs(shifted), 0.0)
    exp_term = _s() * U * (ref_w * (3 * ax + 2) * spread).sum(2)
    K = values.shape[2]
    scale = (ref_w * (np.abs(values) + np.abs(out)[:, :, None, :])).sum(2)
    sums = _s() * n_pool(K) * U * scale
    tiny = _s() * K * 2.0 ** -125 * (np.abs(values).max(axis=2) + np.abs(out))
    return soft + exp_term + sums + tiny


def storage_bound(want, bound, f16):
    want = np.abs(want)
    return bound + (2.0 ** -11 * (want + bound) + 2.0 ** -25 if f16 else U * (want + bound))


# ---------------------------------------------------------------------------- float32 emulation of the two product schemes (CPU)
_F = np.float32


def _rtz16(x):
    """fp32 -> fp16 toward zero (v_cvt_pkrtz), as fp32"""
    x = np.asarray(x, _F)
    h = x.astype(np.float16)
    hf = h.astype(_F)
    over = np.abs(hf) > np.abs(x)
    toward = np.nextafter(h, np.float16(0)).astype(_F)
    out = np.where(over, toward, hf)
    return np.where(np.isinf(out), np.sign(x) * _F(65504.0), out).astype(_F)


def emulate_layer(x, layer, mode, exact_input=False, sequential=False, drop_w_lo=False):
    """One layer as the tile kernels compute it, in float32 numpy: operands split into fp16 hi + lo (activations toward zero,
    weights to nearest), the three products hi*hi + lo*hi + hi*lo (half: the one product of the rounded operands), k-blocks of
    32 accumulated in fp32 on top of the bias.  (A plain float32 matmul per block -- 31 sequential roundings instead of the tree the
    bound models -- stays inside the bound too, at up to 0.8 of it for half products; it is the model that is emulated here.)
    drop_w_lo: a WRONG split scheme that leaves out the product with the weights' lo half (a mistake of 2^-12 of a term): the
    CPU tests show with it that the bound tells such a mistake from rounding."""
    W, b, relu = layer
    x, W = np.asarray(x, _F), np.asarray(W, _F)
    K, N = W.shape
    Kp = (K + 15) // 16 * 16
    xp = np.zeros(x.shape[:-1] + (Kp,), _F)
    xp[..., :K] = x
    Wp = np.zeros((Kp, N), _F)
    Wp[:K] = W
    acc = np.broadcast_to(np.asarray(b, _F), x.shape[:-1] + (N,)).copy()
    if mode == "half":
        xh, wh = xp.astype(np.float16).astype(_F), Wp.astype(np.float16).astype(_F)
        parts = [(wh, xh)]
    else:
        xh = xp if exact_input else _rtz16(xp)
        xl = np.zeros_like(xp) if exact_input else _rtz16(xp - xh)
        wh = Wp.astype(np.float16).astype(_F)
        wl = (Wp - wh).astype(np.float16).astype(_F)
        parts = [(wh, xh), (wh, xl)] if drop_w_lo else [(wh, xh), (wl, xh), (wh, xl)]
    for k0 in range(0, Kp, 32):                          # one matrix instruction per product and k-block, as (1) models it: the
        for w_, x_ in parts:                             # block's exact products summed and rounded once, then added in fp32
            if sequential:                               # (a plain float32 sum of the block's products, one rounding per term)
                block = np.zeros_like(acc)
                for k in range(k0, min(k0 + 32, Kp)):
                    block = (block + x_[..., k:k + 1] * w_[k]).astype(_F)
            else:
                block = (x_[..., k0:k0 + 32].astype(D) @ w_[k0:k0 + 32].astype(D)).astype(_F)
            acc = (acc + block).astype(_F)
    return np.maximum(acc, _F(0)) if relu else acc


def emulate_chain(x, layers, mode, exact_input=False, sequential=False, drop_w_lo=False):
    for l, layer in enumerate(layers):
        x = emulate_layer(x, layer, mode, exact_input and l == 0, sequential, drop_w_lo)
    return x

"""GPU: EVERY dispatch form of every training backward kernel (csrc/elo_backward.hip, through the autograd Functions of _ops.py)
against float64 autograd over tests/twins_torch.py, with the inputs where such kernels go wrong: exact ties in the max-pool (post-ReLU
zeros, a channel equal on all K slots, all-masked points, points whose masked +-0 beats every valid product), softmax pools with
all-masked points, a single valid slot, a masked logit above every valid one and exponentials that underflow, softmax_valid at every
partial-sum split, and gathers whose atomics pile up on a few hot cells.  Each case is built to reach ONE form, named in its id:
  masked_maxpool     bwd_vec<K> (K 4/8/16/32; C % 4 == 0; x, grad_out, grad_x 16-byte aligned) | bwd (scalar: any other case)
                     fwd_vec (C % 4 == 0, x and out aligned, any K) | fwd (scalar)
  masked_softmax_pool bwd_vec<K> (K 4/6/8), bwd_vec2<K> (K 16/32; C and values stride % 4 == 0, all aligned) | bwd (scalar)
  softmax_valid      bwd_elementwise (C % 4 == 0: the forward's merged (max, denominator)) | bwd_block (C % 4 != 0)
Also: the forms that the source says give the same bits do (torch.equal on one input run through both)."""
import numpy as np
import pytest
import torch

import twins_torch as twin
from backward_check import _boundary_safe_points, _check
from conftest import load_pkg
from forms_inputs import at_offset as _at_offset                   # (4 bytes past a 16-byte boundary: the kernels' scalar forms)
from forms_inputs import cv_encode1_inputs, cv_encode2_inputs
from forms_inputs import maxpool_inputs as _maxpool_inputs
from forms_inputs import slots as _slots
from forms_inputs import softmax_pool_inputs as _softmax_pool_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- masked max-pool
MAXPOOL_BWD = [pytest.param(K, C, False, id="bwd_vec<%d>-K%d-C%d" % (K, K, C)) for K, C in
               ((4, 16), (4, 128), (8, 32), (8, 64), (16, 64), (16, 16), (32, 128), (32, 32))]
MAXPOOL_BWD += [pytest.param(K, C, False, id="bwd_scalar-K%d-C%d" % (K, C)) for K, C in
                ((1, 64), (5, 64), (6, 32), (9, 16), (8, 3), (16, 6), (32, 3))]
MAXPOOL_BWD += [pytest.param(8, 64, True, id="bwd_scalar-K8-C64-x_at_4_byte_offset")]


@pytest.mark.parametrize("K,C,offset", MAXPOOL_BWD)
def test_masked_maxpool_backward(K, C, offset):
    ops = load_pkg("_ops")
    rng = np.random.default_rng(K * 1000 + C)
    x, m = _maxpool_inputs(rng, 2, 301, K, C)
    hip = (lambda x_, m_: ops.masked_maxpool(_at_offset(x_), m_)) if offset else ops.masked_maxpool
    _check(hip, twin.masked_maxpool, [t(x), t(m)], wrt=[0])


@pytest.mark.parametrize("K,C,offset", [pytest.param(K, C, o, id="%s-K%d-C%d%s" % ("fwd_scalar" if o or C % 4 else "fwd_vec", K, C,
                                                                                       "-x_at_4_byte_offset" if o else ""))
                                        for K in (1, 6, 8, 9, 16, 32) for C, o in ((64, False), (64, True), (6, False))])
def test_masked_maxpool_forward(K, C, offset):
    """The products are x * {0, 1} and the maximum is a selection: the forward is exact, in either form."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(K * 77 + C)
    x, m = _maxpool_inputs(rng, 2, 301, K, C)
    xt = _at_offset(t(x)) if offset else t(x)
    got = ops.masked_maxpool(xt, t(m))
    assert torch.equal(got.double(), twin.masked_maxpool(t(x).double(), t(m).double()))


@pytest.mark.parametrize("K", [8, 16, 32], ids=lambda k: "vec_vs_scalar-K%d" % k)
def test_masked_maxpool_forms_give_the_same_bits(K):
    """elo_features.hip (masked_maxpool_vec_kernel) and elo_backward.hip (masked_maxpool_bwd_vec_kernel): same bits as the scalar
    forms.  One input, once in an aligned buffer (vector forms) and once 4 bytes into its buffer (scalar forms)."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(K)
    x, m = _maxpool_inputs(rng, 2, 301, K, 64)
    go = t(rng.normal(0, 1, (2, 301, 64)).astype(np.float32))
    res = []
    for shift in (False, True):
        leaf = t(x).requires_grad_(True)
        out = ops.masked_maxpool(_at_offset(leaf) if shift else leaf, t(m))
        (g,) = torch.autograd.grad(out, [leaf], go)
        res.append((out.detach(), g))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------------- masked softmax pool
SOFTMAX_BWD = [pytest.param(K, 64, None, id="bwd_%s<%d>-K%d-C64" % ("vec2" if K > 8 else "vec", K, K)) for K in (4, 6, 8, 16, 32)]
SOFTMAX_BWD += [pytest.param(K, 64, (96, 32), id="bwd_%s<%d>-K%d-C64-values_wide96[32:96]" % ("vec2" if K > 8 else "vec", K, K))
                for K in (4, 6, 8, 16, 32)]
SOFTMAX_BWD += [pytest.param(5, 64, None, id="bwd_scalar-K5-C64"), pytest.param(8, 6, None, id="bwd_scalar-K8-C6"),
                pytest.param(6, 64, (98, 0), id="bwd_scalar-K6-C64-values_wide98[0:64]"),
                pytest.param(32, 64, (98, 17), id="bwd_scalar-K32-C64-values_wide98[17:81]"),
                pytest.param(4, 64, (96, 1), id="bwd_scalar-K4-C64-values_wide96[1:65]")]


@pytest.mark.parametrize("K,C,wide", SOFTMAX_BWD)
def test_masked_softmax_pool_backward(K, C, wide):
    """wide = (width, first): values are channels first..first+C of a `width`-channel tensor (a slice, not a copy)."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(K * 100 + C)
    lg, v, m = _softmax_pool_inputs(rng, 2, 301, K, C, wide[0] if wide else None)
    mt = t(m)
    if wide is None:
        _check(ops.masked_softmax_pool, twin.masked_softmax_pool, [t(lg), t(v), mt], wrt=[0, 1])
        return
    s = slice(wide[1], wide[1] + C)
    _check(lambda l, w_: ops.masked_softmax_pool(l, w_[..., s], mt), lambda l, w_: twin.masked_softmax_pool(l, w_[..., s], mt.double()),
           [t(lg), t(v)], wrt=[0, 1])


@pytest.mark.parametrize("K", [4, 6, 32], ids=lambda k: "vec%s_vs_scalar-K%d" % ("2" if k > 8 else "", k))
def test_masked_softmax_pool_backward_forms_give_the_same_bits(K):
    """elo_backward.hip (softmax_pool_bwd_vec_kernel, softmax_pool_bwd_vec2_kernel): same bits as the scalar form.  The values once
    in an aligned buffer, once 4 bytes into theirs."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(K + 5)
    lg, v, m = _softmax_pool_inputs(rng, 2, 301, K, 64)
    go = t(rng.normal(0, 1, (2, 301, 64)).astype(np.float32))
    res = []
    for shift in (False, True):
        a = [t(lg).requires_grad_(True), t(v).requires_grad_(True)]
        out = ops.masked_softmax_pool(a[0], _at_offset(a[1]) if shift else a[1], t(m))
        res.append(torch.autograd.grad(out, a, go))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------------- softmax_valid
def _sv_inputs(rng, B, N, C):
    """Feature / weight (B,N,C) and a cloud whose zero points are invalid: 20 % at random; with B >= 3 element 0 has no valid
    point, element 1 exactly one and element 2 valid points only among the last 20 (the last partial sum's rows)."""
    f = rng.normal(0, 1, (B, N, C)).astype(np.float32)
    w = (3 * rng.normal(0, 1, (B, N, C))).astype(np.float32)
    xyz = rng.normal(0, 10, (B, N, 3)).astype(np.float32)
    xyz[rng.random((B, N)) < 0.2] = 0
    xyz[:, 0] += 1                                                   # (at least one valid point per element ...)
    if B >= 3:                                                       # (... but these)
        xyz[0] = 0
        xyz[1] = 0
        xyz[1, N // 2] = (1.0, -2.0, 0.5)
        xyz[2, :max(N - 20, 0)] = 0
    return f, w, xyz


SV_BWD = [pytest.param(B, N, 64, id="bwd_elementwise-B%d-N%d-C64" % (B, N)) for B in (1, 8) for N in (1, 63, 64, 65, 904, 4096, 4097, 14400)]
SV_BWD += [pytest.param(B, N, C, id="bwd_block-B%d-N%d-C%d" % (B, N, C)) for B, N, C in ((8, 904, 6), (1, 65, 6), (8, 4097, 66), (2, 63, 66))]


@pytest.mark.parametrize("B,N,C", SV_BWD)
def test_softmax_valid_backward(B, N, C):
    ops = load_pkg("_ops")
    rng = np.random.default_rng(B * 100000 + N + C)
    f, w, xyz = _sv_inputs(rng, B, N, C)
    # one point: the softmax weight is 1 and out = f, so d/dweight = s (f - out) g is 0 exactly -- only the feature has a gradient
    _check(ops.softmax_valid, twin.softmax_valid, [t(f), t(w), t(xyz)], wrt=[0] if N == 1 else [0, 1])


# ---------------------------------------------------------------------------------------------------------------- gathers
GC_WRT = [[0], [1], [2], [0, 1], [0, 2], [1, 2], [0, 1, 2]]


@pytest.mark.parametrize("C", [3, 16, 64], ids=lambda c: "C%d" % c)
@pytest.mark.parametrize("H,W,H2,W2,K,masked_at", [pytest.param(8, 113, 16, 225, 16, "origin", id="bwd-down-src16x225-K16"),
                                                   pytest.param(8, 113, 16, 225, 32, "anywhere", id="bwd-down-src16x225-K32-masked_anywhere"),
                                                   pytest.param(16, 225, 8, 113, 8, "origin", id="bwd-up-src8x113-K8")])
def test_group_concat_backward(H, W, H2, W2, K, masked_at, C):
    """group_concat_bwd_kernel with centres off the source grid (strided set-conv centres, finer set-upconv centres), every subset of
    the inputs wanting a gradient (the null-pointer branches)."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(H2 * 10 + K + C)
    B, N = 2, H * W
    idx, m = _slots(rng, B, N, K, H2, W2, masked_at)
    centre = rng.normal(0, 5, (B, N, 3)).astype(np.float32)
    sx = rng.normal(0, 5, (B, H2, W2, 3)).astype(np.float32)
    sf = rng.normal(0, 1, (B, H2, W2, C)).astype(np.float32)
    for wrt in GC_WRT:
        _check(ops.group_concat, twin.group_concat, [t(centre), t(sx), t(sf), t(idx), t(m)], wrt=wrt)


CV_CASES = [pytest.param(8, 4, 57, 4, 16, [0, 1, 2, 3], id="bwd-B8-4x57-K4-C16"), pytest.param(2, 8, 113, 6, 64, [0, 2], id="bwd-B2-8x113-K6-C64"),
            pytest.param(2, 8, 113, 32, 16, [1, 3], id="bwd-B2-8x113-K32-C16"), pytest.param(8, 4, 57, 32, 64, [2, 3], id="bwd-B8-4x57-K32-C64"),
            pytest.param(1, 8, 113, 6, 16, [0], id="bwd-B1-8x113-K6-C16")]


@pytest.mark.parametrize("B,H,W,K,C,wrt", CV_CASES)
def test_cv_encode1_backward(B, H, W, K, C, wrt):
    """cv_encode1_bwd_kernel: centres anywhere (N = 2 H W), neighbours on the H x W grid; the first slot of every 5th centre sits ON
    the centre (d = 0: the norm's gradient is 0 / 1e-10)."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(B * 1000 + K + C)
    xyz1, f1, xyz2, f2, idx, m = cv_encode1_inputs(rng, B, 2 * H * W, H, W, K, C, "anywhere" if K == 32 else "origin")
    _check(ops.cv_encode1, twin.cv_encode1, [t(xyz1), t(f1), t(xyz2), t(f2), t(idx), t(m)], wrt=wrt)


@pytest.mark.parametrize("B,H,W,K,C,wrt", [pytest.param(*p.values[:5], [i for i in p.values[5] if i < 3] or [2], id=p.id) for p in CV_CASES])
def test_cv_encode2_backward(B, H, W, K, C, wrt):
    """cv_encode2_bwd_kernel: centres are the grid's own pixels; the first slot of every 5th pixel is the pixel itself (d = 0)."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(B * 1000 + K + C + 1)
    xyz, f1, cost, idx, m = cv_encode2_inputs(rng, B, H, W, K, C, masked_at="anywhere" if K == 6 else "origin")
    _check(ops.cv_encode2, twin.cv_encode2, [t(xyz), t(f1), t(cost), t(idx), t(m)], wrt=wrt)


# ---------------------------------------------------------------------------------------------------------------- re-projection
@pytest.mark.parametrize("B,H,W,C", [pytest.param(1, 4, 57, 64, id="B1-4x57-C64"), pytest.param(8, 16, 225, 32, id="B8-16x225-C32")])
@pytest.mark.parametrize("warped", [True, False], ids=["bwd-warped", "bwd-q_none"])
def test_warp_project_backward(B, H, W, C, warped):
    """warp_project_bwd_kernel: to the features, the cloud and, warped, the pose; near-identity poses and border-safe points so that
    the double-precision twin puts every point in the kernel's cell.  Zero points only in the warped case (see test_backward_gpu)."""
    ops = load_pkg("_ops")
    rng = np.random.default_rng(B * 10 + H + int(warped))
    N = H * W
    pc = _boundary_safe_points(rng, B, N, H, W)
    feat = rng.normal(0, 1, (B, N, C)).astype(np.float32)
    if not warped:
        _check(lambda x, f: ops.warp_project(x, f, None, None, H, W), lambda x, f: twin.warp_project(x, f, None, None, H, W),
               [t(pc), t(feat)], wrt=[0, 1])
        return
    pc[rng.random((B, N)) < 0.1] = 0
    q = np.concatenate([np.ones((B, 1)), rng.uniform(-3e-4, 3e-4, (B, 3))], 1).astype(np.float32)
    tt = rng.uniform(-0.02, 0.02, (B, 3)).astype(np.float32)
    _check(lambda x, f, q_, t_: ops.warp_project(x, f, q_, t_, H, W), lambda x, f, q_, t_: twin.warp_project(x, f, q_, t_, H, W),
           [t(pc), t(feat), t(q), t(tt)], wrt=[0, 1, 2, 3], tol=2e-4)

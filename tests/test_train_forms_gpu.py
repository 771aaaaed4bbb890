"""GPU: every launch form of the training-layer row kernels of csrc/elo_train.hip against float64, case by case of
tests/train_forms_cases.py, at the bounds tests/train_forms_bounds.py derives from operation counts (every tolerance below is one of
its bounds or constants): elo_bn_stats (both moment vectors, the moving averages), elo_bn_apply, elo_bn_backward (both sums, dz, the
dz = NULL form) and elo_dense_weight_grad (dW, db, with and without db) through L.call with the argument structs; forms that compute the
same chain of operations are compared bit for bit, and so are two calls of anything.  Small companions: elo_pose_compose, elo_pose_loss
and elo_adam_flat beyond one block / one trip.  On failure the message carries the largest share of a bound and where it was.
ELO_TRAIN_FORMS_REPORT=<file>: the worst share per kernel and form is written there (profiles/train_forms_errors.txt)."""
import collections
import os

import numpy as np
import pytest
import torch

import train_forms_bounds as bounds
import train_forms_cases as table
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = collections.OrderedDict()                       # (kernel, output, form) -> (share, case id)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ELO_TRAIN_FORMS_REPORT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# worst |got - float64| / bound per kernel, output and form (tests/test_train_forms_gpu.py; a share <= 1 passes)\n")
            for (kernel, output, form), (s, where) in WORST.items():
                f.write("%-22s %-7s %-14s %8.4f  %s\n" % (kernel, output, form, s, where))


def within(kernel, output, form, case_id, got, want, bound):
    """Assert |got - want| <= bound everywhere; the message (and the report) carry the largest share."""
    s, at = bounds.share(got, want, bound)
    key = (kernel, output, form)
    if key not in WORST or s > WORST[key][0]:
        WORST[key] = (s, case_id)
    print("%s %s %s: largest share of the bound %.4f at %s" % (kernel, output, case_id, s, at))
    assert s <= 1.0, "%s %s of %s: %.4g bounds at %s" % (kernel, output, case_id, s, at)


def dev(a, off=0):
    """A float32 device tensor of a numpy array; off = 4: a contiguous view 4 bytes into its storage."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if not off:
        return t.to(DEV)
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == off
    return view


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


ptr = lambda t: t.data_ptr() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def weight_grad(L, c, x, g, with_db=True):
    dW, db = nans(c.cin, c.cout), nans(c.cout) if with_db else None
    scratch = nans(L.lib().elo_weight_grad_slices(c.rows, c.cin, c.cout) * (c.cin * c.cout + c.cout))
    a = L.WeightGradArgs(c.rows, c.cin, c.cout, x.data_ptr(), g.data_ptr(), dW.data_ptr(), ptr(db), scratch.data_ptr())
    assert L.wgrad_form(a) == "%s@%dx%dw%d" % ((c.kernel,) + c.grid)                           # asked again with the real pointers
    L.call("elo_dense_weight_grad", a, x)
    return dW, db


@pytest.mark.parametrize("case", table.WGRAD, ids=table.wgrad_id)
def test_weight_grad_form_matches_float64(case):
    L = load_pkg("_lib")
    xn, gn = table.wgrad_inputs(case)
    x, g = dev(xn, case.x_off), dev(gn, case.g_off)
    dW, db = weight_grad(L, case, x, g)
    ref = bounds.wgrad_reference(xn, gn)
    cid = table.wgrad_id(case)
    within("elo_dense_weight_grad", "dW", case.kernel, cid, dW.cpu().numpy(), *ref["dW"])
    within("elo_dense_weight_grad", "db", case.kernel, cid, db.cpu().numpy(), *ref["db"])
    dW2, db2 = weight_grad(L, case, x, g)                                                      # no atomics: the same bits on every call
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    dW3, _ = weight_grad(L, case, x, g, with_db=False)                                         # db = NULL changes nothing of dW
    assert torch.equal(dW, dW3)


@pytest.mark.parametrize("rows", [5, 257, 4096])
def test_weight_grad_scalar_and_vector_loads_give_the_same_bits(rows):
    """Scalar and vector loads of an operand feed the same fmaf chain: (64, 64) aligned (x and g as vectors), x 4 bytes off (x one
    channel per tile) and g 4 bytes off give equal dW and db."""
    L = load_pkg("_lib")
    by_off = {(c.x_off, c.g_off): c for c in table.WGRAD if (c.cin, c.cout, c.rows) == (64, 64, rows)}
    assert sorted(by_off) == [(0, 0), (0, 4), (4, 0)] and len({c.kernel for c in by_off.values()}) == 3
    xn, gn = table.wgrad_inputs(by_off[(0, 0)])
    res = {off: weight_grad(L, c, dev(xn, c.x_off), dev(gn, c.g_off)) for off, c in by_off.items()}
    for off in ((4, 0), (0, 4)):
        assert torch.equal(res[off][0], res[(0, 0)][0]) and torch.equal(res[off][1], res[(0, 0)][1]), off


# --------------------------------------------------------------------------------------------------------------------- batch norm
def bn_stats(L, c, z, rm, rv):
    mean, invstd = nans(c.groups, c.C), nans(c.groups, c.C)
    rm, rv = (rm.clone(), rv.clone()) if c.running else (None, None)
    scratch = nans(L.lib().elo_bn_scratch_floats(c.C, c.groups))
    L.call("elo_bn_stats", L.BnStatsArgs(c.M * c.groups, c.C, z.data_ptr(), scratch.data_ptr(), float(table.BN_EPS), float(table.BN_MOMENTUM),
                                         mean.data_ptr(), invstd.data_ptr(), ptr(rm), ptr(rv), c.groups), z)
    return mean, invstd, rm, rv


def bn_apply(L, c, t):
    y = nans(*t["z"].shape)
    L.call("elo_bn_apply", L.BnApplyArgs(c.M * c.groups, c.C, t["z"].data_ptr(), t["mean"].data_ptr(), t["invstd"].data_ptr(), t["gamma"].data_ptr(),
                                         t["beta"].data_ptr(), c.relu, y.data_ptr(), c.groups), y)
    return y


def bn_backward(L, c, t, with_dz=True):
    sums, dz = nans(c.groups, 2, c.C), nans(*t["z"].shape) if with_dz else None
    scratch = nans(L.lib().elo_bn_scratch_floats(c.C, c.groups))
    L.call("elo_bn_backward", L.BnBackwardArgs(c.M * c.groups, c.C, t["dy"].data_ptr(), t["z"].data_ptr(), t["mean"].data_ptr(), t["invstd"].data_ptr(),
                                               t["gamma"].data_ptr(), t["beta"].data_ptr(), c.relu, scratch.data_ptr(), sums.data_ptr(), ptr(dz),
                                               c.groups), sums)
    return sums, dz


@pytest.mark.parametrize("case", table.BN, ids=table.bn_id)
def test_batch_norm_case_matches_float64(case):
    L = load_pkg("_lib")
    assert L.bn_parts(case.M, case.C) == table.bn_parts(case.M, case.C)
    i = table.bn_inputs(case)
    t = {k: dev(v) for k, v in i.items() if k != "tie"}
    cid, form = table.bn_id(case), "C%d/%s" % (case.C, case.edge)
    G, par = case.groups, (i["mean"], i["invstd"], i["gamma"], i["beta"], case.relu, case.groups)

    got = bn_stats(L, case, t["z"], t["rm"], t["rv"])
    ref = bounds.stats_reference(i["z"], G, table.BN_EPS, table.BN_MOMENTUM, *((i["rm"], i["rv"]) if case.running else ()))
    for name, g in zip(("mean", "invstd", "rm", "rv"), got):
        if g is not None:
            within("elo_bn_stats", name, form, cid, g.cpu().numpy(), *ref[name])
    assert all(a is b is None or torch.equal(a, b) for a, b in zip(got, bn_stats(L, case, t["z"], t["rm"], t["rv"])))

    y = bn_apply(L, case, t)
    within("elo_bn_apply", "y", form, cid, y.cpu().numpy(), *bounds.apply_reference(i["z"], *par))
    assert bool((y.cpu().numpy()[i["tie"]] == 0).all())                                        # a placed tie: exactly 0, with and without ReLU
    assert torch.equal(y, bn_apply(L, case, t))

    sums, dz = bn_backward(L, case, t)
    ref = bounds.backward_reference(i["dy"], i["z"], *par)
    within("elo_bn_backward", "sums", form, cid, sums.cpu().numpy(), *ref["sums"])
    within("elo_bn_backward", "dz", form, cid, dz.cpu().numpy(), *ref["dz"])
    sums2, dz2 = bn_backward(L, case, t)
    assert torch.equal(sums, sums2) and torch.equal(dz, dz2)
    sums3, _ = bn_backward(L, case, t, with_dz=False)                                          # dz = NULL: the same two launches
    assert torch.equal(sums, sums3)


def _big_inputs():
    """table.BN_BIG's tensors made on the device: as table.bn_inputs, placed ties included."""
    c = table.BN_BIG
    gen = torch.Generator(device=DEV).manual_seed(c.M)
    rn = lambda *s: torch.randn(*s, generator=gen, device=DEV, dtype=torch.float32)
    small = table.bn_inputs(table.Bn(c.C, 2, 1, c.relu, 0, "two"))                             # the per-channel vectors (ties in channels 0, 1)
    t = {k: dev(small[k]) for k in ("mean", "invstd", "gamma", "beta")}
    z, dy = rn(c.M, c.C) * 1.5 + 0.3, rn(c.M, c.C)
    z[:, :2] = (torch.round(rn(c.M, 2) * 8) / 8 + 0.5).clamp(-3, 4)
    z[::3, :2] = float(table.TIE_Z)
    tie = torch.zeros(z.shape, dtype=torch.bool, device=DEV)
    tie[:, :2] = z[:, :2] == float(table.TIE_Z)
    for _ in range(4):
        pre, bound = bounds.preactivation(z, t["mean"], t["invstd"], t["gamma"], t["beta"], 1)
        near = (pre.abs() <= 4 * bound) & ~tie
        if not bool(near.any()):
            break
        z[near] += 1.0
    pre, bound = bounds.preactivation(z, t["mean"], t["invstd"], t["gamma"], t["beta"], 1)
    assert bool((pre[tie] == 0).all()) and bool((pre[~tie].abs() > bound[~tie]).all()) and bool(tie[:, 0].any()) and bool(tie[:, 1].any())
    t.update(z=z, dy=dy)
    return c, t, tie


def test_bn_apply_beyond_the_block_cap():
    """131075 rows of 256 channels: 8193 blocks' worth of float4, launched on 8192 -- the grid stride wraps and the loop has a tail."""
    L = load_pkg("_lib")
    c, t, tie = _big_inputs()
    y = bn_apply(L, c, t)
    par = (t["mean"], t["invstd"], t["gamma"], t["beta"], c.relu, 1)
    within("elo_bn_apply", "y", "C256/blocks", table.bn_id(c), y, *bounds.apply_reference(t["z"], *par))
    assert bool((y[tie] == 0).all())


def test_bn_backward_beyond_the_block_cap():
    L = load_pkg("_lib")
    c, t, tie = _big_inputs()
    sums, dz = bn_backward(L, c, t)
    ref = bounds.backward_reference(t["dy"], t["z"], t["mean"], t["invstd"], t["gamma"], t["beta"], c.relu, 1)
    within("elo_bn_backward", "sums", "C256/blocks", table.bn_id(c), sums, *ref["sums"])
    within("elo_bn_backward", "dz", "C256/blocks", table.bn_id(c), dz, *ref["dz"])


# --------------------------------------------------------------------------------- the pose algebra and Adam beyond one block / trip
@pytest.mark.parametrize("coarse", [True, False])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_pose_compose_beyond_one_block(B, coarse):
    """elo_pose_compose on 64-thread blocks: one element, a full block, one element into the second, a third block with a tail."""
    from test_train_kernels_gpu import _literal_pose
    ops = load_pkg("_ops")
    rng = np.random.default_rng(B)
    mk = lambda *s: rng.normal(0, 1, s)
    inputs = (mk(B, 4) * 2.0, mk(B, 3)) + (() if coarse else (mk(B, 4), mk(B, 3) * 3.0))
    gq, gt, gqn = mk(B, 4), mk(B, 3), mk(B, 4)
    ins64 = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in inputs]
    want = _literal_pose(ins64[0], ins64[1], None if coarse else ins64[2], None if coarse else ins64[3])
    ((want[0] * torch.tensor(gq)).sum() + (want[1] * torch.tensor(gt)).sum() + (want[2] * torch.tensor(gqn)).sum()).backward()
    ins = [torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True) for x in inputs]
    got = ops.pose_compose(ins[0], ins[1], None if coarse else ins[2], None if coarse else ins[3])
    d = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)
    ((got[0] * d(gq)).sum() + (got[1] * d(gt)).sum() + (got[2] * d(gqn)).sum()).backward()
    for g, w in zip(got, want):
        assert float((g.detach().cpu().double() - w.detach()).abs().max()) <= bounds.POSE_VALUE_REL * max(1.0, float(w.detach().abs().max()))
    for a, b in zip(ins, ins64):
        assert float((a.grad.cpu().double() - b.grad).abs().max()) <= bounds.POSE_GRAD_REL * max(1e-3, float(b.grad.abs().max())), a.shape


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_pose_loss_beyond_one_trip(B):
    """elo_pose_loss is one wave: idle lanes in the butterfly (B = 1, 63), a full wave, and the e += 64 loop (65, 130: three trips)."""
    pm = load_pkg("pwclo_model")
    rng = np.random.default_rng(100 + B)
    poses = [rng.normal(0, 1, (B, 4 if i % 2 == 0 else 3)) for i in range(8)]
    q_gt, t_gt = rng.normal(0, 1, (B, 4)), rng.normal(0, 1, (B, 3, 1))
    p64 = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in poses]
    w64 = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (0.3, -2.5)]
    want = pm.get_loss(*p64, torch.tensor(q_gt), torch.tensor(t_gt), *w64)
    (want * 1.7).backward()
    p32 = [torch.tensor(x, dtype=torch.float32, device=DEV, requires_grad=True) for x in poses]
    w32 = [torch.tensor(v, dtype=torch.float32, device=DEV, requires_grad=True) for v in (0.3, -2.5)]
    got = pm.get_loss(*p32, torch.tensor(q_gt, dtype=torch.float32, device=DEV), torch.tensor(t_gt, dtype=torch.float32, device=DEV), *w32)
    (got * 1.7).backward()
    assert abs(float(got.detach()) - float(want.detach())) <= bounds.LOSS_VALUE_REL * abs(float(want.detach()))
    for a, b in zip(p32 + w32, p64 + w64):
        assert float((a.grad.cpu().double() - b.grad).abs().max()) <= bounds.POSE_GRAD_REL * max(1e-4, float(b.grad.abs().max()))


@pytest.mark.parametrize("n", [1, 3, 1025, 1026, 1027])
def test_adam_flat_one_step_matches_float64(n):
    """elo_adam_flat on 256-thread blocks of float4: a lone scalar tail, a second block of one full quad + a tail of 1, 2, 3."""
    L = load_pkg("_lib")
    rng = np.random.default_rng(n)
    f = np.float32
    p, g, m = (rng.normal(0, 1, n).astype(f) for _ in range(3))
    v = (rng.normal(0, 1, n) ** 2).astype(f)
    b1, b2, lr, eps, t = 0.9, 0.999, 1e-3, 1e-8, 3
    hyper = np.array([lr / (1 - b1 ** t), 1 / np.sqrt(1 - b2 ** t), eps, 0], f)
    T = [dev(a) for a in (p, g, m, v, hyper)]
    before = T[1].clone()
    L.call("elo_adam_flat", L.AdamFlatArgs(n, T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), T[3].data_ptr(), T[4].data_ptr(), b1, b2, 1 - b1, 1 - b2), T[0])
    d = lambda a: np.asarray(a, np.float64)
    c = lambda x: float(f(x))                                                   # the scalars as the kernel receives them
    m64 = c(b1) * d(m) + c(1 - b1) * d(g)
    v64 = c(b2) * d(v) + c(1 - b2) * d(g) * d(g)
    p64 = d(p) - float(hyper[0]) * (m64 / (np.sqrt(v64) * float(hyper[1]) + float(hyper[2])))
    assert torch.equal(T[1], before)
    assert np.abs(T[0].cpu().numpy() - p64).max() <= bounds.ADAM_PARAM_REL * max(1.0, np.abs(p64).max())
    assert np.abs(T[2].cpu().numpy() - m64).max() <= bounds.ADAM_MOMENT_REL * max(1e-3, np.abs(m64).max())
    assert np.abs(T[3].cpu().numpy() - v64).max() <= bounds.ADAM_MOMENT_REL * max(1e-3, np.abs(v64).max())

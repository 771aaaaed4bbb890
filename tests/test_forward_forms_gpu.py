"""GPU: EVERY forward form of the per-operator feature kernels (csrc/elo_features.hip, through _ops.py) against the float64
restatement of tests/twins_torch.py on the same inputs.  The cases are the table of tests/forward_forms_cases.py; each is asked a
second time, with the call's real pointers, which kernel it launches (the elo_*_form queries of include/elo.h).

Inputs (tests/forms_inputs.py): prefix-ones masks with an all-masked, a one-valid and an all-valid point at fixed places; masked slots
at cell (0,0,0) or anywhere; half the slots on 8 hot cells; every 5th centre with a neighbour ON it (d = 0); pool logits scaled x40 on
every other point, masked logits of 1e3 above every valid one and (fp32) one point whose valid logits lie below the masked -1e10.
With fp16 storage the feature tensors hold fp16-representable values (the clouds, indices and masks are fp32 / int32 in either
storage type).

Encode kernels and group_concat: p, g*m, g*m - p, the feature copies and the masked zeros are copies, 0/1 products and ONE correctly
rounded subtraction -- they must EQUAL the float64 reference rounded to fp32 (and, in fp16 storage, once more to half).  The norm
column and the pool are held to the bounds derived in tests/forward_forms_bounds.py.  Each test prints the worst error it saw, in
units of its bound's unit (profiles/forward_forms_errors.txt records them; the asserted bounds never come from there)."""
import numpy as np
import pytest
import torch

import forward_forms_bounds as bounds
import forward_forms_cases as table
import twins_torch as twin
from conftest import load_pkg
from forms_inputs import as_half_values, at_offset, cv_encode1_inputs, cv_encode2_inputs, pool_forward_inputs, slots, softmax_pool_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cases(op):
    return [pytest.param(c, id=table.case_id(c)) for c in table.CASES if c.op == op]


def _features(case, *arrays):
    """the feature arrays as the case stores them: (float64 reference inputs, the tensors handed to the kernel)"""
    if case.dtype == "f16":
        arrays = [as_half_values(a) for a in arrays]
    dev = [t(a) for a in arrays]
    return [d.double() for d in dev], [at_offset(d.half() if case.dtype == "f16" else d, case.offset) for d in dev]


def _expected(ref64, case):
    e = ref64.float()
    return e.half() if case.dtype == "f16" else e


def _check_encoded(got, ref64, case, norm_column, what):
    """every column exact but the norm, which is held to forward_forms_bounds.norm_bound"""
    want = _expected(ref64, case)
    assert got.dtype == want.dtype and got.shape == want.shape
    if norm_column is None:
        assert torch.equal(got, want), what
        return 0.0
    assert torch.equal(got[..., :norm_column], want[..., :norm_column]), what + ": geometry columns"
    assert torch.equal(got[..., norm_column + 1:], want[..., norm_column + 1:]), what + ": feature columns"
    ref = ref64[..., norm_column]
    err = (got[..., norm_column].double() - ref).abs()
    f16 = case.dtype == "f16"
    ratio = float(((err - ((bounds.HALF_REL * ref + bounds.HALF_ABS) if f16 else 0)).clamp(min=0) / (bounds.U32 * ref)).max())
    print("FORM_ERROR %s %s %s norm %.3f u (bound 4)" % (case.op, case.dtype, case.form, ratio))
    assert bool((err <= bounds.norm_bound(ref, f16)).all()), "%s: norm column off by %.3f u" % (what, ratio)
    return ratio


@pytest.mark.parametrize("case", _cases("encode1"))
def test_cv_encode1_forward(case):
    ops = load_pkg("_ops")
    rng = np.random.default_rng(table.rows(case) + case.C)
    xyz1, f1, xyz2, f2, idx, m = cv_encode1_inputs(rng, case.B, case.N, case.H, case.W, case.K, case.C, "anywhere" if case.C % 4 == 2 else "origin")
    (f1_64, f2_64), (f1_k, f2_k) = _features(case, f1, f2)
    args = (t(xyz1), f1_k, t(xyz2), f2_k, t(idx), t(m))
    assert ops.cv_encode1_form(*args) == case.form
    got = ops.cv_encode1(*args)
    ref = twin.cv_encode1(t(xyz1).double(), f1_64, t(xyz2).double(), f2_64, t(idx), t(m).double())
    _check_encoded(got, ref, case, 9, table.case_id(case))
    masked = t(m) == 0
    assert bool(masked.any()) and bool((got[masked][:, 10 + case.C:] == 0).all())          # the masked zeros, said once more in plain words


@pytest.mark.parametrize("case", _cases("encode2"))
def test_cv_encode2_forward(case):
    ops = load_pkg("_ops")
    rng = np.random.default_rng(table.rows(case) + case.C + case.Cc)
    xyz, f1, cost, idx, m = cv_encode2_inputs(rng, case.B, case.H, case.W, case.K, case.C, case.Cc, "anywhere" if case.K == 5 else "origin")
    (f1_64, cost_64), (f1_k, cost_k) = _features(case, f1, cost)
    args = (t(xyz), f1_k, cost_k, t(idx), t(m))
    assert ops.cv_encode2_form(*args) == case.form
    got_cat, got_rest = ops.cv_encode2(*args)
    ref_cat, ref_rest = twin.cv_encode2(t(xyz).double(), f1_64, cost_64, t(idx), t(m).double())
    _check_encoded(got_cat, ref_cat, case, 9, table.case_id(case) + " xyz_cat")
    _check_encoded(got_rest, ref_rest, case, None, table.case_id(case) + " rest")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("C,off_form,aligned_form", [(16, "col64", "staged128"), (64, "vec32", "staged64")], ids=["C16", "C64"])
def test_cv_encode1_forms_give_the_same_bits(C, off_form, aligned_form, dtype):
    """vec, col and staged all take their row facts from resolve_rows and convert in the same order: one input, once in 16-byte aligned
    feature tensors (staged) and once 8 bytes off (the column-owner form at C = 16, the vec form at C = 64)."""
    ops = load_pkg("_ops")
    if dtype == "f16" and C == 64:
        aligned_form = "staged128"                       # (fp16 rows are half as long: 128 of them fit the tile)
    B, N, K = table.MID7
    rng = np.random.default_rng(C)
    xyz1, f1, xyz2, f2, idx, m = cv_encode1_inputs(rng, B, N, table.GRID[0], table.GRID[1], K, C)
    conv = (lambda a: t(as_half_values(a)).half()) if dtype == "f16" else t
    res = []
    for nbytes, form in ((0, aligned_form), (8, off_form)):
        args = (t(xyz1), at_offset(conv(f1), nbytes), t(xyz2), at_offset(conv(f2), nbytes), t(idx), t(m))
        assert ops.cv_encode1_form(*args) == form
        res.append(ops.cv_encode1(*args))
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("C", [3, 16, 64], ids=lambda c: "C%d" % c)
@pytest.mark.parametrize("masked_at", ["origin", "anywhere"])
def test_group_concat_forward(C, masked_at):
    """One staged-tile kernel; 2 x 113 x 5 = 1130 rows (17 tiles of 64 and 42 rows).  g*m - centre is one correctly rounded subtraction."""
    ops = load_pkg("_ops")
    B, N, K, (H2, W2) = 2, 113, 5, table.GRID
    rng = np.random.default_rng(C)
    idx, m = slots(rng, B, N, K, H2, W2, masked_at)
    centre = rng.normal(0, 5, (B, N, 3)).astype(np.float32)
    sx = rng.normal(0, 5, (B, H2, W2, 3)).astype(np.float32)
    sf = rng.normal(0, 1, (B, H2, W2, C)).astype(np.float32)
    idx[0, 2, 0], sx[0, 0, 0] = (0, 0, 0), centre[0, 2]  # a neighbour ON its centre (point 2 has every slot valid)
    got = ops.group_concat(t(centre), t(sx), t(sf), t(idx), t(m))
    ref = twin.group_concat(t(centre).double(), t(sx).double(), t(sf).double(), t(idx), t(m).double())
    assert (B * N * K) % 64 and torch.equal(got, ref.float())
    assert m[0, 2, 0] == 1 and bool((got[0, 2, 0, :3] == 0).all())


@pytest.mark.parametrize("case", _cases("pool"))
def test_masked_softmax_pool_forward(case):
    """|out - float64| <= constant(form, K) * UNIT elementwise (tests/forward_forms_bounds.py: K + 3 scalar, J + 5 wave<J>, 4K for the
    online quarter-wave form; fp16 storage: plus half an ulp of the result), and an all-masked point is the plain mean of its K values."""
    ops, tuning = load_pkg("_ops"), load_pkg("tuning")
    rng = np.random.default_rng(case.K * 100 + case.C)
    width, first = case.wide or (case.C, 0)
    lg, v, m = pool_forward_inputs(rng, case.B, case.N, case.K, case.C, width, case.dtype == "f16")
    (lg64, v64), (lg_k, v_k) = _features(case._replace(offset=0), lg, v)
    v_k = at_offset(v_k, case.offset)[..., first:first + case.C]
    v64 = v64[..., first:first + case.C]
    with tuning.override(**dict(case.tuning or ())):
        assert ops.masked_softmax_pool_form(lg_k, v_k, t(m)) == case.form
        got = ops.masked_softmax_pool(lg_k, v_k, t(m))
    ref, unit, scale = bounds.pool_reference(lg64, v64, t(m).double())
    f16 = case.dtype == "f16"
    assert got.dtype == (torch.float16 if f16 else torch.float32) and bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs()
    slack = case.K * bounds.POOL_ABS * scale + ((bounds.HALF_REL * ref.abs() + bounds.HALF_ABS) if f16 else 0)
    ratio = float(((err - slack).clamp(min=0) / unit).max())
    const = bounds.pool_constant(case.form, case.K)
    print("FORM_ERROR pool %s %s K=%d C=%d %.3f UNIT (bound %d)" % (case.dtype, case.form, case.K, case.C, ratio, const))
    assert bool((err <= bounds.pool_bound(case.form, case.K, unit, scale, f16, ref)).all()), "worst error %.3f UNIT, bound %d" % (ratio, const)
    mean = v64.mean(2)[:, 0]                              # point 0 of every batch element is all masked
    assert bool((t(m)[:, 0] == 0).all())
    assert bool(((got.double()[:, 0] - mean).abs() <= bounds.pool_bound(case.form, case.K, unit, scale, f16, ref)[:, 0]).all())


@pytest.mark.parametrize("refusal", table.REFUSALS, ids=lambda r: r.why.replace(" ", "_"))
def test_fp16_refusals_raise_and_launch_nothing(refusal):
    """What fp16 storage cannot take raises through _ops (there is no scalar fp16 kernel to fall to), before any launch: the stream
    has seen no kernel error afterwards and the query refuses the same block."""
    ops, L = load_pkg("_ops"), load_pkg("_lib")
    case = refusal.case
    rng = np.random.default_rng(0)
    if case.op == "pool":
        lg, v, m = softmax_pool_inputs(rng, case.B, case.N, case.K, case.C)
        args = (t(lg).half(), at_offset(t(v).half(), case.offset), t(m))
        call, query = ops.masked_softmax_pool, ops.masked_softmax_pool_form
    elif case.op == "encode1":
        xyz1, f1, xyz2, f2, idx, m = cv_encode1_inputs(rng, case.B, case.N, case.H, case.W, case.K, case.C)
        args = (t(xyz1), at_offset(t(f1).half(), case.offset), t(xyz2), at_offset(t(f2).half(), case.offset), t(idx), t(m))
        call, query = ops.cv_encode1, ops.cv_encode1_form
    else:
        xyz, f1, cost, idx, m = cv_encode2_inputs(rng, case.B, case.H, case.W, case.K, case.C, case.Cc)
        args = (t(xyz), at_offset(t(f1).half(), case.offset), at_offset(t(cost).half(), case.offset), t(idx), t(m))
        call, query = ops.cv_encode2, ops.cv_encode2_form
    for fn in (query, call):
        with pytest.raises(L.EloError, match="fp16 needs"):
            fn(*args)
    torch.cuda.synchronize()

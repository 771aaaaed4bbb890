"""CPU: the case table of tests/train_forms_cases.py against the library's own choices (elo_dense_weight_grad_form and elo_bn_parts of
include/elo.h read the argument block only: no GPU, fake addresses of the case's alignment), all 42 weight-gradient kernels and every
batch-norm edge covered, the host-side refusals of the launchers and of the two queries, and the bounds of tests/train_forms_bounds.py
against float32 restatements of each kernel's order of operations: a faithful restatement stays within HALF of every bound on every
case, and each deliberately wrong one (bounds.MUTANTS) lands at least 5 bounds away on a case the test names."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_forms_bounds as bounds
import train_forms_cases as table
from conftest import ROOT, load_pkg

BASE = 0x7f0000000000                                    # fake device addresses, 16 MB apart and 4 KB aligned: never dereferenced
P = [BASE + (i << 24) for i in range(12)]


def wgrad_args(c, db=True):
    L = load_pkg("_lib")
    return L.WeightGradArgs(c.rows, c.cin, c.cout, P[0] + c.x_off, P[1] + c.g_off, P[2], P[3] if db else None, P[4])


def expected_name(c):
    return "%s@%dx%dw%d" % ((c.kernel,) + c.grid)


# ------------------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", table.WGRAD, ids=table.wgrad_id)
def test_weight_grad_case_reaches_the_form_it_names(case):
    L = load_pkg("_lib")
    for db in (True, False):
        assert L.wgrad_form(wgrad_args(case, db)) == expected_name(case)
    p = table.wgrad_plan(case.rows, case.cin, case.cout, case.x_off, case.g_off)              # the restatement the bounds count with
    assert p["slices"] == L.lib().elo_weight_grad_slices(case.rows, case.cin, case.cout)
    f = L.wgrad_form_fields(L.lib().elo_dense_weight_grad_form(ctypes.byref(wgrad_args(case))))
    assert {k: p[k] for k in f} == f


def test_all_42_weight_grad_kernels_have_a_case_at_every_row_count():
    L = load_pkg("_lib")
    assert len(L.WGRAD_FORMS) == len(set(L.WGRAD_FORMS)) == 42
    for rows in table.WGRAD_ROWS:
        assert {c.kernel for c in table.WGRAD_SMALL if c.rows == rows} == set(L.WGRAD_FORMS), rows
    # the source compiles exactly these: CI in 1..4 x CO in {1, 2, 4}, each in the four / two (CI = 3) load forms of the ELO_WG macro
    src = open(os.path.join(ROOT, "efficientlo-net_amd", "csrc", "elo_train.hip")).read()
    pairs = re.findall(r"ELO_WG\((\d), (\d)\);", src)
    assert sorted(pairs) == sorted((str(ci), str(co)) for ci in (1, 2, 3, 4) for co in (1, 2, 4))
    assert sum(2 if ci == "3" else 4 for ci, _ in pairs) == 42


def test_weight_grad_rows_reach_the_trips_and_slices_they_are_for():
    plan = lambda rows, cin=64, cout=64: table.wgrad_plan(rows, cin, cout)
    groups = lambda rows: (rows + 3) // 4
    owns = lambda rows, cin=64, cout=64: [max(0, min(groups(rows), (s + 1) * plan(rows, cin, cout)["per_slice"]) - s * plan(rows, cin, cout)["per_slice"])
                                          for s in range(plan(rows, cin, cout)["slices"])]
    assert [plan(r)["slices"] for r in table.WGRAD_ROWS] == [1, 1, 1, 1, 1, 2, 3, 33]
    assert [groups(r) for r in (1, 3, 5, 33, 65)] == [1, 1, 2, 9, 17]          # a lone partial group; < U = 4 groups; a second half-trip that is ragged
    assert all(r % 4 for r in (1, 3, 5, 33, 65, 129, 257))                     # the last group is partial
    assert owns(129) == [17, 16] and owns(257) == [22, 22, 21]
    assert owns(4096)[-2:] == [32, 0] and len(owns(4096)) == 33               # 33 slices of 32 groups over 1024 groups: the last owns nothing
    cap = owns(16391, 256, 256)
    assert len(cap) == 128 == (32 << 20) // (256 * 256 * 4) and cap.count(0) == 3 and sum(cap) == groups(16391)
    cap = owns(262149, 1, 1)
    assert len(cap) == 2048 and sum(cap) == groups(262149)
    grids = {(c.cin, c.cout): c.grid for c in table.WGRAD_MORE}
    assert grids[(138, 64)] == (3, 1, 3) and grids[(80, 128)] == (2, 2, 4) and grids[(272, 256)] == (5, 4, 4) and grids[(320, 64)] == (5, 1, 4)
    assert {c.kernel for c in table.WGRAD_MORE if c.x_off} == {"ci4co4/xsgv"} and {c.kernel for c in table.WGRAD_MORE if c.g_off} == {"ci4co4/xvgs"}
    assert {c.kernel for c in table.WGRAD_MORE if c.cin == 320} == {"ci4co4/xvgv"}              # idle waves on the vector form of x


@pytest.mark.parametrize("case", table.BN + [table.BN_BIG], ids=table.bn_id)
def test_batch_norm_case_has_the_parts_the_bounds_count_with(case):
    L = load_pkg("_lib")
    assert L.bn_parts(case.M, case.C) == table.bn_parts(case.M, case.C)
    assert L.lib().elo_bn_scratch_floats(case.C, case.groups) == 2 * case.C * table.BN_MAX_PARTS * case.groups
    assert case is table.BN_BIG or case.M == table.BN_EDGES[case.edge](1024 // case.C)


@pytest.mark.parametrize("C", table.BN_WIDTHS)
def test_batch_norm_cases_reach_every_edge_of_a_width(C):
    rpb = 1024 // C
    mine = [c for c in table.BN if c.C == C]
    assert {c.edge for c in mine} == set(table.BN_EDGES)
    iters = lambda c: (c.M + rpb - 1) // rpb
    assert any(c.M < rpb for c in mine) and any(c.M == 1 and c.running for c in mine)                       # below one block iteration; the M > 1 guard
    assert any(table.bn_parts(c.M, C) > 1 and iters(c) % 8 and iters(c) % 4 and c.M % rpb for c in mine)    # a ragged unrolled trip in both reductions
    assert any(iters(c) == 8 and c.M % rpb for c in mine) and any(iters(c) == 9 for c in mine)              # one trip exactly (its last rows dead); one over
    cap = [c for c in mine if c.edge == "cap"]
    assert cap and all(table.bn_parts(c.M, C) == table.BN_MAX_PARTS and table.bn_per(c.M, C) == 9 for c in cap)
    assert all(511 * 9 * rpb >= c.M and c.M * C * 4 <= 17 << 20 for c in cap)                               # blocks that own no row; 16 MB and a bit
    assert {c.groups for c in mine} == {1, 2, 3, 64} and {c.relu for c in mine} == {0, 1} and {c.running for c in mine} == {0, 1}


def test_the_big_case_is_beyond_the_block_cap_of_the_elementwise_kernels():
    c = table.BN_BIG
    n4 = c.M * (c.C // 4)
    assert (n4 + 1023) // 1024 > 8192 and 0 < n4 % (4 * 8192 * 256) < 256       # the grid stride wraps; a tail after the unrolled loop, in one block only


def test_the_caps_the_bounds_rely_on():
    """The float64 references have no cap of their own; what the BOUNDS assume is stated here."""
    for c in table.BN + [table.BN_BIG]:
        assert c.M < 2 ** 24 and 1 <= c.groups <= 64                                           # (float)M is exact; the launchers' group limit
        assert 1 <= table.bn_parts(c.M, c.C) <= table.BN_MAX_PARTS
    for c in table.WGRAD:
        p = table.wgrad_plan(c.rows, c.cin, c.cout)
        assert c.rows * max(c.cin, c.cout) < 2 ** 31 and 1 <= p["slices"] <= 2048 and p["slices"] * c.cin * c.cout * 4 <= 32 << 20
        assert bounds.gam(bounds.wgrad_terms(c.rows, c.cin, c.cout)[0]) < 1e-3


# ------------------------------------------------------------------------------------------------------------ the ABI and the refusals
def test_the_two_queries_are_declared_bound_and_additive():
    L = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "elo.h")).read()
    assert re.search(r"\bint elo_dense_weight_grad_form\(const elo_weight_grad_args \*a\);", header)
    assert re.search(r"\bint elo_bn_parts\(long rows_per_group, int C\);", header)
    assert ("elo_dense_weight_grad_form", ctypes.c_int, [ctypes.POINTER(L.WeightGradArgs)]) in L.SYMBOLS
    assert ("elo_bn_parts", ctypes.c_int, [ctypes.c_long, ctypes.c_int]) in L.SYMBOLS
    assert L.ABI_VERSION == 26                                                 # additive: no struct moved
    m = re.search(r"#define ELO_WGRAD_FORM\(CI, CO, xv, gv, waves, gy, gz\) \\\n\s*\((.*)\)\n", header).group(1)
    pack = lambda **k: eval(m, {}, k)                                          # the header's packing is the binding's
    for f in (dict(CI=3, CO=4, xv=0, gv=1, waves=3, gy=3, gz=1), dict(CI=4, CO=1, xv=1, gv=0, waves=4, gy=2047, gz=4095),
              dict(CI=1, CO=2, xv=1, gv=1, waves=1, gy=1, gz=1)):
        assert L.wgrad_form_fields(pack(**f)) == f
    assert L.wgrad_form_name(pack(CI=4, CO=4, xv=1, gv=0, waves=4, gy=5, gz=1)) == "ci4co4/xvgs@5x1w4"


def test_weight_grad_refusals_are_the_same_in_the_query_and_the_launcher():
    L = load_pkg("_lib")
    lib = L.lib()
    good = table.WGRAD[0]

    def both(a, status, words):
        for fn, extra in ((lib.elo_dense_weight_grad_form, ()), (lib.elo_dense_weight_grad, (None,))):
            assert fn(ctypes.byref(a) if a is not None else None, *extra) == status and words in lib.elo_last_error(), (fn, words)

    both(None, -1, b"null argument block")
    for field in ("rows", "Cin", "Cout"):
        for bad in (0, -3):
            a = wgrad_args(good)
            setattr(a, field, bad)
            both(a, -1, b"bad sizes")
    for field in ("x", "g", "dW", "scratch"):
        a = wgrad_args(good)
        setattr(a, field, None)
        both(a, -1, b"null tensor pointer")
    a = wgrad_args(good)
    a.rows, a.Cin, a.Cout = 1 << 25, 64, 16                                    # rows * width = 2^31
    both(a, -2, b"rows * width >= 2^31")
    a.rows -= 1
    assert L.wgrad_form(a) == "ci4co1/xvgv@1x1w1"                              # 2^31 - 64: taken
    a.rows, a.Cin, a.Cout = 1 << 25, 16, 64
    both(a, -2, b"rows * width >= 2^31")
    a = wgrad_args(good)
    a.rows, a.Cin, a.Cout = 4, 16 * 4 * 2048, 16                               # 2048 blocks in y: does not pack
    both(a, -2, b"blocks of dW")
    a.Cin, a.Cout = 16 * 4 * 512, 16 * 4 * 513                                 # 262656 blocks: more than 65535 workgroups of 4 waves
    both(a, -2, b"blocks of dW")
    with pytest.raises(L.EloError):
        L.wgrad_form(a)
    a = wgrad_args(good, db=False)                                             # db is optional
    assert L.wgrad_form(a) == expected_name(good)


def test_batch_norm_refusals_on_the_host():
    """elo_bn_parts and the three launchers refuse before anything is launched: widths, pointers, rows, groups."""
    L = load_pkg("_lib")
    lib = L.lib()
    for C in (0, 2, 3, 12, 24, 257, 512, -8):
        assert lib.elo_bn_parts(100, C) == -2 and b"not a power of two in 4..256" in lib.elo_last_error()
    for rows in (0, -1):
        assert lib.elo_bn_parts(rows, 64) == -1 and b"no rows" in lib.elo_last_error()
    assert [L.bn_parts(1, C) for C in table.BN_WIDTHS] == [1] * 7
    with pytest.raises(L.EloError):
        L.bn_parts(5, 12)

    stats = lambda **k: L.BnStatsArgs(**dict(dict(rows=96, C=16, z=P[0], scratch=P[1], eps=1e-3, momentum=0.3, mean=P[2], invstd=P[3],
                                                  running_mean=P[4], running_var=P[5], groups=1), **k))
    apply_ = lambda **k: L.BnApplyArgs(**dict(dict(rows=96, C=16, z=P[0], mean=P[2], invstd=P[3], gamma=P[6], beta=P[7], relu=1, y=P[8], groups=1), **k))
    back = lambda **k: L.BnBackwardArgs(**dict(dict(rows=96, C=16, dy=P[9], z=P[0], mean=P[2], invstd=P[3], gamma=P[6], beta=P[7], relu=1,
                                                    scratch=P[1], sums=P[10], dz=P[11], groups=1), **k))
    entries = (("elo_bn_stats", stats, ("z", "scratch", "mean", "invstd")), ("elo_bn_apply", apply_, ("z", "mean", "invstd", "gamma", "beta", "y")),
               ("elo_bn_backward", back, ("dy", "z", "mean", "invstd", "gamma", "beta", "scratch", "sums", "dz")))

    def refused(entry, a, status, words):
        assert getattr(lib, entry)(ctypes.byref(a), None) == status and words in lib.elo_last_error(), (entry, words, lib.elo_last_error())

    for entry, make, pointers in entries:
        assert getattr(lib, entry)(None, None) == -1 and b"null argument block" in lib.elo_last_error()
        for C in (3, 12, 512):
            refused(entry, make(C=C), -2, b"not a power of two in 4..256")
        for rows in (0, -96):
            refused(entry, make(rows=rows), -1, b"no rows")
        for name in pointers:
            for off in (4, 8):
                refused(entry, make(**{name: P[0] + off}), -1, b"null or unaligned tensor pointer")
            if not (entry == "elo_bn_backward" and name == "dz"):               # (dz = NULL is a form of elo_bn_backward)
                refused(entry, make(**{name: None}), -1, b"null or unaligned tensor pointer")
        refused(entry, make(rows=65 * 96, groups=65), -1, b"do not split into 65 groups")
        refused(entry, make(rows=97, groups=2), -1, b"do not split into 2 groups")
        refused(entry, make(rows=98, groups=3), -1, b"do not split into 3 groups")
    refused("elo_bn_stats", stats(running_var=None), -1, b"running_mean and running_var go together")
    refused("elo_bn_stats", stats(running_mean=None), -1, b"running_mean and running_var go together")


# ------------------------------------------------------------------------------------------ the bounds against float32 restatements
def _bn_shares(c, i, mutant=None):
    """{output: (share of its bound, where)} of the float32 restatements of the three batch-norm entry points on case c."""
    G, out = c.groups, {}
    ref = bounds.stats_reference(i["z"], G, table.BN_EPS, table.BN_MOMENTUM, *((i["rm"], i["rv"]) if c.running else ()))
    got = bounds.stats_f32(i["z"], G, table.BN_EPS, table.BN_MOMENTUM, *((i["rm"], i["rv"]) if c.running else ()), mutant=mutant)
    for name, g in zip(("mean", "invstd", "rm", "rv"), got):
        if g is not None:
            out[name] = bounds.share(g, *ref[name])
    par = (i["mean"], i["invstd"], i["gamma"], i["beta"], c.relu, G)
    out["y"] = bounds.share(bounds.apply_f32(i["z"], *par), *bounds.apply_reference(i["z"], *par))
    ref = bounds.backward_reference(i["dy"], i["z"], *par)
    sums, dz = bounds.backward_f32(i["dy"], i["z"], *par, mutant=mutant)
    out["sums"], out["dz"] = bounds.share(sums, *ref["sums"]), bounds.share(dz, *ref["dz"])
    return out


@pytest.mark.parametrize("case", table.BN, ids=table.bn_id)
def test_batch_norm_restatements_stay_within_half_of_every_bound(case):
    i = table.bn_inputs(case)
    # the inputs: ties where they were placed (both signs of zero), every other pre-activation beyond its own rounding bound
    pre, bound = bounds.preactivation(i["z"], i["mean"], i["invstd"], i["gamma"], i["beta"], case.groups)
    tie = i["tie"]
    assert tie[:, 0].any() and tie[:, 1].any() and not tie[:, 2:].any() and (pre[tie] == 0).all() and (bound[tie] == 0).all()
    assert (np.abs(pre[~tie]) > bound[~tie]).all()
    f32 = ((i["z"] - np.repeat(i["mean"], case.M, 0)) * np.repeat(i["invstd"], case.M, 0)) * i["gamma"] + i["beta"]
    assert not np.signbit(f32[tie[:, 0], 0]).any() and np.signbit(f32[tie[:, 1], 1]).all()       # +0 under gamma = 1, -0 under gamma = -1
    assert ((f32 > 0) == (pre > 0)).all()                                      # the fp32 decision IS the float64 one: nothing to exclude later
    if case.M == 1:
        ref = bounds.stats_reference(i["z"], case.groups, table.BN_EPS, table.BN_MOMENTUM, i["rm"], i["rv"])
        assert (ref["invstd"][0] == float(table.BN_EPS) ** -0.5).all()         # one row: the variance is 0 ...
        keep = (1 - float(table.BN_MOMENTUM)) ** case.groups
        assert np.allclose(ref["rv"][0], keep * i["rv"].astype(np.float64), rtol=1e-12)          # ... and the moving variance takes it (M > 1 guard)
    shares = _bn_shares(case, i)
    print("restatement %s: %s" % (table.bn_id(case), {k: round(v[0], 3) for k, v in shares.items()}))
    assert all(s <= 0.5 for s, _ in shares.values()), shares


def _subset(c):
    """Channel subsets (first, last and some between) for the shapes whose full restatement would take seconds."""
    pick = lambda n: np.arange(n) if c.cin * c.cout <= 8192 and c.rows <= 5000 else np.unique(np.linspace(0, n - 1, 12).astype(int))
    return pick(c.cin), pick(c.cout)


def _wgrad_shares(c, mutant=None):
    x, g = table.wgrad_inputs(c)
    ref = bounds.wgrad_reference(x, g)
    ci, co = _subset(c)
    dW, db = bounds.wgrad_f32(x[:, ci], g[:, co], table.wgrad_plan(c.rows, c.cin, c.cout, c.x_off, c.g_off), mutant=mutant)
    return {"dW": bounds.share(dW, ref["dW"][0][np.ix_(ci, co)], ref["dW"][1][np.ix_(ci, co)]), "db": bounds.share(db, ref["db"][0][co], ref["db"][1][co])}


@pytest.mark.parametrize("case", [c for c in table.WGRAD if not (c.x_off or c.g_off)], ids=table.wgrad_id)      # (the offset cases: same numbers)
def test_weight_grad_restatement_stays_within_half_of_every_bound(case):
    shares = _wgrad_shares(case)
    print("restatement %s: %s" % (table.wgrad_id(case), {k: round(v[0], 3) for k, v in shares.items()}))
    assert all(s <= 0.5 for s, _ in shares.values()), shares


_bn = lambda **k: [c for c in table.BN if all(getattr(c, f) == v for f, v in k.items())]
_wg = lambda cin, cout, rows: [c for c in table.WGRAD if (c.cin, c.cout, c.rows, c.x_off, c.g_off) == (cin, cout, rows, 0, 0)]
# where each mutant is looked for: small cases in which the mistake is a large part of the result
MUTANT_CASES = {
    "biased_moving_variance": _bn(C=16, M=2, groups=1), "momentum_on_the_wrong_term": _bn(C=16, M=2, groups=1),
    "last_group_only": _bn(C=16, edge="ragged", groups=2) + _bn(C=16, edge="ragged", groups=3),
    "mask_from_z": _bn(C=16, edge="ragged", groups=1), "ge_at_ties": _bn(C=16, edge="ragged", groups=1) + _bn(C=256, edge="over", groups=1),
    "xhat_term_dropped": _bn(C=16, edge="ragged", groups=1), "m_minus_1": _bn(C=16, M=2, groups=1) + _bn(C=16, edge="ragged", groups=1),
    "last_partial_group_dropped": _wg(64, 64, 5) + _wg(1, 1, 33), "tile_order": _wg(32, 16, 33) + _wg(64, 64, 257),
    "db_per_block": _wg(320, 64, 5) + _wg(138, 64, 257)}


@pytest.mark.parametrize("mutant", bounds.MUTANTS)
def test_a_wrong_restatement_misses_the_bounds_by_five(mutant):
    cases = MUTANT_CASES[mutant]
    assert cases
    caught = []
    for c in cases:
        shares = _bn_shares(c, table.bn_inputs(c), mutant) if isinstance(c, table.Bn) else _wgrad_shares(c, mutant)
        caught += [((table.bn_id if isinstance(c, table.Bn) else table.wgrad_id)(c), name, s) for name, (s, _) in shares.items() if s >= 5]
    print("mutant %s is caught on: %s" % (mutant, ", ".join("%s %s (%.3g bounds)" % hit for hit in caught)))
    assert caught, mutant

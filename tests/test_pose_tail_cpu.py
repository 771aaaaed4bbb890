"""CPU: the case table of tests/pose_tail_cases.py against the library's own launch decisions (elo_softmax_valid_parts,
elo_pose_head_form and elo_mlp_sv_parts read the argument blocks only: no GPU, fake addresses), the table's completeness computed from
the table, the refusals with nothing launched, the float64 statements of tests/pose_tail_reference.py pinned to oracle/ops_np.py, a
float32 emulation of every summation form held within HALF the bound tests/pose_tail_bounds.py derives, and the cell tests' 2 % cap on
the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest

import pose_tail_bounds as bounds
import pose_tail_cases as table
import pose_tail_reference as R
from conftest import ROOT, load_pkg
from oracle import ops_np as O

BASE = 0x7f0000000000                                    # fake device addresses, 4 KB apart and 16-byte aligned: never dereferenced
ids = lambda v: v.name if hasattr(v, "name") else str(v)


def _ptr(i):
    return BASE + 4096 * i


def fake_head(L, B=2, N=100, C=64, hidden=256, storage="f32", q_coarse=False, t_coarse=False, ready_parts=0, clear_C=None, clear_cells=0):
    a = L.PoseHeadArgs()
    a.batch, a.npoints, a.C, a.hidden = B, N, C, hidden
    for i, f in enumerate(("feature", "weight", "xyz", "W_big", "b_big", "W_q", "b_q", "W_t", "b_t", "q", "t", "q_norm", "scratch")):
        setattr(a, f, _ptr(1 + i))
    a.q_coarse, a.t_coarse = (_ptr(20) if q_coarse else None), (_ptr(21) if t_coarse else None)
    a.feat_dtype = L.ELO_F16 if storage == "f16" else L.ELO_F32
    a.ready_parts = ready_parts
    if clear_C is not None:
        a.clear_scratch, a.clear_xyz, a.clear_feat, a.clear_cells, a.clear_C = _ptr(30), _ptr(31), (_ptr(32) if clear_C else None), clear_cells or 8, clear_C
    return a


def fake_warp(L, a, B, N, H, W, C, other=False):
    """The warp block of elo_pose_head_warp on the buffers `a` clears (`other`: on buffers of its own -- refused)"""
    a.clear_scratch, a.clear_xyz, a.clear_feat, a.clear_cells, a.clear_C = _ptr(30), _ptr(31), (_ptr(32) if C else None), B * H * W, C
    w = L.WarpProjectArgs()
    w.batch, w.npoints, w.C, w.H, w.W = B, N, C, H, W
    w.az_res, w.vert_res, w.vert_off = 0.1, 0.1, 1.0
    w.xyz, w.feat, w.warped = _ptr(40), (_ptr(41) if C else None), _ptr(42)
    w.out_xyz, w.out_feat, w.scratch = _ptr(31), (_ptr(32) if C else None), (_ptr(33) if other else _ptr(30))
    w.prepared, w.feat_dtype = 1, a.feat_dtype
    return w


def fake_ride(L, case):
    """The MLP launch of a (d) case: one 64 -> 64 layer over one 64-wide source with sv_feature; the paired form two such jobs (the
    second one's output are the features)."""
    from test_fused_shapes_cpu import fake_mlp
    rows = case.B * case.N
    storage = case.storage
    if case.pair:
        a, b = (fake_mlp(L, (64,), (64,), rows, None, storage) for _ in range(2))
    else:
        a, b = fake_mlp(L, (64,), (64,), rows, None, storage), None
        a.sv_feature = _ptr(50)
    a.sv_scratch, a.sv_xyz, a.sv_npoints = _ptr(51), _ptr(52), case.N
    return a, b


def ride_parts(case_or_shape):
    """elo_mlp_sv_parts of a (d) case under the tuning that forces its tile height"""
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    case = case_or_shape if hasattr(case_or_shape, "tile") else table.Ride("x", 1, case_or_shape[0], case_or_shape[1], "f32", "random", None, False)
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(case.tile)):
        a, b = fake_ride(L, case)
        return L.lib().elo_mlp_sv_parts(ctypes.byref(a), ctypes.byref(b) if b is not None else None)


def ask(case):
    """The form's name (or the negative status) the library answers for a table case"""
    L = load_pkg("_lib")
    w = None
    if isinstance(case, table.Head):
        a = fake_head(L, case.B, case.N, case.C, case.hidden, case.storage, case.coarse, case.coarse)
    elif isinstance(case, table.Merge):
        a = fake_head(L, case.B, 100, ready_parts=case.parts)
    elif isinstance(case, table.Ride):
        a = fake_head(L, case.B, case.N, storage=case.storage, ready_parts=ride_parts(case))
    else:
        a = fake_head(L, case.B, 17, storage=case.storage)
        w = fake_warp(L, a, case.B, case.N, case.H, case.W, case.C)
    rc = L.lib().elo_pose_head_form(ctypes.byref(a), ctypes.byref(w) if w is not None else None)
    return L.tail_form_name(rc) if rc >= 0 else rc


FORM_CASES = table.HEAD + table.MERGE + table.RIDE + table.WARP


@pytest.mark.parametrize("case", FORM_CASES, ids=ids)
def test_case_takes_the_form_it_names(case):
    assert ask(case) == table.expected_form(case)


def test_the_slice_count_is_the_librarys():
    L = load_pkg("_lib")
    for N in list(range(1, 300)) + list(range(3900, 4300)) + [8192, 8193, 150000, 2 ** 31 - 1]:
        assert L.lib().elo_softmax_valid_parts(N) == table.sv_parts(N), N
    assert load_pkg("_ops").softmax_valid_parts(4097) == 64


def test_enumerators_of_the_header_and_the_binding_agree():
    L = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "elo.h")).read()
    enums = {name: int(v) for name, v in re.findall(r"\b(ELO_TAIL_[A-Z0-9_]+)\s*=\s*(\d+)", header)}
    assert tuple(n for n, _ in sorted(((n, v) for n, v in enums.items() if n.startswith("ELO_TAIL_PARTIALS_")), key=lambda nv: nv[1])) == \
        tuple("ELO_TAIL_PARTIALS_" + p.upper() for p in L.TAIL_PARTIALS)
    assert [enums["ELO_TAIL_" + m.upper()] for m in L.TAIL_MERGES] == [0, 1]
    assert [enums["ELO_TAIL_HEAD_" + h.upper()] for h in L.TAIL_HEADS] == [0, 1]
    assert len(enums) == len(L.TAIL_PARTIALS) + len(L.TAIL_MERGES) + len(L.TAIL_HEADS)
    macro = re.search(r"#define ELO_TAIL_FORM\(partials, merge, head, wide, warp, parts\) \\\n\s*\(\(partials\) \| \(merge\) << (\d+) \| \(head\) << (\d+) \| "
                      r"\(wide\) << (\d+) \| \(warp\) << (\d+) \| \(parts\) << (\d+)\)", header)
    assert macro and tuple(int(g) for g in macro.groups()) == (2, 3, 4, 5, 8)
    assert L.tail_form_name(1 | 0 << 2 | 0 << 3 | 4 << 8) == "f32x4/trips16/model"
    assert L.tail_form_name(0 | 1 << 2 | 1 << 3 | 1 << 4 | 1 << 5 | 512 << 8) == "readyx512/trips32/generic+wide+warp"
    for query in ("elo_softmax_valid_parts", "elo_pose_head_form"):
        assert re.search(r"\bint %s\(" % query, header) and any(name == query for name, _r, _a in L.SYMBOLS)


# ---------------------------------------------------------------------------- completeness, computed from the table
def test_every_enumerator_is_reached_by_some_case():
    L = load_pkg("_lib")
    forms = [table.expected_form(c) for c in FORM_CASES]
    split = [re.match(r"([a-z0-9]+)x(\d+)/(trips\d+)/(model|generic)(\+wide)?(\+warp)?$", f).groups() for f in forms]
    assert {s[0] for s in split} == set(L.TAIL_PARTIALS)
    assert {s[2] for s in split} == set(L.TAIL_MERGES) and {s[3] for s in split} == set(L.TAIL_HEADS)
    assert {bool(s[4]) for s in split} == {False, True} and {bool(s[5]) for s in split} == {False, True}
    for storage in ("f32", "f16"):                               # both storage types on both head forms and on the wide tail
        assert {(s[3], bool(s[4])) for s in split if s[0] == storage} >= {("model", False), ("generic", False), ("generic", True)}


def test_the_tables_cover_the_paths_the_kernels_take():
    # (a): the N and C lists; slices ragged against 64 rows, longer than 64 (second / third trip), whole waves without a row
    assert {c.N for c in table.SV} == set(table.SV_N) and {c.C for c in table.SV} == set(table.SV_C) and {c.B for c in table.SV} >= {1, 3}
    per = lambda N: -(-N // table.sv_parts(N))
    assert {-(-per(c.N) // 64) for c in table.SV} >= {1, 2, 3} and any(c.N < 4 for c in table.SV) and any(per(c.N) % 64 for c in table.SV)
    assert {c.pattern for c in table.SV} == set(table.PATTERNS) and any(c.none_element is not None for c in table.SV)
    assert any(c.C > 64 and c.C % 64 for c in table.SV) and any(c.C > 128 for c in table.SV)
    # (b): the model head and every generic shape, both storage types, with and without the coarse pose, the pose rows
    shapes = {(c.C, c.hidden) for c in table.HEAD}
    assert shapes == {table.MODEL} | set(table.GENERIC)
    for shape in shapes:
        assert {(c.storage, c.coarse) for c in table.HEAD if (c.C, c.hidden) == shape} >= {("f32", False), ("f32", True), ("f16", False), ("f16", True)} \
            or shape == table.MODEL
    assert {c.N for c in table.HEAD if (c.C, c.hidden) == table.MODEL} >= set(table.HEAD_N) and {c.pose7 for c in table.HEAD} == {"none", "row", "ring"}
    # (c): the parts list; a single trip of 16, one and two trips of 32; group 2 of the four threads sees only empty slices
    assert {c.parts for c in table.MERGE} == set(table.MERGE_PARTS) and {c.top for c in table.MERGE} == {"first", "last"}
    assert any(c.parts > 128 for c in table.MERGE) and any(64 < c.parts <= 128 for c in table.MERGE)
    for p in table.MERGE_PARTS:
        empty = table.merge_empty(p)
        assert len(empty) < p and (p < 5 or {0, p - 1} <= set(empty)) and (p < 7 or set(range(2, p, 4)) <= set(empty))
    # (d): both tile heights at every N, ragged last tiles, more than 64 and 128 tiles, an all-invalid tile, an empty element, pairs
    assert {(c.N, c.tile) for c in table.RIDE} >= {(N, t) for N in table.RIDE_N for t in (16, 32)}
    tiles = {-(-c.N // c.tile) for c in table.RIDE}
    assert {65, 129} <= tiles and any(c.N % c.tile for c in table.RIDE) and {c.storage for c in table.RIDE} == {"f32", "f16"}
    assert any(c.pattern == "tile_out" and c.none_element is not None for c in table.RIDE) and sum(c.pair for c in table.RIDE) == 2
    # (e): N around the 256 points of a workgroup, no features / even fp16 / odd fp32 channel counts, the special points
    assert {c.N for c in table.WARP} >= {1, 255, 256, 257, 600} and all(c.H * c.W <= 4 * 57 for c in table.WARP)
    assert any(c.C == 0 for c in table.WARP) and any(c.C % 2 and c.storage == "f32" for c in table.WARP)
    assert any(c.C and c.C % 2 == 0 and c.storage == "f16" for c in table.WARP)
    assert {c.pose for c in table.WARP} == {"general", "general2", "identity", "shift"}


# ---------------------------------------------------------------------------- (f) refusals, nothing launched
@pytest.mark.parametrize("case", table.REFUSALS, ids=ids)
def test_refusals(case):
    L = load_pkg("_lib")
    fields = dict(case.fields)
    if "q_coarse" not in fields and "t_coarse" not in fields:
        fields.update(q_coarse=False, t_coarse=False)
    a = fake_head(L, **fields)
    w = fake_warp(L, a, 2, 50, 4, 5, 0, other=True) if case.warp else None
    rc = L.lib().elo_pose_head_form(ctypes.byref(a), ctypes.byref(w) if w is not None else None)
    assert rc == case.status and re.search(case.match, L.lib().elo_last_error().decode())
    # the entry point itself answers the same before any HIP call (no device here: a launch could only fail differently)
    entry = L.lib().elo_pose_head_warp(ctypes.byref(a), ctypes.byref(w), None) if w is not None else L.lib().elo_pose_head(ctypes.byref(a), None)
    assert entry == case.status


def test_the_largest_head_that_fits_is_not_refused_and_an_empty_batch_stays_ok():
    L = load_pkg("_lib")
    a = fake_head(L, **table.LDS_FITS)
    assert L.tail_form_name(L.lib().elo_pose_head_form(ctypes.byref(a), None)) == "f32x2/trips16/generic"
    big = dict(next(c for c in table.REFUSALS if c.name == "f_lds_limit").fields)
    a = fake_head(L, B=0, **big)
    assert L.lib().elo_pose_head(ctypes.byref(a), None) == 0


def test_more_than_512_tiles_cannot_ride():
    assert ride_parts(table.RIDE_TOO_MANY_TILES) == 0
    assert ride_parts((8192, 16)) == 512


# ---------------------------------------------------------------------------- the reference
def test_reference_is_pinned_to_the_oracle():
    rng = np.random.default_rng(4)
    B, N, C = 3, 228, 64
    f, w = rng.normal(0, 1, (B, N, C)).astype(np.float32), rng.normal(0, 3, (B, N, C)).astype(np.float32)
    xyz = table.cloud("pin", B, N, "random", none_element=2)
    pooled, stats = R.softmax_valid(f, w, xyz)
    want = O.softmax_valid(f, w, R.valid(xyz))[:, 0]
    assert np.abs(pooled - want).max() < 2e-6 and (pooled[2] == 0).all() and (stats[2, 1] == 0).all()
    params = {"l1_big/weights": rng.normal(0, .1, (64, 256)).astype(np.float32), "l1_big/biases": rng.normal(0, .1, 256).astype(np.float32),
              "l1_q_det/weights": rng.normal(0, .1, (256, 4)).astype(np.float32), "l1_q_det/biases": rng.normal(0, .1, 4).astype(np.float32),
              "l1_t_det/weights": rng.normal(0, .1, (256, 3)).astype(np.float32), "l1_t_det/biases": rng.normal(0, .1, 3).astype(np.float32)}
    order = [params[n + k] for n in ("l1_big", "l1_q_det", "l1_t_det") for k in ("/weights", "/biases")]
    q_c, t_c = table.coarse_pose("pin", B)
    q, t, qn = R.pose(f, w, xyz, *order, q_coarse=q_c, t_coarse=t_c)
    q_det, t_det = O.pose_head(params, want[:, None].astype(np.float32), 1, False)
    oq, ot = O.compose(q_det, t_det, q_c[:, None], t_c[:, None])
    assert np.abs(q - oq).max() < 5e-6 and np.abs(t - ot).max() < 5e-6 and np.abs(qn - O.normalise_q(oq)).max() < 5e-6
    xyz_w = rng.normal(0, 5, (B, 40, 3)).astype(np.float32)
    xyz_w[:, ::7] = 0
    assert np.abs(R.warp(xyz_w, oq, ot) - O.warp(xyz_w, oq[:, None], ot[:, None])).max() < 2e-5


# ---------------------------------------------------------------------------- the emulations against float64, within HALF the bound
RATIOS = {}


def _hold(form, got, want, bound, share=0.5):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    ratio = float((np.abs(got - want) / bound).max()) if got.size else 0.0
    RATIOS[form] = max(RATIOS.get(form, 0.0), ratio)
    assert np.isfinite(bound).all() and ratio <= share, (form, ratio)
    return ratio


def _sv_inputs(case):
    f, w = table.logits_features(case.name, case.B, case.N, case.C)
    return f, w, table.cloud(case.name, case.B, case.N, case.pattern, case.none_element)


@pytest.mark.parametrize("case", table.SV, ids=ids)
def test_partial_sums_and_sv_merge_emulation(case):
    f, w, xyz = _sv_inputs(case)
    parts, ok = table.sv_parts(case.N), R.valid(xyz)
    want, stats = R.softmax_valid(f, w, xyz)
    tb = bounds.partial_sums(bounds.BND, w, f, ok, parts)
    te = bounds.partial_sums(bounds.F32, w, f, ok, parts)
    (pv, pe), Mb, (dv, de) = bounds.merge_seq(bounds.BND, tb, parts)
    got, Me, De = bounds.merge_seq(bounds.F32, te, parts)
    assert np.abs(pv - want).max() <= 1e-12 * (1 + np.abs(want).max()) and np.array_equal(Mb, stats[:, 0])    # BND's value IS the operator
    assert np.abs(dv - stats[:, 1]).max() <= 1e-12 * (1 + stats[:, 1].max())
    assert np.array_equal(Me, stats[:, 0])                       # the maximum is exact
    some = stats[:, 1] > 0
    assert (got[~some] == 0).all() and (np.asarray(De)[~some] == 0).all()
    _hold("partial+sv_merge", got[some], want[some], pe[some])
    _hold("partial+sv_merge/den", np.asarray(De)[some], stats[:, 1][some], de[some])


@pytest.mark.parametrize("case", [c for c in table.HEAD if c.pattern != "random" or c.C != 64 or c.N in (65, 4097)], ids=ids)
def test_partial_sums_and_head_merge_emulation(case):
    f, w = table.logits_features(case.name, case.B, case.N, case.C, case.storage)
    xyz = table.cloud(case.name, case.B, case.N, case.pattern)
    parts, ok = table.sv_parts(case.N), R.valid(xyz)
    want, _ = R.softmax_valid(f, w, xyz)
    pv, pe = bounds.head_pool(bounds.BND, bounds.partial_sums(bounds.BND, w, f, ok, parts), parts, case.C)
    got = bounds.head_pool(bounds.F32, bounds.partial_sums(bounds.F32, w, f, ok, parts), parts, case.C)
    assert np.abs(pv - want).max() <= 1e-12 * (1 + np.abs(want).max())
    _hold("partial+head_merge", got, want, np.maximum(pe, 1e-300))


@pytest.mark.parametrize("case", table.MERGE, ids=ids)
def test_in_head_merge_emulation(case):
    mx, den, acc = table.merge_triples(case)
    want = R.merge_triples(mx, den, acc)
    pv, pe = bounds.merge_head(bounds.BND, bounds.lift_triple(bounds.BND, mx, den, acc), case.parts)
    got = bounds.merge_head(bounds.F32, bounds.lift_triple(bounds.F32, mx, den, acc), case.parts)
    assert np.abs(pv - want).max() <= 1e-12 * (1 + np.abs(want).max())
    _hold("head_merge/trips16" if case.parts <= 64 else "head_merge/trips32", got, want, pe)
    # ... and sv_merge on the same triples (the head's channels 64.. and the stand-alone op's second launch)
    (sv, se), _m, _d = bounds.merge_seq(bounds.BND, bounds.lift_triple(bounds.BND, mx, den, acc), case.parts)
    got = bounds.merge_seq(bounds.F32, bounds.lift_triple(bounds.F32, mx, den, acc), case.parts)[0]
    assert np.abs(sv - want).max() <= 1e-12 * (1 + np.abs(want).max())
    _hold("sv_merge", got, want, se)


def test_the_merge_bound_sees_a_wrong_trip_stride_and_a_counted_empty_slice():
    """The bound has teeth: the trips32 form walked with a trip stride of 4 * 16 (slices counted twice) leaves it by orders of magnitude."""
    case = next(c for c in table.MERGE if c.parts == 257 and c.top == "last")
    mx, den, acc = table.merge_triples(case)
    want = R.merge_triples(mx, den, acc)
    _pv, pe = bounds.merge_head(bounds.BND, bounds.lift_triple(bounds.BND, mx, den, acc), case.parts)
    wrong = bounds.merge_head(bounds.F32, bounds.lift_triple(bounds.F32, mx, den, acc), case.parts, mine=32, stride=64)
    assert (np.abs(wrong - want) / pe).max() > 100


def test_expf_in_the_four_to_one_combine_is_an_equivalent_mutant():
    """exp_acc replaced by the library expf in the head's 4-to-1 combine cannot be told apart within the derived bound: the four
    arguments are differences of maxima (a handful of units at most where a group still counts), where one ulp of either
    exponential is far inside the (3|x| + 2) u the bound grants -- the emulation of the mutant stays within half the bound as well."""
    worst = 0.0
    for case in table.MERGE:
        mx, den, acc = table.merge_triples(case)
        want = R.merge_triples(mx, den, acc)
        _pv, pe = bounds.merge_head(bounds.BND, bounds.lift_triple(bounds.BND, mx, den, acc), case.parts)
        got = bounds.merge_head(bounds.F32, bounds.lift_triple(bounds.F32, mx, den, acc), case.parts, combine_libm=True)
        worst = max(worst, _hold("head_merge/expf-combine (mutant)", got, want, pe))
    assert worst <= 0.5


@pytest.mark.parametrize("case", table.RIDE, ids=ids)
def test_tile_ride_emulation(case):
    """mlp_sv_kernel's reduction on stand-in logits (the MLP that produces them is tests/test_fused_shapes_*'s subject)."""
    f, w = table.logits_features(case.name, case.B, case.N, 64, case.storage)
    xyz = table.ride_cloud(case)
    ok = R.valid(xyz)
    want, _ = R.softmax_valid(f, w, xyz)
    tiles = -(-case.N // case.tile)
    assert ride_parts(case) == tiles                             # the expected `parts` is the library's
    tb = bounds.ride_sums(bounds.BND, w, f, ok, case.tile)
    te = bounds.ride_sums(bounds.F32, w, f, ok, case.tile)
    pv, pe = bounds.merge_head(bounds.BND, tb, tiles)
    got = bounds.merge_head(bounds.F32, te, tiles)
    assert np.abs(pv - want).max() <= 1e-12 * (1 + np.abs(want).max())
    _hold("ride+head_merge", got, want, np.maximum(pe, 1e-300))
    if case.pattern == "tile_out":                               # the all-invalid tile holds what the kernel writes there
        assert np.isneginf(te[0][:, 1]).all() and (te[1][:, 1] == 0).all() and (te[2][:, 1] == 0).all()


def test_head_and_composition_bound_holds_for_float32_arithmetic():
    """The dense layers and the composition in plain float32 (sequential sums) stay within half their bound on random weights."""
    F = np.float32
    for C, hidden in (table.MODEL,) + table.GENERIC:
        name = "headbound_%d_%d" % (C, hidden)
        rng = table.rng_of(name)
        B = 3
        pooled = rng.normal(0, 1, (B, C)).astype(F)
        Wb, bb, Wq, bq, Wt, bt = table.head_weights(name, C, hidden)
        q_c, t_c = table.coarse_pose(name, B)
        for coarse in (False, True):
            raw, _big = R.head(pooled, Wb, bb, Wq, bq, Wt, bt)
            e_raw = bounds.head_bound(pooled, np.zeros((B, C)), Wb, bb, Wq, bq, Wt, bt)
            big32 = bb.copy()[None].repeat(B, 0)
            for c in range(C):
                big32 = (big32 + (pooled[:, c:c + 1] * Wb[c][None]).astype(F)).astype(F)
            raw32 = np.concatenate([bq[None].repeat(B, 0), bt[None].repeat(B, 0)], -1)
            W7 = np.concatenate([Wq, Wt], -1)
            for j in range(hidden):
                raw32 = (raw32 + (big32[:, j:j + 1] * W7[j][None]).astype(F)).astype(F)
            _hold("head/raw", raw32, raw, e_raw)
            args = (q_c, t_c) if coarse else (None, None)
            want = R.compose(raw, *args)
            eb = bounds.pose_bound(R, raw, e_raw, *args)
            got = O.compose(O.normalise_q(raw32[:, None, :4]), raw32[:, None, 4:], q_c[:, None], t_c[:, None]) if coarse else \
                (O.normalise_q(raw32[:, :4]), raw32[:, 4:])
            _hold("head/q", got[0], want[0], eb[0])
            _hold("head/t", got[1], want[1], eb[1])
            _hold("head/q_norm", O.normalise_q(got[0]), want[2], eb[2])


# ---------------------------------------------------------------------------- (e) the cell tests' cap, on the reference alone
@pytest.mark.parametrize("case", table.WARP, ids=ids)
def test_warp_cases_stay_under_the_excluded_cap_and_hold_their_special_points(case):
    xyz, special = table.warp_cloud(case, R)
    _Wb, _bb, _Wq, b_q, _Wt, b_t = table.pose_weights(case, case.B)
    q, t, _qn = R.compose(np.concatenate([b_q, b_t])[None].repeat(case.B, 0).astype(np.float64))
    warped = R.warp(xyz, q, t)
    col, tmp, r = R.cell_coordinates(warped, case.H, case.W)
    near = lambda v: np.abs(v - np.round(v)) < table.BORDER
    excluded = ((near(col) | near(tmp)) & (r > 0)) | ((r > 0) & (r < table.ORIGIN_RANGE))
    assert excluded.mean(-1).max() <= table.EXCLUDED_CAP and excluded.sum() == (case.B if "origin" in special else 0)   # (drawn 0.2 of a cell inside)
    assert (R.valid(xyz).sum(-1) >= min(case.N, 1)).all()
    cell = R.cells(warped, case.H, case.W)
    if "ties" in special:
        for b in range(case.B):
            _img, _f, won = R.project(warped[b].astype(np.float32), None, cell[b], case.H, case.W)
            for i, j in special["ties"]:
                assert cell[b, i] == cell[b, j] and won[i] and won[j]
        assert np.array_equal(warped.astype(np.float32)[R.valid(xyz)], xyz[R.valid(xyz)])   # the identity pose passes points through
    if "origin" in special:                                      # float32 statement: the valid point lands on (+0, +0, +0), zero cell kind 0
        i = special["origin"]
        w32 = R.warp32(xyz, q, t)
        assert R.valid(xyz)[:, i].all() and (w32[:, i] == 0).all() and not np.signbit(w32[:, i]).any()
        assert (R.cells(w32.astype(np.float64), case.H, case.W)[:, i] == (case.H - 1) * case.W + case.W // 2).all()
        assert r[:, i].max() < table.ORIGIN_RANGE and 1.0 / case.N <= table.EXCLUDED_CAP    # (float64 leaves it 1e-10 beside the origin)
        assert np.array_equal(w32.view(np.uint32)[~R.valid(xyz)], warped.astype(np.float32).view(np.uint32)[~R.valid(xyz)])
    zeros = ~R.valid(xyz)
    if zeros.any():                                              # the zero cell of the case's pose (pose_tail_cases.py: by the signs of t)
        kind_col = {"general": case.W // 2, "identity": case.W // 2, "general2": 0, "shift": case.W - 1}[case.pose]
        assert (cell[zeros] == (case.H - 1) * case.W + kind_col).all()


def test_zz_print_the_emulations_ratios(capsys):
    with capsys.disabled():
        for form in sorted(RATIOS):
            print("\nPOSE_TAIL_CPU %-28s worst emulation error / bound = %.3f" % (form, RATIOS[form]), end="")

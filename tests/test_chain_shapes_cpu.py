"""CPU: the case table of tests/chain_shapes_cases.py against the library's own launch ladders (the elo_*_form queries on fake
addresses: every run answers the chain form under the table's tuning, the ladder's edges answer tile forms), the table's
completeness computed from the table, and the bounds of tests/fused_shapes_bounds.py on these inputs before any GPU sees them: a
float32 emulation of the product schemes within the bound at half units, a plain sequential accumulation within the full bound, and
the same emulation WITHOUT the weights' lo product beyond the full bound on every split-products case."""
import ctypes

import numpy as np
import pytest

import chain_shapes_cases as chain
import fused_shapes_bounds as bounds
import fused_shapes_reference as R
from conftest import load_pkg
from oracle import grouping as G
from oracle import ops_np as O
from test_fused_shapes_cpu import _f32_geometry, _f32_softmax_pool, _store, _worst, fake_cv, fake_mlp, fake_setconv


def _no_chain_kernels():
    return bool(load_pkg("_lib").lib().elo_dense_f32())              # the fp32-MFMA comparison build


def _fake(part, case, storage, products, job=0, **over):
    L = load_pkg("_lib")
    if part == "mlp":
        f = dict(srcs=(64, case.C), layers=(128, 64), rows=case.rows, stage2=(case.C, 64, (128, 64)))
        f.update(over)
        return fake_mlp(L, f["srcs"], f["layers"], f["rows"], f["stage2"], storage, products)
    if part == "setconv":
        f = dict(K=case.K, C=64, layers=case.layers, group=case.group, idx_out=False)
        f.update(over)
        return fake_setconv(L, case.B, case.n, f["K"], f["C"], f["layers"], case.centre, f["group"], storage, products, grid=case.grid,
                            idx_out=f["idx_out"])
    return fake_cv(L, case.stage, case.B, case.K, over.get("C", case.C), storage, products, grid=case.grid, n=case.n)


def ask(part, case, storage, products, tuning_fields=chain.CHAIN_TUNING, tweak=None, **over):
    """the form's name (or the negative status) of a table case, asked of the library under the tuning the GPU test runs it with"""
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    lib = L.lib()
    with tuning.override(**tuning_fields):
        a = _fake(part, case, storage, products, **over)
        if tweak:
            tweak(a)
        if part in ("mlp", "setconv"):
            b = _fake(part, case, storage, products, 1, **over) if case.pair else None
            query = lib.elo_mlp_fused_form if part == "mlp" else lib.elo_setconv_fused_form
            rc = query(ctypes.byref(a), ctypes.byref(b) if b is not None else None)
        else:
            rc = (lib.elo_cv_stage1_form if case.stage == 1 else lib.elo_cv_stage2_form)(ctypes.byref(a))
    return L.fused_form_name(rc) if rc >= 0 else rc


ALL_RUNS = [(part,) + run for part in ("cv", "setconv", "mlp") for run in chain.runs(part)]
_ids = lambda v: v if isinstance(v, str) else v.name


@pytest.mark.parametrize("part,case,storage,products", ALL_RUNS, ids=_ids)
def test_case_takes_the_chain_form(part, case, storage, products):
    if _no_chain_kernels():
        pytest.skip("the fp32-MFMA comparison build has no chain kernels")
    assert ask(part, case, storage, products) == "chain/" + products
    twin = ask(part, case, storage, products, chain.TILE_TUNING)       # the same call with the chain forms off: its tile twin
    assert twin in ("tile16/" + products, "tile32/" + products), twin


@pytest.mark.parametrize("case,storage,products", chain.runs("pair"), ids=_ids)
def test_pair_case_takes_the_heterogeneous_chain_launch(case, storage, products):
    if _no_chain_kernels():
        pytest.skip("the fp32-MFMA comparison build has no chain kernels")
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    query = L.lib().elo_cv_stage1_setconv_chain_form
    blocks = lambda: [ctypes.byref(x) for x in (_fake("cv", case.cv, storage, products), _fake("setconv", case.sc, storage, products),
                                                _fake("setconv", case.sc, storage, products, 1))]
    with tuning.override(**chain.CHAIN_TUNING):
        assert query(*blocks()) == 1
        assert ask("cv", case.cv, storage, products) == "chain/" + products == ask("setconv", case.sc, storage, products)
    with tuning.override(**chain.TILE_TUNING):
        assert query(*blocks()) == 0


# ---------------------------------------------------------------------------- the ladder's edges answer tile forms
def test_the_edges_of_the_ladders_answer_tile_forms():
    if _no_chain_kernels():
        pytest.skip("the fp32-MFMA comparison build has no chain kernels")
    by = {c.name: c for part in ("cv", "setconv", "mlp") for c in chain.CASES[part]}
    tile = lambda form: isinstance(form, str) and form.startswith("tile")
    for name in ("d01", "e01"):
        assert ask("cv", by[name], "f32", "split") == "chain/split"
        for C in (8, 24, 40):                                          # no chain instance for these channel counts
            assert tile(ask("cv", by[name], "f32", "split", C=C)), (name, C)
        checked = ask("cv", by[name], "f32", "split", dict(chain.CHAIN_TUNING, range_check=1))
        assert checked in ("tile16/checked", "tile32/checked"), checked
        assert tile(ask("cv", by[name], "f32", "split", chain.TILE_TUNING))
    sc = by["f01"]
    assert ask("setconv", sc, "f32", "split") == "chain/split"
    assert tile(ask("setconv", sc, "f32", "split", K=12))
    assert tile(ask("setconv", sc, "f32", "split", C=32))
    assert tile(ask("setconv", sc, "f32", "split", layers=(64, 64)))
    assert tile(ask("setconv", sc, "f32", "split", idx_out=True))
    assert ask("setconv", sc, "f32", "split", dict(chain.CHAIN_TUNING, range_check=1)).endswith("/checked")
    wide = by["f06"]                                                   # 16 x 32 = 512 slots: the chain; 27 x 19 = 513: the tile kernel
    assert wide.group[0] * wide.group[1] == 512 and ask("setconv", wide, "f32", "split") == "chain/split"
    assert tile(ask("setconv", wide, "f32", "split", group=(27, 19) + wide.group[2:]))
    mlp = by["g05"]
    assert ask("mlp", mlp, "f32", "split") == "chain/split"

    def shifted(a):
        a.src[1] = a.src[1] + 4                                        # a source at a 4-byte offset: no 16-byte vector loads
    assert tile(ask("mlp", mlp, "f32", "split", tweak=shifted))
    assert tile(ask("mlp", mlp, "f32", "split", layers=(128, 32)))
    assert ask("mlp", mlp, "f32", "split", dict(chain.CHAIN_TUNING, range_check=1)).endswith("/checked")
    # the default tuning (row thresholds -1): cases this small answer tile forms
    for part in ("setconv", "mlp"):
        for case in chain.CASES[part]:
            assert tile(ask(part, case, "f16", "half", dict(chain_forms=1))), case.name


# ---------------------------------------------------------------------------- completeness, computed from the table
def test_part_a_covers_the_pools_the_chunks_and_the_workgroup_counts():
    cv = chain.CV
    assert {c.K for c in cv} == set(chain.CV_K) and {c.C for c in cv} == set(chain.CV_CHANNELS)
    for stage in (1, 2):
        mine = [c for c in cv if c.stage == stage]
        for C in chain.CV_CHANNELS:                                    # every (C, storage, products) instance at two or more K
            assert len({c.K for c in mine if c.C == C}) >= 2, (stage, C)
        assert sum(c.far for c in mine) == 1 and all(not c.relu_last for c in mine if c.far)
        assert any(c.n != c.grid[0] * c.grid[1] for c in mine) == (stage == 1)
        assert {chain.cv_pool(c) for c in mine} == ({"k6", "chunks"} if stage == 1 else {"k6", "chunks", "inwave4"})
    # stage 2 at K = 4: the in-wave pool with the ReLU, the LDS pool without it and with ordinary logits
    assert any(c.stage == 2 and c.K == 4 and c.relu_last for c in cv)
    assert any(c.stage == 2 and c.K == 4 and not c.relu_last and not c.far for c in cv)
    # the generic loop: one full chunk, partial chunks, two to four chunks with and without a ragged tail
    generic = {chain.chunks(c.K) for c in cv if chain.cv_pool(c) == "chunks"}
    assert {(1, 8), (2, 8), (4, 8)} <= generic and {(1, k) for k in (1, 2, 3, 5, 7)} <= generic
    assert {(2, 1), (2, 4), (3, 4), (4, 7)} <= generic
    assert {n for n, _last in generic} == {1, 2, 3, 4}
    # K that divide 128 and K that leave dead rows; K that straddle the 16-row waves
    assert any(chain.ROWS % c.K == 0 for c in cv) and {chain.ROWS - chain.per_workgroup(K) * K for K in chain.CV_K} >= {0, 2, 3, 4, 8}
    assert any(16 % c.K for c in cv) and any(16 % c.K == 0 for c in cv)
    rel = {chain.points_of(c) - chain.per_workgroup(c.K) for c in cv}
    assert {-1, 0, 1} <= rel and any(chain.points_of(c) == 1 for c in cv)
    assert {chain.workgroups(c) for c in cv} >= {1, 3, 7, 8, 9, 17}
    assert all(chain.workgroups(c) <= 17 and chain.points_of(c) * c.K < 2200 for c in cv)
    # one point in the last workgroup, behind fewer than 8, exactly 8 and 8 q + r workgroups
    assert any(chain.workgroups(c) > 1 and chain.points_of(c) % chain.per_workgroup(c.K) == 1 for c in cv)
    assert {c.B for c in cv} == {1, 3}
    assert any(c.B == 3 and c.n % chain.per_workgroup(c.K) for c in cv)               # a batch seam inside a workgroup
    assert len({c.name for c in cv}) == len(cv)


def test_part_b_covers_the_shapes_the_pools_the_centres_and_the_windows():
    sc = chain.SETCONV
    assert {(c.layers, c.K) for c in sc} >= {(s, K) for s in (chain.S1, chain.S2, chain.S3) for K in (8, 16, 32)}
    for K in (8, 16):
        assert {chain.setconv_pool(c) for c in sc if c.K == K} == {"inwave", "lds"}, K
    assert {chain.setconv_pool(c) for c in sc if c.K == 32} == {"lds"} and {c.relu_last for c in sc if c.K == 32} == {True, False}
    assert any(not c.relu_last and len(c.layers) == 3 and c.layers[-1] == 128 for c in sc)   # four passes of the last layer, LDS pool
    assert {c.centre for c in sc} == {"hw", "pixel"} and {c.pair for c in sc} == {True, False}
    assert {c.group[3:] for c in sc} == {(1, 1), (2, 2), (1, 2)}
    slots = lambda c: c.group[0] * c.group[1]
    assert any(slots(c) < c.K for c in sc) and any(slots(c) > 64 for c in sc) and any(slots(c) == 512 and c.grid[1] >= 16 for c in sc)
    assert all(slots(c) <= 512 for c in sc)
    rel = {chain.points_of(c) - chain.per_workgroup(c.K) for c in sc}
    assert {-1, 0, 1} <= rel and {chain.workgroups(c) for c in sc} >= {1, 9} and {c.B for c in sc} == {1, 3}
    assert any(c.B == 3 and c.n % chain.per_workgroup(c.K) for c in sc)
    assert all(chain.workgroups(c) <= 17 for c in sc)
    short = none = halves = False
    for case in sc:
        inp = chain.setconv_inputs(case, "f32")
        centre, (_idx, mask) = chain.setconv_centres(inp), _slots(case, inp)
        found = mask.sum(-1)
        invalid = (centre == 0).all(-1)
        assert invalid.any(), case.name                                 # an all-zero centre ...
        assert (found[invalid] == 0).all()
        if case.centre == "hw":                                         # ... and a repeated one in the list
            hw = inp["centre_hw"]
            assert (hw[:, 2] == hw[:, 3]).all() and (hw[:, 0] == np.array(inp["xyz1_grid"].shape[1:3]) - 1).all(), case.name
        short = short or bool(((found > 0) & (found < case.K)).any())
        if case.K == 16 and chain.setconv_pool(case) == "inwave":      # the in-wave maximum's last step joins rows 0..7 and 8..15 of a point
            halves = halves or bool((mask[..., 8:].sum(-1) >= 4).sum() >= 4)
        if case.group[2] < 100:
            none = none or bool(((found == 0) & ~invalid).any())
    assert short and none and halves     # a radius that leaves centres short of K neighbours; a non-zero centre that finds none


def test_part_c_covers_the_rows_the_channels_and_the_flags():
    mlp = chain.MLP
    assert {c.rows for c in mlp} == {1, 15, 16, 17, 127, 128, 129, 1025} and {c.C for c in mlp} == set(chain.CV_CHANNELS)
    assert {c.pair for c in mlp} == {True, False} and {c.relu_last for c in mlp} == {(a, b) for a in (True, False) for b in (True, False)}
    assert [c.pair for c in mlp if c.clear] == [True]
    assert {chain.workgroups(c) for c in mlp} == {1, 2, 9}


def test_part_d_covers_the_sub_grids():
    assert [(chain.workgroups(c.cv), chain.workgroups(c.sc)) for c in chain.PAIR] == [(1, 1), (3, 5), (9, 8)]
    assert all(c.cv.stage == 1 and c.sc.layers == chain.S1 and c.sc.pair for c in chain.PAIR)
    assert {c.cv.C for c in chain.PAIR} == set(chain.CV_CHANNELS) and {c.sc.K for c in chain.PAIR} == {8, 16, 32}


def test_mask_patterns_of_the_pregrouped_inputs():
    """per batch element an all-clear point, a point with one live slot and an all-set point; clear slots gather cell (0, 0, 0)"""
    for case in chain.CV + [c.cv for c in chain.PAIR]:
        inp = chain.cv_inputs(case, "f32")
        per_point = inp["mask"].sum(-1)
        assert (inp["idx"][inp["mask"] == 0] == 0).all()
        if case.n >= 3:
            assert all({0, 1, case.K} <= set(per_point[b].astype(int)) or case.K == 1 for b in range(case.B)), case.name


# ---------------------------------------------------------------------------- a correct implementation fits the bound, a wrong one does not
_SLOTS = {}


def _slots(case, inp, job=0):
    """idx / mask of a set-conv case from the grouping oracle, for the case's centres"""
    hit = _SLOTS.get((case.name, job))
    if hit is None:
        kh, kw, dist, sh, sw = case.group
        grid = inp["xyz1_grid"]
        B, H, W, _ = grid.shape
        centres = inp["centre_hw"] if "centre_hw" in inp else O.get_hw_idx(B, H, W)
        sel, _valid, _indis, mask = G.fused_conv_random_k(grid, inp["src_xyz"], np.ascontiguousarray(centres), inp["order"], H, W, centres.shape[1],
                                                          kh, kw, case.K, 0, dist, sh, sw)
        mask = mask.reshape(B, centres.shape[1], case.K)
        assert 0 < mask.mean() < 1 and (sel[mask == 0] == 0).all(), case.name
        hit = _SLOTS[(case.name, job)] = (sel, mask)
    return hit


def _emulate_mlp(case, storage, products, **emu):
    """[(what, emulated fp32 value, expect(**kwargs) -> (want, bound))] of an MLP case's two outputs"""
    inp = chain.mlp_inputs(case, storage)
    got = bounds.emulate_chain(np.concatenate(inp["sources"], -1), inp["layers"], products, **emu)
    stored = _store(got, storage)                                     # the second stage continues with the first one AS STORED
    got2 = bounds.emulate_chain(np.concatenate([inp["before"], stored, inp["after"]], -1), inp["layers2"], products, **emu)
    return [("out", got, lambda **kw: bounds.mlp_expect(R, inp, products, storage, **kw)),
            ("out2", got2, lambda **kw: bounds.mlp_expect(R, inp, products, storage, first_stage=stored.astype(np.float64), **kw))]


def _emulate_setconv(case, storage, products, **emu):
    inp = chain.setconv_inputs(case, storage)
    centre, (idx, mask) = chain.setconv_centres(inp), _slots(case, inp)
    m = mask[..., None]
    g = lambda grid: grid[idx[..., 0], idx[..., 1], idx[..., 2]]
    x = np.concatenate([g(inp["src_xyz"]) * m - centre[:, :, None, :], g(inp["src_feat"]) * m], -1).astype(np.float32)
    got = (bounds.emulate_chain(x, inp["layers"], products, **emu) * m).max(axis=2)
    return [("pooled", got, lambda **kw: bounds.setconv_expect(R, inp, centre, idx, mask, products, storage, **kw))]


def _emulate_cv(case, storage, products, **emu):
    inp = chain.cv_inputs(case, storage)
    idx, mask, L = inp["idx"], inp["mask"], inp["layers"]
    m = mask[..., None]
    g = lambda grid: grid[idx[..., 0], idx[..., 1], idx[..., 2]]
    em = lambda x, names: bounds.emulate_chain(x, [L[n] for n in names], products, **emu)
    half = products == "half"
    if case.stage == 1:
        geo = _f32_geometry(inp["xyz1"], g(inp["xyz2"]), m)
        f1 = np.broadcast_to(inp["feat1"][:, :, None, :], idx.shape[:3] + (case.C,))
        x = em(np.concatenate([geo, f1, g(inp["feat2"]) * m], -1), ["cv0", "cv1", "cv2"])
        logits = em(np.concatenate([em(geo, ["cv_xyz"]), x], -1), ["sum_cv0", "sum_cv1"])
        values = x.astype(np.float16).astype(np.float32) if half else x
        expect = bounds.cv1_expect
    else:
        B, H, W, C = inp["feat1"].shape
        geo = _f32_geometry(inp["xyz1"].reshape(B, H * W, 3), g(inp["xyz1"]), m)
        grouped = (g(inp["cost"]) * m).astype(np.float32)
        f1 = np.broadcast_to(inp["feat1"].reshape(B, H * W, 1, C), idx.shape[:3] + (C,))
        logits = em(np.concatenate([em(geo, ["xyz_enc"]), f1, grouped], -1), ["sum_cost0", "sum_cost1"])
        values = grouped.astype(np.float16).astype(np.float32) if half else grouped
        expect = bounds.cv2_expect

    def expected(**kw):
        want, bound, spread = expect(R, inp, products, storage, **kw)
        assert case.far or spread < 30.0, "the first-order softmax term needs |l - max| < 30 on the slots that carry weight (%.1f)" % spread
        return want, bound
    return [("pooled", _f32_softmax_pool(logits, values, mask), expected)]


_EMULATE = {"mlp": _emulate_mlp, "setconv": _emulate_setconv, "cv": _emulate_cv}
_PAIR_RUNS = [(part, c.cv if part == "cv" else c.sc, s, p) for part in ("cv", "setconv") for c, s, p in chain.runs("pair")]


@pytest.mark.parametrize("part,case,storage,products", ALL_RUNS + _PAIR_RUNS, ids=_ids)
def test_emulation_stays_within_the_bound_at_half_units(part, case, storage, products):
    for what, got, expected in _EMULATE[part](case, storage, products):
        with bounds.units_scaled(0.5):
            want, bound = expected(stored=False)
        _worst(got, want, bound, what)


@pytest.mark.parametrize("part,case,storage,products", ALL_RUNS + _PAIR_RUNS, ids=_ids)
def test_plain_float32_accumulation_stays_within_the_full_bound(part, case, storage, products):
    for what, got, expected in _EMULATE[part](case, storage, products, sequential=True):
        want, bound = expected(stored=False)
        _worst(got, want, bound, what + ", plain float32 accumulation")


def depends_on_a_product(part, case):
    """stage 2 pools the GATHERED cost: where the logits cannot move the weights (far: fp32 cannot resolve them at -3e10) nothing
    of its output comes from a matrix product"""
    return not (part == "cv" and case.stage == 2 and case.far)


_SPLIT_RUNS = [r for r in ALL_RUNS + _PAIR_RUNS if r[3] == "split" and depends_on_a_product(r[0], r[1])]


@pytest.mark.parametrize("part,case,storage,products", _SPLIT_RUNS, ids=_ids)
def test_the_bound_tells_a_dropped_lo_product_from_rounding(part, case, storage, products):
    """the emulation with the weights' lo product left out -- a 2^-12 mistake per term -- exceeds the FULL bound somewhere, on every
    split-products run (none may fail to show it)"""
    beyond = 0
    for _what, got, expected in _EMULATE[part](case, storage, products, drop_w_lo=True):
        want, bound = expected(stored=False)
        beyond += int((np.abs(np.asarray(got, np.float64) - want) > bound).sum())
    assert beyond > 0, "%s: a dropped lo product stays within the bound everywhere" % case.name


def test_the_far_stage_2_case_is_the_only_run_left_out_of_the_dropped_product_test():
    left = {r[1].name for r in ALL_RUNS + _PAIR_RUNS if r[3] == "split"} - {r[1].name for r in _SPLIT_RUNS}
    assert left == {c.name for c in chain.CV if c.stage == 2 and c.far}


def test_in_wave_softmax_needs_no_more_roundings_than_n_pool():
    """rr_pool_softmax4_inwave: three scan adds per sum, the product e * v, one divide -- softmax_chunk8's order, without its merge"""
    assert 3 + 1 + 1 <= bounds.n_pool(4)

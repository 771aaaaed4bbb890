"""CPU: the case table of tests/fused_shapes_cases.py against the library's own launch ladders (the elo_*_form queries of the fused
entry points read the argument block only: no GPU, fake addresses), the table's completeness computed from the table, the
refusals of part D with nothing launched, the float64 statements of tests/fused_shapes_reference.py against oracle/ops_np.py, and
a float32 emulation of the split and half product schemes held within HALF of the bound tests/fused_shapes_bounds.py derives."""
import ctypes
import os
import re

import numpy as np
import pytest

import fused_shapes_bounds as bounds
import fused_shapes_cases as table
import fused_shapes_reference as R
from conftest import ROOT, load_pkg
from oracle import grouping as G
from oracle import ops_np as O
from util_params import shuffle_fn

BASE = 0x7f0000000000                                    # fake device addresses, 4 KB apart and 16-byte aligned: never dereferenced
PRODUCTS = {"split": 0, "half": 1, "checked": 0}


def _ptr(i):
    return BASE + 4096 * i


def _dense(L, K, N, products="split"):
    return L.Dense(_ptr(90), _ptr(91), K, N, 1, None, PRODUCTS[products])


def _chain(L, K, widths, products="split", mixed=False):
    arr = (L.Dense * 3)()
    for i, n in enumerate(widths):
        arr[i] = _dense(L, K, n, "half" if mixed and i == len(widths) - 1 and products == "split" else products)
        K = n
    return arr


def fake_mlp(L, srcs, layers, rows, stage2=None, storage="f32", products="split", mixed=False):
    a = L.MlpArgs()
    a.rows, a.n_sources, a.n_layers, a.out = rows, len(srcs), len(layers), _ptr(10)
    a.layers = _chain(L, sum(srcs), layers, products, mixed)
    a.feat_dtype = L.ELO_F16 if storage == "f16" else L.ELO_F32
    for i, w in enumerate(srcs):
        a.src[i], a.src_width[i] = _ptr(1 + i), w
    if stage2:
        wb, wa, l2 = stage2
        a.n_layers2, a.layers2, a.out2 = len(l2), _chain(L, wb + layers[-1] + wa, l2, products), _ptr(11)
        a.before, a.w_before, a.after, a.w_after = (_ptr(12) if wb else None), wb, (_ptr(13) if wa else None), wa
    return a


def fake_setconv(L, B, n, K, C, layers, centre="xyz", group=None, storage="f32", products="split", mixed=False, grid=None, idx_out=False):
    """grid: the queried (H2, W2) where it is not the table's 3 x 7; idx_out: the grouping also returns its indices and mask"""
    H2, W2 = grid or table.GRID
    H = W = 0
    spec = L.GroupSpec(None, 0, 0, 0.0, 0, 0, None, None, None)
    if group:
        kh, kw, dist, sh, sw = group
        H, W = H2 * sh - (sh - 1), W2 * sw - (sw - 1)
        spec = L.GroupSpec(_ptr(20), kh, kw, dist, sh, sw, _ptr(45) if idx_out else None, _ptr(46) if idx_out else None, None)
    elif centre == "hw":
        H, W = 5, 9
    return L.SetconvArgs(B, n, K, H, W, H2, W2, C, _ptr(21) if H else None, _ptr(22) if centre == "hw" else None,
                         _ptr(23) if centre == "xyz" else None, _ptr(24), _ptr(25) if C else None,
                         None if group else _ptr(26), None if group else _ptr(27), len(layers), _chain(L, 3 + C, layers, products, mixed),
                         _ptr(28), _ptr(29) if centre == "hw" else None, spec, L.ELO_F16 if storage == "f16" else L.ELO_F32)


def fake_cv(L, stage, B, K, C, storage="f32", products="split", mixed=False, grid=None, n=None):
    """grid: the queried (H, W) where it is not the table's 3 x 7; n: stage 1's points per batch element where they are not H * W"""
    H, W = grid or table.GRID
    n = H * W if n is None else n
    code = L.ELO_F16 if storage == "f16" else L.ELO_F32
    none = L.GroupSpec(None, 0, 0, 0.0, 0, 0, None, None, None)
    d = lambda k, n, last=False: _dense(L, k, n, "half" if mixed and last and products == "split" else products)
    if stage == 1:
        return L.Cv1Args(B, n, K, H, W, C, _ptr(30), _ptr(31), _ptr(32), _ptr(33), _ptr(34), _ptr(35), d(10 + 2 * C, 128), d(128, 64),
                         d(64, 64), d(10, 64), d(128, 128), d(128, 64, True), _ptr(36), none, code)
    return L.Cv2Args(B, n, K, H, W, C, _ptr(30), _ptr(31), _ptr(32), _ptr(34), _ptr(35), d(10, 64), d(128 + C, 128), d(128, 64, True),
                     _ptr(36), none, code)


def ask(part, case, storage, products):
    """(the form's name or the negative status) of a table case, asked of the library under the tuning the GPU test runs it with"""
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(case.tile), range_check=1 if products == "checked" else 0):
        if part == "mlp":
            a = fake_mlp(L, case.srcs, case.layers, case.rows, case.stage2, storage, products)
            b = fake_mlp(L, case.srcs, case.layers, case.rows, case.stage2, storage, products) if case.pair else None
            rc = L.lib().elo_mlp_fused_form(ctypes.byref(a), ctypes.byref(b) if b is not None else None)
        elif part == "setconv":
            a = fake_setconv(L, case.B, case.n, case.K, case.C, case.layers, case.centre, case.group, storage, products)
            b = fake_setconv(L, case.B, case.n, case.K, case.C, case.layers, case.centre, case.group, storage, products) if case.pair else None
            rc = L.lib().elo_setconv_fused_form(ctypes.byref(a), ctypes.byref(b) if b is not None else None)
        else:
            a = fake_cv(L, case.stage, case.B, case.K, table.cv_channels(case, storage), storage, products)
            rc = (L.lib().elo_cv_stage1_form if case.stage == 1 else L.lib().elo_cv_stage2_form)(ctypes.byref(a))
    return L.fused_form_name(rc) if rc >= 0 else rc


ALL_RUNS = [(part,) + run for part in ("mlp", "setconv", "cv") for run in table.runs(part)]


@pytest.mark.parametrize("part,case,storage,products", ALL_RUNS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_case_takes_the_form_it_names(part, case, storage, products):
    assert ask(part, case, storage, products) == table.expected_form(case, products)


def test_enumerators_of_the_header_and_the_binding_agree():
    L = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "elo.h")).read()
    enums = {name: int(v) for name, v in re.findall(r"\b(ELO_FUSED_[A-Z_]+)\s*=\s*(\d+)", header)}
    families = [n[len("ELO_FUSED_"):].lower() for n, _ in sorted(enums.items(), key=lambda nv: nv[1]) if n[10:] not in ("SPLIT", "HALF", "CHECKED")]
    assert tuple(families) == L.FUSED_FAMILIES and [enums["ELO_FUSED_" + f.upper()] for f in families] == list(range(len(families)))
    assert tuple(enums["ELO_FUSED_" + p.upper()] for p in L.FUSED_PRODUCTS) == (0, 1, 2)
    macro = re.search(r"#define ELO_FUSED_FORM\(family, rows, products\) \(\(family\) \| \(rows\) << (\d+) \| \(products\) << (\d+)\)", header)
    assert macro and (int(macro.group(1)), int(macro.group(2))) == (4, 12)
    assert L.fused_form_name(1 | 0 << 4 | 1 << 12) == "chain/half" and L.fused_form_name(0 | 16 << 4 | 2 << 12) == "tile16/checked"
    assert L.fused_form_name(4 | 32 << 4) == "sv_ride32/split"
    for query in L.FUSED_QUERIES:
        assert re.search(r"\bint %s\(" % query, header) and any(name == query for name, _r, _a in L.SYMBOLS)


# ---------------------------------------------------------------------------- completeness, computed from the table
def test_part_a_covers_the_k_loop_the_column_blocks_and_the_gathers():
    mlp = table.MLP
    classes = {table.k_loop_class(k) for c in mlp for k in table.layer_inputs(c)}
    first = {table.k_loop_class(table.layer_inputs(c)[0]) for c in mlp} | \
            {table.k_loop_class(c.stage2[0] + c.layers[-1] + c.stage2[1]) for c in mlp if c.stage2}    # the layers fed by a gather
    want = {(np_, tail) for np_ in range(7) for tail in (False, True)} - {(0, False)}                    # (K >= 1: at least one block)
    assert first == want and classes == want, (sorted(want - first), sorted(want - classes))
    widths = {n for c in mlp for n in table.layer_widths(c)}
    assert {-(-n // 16) for n in widths} == set(range(1, 9))                                             # CB = 1..8
    assert {1, 5, 16, 20, 40, 50, 72, 100, 128} <= widths and any(n % 4 for n in widths) and any(n % 16 and n % 4 == 0 for n in widths)
    for tile in (16, 32):
        for tpw in (1, 2):                               # column blocks per wave: 1 up to four blocks, 2 above
            assert any(c.tile == tile and (-(-n // 16) > 4) == (tpw == 2) for c in mlp for n in table.layer_widths(c)), (tile, tpw)
        # every (pairs, tail) class with one and with two row blocks
        assert {table.k_loop_class(k) for c in mlp if c.tile == tile for k in table.layer_inputs(c)} == want, tile
    assert {c.srcs for c in mlp} >= {(1,), (3,), (7,), (20,), (33,), (64, 6), (8, 8, 8), (40, 24, 12), (128, 64), (64, 64, 64)}
    assert {c.rows for c in mlp} == {1, 15, 16, 17, 33, 95} and {len(c.layers) for c in mlp} == {1, 2, 3}
    assert any(c.layers[:2] == (20, 100) for c in mlp)
    assert {(c.stage2[0], c.stage2[1]) for c in mlp if c.stage2} == {(0, 0), (10, 0), (0, 7), (16, 64), (12, 20)}
    assert any(c.pair and c.stage2 for c in mlp) and any(c.pair and not c.stage2 for c in mlp)
    for storage in table.STORAGES:                       # both gathers of the first stage and of the second, per storage
        vec = {all(table.vector_path(w, storage) for w in c.srcs) for c in mlp}
        vec2 = {all(table.vector_path(w, storage) for w in c.stage2[:2] if w) for c in mlp if c.stage2 and sum(c.stage2[:2])}
        assert vec == {True, False} and vec2 == {True, False}, storage
    # a ragged last tile whose second-stage gather clamps its rows, and a one-row launch
    assert any(c.stage2 and c.rows % c.tile and not all(table.vector_path(w, "f32") for w in c.stage2[:2] if w) for c in mlp)
    assert table.MlpCase is type(mlp[0]) and len({c.name for c in mlp}) == len(mlp)


def test_part_b_covers_the_gathers_the_centre_sources_and_the_tile_seams():
    sc = table.SETCONV
    assert {c.K for c in sc} == {1, 3, 5, 7, 8, 12, 16, 20, 32} and {c.C for c in sc} == {0, 3, 4, 7, 8, 12, 20, 64}
    assert {c.B for c in sc} == {1, 3} and {7, 11, 1} <= {c.n for c in sc}
    assert {(c.centre, bool(c.group)) for c in sc} == {("xyz", False), ("hw", False), ("hw", True), ("pixel", True)}
    assert any(c.pair and c.group for c in sc) and any(c.pair and not c.group for c in sc)
    for storage in table.STORAGES:
        assert {table.vector_path(c.C, storage) for c in sc if not c.group} == {True, False}
        assert any(not table.vector_path(c.C, storage) and c.C for c in sc if not c.group)           # the element-wise gather's `* mask`
    for tile in (16, 32):
        seams = [table.tiles_of(c.B * c.n, c.K, tile) for c in sc if c.tile == tile]
        assert any(last == 1 and n > 1 for _P, n, last in seams), tile                                # a last tile with one live point
        assert any(c.tile == tile and c.B > 1 and c.n % (tile // c.K) for c in sc), tile              # a tile across two batch elements
        assert any(c.tile == tile and tile % c.K for c in sc), tile                                   # dead rows behind the last point
    assert all(c.tile == 32 for c in sc if c.K > 16) and any(c.n == 1 for c in sc)
    assert {-(-n // 16) for c in sc for n in c.layers} >= {1, 2, 3, 4, 5, 7, 8}
    assert {table.k_loop_class(k) for c in sc for k in table.layer_inputs(c)} >= {(0, True), (1, False), (1, True), (2, False), (2, True)}


def test_part_c_covers_the_pooling_branches_and_the_channel_grid():
    cv = table.CV
    for stage in (1, 2):
        mine = [c for c in cv if c.stage == stage]
        assert {c.K for c in mine} >= {1, 3, 5, 8, 12, 20, 32} and {table.pool_branch(c.K) for c in mine} == {"k4", "k6", "mult8", "other"}
        assert {c.C[0] for c in mine} == {4, 8, 24, 40, 64} and {c.C[1] for c in mine} == {8, 24, 40, 64}
        assert {c.B for c in mine} == {1, 2} and {c.tile for c in mine} == {16, 32} and any(c.far for c in mine)
        assert any(c.tile % c.K for c in mine) and all(c.tile == 32 for c in mine if c.K > 16)
    for part in table.CASES:
        assert len(table.CHECKED[part]) == 3 and set(table.CHECKED[part]) <= {c.name for c in table.CASES[part]}


def test_mask_patterns_of_the_pregrouped_inputs():
    """per batch element an all-clear point, a point with one live slot and an all-set point; clear slots gather cell (0, 0, 0)"""
    for case in [c for c in table.SETCONV if not c.group and c.n >= 3]:
        inp = table.setconv_inputs(case, "f32")
        per_point = inp["mask"].sum(-1)
        for b in range(case.B):
            assert {0, 1, case.K} <= set(per_point[b].astype(int)) or case.K == 1, case.name
        assert (inp["idx"][inp["mask"] == 0] == 0).all()
    for case in table.CV:
        inp = table.cv_inputs(case, "f32")
        per_point = inp["mask"].sum(-1)
        assert all({0, 1, case.K} <= set(per_point[b].astype(int)) or case.K == 1 for b in range(case.B)), case.name


# ---------------------------------------------------------------------------- part D: refusals, nothing launched
def _refusal_args(L, r, job=0):
    w, storage = r.what, "f16" if r.what.get("f16") else "f32"
    mixed = bool(w.get("mixed"))
    if r.op == "mlp":
        pair_mixed = mixed and w.get("pair")
        return fake_mlp(L, w["srcs"], w["layers"], w["rows"], w.get("stage2"), storage,
                        "half" if pair_mixed and job else "split", mixed and not pair_mixed)
    if r.op == "setconv":
        return fake_setconv(L, 3, 7, w["K"], w["C"], w["layers"], storage=storage, mixed=mixed)
    return fake_cv(L, 1 if r.op == "cv1" else 2, 1, w["K"], w["C"], storage, mixed=mixed)


@pytest.mark.parametrize("r", table.REFUSALS, ids=lambda r: r.name)
def test_refusals_answer_their_code_and_launch_nothing(r):
    """The form query AND the entry point (a null stream, fake tensor addresses: anything that reached a launch would fault or
    report a launch error) return the refusal's status with its message."""
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    lib = L.lib()
    a = _refusal_args(L, r)
    b = _refusal_args(L, r, 1) if r.what.get("pair") else None
    bref = ctypes.byref(b) if b is not None else None
    query, entry = {"mlp": (lib.elo_mlp_fused_form, lib.elo_mlp_fused2), "setconv": (lib.elo_setconv_fused_form, lib.elo_setconv_fused2),
                    "cv1": (lib.elo_cv_stage1_form, lib.elo_cv_stage1_fused), "cv2": (lib.elo_cv_stage2_form, lib.elo_cv_stage2_fused)}[r.op]
    args = (ctypes.byref(a), bref) if r.op in ("mlp", "setconv") else (ctypes.byref(a),)
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(r.what.get("tile", 32))):
        asked, said = query(*args), lib.elo_last_error()
        # the entry point runs the same function up to the launch: it is called on these made-up addresses ONLY once the query has
        # refused them (a regression then fails here, on the host, and launches nothing on a machine that has a GPU)
        assert asked == r.status and r.message.encode() in said, (asked, said)
        got, told = entry(*args, None), lib.elo_last_error()
    assert got == r.status and r.message.encode() in told, (got, told)
    with pytest.raises(L.EloError, match=re.escape(r.message)):
        with tuning.override(chain_forms=0, small_tile_units=table.tile_units(r.what.get("tile", 32))):
            L.fused_form({"mlp": "elo_mlp_fused_form", "setconv": "elo_setconv_fused_form", "cv1": "elo_cv_stage1_form",
                          "cv2": "elo_cv_stage2_form"}[r.op], a, b)


@pytest.mark.parametrize("srcs,tile", table.WIDEST)
def test_the_widest_concatenation_below_the_lds_limit_is_taken(srcs, tile):
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(tile)):
        assert L.fused_form("elo_mlp_fused_form", fake_mlp(L, srcs, (16,), 95)) == "tile%d/split" % tile
        wide = fake_setconv(L, 3, 7, 8, sum(srcs) - 3 - (sum(srcs) - 3) % 16 + 13, (16,))               # 3 + C = the same column count
        assert L.fused_form("elo_setconv_fused_form", wide) == "tile%d/split" % tile


def test_queries_validate_like_the_entry_points_and_answer_the_other_families():
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    lib = L.lib()
    assert lib.elo_mlp_fused_form(None, None) == -1 and b"elo_mlp_fused_form: null argument block" in lib.elo_last_error()
    assert lib.elo_setconv_fused_form(None, None) == -1 and lib.elo_cv_stage1_form(None) == -1 and lib.elo_cv_stage2_form(None) == -1
    empty = fake_mlp(L, (8,), (16,), 0)
    assert L.fused_form("elo_mlp_fused_form", empty) == "tile32/split"                                  # nothing is launched
    if lib.elo_dense_f32():
        return
    with tuning.override(chain_forms=1, mlp_chain_rows=0):                                               # the model's two-stage shape: the chain kernel
        chain = fake_mlp(L, (64, 32), (128, 64), 64, (32, 64, (128, 64)), products="half")
        assert L.fused_form("elo_mlp_fused_form", chain) == "chain/half"
    with tuning.override(chain_forms=1):
        assert L.fused_form("elo_cv_stage1_form", fake_cv(L, 1, 1, 6, 64)) == "chain/split"
        assert L.fused_form("elo_cv_stage2_form", fake_cv(L, 2, 1, 4, 16)) == "chain/split"
        assert L.fused_form("elo_cv_stage1_form", fake_cv(L, 1, 1, 6, 24)) == "tile16/split"             # (no chain form for C = 24)
    sv = fake_mlp(L, (64,), (64,), 64)
    sv.sv_npoints, sv.sv_scratch, sv.sv_xyz, sv.sv_feature = 32, _ptr(40), _ptr(41), _ptr(42)
    with tuning.override(chain_forms=0, small_tile_units=0):
        assert L.fused_form("elo_mlp_fused_form", sv) == "sv_ride32/split"


# ---------------------------------------------------------------------------- the statements against the oracle
def _params(rng, scope, k, n):
    return {scope + "/weights": (rng.normal(0, 1, (k, n)) / np.sqrt(k)).astype(np.float32), scope + "/biases": (0.1 * rng.normal(0, 1, n)).astype(np.float32),
            scope + "/bn/gamma": (0.5 + rng.random(n)).astype(np.float32), scope + "/bn/beta": (0.1 * rng.normal(0, 1, n)).astype(np.float32),
            scope + "/bn/moving_mean": (0.1 * rng.normal(0, 1, n)).astype(np.float32),
            scope + "/bn/moving_variance": (0.5 + rng.random(n)).astype(np.float32)}


def _folded(params, scope):
    """(W, b, relu=True) with the inference batch norm folded in, float64"""
    d = lambda leaf: params[scope + "/" + leaf].astype(np.float64)
    s = d("bn/gamma") / np.sqrt(d("bn/moving_variance") + np.float64(O.BN_EPS))
    return d("weights") * s, (d("biases") - d("bn/moving_mean")) * s + d("bn/beta"), True


def _scene(rng, B, H, W):
    az = np.linspace(-1.2, 1.2, W)[None, :] + 0.0 * np.arange(H)[:, None]
    el = np.linspace(-0.3, 0.1, H)[:, None] + 0.0 * az
    r = 8.0 + 3.0 * rng.random((B, H, W))
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1).astype(np.float32)
    return xyz


def _agrees(statement, oracle, what):
    """to float32 rounding: the oracle evaluates the same expression in float32 (a 1x1 convolution of up to 192 inputs, batch norm
    as four more operations, up to six layers): 1e-5 of the tensor's scale"""
    oracle = np.asarray(oracle, np.float64).reshape(statement.shape)
    err = np.abs(statement - oracle).max()
    scale = max(1.0, float(np.abs(oracle).max()))
    print("statement vs oracle, %s: %.2e of scale %.2f" % (what, err, scale))
    assert err <= 1e-5 * scale, (what, err, scale)


def _groups(trace):
    return [(ev[2], nxt[2]) for ev, nxt in zip(trace.events, trace.events[1:]) if ev[1] == "group" and nxt[1] == "group"][::2]


def test_setconv_statement_agrees_with_the_oracle_down_conv():
    rng = np.random.default_rng(11)
    B, H, W, C, K, mlp = 1, 8, 57, 64, 16, [64, 64, 128]
    xyz, feat = _scene(rng, B, H, W), rng.normal(0, 1, (B, H, W, C)).astype(np.float32)
    params, k = {}, 3 + C
    for i, n in enumerate(mlp):
        params.update(_params(rng, "dc/conv%d" % i, k, n))
        k = n
    sel = O.get_selected_idx(B, 2, 2, (H + 1) // 2, (W + 1) // 2)
    with O.discrete_trace() as tr:
        want, new_xyz = O.down_conv(params, shuffle_fn, xyz, feat, sel, K, [5, 9], 12.0, mlp, "dc")
    (idx, mask), = _groups(tr)
    ref = R.setconv(new_xyz.reshape(B, -1, 3), xyz, feat, idx, mask[..., 0], [_folded(params, "dc/conv%d" % i) for i in range(3)])
    assert 0 < mask.mean() < 1
    _agrees(ref["out"], want, "down_conv")


def test_setconv_and_mlp_statements_agree_with_the_oracle_up_conv_and_flow_predictor():
    rng = np.random.default_rng(12)
    B, H, W, C1 = 1, 8, 113, 32
    xyz1 = _scene(rng, B, H, W)
    xyz2 = np.ascontiguousarray(xyz1[:, ::2, ::2])
    feat1, feat2 = rng.normal(0, 1, (B, H, W, C1)).astype(np.float32), rng.normal(0, 1, xyz2.shape[:3] + (64,)).astype(np.float32)
    params = {}
    for name, k, n in (("up/up_1_0", 67, 128), ("up/up_1_1", 128, 64), ("up/up_2_0", 64 + C1, 128), ("up/up_2_1", 128, 64),
                       ("fp/conv_predictor0", C1 + 64 + 64, 128), ("fp/conv_predictor1", 128, 64)):
        params.update(_params(rng, name, k, n))
    taps = {}
    with O.discrete_trace() as tr:
        up = O.up_conv(params, shuffle_fn, xyz1, xyz2, feat1, feat2, [7, 15], 2, 2, 8, 6.0, [128, 64], [128, 64], "up", taps=taps)
    (idx, mask), = _groups(tr)
    ref = R.setconv(xyz1.reshape(B, -1, 3), xyz2, feat2, idx, mask[..., 0], [_folded(params, "up/up_1_%d" % j) for j in range(2)])
    _agrees(ref["out"], taps["pooled"], "up_conv stage 1")
    f1 = feat1.reshape(B * H * W, C1)
    st2 = R.mlp([taps["pooled"].reshape(-1, 64), f1], [_folded(params, "up/up_2_%d" % j) for j in range(2)])
    _agrees(st2["out"], up, "up_conv stage 2")
    cost = rng.normal(0, 1, (B, H * W, 64)).astype(np.float32)
    pred = O.flow_predictor(params, feat1.reshape(B, H * W, C1), up, cost, [128, 64], "fp")
    st = R.mlp_stage2(up.reshape(-1, 64), f1, cost.reshape(-1, 64), [_folded(params, "fp/conv_predictor%d" % j) for j in range(2)])
    _agrees(st["out"], pred, "flow_predictor")


def test_cost_volume_statements_agree_with_the_oracle():
    rng = np.random.default_rng(13)
    B, H, W, C = 1, 8, 57, 32
    xyz1 = _scene(rng, B, H, W)
    xyz2 = (xyz1 + rng.normal(0, 0.05, xyz1.shape)).astype(np.float32)
    f1, f2 = rng.normal(0, 1, (B, H, W, C)).astype(np.float32), rng.normal(0, 1, (B, H, W, C)).astype(np.float32)
    params = {}
    for name, k, n in (("cv/CV_0", 10 + 2 * C, 128), ("cv/CV_1", 128, 64), ("cv/CV_2", 64, 64), ("cv/CV_xyz", 10, 64), ("cv/sum_CV_0", 128, 128),
                       ("cv/sum_CV_1", 128, 64), ("cv/sum_xyz_encoding", 10, 64), ("cv/sum_cost_volume_0", 128 + C, 128),
                       ("cv/sum_cost_volume_1", 128, 64)):
        params.update(_params(rng, name, k, n))
    taps = {}
    with O.discrete_trace() as tr:
        want = O.cost_volume(params, shuffle_fn, xyz1, xyz2, f1, f2, [3, 5], [5, 15], 4, 6, 2.0, [128, 64, 64], [128, 64], "cv", taps=taps)
    (idx_q, mask_q), (idx_p, mask_p) = _groups(tr)
    f = lambda name: _folded(params, "cv/" + name)
    layers1 = {"cv0": f("CV_0"), "cv1": f("CV_1"), "cv2": f("CV_2"), "cv_xyz": f("CV_xyz"), "sum_cv0": f("sum_CV_0"), "sum_cv1": f("sum_CV_1")}
    st1 = R.cv_stage1(xyz1.reshape(B, -1, 3), f1.reshape(B, -1, C), xyz2, f2, idx_q, mask_q[..., 0], layers1)
    _agrees(st1["out"], taps["stage1"], "cost_volume stage 1")
    layers2 = {"xyz_enc": f("sum_xyz_encoding"), "sum_cost0": f("sum_cost_volume_0"), "sum_cost1": f("sum_cost_volume_1")}
    st2 = R.cv_stage2(xyz1, f1, taps["stage1"], idx_p, mask_p[..., 0], layers2)
    _agrees(st2["out"], want, "cost_volume stage 2")


# ---------------------------------------------------------------------------- a correct implementation fits the bound
def test_per_layer_units_stay_below_what_the_suite_already_asserts():
    for K in range(1, 257):
        assert bounds.u_split(K) <= bounds.ASSERTED_SPLIT and bounds.u_half(K) <= bounds.ASSERTED_HALF, K


def _at_half_units(expect, *args, **kwargs):
    """the statement and its bound with every rounding unit of the arithmetic HALVED (bounds.units_scaled): half the bound for split
    products; with half products an fp16 rounding flip stays a whole step, but only values within reach of half the error flip"""
    with bounds.units_scaled(0.5):
        return expect(*args, stored=False, **kwargs)


def _worst(got, want, bound, what):
    """the emulation's fp32 value (before the storage rounding, which is a rounding of its own and reaches its half ulp) against the
    bound at half units"""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.isfinite(err).all() and (bound >= 0).all(), what
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    assert ok.all(), "%s: the emulation is at %.2f of the bound at half units" % (what, ratio)
    return ratio


def _store(x, storage):
    x = np.asarray(x, np.float32)
    return x.astype(np.float16).astype(np.float32) if storage == "f16" else x


def _emulation_runs(part):
    return [pytest.param(c, s, p, id="%s-%s-%s" % (c.name, s, p)) for c, s, p in table.runs(part) if p != "checked"]


@pytest.mark.parametrize("case,storage,products", _emulation_runs("mlp"))
def test_emulated_mlp_stays_within_half_the_bound(case, storage, products):
    inp = table.mlp_inputs(case, storage)
    x = np.concatenate(inp["sources"], -1)
    got = bounds.emulate_chain(x, inp["layers"], products)          # (an fp16 input splits into itself and a zero lo)
    want, bound = _at_half_units(bounds.mlp_expect, R, inp, products, storage)
    _worst(got, want, bound, "out")
    if case.stage2:
        got = _store(got, storage)                                   # the second stage continues with the first one AS STORED
        parts = [p for p in (inp["before"], got, inp["after"]) if p is not None]
        got2 = bounds.emulate_chain(np.concatenate(parts, -1), inp["layers2"], products)
        want2, bound2 = _at_half_units(bounds.mlp_expect, R, inp, products, storage, first_stage=got.astype(np.float64))
        _worst(got2, want2, bound2, "out2")


@pytest.mark.parametrize("case,storage,products", _emulation_runs("mlp"))
def test_plain_float32_accumulation_stays_within_the_full_bound(case, storage, products):
    """The emulation above sums a k-block the way the bound models a matrix instruction (exactly, one rounding).  A PLAIN float32
    accumulation of the same products -- every k-block a float32 matmul, up to 31 sequential roundings where the model has a tree
    of 5 -- is held to the FULL bound: it fits, with less room (up to 0.8 of the bound for half products), which is how much rests
    on the instruction's summation being no worse than the model."""
    inp = table.mlp_inputs(case, storage)
    got = bounds.emulate_chain(np.concatenate(inp["sources"], -1), inp["layers"], products, sequential=True)
    want, bound = bounds.mlp_expect(R, inp, products, storage, stored=False)
    _worst(got, want, bound, "out, plain float32 accumulation")


def _f32_geometry(p, g, m):
    p, g, m = np.asarray(p, np.float32), np.asarray(g, np.float32), np.asarray(m, np.float32)
    pk = np.broadcast_to(p[:, :, None, :], g.shape)
    gm = g * m
    d = gm - pk
    e = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + np.float32(1e-20), dtype=np.float32)
    return np.concatenate([pk, gm, d, e[..., None]], -1).astype(np.float32)


def _slots(case, inp):
    """idx / mask of a set-conv case: the table's, or -- in-kernel grouping -- what the grouping oracle gives for the case's centres"""
    if not case.group:
        return inp["idx"], inp["mask"]
    kh, kw, dist, sh, sw = case.group
    grid = inp["xyz1_grid"]
    B, H, W, _ = grid.shape
    centres = inp["centre_hw"] if "centre_hw" in inp else O.get_hw_idx(B, H, W)
    sel, _valid, _indis, mask = G.fused_conv_random_k(grid, inp["src_xyz"], np.ascontiguousarray(centres), inp["order"], H, W, centres.shape[1],
                                                      kh, kw, case.K, 0, dist, sh, sw)
    mask = mask.reshape(B, centres.shape[1], case.K)
    assert 0 < mask.mean() < 1 and (sel[mask == 0] == 0).all(), case.name
    return sel, mask


@pytest.mark.parametrize("case,storage,products", _emulation_runs("setconv"))
def test_emulated_setconv_stays_within_half_the_bound(case, storage, products):
    inp = table.setconv_inputs(case, storage)
    centre, (idx, mask) = table.setconv_centres(inp), _slots(case, inp)
    m = mask[..., None]
    g = lambda grid: grid[idx[..., 0], idx[..., 1], idx[..., 2]]
    x = np.concatenate([g(inp["src_xyz"]) * m - centre[:, :, None, :], g(inp["src_feat"]) * m], -1).astype(np.float32)
    y = bounds.emulate_chain(x, inp["layers"], products)  # (an fp16 feature splits into itself and a zero lo)
    got = (y * m).max(axis=2)
    want, bound = _at_half_units(bounds.setconv_expect, R, inp, centre, idx, mask, products, storage)
    _worst(got, want, bound, "pooled")


def _f32_softmax_pool(logits, values, mask):
    F = np.float32
    l = np.where(mask[..., None] == 1.0, logits, F(-1e10)).astype(F)
    x = (l - l.max(axis=2, keepdims=True)).astype(F)
    with np.errstate(under="ignore"):
        e = np.exp2((x * F(1.44269504088896)).astype(F)).astype(F)
    den, acc = np.zeros(e.shape[:2] + e.shape[3:], F), np.zeros(e.shape[:2] + e.shape[3:], F)
    for k in range(e.shape[2]):
        den = den + e[:, :, k]
        acc = acc + e[:, :, k] * values[:, :, k]
    return (acc / den).astype(F)


@pytest.mark.parametrize("case,storage,products", _emulation_runs("cv"))
def test_emulated_cost_volume_stays_within_half_the_bound(case, storage, products):
    inp = table.cv_inputs(case, storage)
    idx, mask, L = inp["idx"], inp["mask"], inp["layers"]
    m = mask[..., None]
    g = lambda grid: grid[idx[..., 0], idx[..., 1], idx[..., 2]]
    em = lambda x, names: bounds.emulate_chain(x, [L[n] for n in names], products)
    half = products == "half"
    if case.stage == 1:
        geo = _f32_geometry(inp["xyz1"], g(inp["xyz2"]), m)
        f1 = np.broadcast_to(inp["feat1"][:, :, None, :], idx.shape[:3] + (inp["C"],))
        x = em(np.concatenate([geo, f1, g(inp["feat2"]) * m], -1), ["cv0", "cv1", "cv2"])
        logits = em(np.concatenate([em(geo, ["cv_xyz"]), x], -1), ["sum_cv0", "sum_cv1"])
        values = x.astype(np.float16).astype(np.float32) if half else x
        want, bound, spread = _at_half_units(bounds.cv1_expect, R, inp, products, storage)
    else:
        B, H, W, C = inp["feat1"].shape
        geo = _f32_geometry(inp["xyz1"].reshape(B, H * W, 3), g(inp["xyz1"]), m)
        grouped = (g(inp["cost"]) * m).astype(np.float32)
        f1 = np.broadcast_to(inp["feat1"].reshape(B, H * W, 1, C), idx.shape[:3] + (C,))
        logits = em(np.concatenate([em(geo, ["xyz_enc"]), f1, grouped], -1), ["sum_cost0", "sum_cost1"])
        values = grouped.astype(np.float16).astype(np.float32) if half else grouped
        want, bound, spread = _at_half_units(bounds.cv2_expect, R, inp, products, storage)
    assert spread < 30.0, "the first-order softmax term needs |l - max| < 30 on the slots that carry weight (%.1f)" % spread
    got = _f32_softmax_pool(logits, values, mask)
    _worst(got, want, bound, "pooled")

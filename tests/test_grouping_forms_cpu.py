"""CPU: the case table of tests/grouping_forms_cases.py is what it says it is.

* every form enumerator of the four grouping queries (include/elo.h: elo_fused_conv_{random,select}_k[_dense]_form; host
  arithmetic, no device) is reached, every case lands on the form it names, each boundary pair on two different forms, and the
  refused sizes are refused;
* every placed case has the property it is named for -- the ties sit at the stated ranks and nowhere else among ranks 0..K+1,
  the isolators have no equal pair and the stated candidate count, the neighbour at d == r2 is taken and its outward twin is
  not -- established from float32 numpy (the arithmetic contract's operation order) and the oracle's outputs;
* the oracle equals the reference's stored outputs (tests/golden/grouping_forms_ref.npz, from the reference's own kernel
  bodies: tests/golden/make_grouping_forms_ref.py) on every case, windows up to 5000 slots and K up to 117 included, and the
  live reference build where oracle/_ref exists.
"""
import os
import re

import numpy as np
import pytest

import grouping_forms_cases as T
from conftest import GOLDEN, ROOT, expand_prefix, load_pkg
from oracle import grouping as G

RUN = [c for c in T.CASES if c["refuse"] is None]
REFUSED = [c for c in T.CASES if c["refuse"] is not None]
PLACED = [c for c in T.CASES if c["kind"] == "placed"]
names = lambda cases: [c["name"] for c in cases]


@pytest.fixture(scope="module")
def stored():
    return np.load(os.path.join(GOLDEN, "grouping_forms_ref.npz"))


def _K(case):
    return T.resolve_K(case, load_pkg("_lib").lib().elo_fused_conv_random_k_dense_fits)


@pytest.fixture(scope="module")
def oracle_outputs():
    cache = {}

    def get(case):
        if case["name"] not in cache:
            fn = G.fused_conv_random_k if case["op"] == "random" else G.fused_conv_select_k
            cache[case["name"]] = fn(*T.oracle_args(case, _K(case)))
        return cache[case["name"]]
    return get


def _form(case, want_valid=True):
    fc, tuning = load_pkg("fused_conv"), load_pkg("tuning")
    with tuning.override(**case["tuning"]):
        return fc.grouping_form(case["op"], T.batch_of(case), case["H"], case["W"], case["N"], case["kH"], case["kW"], _K(case),
                                case["fc"], case["dist"], case["sh"], case["sw"], want_valid=want_valid, dense=case["dense"])


# ---------------------------------------------------------------------------------------------------------------- the queries
def test_the_queries_are_declared_bound_and_named():
    L = load_pkg("_lib")
    header = open(os.path.join(ROOT, "include", "elo.h")).read()
    for query in L.GROUPING_QUERIES:
        assert re.search(r"^int %s\(const elo_group_args \*a\);" % query, header, re.M)
        assert any(name == query for name, _r, _a in L.SYMBOLS)
    enum = lambda prefix: {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\b%s(\w+) = (\d+)" % prefix, header)}
    assert enum("ELO_RANDOM_(?!DENSE)") == {n: i for i, n in enumerate(L.RANDOM_FORMS)}
    assert enum("ELO_RANDOM_DENSE_") == {n: i for i, n in enumerate(L.RANDOM_DENSE_FORMS)}
    assert enum("ELO_SELECT_(?!PATH|DENSE)") == {n: i for i, n in enumerate(L.SELECT_STORES)}
    assert enum("ELO_SELECT_PATH_") == {n: i for i, n in enumerate(L.SELECT_PATHS)}
    assert enum("ELO_SELECT_DENSE_") == {n: i for i, n in enumerate(L.SELECT_DENSE_WAVES)}
    assert L.grouping_form_name("elo_fused_conv_select_k_form", 1 | 2 << 4) == "reg3/mid"
    assert L.grouping_form_name("elo_fused_conv_select_k_form", 4) == "lds2"
    assert L.grouping_form_name("elo_fused_conv_select_k_dense_form", 2 | 1 << 4) == "w16+counts"
    assert L.ABI_VERSION == 26                                    # additive: no struct moved


@pytest.mark.parametrize("name", names(RUN))
def test_each_case_takes_the_form_it_names(name):
    case = T.BY_NAME[name]
    counts = case["op"] == "select" and case["dense"]
    assert _form(case, want_valid=True) == case["form"] + ("+counts" if counts else "")
    assert _form(case, want_valid=False) == case["form"]


@pytest.mark.parametrize("name", names(REFUSED))
def test_refused_sizes_are_refused_by_the_query(name):
    case = T.BY_NAME[name]
    L = load_pkg("_lib")
    with pytest.raises(L.EloError, match=r"status %d\)" % case["refuse"]):
        _form(case)
    if "kmax" in name:                                            # one fewer is the largest K that fits
        assert L.lib().elo_fused_conv_random_k_dense_fits(case["kH"], case["kW"], _K(case) - 1, case["sh"], case["sw"]) == 1
        assert L.lib().elo_fused_conv_random_k_dense_fits(case["kH"], case["kW"], _K(case), case["sh"], case["sw"]) == 0


def test_every_enumerator_is_reached_by_some_case():
    L = load_pkg("_lib")
    reached = {}
    for case in RUN:
        query = "elo_fused_conv_%s_k%s_form" % (case["op"], "_dense" if case["dense"] else "")
        reached.setdefault(query, set()).update((_form(case, True), _form(case, False)))
    assert reached["elo_fused_conv_random_k_form"] == set(L.RANDOM_FORMS)
    assert reached["elo_fused_conv_random_k_dense_form"] == set(L.RANDOM_DENSE_FORMS)
    # every store with every path it can take: rounds <= 7 / above, by J (a J = 8 window takes K <= 8 only: no MID there)
    assert reached["elo_fused_conv_select_k_form"] == {"reg2/small", "reg2/mid", "reg3/small", "reg3/mid", "reg8/small", "reg8/rounds",
                                                       "lds4", "lds2", "lds1"}
    assert reached["elo_fused_conv_select_k_dense_form"] == {w + c for w in L.SELECT_DENSE_WAVES for c in ("", "+counts")}
    paths = {f.split("/")[1] for f in reached["elo_fused_conv_select_k_form"] if "/" in f} | {"swaps"}
    assert paths == set(L.SELECT_PATHS)


@pytest.mark.parametrize("a,b", [
    ("random/4x4/K4/fc0", "random/1x17/K4/fc0"), ("random/4x8/K4/fc0", "random/3x11/K4/fc0"),           # 16 | 17 and 32 | 33 slots
    ("random/3x11/K16/fc0", "random/3x11/K17/fc0"), ("random/5x15/K16/fc1", "random/5x15/K17/fc1"),     # K of 16 | 17
    ("select/8x16/K7", "select/3x43/K7"), ("select/8x16/K32", "select/3x43/K32"),                       # 128 | 129 slots
    ("select/12x16/K7", "select/1x193/K7"), ("select/12x16/K9", "select/1x193/K9"),                     # 192 | 193
    ("select/16x32/K8", "select/19x27/K8"),                                                             # 512 | 513
    ("select/8x8/K7", "select/8x8/K8"), ("select/1x257/K7", "select/1x257/K8"), ("select/1x257/K8", "select/1x257/K9"),   # K of 7 | 8 | 9
    ("select/12x16/K32", "select/12x16/K33"), ("select/8x8/K32", "select/8x8/K33"),                     # K of 32 | 33
    ("select/5x15/K6/fc1/populated", "placed/reg2_small/ties"),                                         # flag_copy
    ("select/35x52/K9", "select/3x607/K9"), ("select/52x63/K9", "select/29x113/K9"),                    # 1820 | 1821, 3276 | 3277 slots
    ("random_dense/rows2/h5w37", "random_dense/rows4/h5w37"), ("random_dense/rows4/h5w37", "random_dense/rows4/kmax"),
    ("select_dense/w4/k1", "select_dense/w8/k1"), ("select_dense/w8/k1", "select_dense/w16/k1")])
def test_each_boundary_pair_lands_on_two_forms(a, b):
    ca, cb = T.BY_NAME[a], T.BY_NAME[b]
    assert (ca["op"], ca["dense"]) == (cb["op"], cb["dense"])
    assert _form(ca) != _form(cb)
    slots = lambda c: c["kH"] * c["kW"]
    if not ca["dense"] and ca["fc"] == cb["fc"] and ca["K"] == cb["K"]:
        assert slots(cb) == slots(ca) + 1                         # a window-size step: the pair sits on its two sides


def test_the_window_steps_are_met_exactly():
    """16 | 17, 32 | 33, 64 | 65, 128 | 129, 192 | 193, 256 | 257, 512 | 513, 1820 | 1821, 3276 | 3277 slots and the 5000-slot limit."""
    have = {c["kH"] * c["kW"] for c in RUN if not c["dense"]}
    assert {16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 1820, 1821, 3276, 3277, 5000} <= have


# ---------------------------------------------------------------------------------------------------------------- named properties
def _sorted_in_range(case, b, n=0):
    d, valid, hit, hw = T.window_distances(case, b, n)
    return np.sort(d[hit]), d, valid, hit, hw


def _selected(out, b, n=0):
    sel, _valid, _indis, mask = out
    return [tuple(int(v) for v in row[1:]) for row, m in zip(sel[b, n], mask[b, n, :, 0]) if m == 1]


@pytest.mark.parametrize("name", names(PLACED))
def test_placed_cases_have_the_property_they_are_named_for(name, oracle_outputs):
    case = T.BY_NAME[name]
    fams = T.inputs(case)["families"]
    out = oracle_outputs(case)
    K = case["K"]
    by_name = {f["name"]: b for b, f in enumerate(fams)}
    for b, f in enumerate(fams):
        s, d, valid, hit, hw = _sorted_in_range(case, b)
        chosen = _selected(out, b)
        at = lambda pos: tuple(int(v) for v in hw[pos])
        if f["in_range"] is not None:
            assert hit.sum() == f["in_range"], f["name"]
        if f["name"] == "eps_centre_at":                                   # the centre itself counts as empty: every output zero
            assert T.sq3(f["centre"]) == T.EPS and not any(o[b, 0].any() for o in out)
            continue
        # equal neighbours among ranks 0 .. K + 1 of the in-range distances: exactly the stated ones
        want = {(r, r + 1) for tie in f["ties"] for r in tie[:-1]}
        have = {(r, r + 1) for r in range(min(K + 1, len(s) - 1)) if s[r] == s[r + 1]}
        assert have == want, (f["name"], have, want)
        for tie in f["ties"]:
            assert tie == tuple(range(tie[0], tie[0] + len(tie)))
        assert len(chosen) == min(K, int(hit.sum())) and len(set(chosen)) == len(chosen)
        # the oracle's selection is the K smallest distances, in order
        order = {at(p): d[p] for p in range(d.size) if hit[p]}
        assert [order[c] for c in chosen] == list(s[:len(chosen)]), f["name"]
        marks = f["marks"] if "marks" in f else {}
        if f["name"] == "tie_swapped":
            # the twin at the LATER visiting position comes first: the first swap moved array position 0 behind it
            assert d[marks["first"]] == d[marks["second"]] and marks["second"] == 0 < marks["first"]
            assert chosen[1] == at(marks["first"]) and chosen[2] == at(marks["second"])
        if f["name"] == "tie_K_Kp1":
            assert chosen == _selected(out, by_name["control"])          # a tie beyond the boundary changes nothing
        if f["name"] == "two_at_centre":
            assert s[0] == s[1] == T.EPS and s[2] > T.EPS
        if f["name"] in ("r2_edge", "r2_edge_tied"):
            for pos in marks["edge"]:
                assert d[pos] == np.float32(9.0) and hit[pos] and at(pos) in chosen
            twin = marks["twin"]
            q, e = T.inputs(case)["xyz2"][b][at(twin)], T.inputs(case)["xyz2"][b][at(marks["edge"][0])]
            assert q[0] == np.nextafter(e[0], np.float32(9)) and (q[1:] == e[1:]).all()     # one float further out along x
            assert np.float32(9.0) < d[twin] < np.float32(9.00001) and valid[twin] and not hit[twin] and at(twin) not in chosen
        if f["name"] == "eps_neighbour":
            q = T.inputs(case)["xyz2"][b][at(marks["at"])], T.inputs(case)["xyz2"][b][at(marks["above"])]
            assert T.sq3(q[0]) == T.EPS and T.sq3(q[1]) > T.EPS and q[1][0] == np.nextafter(q[0][0], np.float32(1)) and (q[1][1:] == q[0][1:]).all()
            assert not valid[marks["at"]] and hit[marks["above"]] and at(marks["above"]) in chosen and at(marks["at"]) not in chosen
            assert out[1][b, 0].sum() == valid.sum() == 4
        if f["name"] == "eps_centre_above":
            assert T.sq3(f["centre"]) > T.EPS and out[2][b, 0].sum() == 4 and len(chosen) == 4
        if f["name"] in ("mid_over_64", "small_no_bound"):
            assert len(np.unique(s)) == len(s)                            # no tie anywhere in range
            if f["name"] == "mid_over_64":
                assert T.mid_k_candidates(d, hit, K) == 97 and hit.all()
            else:
                assert T.small_k_bound_is_none(hit) and hit.sum() > 64
        elif f["rest"] == "near" and not f["ties"]:
            assert len(np.unique(s)) == len(s)


def test_the_tie_families_need_the_rank_forms_to_notice(oracle_outputs):
    """In every tie family that touches ranks 0..K the tied neighbours have different payloads, so an order other than the
    reference's is visible in the output; the families beyond the boundary and the in-range counts do not tie at all."""
    for case in PLACED:
        for b, f in enumerate(T.inputs(case)["families"]):
            s, d, valid, hit, hw = _sorted_in_range(case, b)
            for tie in f["ties"]:
                pos = [p for p in range(d.size) if hit[p] and d[p] == s[tie[0]]]
                assert len(pos) == len(tie) and len({tuple(hw[p]) for p in pos}) == len(tie)


@pytest.mark.parametrize("P", [4, 8, 16])
def test_dense_isolator_leaves_one_slot_class_empty_without_a_tie(P):
    case = T.BY_NAME["select_dense/w%d/empty_class" % P]
    perm = T.inputs(case)["perm"]
    for n in range(0, case["N"], 7):
        s, d, valid, hit, hw = _sorted_in_range(case, 0, n)
        assert hit.sum() > 32 and len(np.unique(s)) == len(s)             # the 32-entry candidate list overflows, no tie
        assert any(not valid[perm % 8 == cls].any() for cls in range(8))  # a class (raster slot % 8) without a pixel


@pytest.mark.parametrize("P", [4, 8, 16])
def test_dense_tied_windows_hold_one_tie_each_at_a_rank_that_moves(P):
    """The dense placed-tie cloud: hundreds of centres with exactly ONE pair of equal distances among the nearest K + 1, at two
    different pixels, the pair's rank taking every value 0..K; as many whose only tie lies beyond (it must change nothing);
    and the cloud is no integer lattice."""
    case = T.BY_NAME["select_dense/w%d/tied_window" % P]
    K = case["K"]
    single, beyond, ranks = 0, 0, set()
    for n in range(case["N"]):
        s, d, valid, hit, hw = _sorted_in_range(case, 0, n)
        ties = [r for r in range(len(s) - 1) if s[r] == s[r + 1]]
        if len(ties) == 1 and ties[0] <= K:
            assert len({tuple(hw[p]) for p in range(d.size) if hit[p] and d[p] == s[ties[0]]}) == 2
            single += 1
            ranks.add(ties[0])
        elif len(ties) == 1:
            beyond += 1
    assert single >= 200 and beyond >= 200 and ranks == set(range(K + 1)), (single, beyond, ranks)
    xyz2 = T.inputs(case)["xyz2"]
    assert (xyz2 != np.round(xyz2)).any(-1).mean() > 0.75


def test_flag_copy_meets_an_empty_and_a_populated_slot_0(oracle_outputs):
    empty, full = (oracle_outputs(T.BY_NAME["select/5x15/K6/fc1/" + tag]) for tag in ("empty", "populated"))
    lonely = (empty[2].sum((2, 3)) == 0) & (empty[1].sum((2, 3)) > 0)     # a live centre, neighbours exist, none in range
    assert lonely.any() and (empty[3][lonely] == 1).all() and not empty[0][lonely][..., 1:].any()
    assert (full[2].sum((2, 3)) > 6).any()


@pytest.mark.parametrize("op", ["random", "select"])
def test_packing_limit_cases_select_the_last_rows_and_columns(op, oracle_outputs):
    """(h << 16) | w at its limits: neighbours in column 65534 (also reached through the wrap from column 0) and in row 32766
    are among the selected ones."""
    sel, _v, _i, mask = oracle_outputs(T.BY_NAME[op + "/pack/w65535"])
    taken = sel[mask[..., 0] == 1]
    assert taken[:, 2].max() == 65534 and (sel[0, 0][mask[0, 0, :, 0] == 1][:, 2] >= 65533).any() and taken[:, 1].max() == 0
    sel, _v, _i, mask = oracle_outputs(T.BY_NAME[op + "/pack/h32767"])
    taken = sel[mask[..., 0] == 1]
    assert taken[:, 1].max() == 32766 and taken[:, 2].max() == 0


# ---------------------------------------------------------------------------------------------------------------- oracle == reference
@pytest.mark.parametrize("name", names(RUN))
def test_oracle_equals_the_reference_outputs(name, stored, oracle_outputs):
    case = T.BY_NAME[name]
    sel, valid, indis, mask = oracle_outputs(case)
    KT = case["kH"] * case["kW"]
    assert np.array_equal(sel, stored[name + "/sel"])
    assert np.array_equal(mask[..., 0], stored[name + "/mask"])
    assert np.array_equal(valid, expand_prefix(stored[name + "/n_valid"], KT))
    assert np.array_equal(indis, expand_prefix(stored[name + "/n_indis"], KT))
    if G.have_ref():
        fn = G.fused_conv_random_k if case["op"] == "random" else G.fused_conv_select_k
        for x, y in zip((sel, valid, indis, mask), fn(*T.oracle_args(case, _K(case)), impl="ref")):
            assert np.array_equal(x, y)


def test_the_fixture_holds_exactly_the_table(stored):
    assert set(stored.files) == {"%s/%s" % (c["name"], k) for c in RUN for k in ("sel", "mask", "n_valid", "n_indis")}

"""The case table of tests/test_grouping_forms_{cpu,gpu}.py: the grouping kernels (csrc/elo_grouping.hip and the shared device
forms of csrc/elo_group_device.h) at every form boundary their launchers have, with exact ties PLACED at chosen ranks and
visiting positions.  numpy only; every case is rebuilt from its name (seeded), so tests/golden/grouping_forms_ref.npz stores
the reference's OUTPUTS only.

A case is a dict: name, op ("random" / "select"), dense (the LDS-tiled entry point), tuning (elo_tuning fields forced while it
runs), form (what the library's form query must answer, as _lib.grouping_form_name spells it) or refuse (the elo_status the
entry point and the query must answer), and the call: H, W, N, kH, kW, K, fc, dist, sh, sw.  inputs(case) adds the arrays
(xyz1, xyz2, idx, perm) and, for the placed cases, `families`: one batch element per family, whose centre 0 is the designed one.

(a) form boundaries      random clouds (normal, 10 % empty pixels) at both sides of every threshold of the four launchers
(b) placed ties          a centre on an integer lattice point, chosen neighbours at centre + small integer offsets (squared
                         distances exact in float32 and chosen here, several offsets per norm so the payloads differ), the
                         rest of the window at distinct, inexact, larger distances; each chosen neighbour at a chosen visiting
                         position through random_hw
(c) path isolators       no tie anywhere, yet the rank form at hand must give up (or must not)
(d) the clouds of (b) with every pixel a centre: what fused.cv_stage1 groups in-kernel (tests/test_grouping_forms_gpu.py)
"""
import functools
import math
import zlib

import numpy as np

ELO_ERR_ARG, ELO_ERR_LIMIT = -1, -2
EPS = np.float32(1e-10)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, op, H, W, N, win, K, fc=0, dist=1000.0, stride=(1, 1), dense=False, tuning=None, form=None, refuse=None, **more):
    c = dict(name=name, op=op, dense=dense, tuning=tuning or {}, form=form, refuse=refuse, H=H, W=W, N=N, kH=win[0], kW=win[1],
             K=K, fc=fc, dist=float(dist), sh=stride[0], sw=stride[1], kind="cloud", B=1)
    c.update(more)
    return c


# ------------------------------------------------------------------------------------------------------------ (a) boundaries
def _select_form(KT, K, fc):
    """The form the header (include/elo.h, elo_fused_conv_select_k_form) promises for a window of KT slots."""
    if fc == 0 and ((KT <= 512 and K <= 8) or (KT <= 192 and K <= 32)):
        J = 2 if KT <= 128 else 3 if KT <= 192 else 8
        rounds = min(K, KT)
        return "reg%d/%s" % (J, "small" if rounds <= 7 else "mid" if J <= 3 else "rounds")
    return "lds4" if KT <= 1820 else "lds2" if KT <= 3276 else "lds1"


def _boundary_cases():
    out = []
    # ---- random-k, general kernel: 16 / 17 and 32 / 33 slots, K of 16 / 17 above them, K > KT, a block with shadowing groups
    for win, K, N, form in (((4, 4), 4, 17, "g16u1"), ((1, 17), 4, 9, "g32u1"), ((4, 8), 4, 9, "g32u1"), ((3, 11), 4, 17, "g16u4"),
                            ((3, 11), 16, 17, "g16u4"), ((3, 11), 17, 9, "g32u2"), ((5, 15), 16, 33, "g16u4"),
                            ((5, 15), 17, 17, "g32u2"), ((3, 3), 12, 17, "g16u1"), ((3, 11), 40, 9, "g32u2")):
        for fc in (0, 1):
            out.append(_case("random/%dx%d/K%d/fc%d" % (win + (K, fc)), "random", 6, 24, N, win, K, fc=fc, dist=2.5, form=form))
    # ---- select-k, general kernel: the register windows (J = 2 / 3 / 8), K of 7 / 8 / 9, K of 32 / 33, the LDS form behind them
    for win in ((8, 8), (5, 13), (8, 16), (3, 43), (12, 16), (1, 193), (16, 16), (1, 257), (16, 32), (19, 27)):
        KT = win[0] * win[1]
        for K in (7, 8, 9) + ((32, 33) if KT in (64, 128, 129, 192) else ()):
            out.append(_case("select/%dx%d/K%d" % (win + (K,)), "select", 6, max(24, win[1] + 3), 40, win, K,
                             dist=3.0 if K < 30 else 1000.0, form=_select_form(KT, K, 0)))
    # K >= KT: rounds = KT decides the path; K > 32 is the LDS form whatever the window
    for win, K in (((2, 3), 8), ((3, 3), 9), ((3, 3), 12), ((1, 5), 40)):
        out.append(_case("select/%dx%d/K%d" % (win + (K,)), "select", 6, 24, 40, win, K, dist=4.0, form=_select_form(win[0] * win[1], K, 0)))
    # flag_copy = 1 always takes the LDS form; its copy fires on a populated slot 0 and on an empty one
    out.append(_case("select/5x15/K6/fc1/populated", "select", 6, 24, 40, (5, 15), 6, fc=1, dist=1000.0, form="lds4"))
    out.append(_case("select/5x15/K6/fc1/empty", "select", 6, 24, 40, (5, 15), 6, fc=1, dist=0.05, form="lds4"))
    # the waves-per-block steps of the LDS form (1820 / 1821 and 3276 / 3277 slots) and the largest window
    for win, form in (((35, 52), "lds4"), ((3, 607), "lds2"), ((52, 63), "lds2"), ((29, 113), "lds1"), ((100, 50), "lds1")):
        out.append(_case("select/%dx%d/K9" % win, "select", 4, max(50, win[1] + 3), 21, win, 9, dist=3.0, form=form))
    # ---- random-k, LDS-tiled: both tile heights forced; ragged tile rows (H % 4 = 1, 2, 3), W < 64 and W % 64 != 0, strides,
    # flag_copy, a window taller than the grid, K dividing the thread count (the `even` read-out) and not
    for rows in (2, 4):
        t = dict(random_dense_rows=rows)
        f = "rows%d" % rows
        for tag, H, W, win, K, fc, stride in (("h5w37", 5, 37, (3, 5), 4, 0, (1, 1)), ("h6w70", 6, 70, (5, 9), 3, 1, (1, 1)),
                                              ("h7w70tall", 7, 70, (9, 7), 5, 0, (1, 1)), ("h7w130s23", 7, 130, (5, 9), 8, 1, (2, 3)),
                                              ("h9w64s23", 9, 64, (3, 5), 16, 0, (2, 3))):
            out.append(_case("random_dense/%s/%s" % (f, tag), "random", H, W, H * W, win, K, fc=fc, dist=2.5, stride=stride,
                             dense=True, tuning=t, form=f, B=2))
        # the largest K the library admits for a 3x5 window (found by asking it: test files) -- 2 rows fit, 4 do not
        out.append(_case("random_dense/%s/kmax" % f, "random", 3, 20, 60, (3, 5), "kmax", dist=2.5, dense=True, tuning=t, form="rows2"))
        out.append(_case("random_dense/%s/kmax+1" % f, "random", 3, 20, 60, (3, 5), "kmax+1", dist=2.5, dense=True, tuning=t,
                         refuse=ELO_ERR_LIMIT))
    # ---- select-k, LDS-tiled, at 4 / 8 / 16 waves per tile (each with and without the count masks: the tests run both)
    for P in (4, 8, 16):
        t = dict(select_dense_waves=P)
        f = "w%d" % P
        for tag, H, W, win, K in (("h1w65", 1, 65, (3, 5), 7), ("w3wrap", 3, 3, (3, 7), 1), ("w1wrap", 2, 1, (3, 3), 7),
                                  ("512slots", 4, 70, (16, 32), 7), ("k1", 5, 37, (5, 15), 1)):
            out.append(_case("select_dense/%s/%s" % (f, tag), "select", H, W, H * W, win, K, dist=1000.0 if "wrap" in tag else 4.0,
                             dense=True, tuning=t, form=f, B=1 if tag == "512slots" else 2))
        out.append(_case("select_dense/%s/513slots" % f, "select", 4, 70, 280, (19, 27), 7, dense=True, tuning=t, refuse=ELO_ERR_LIMIT))
        out.append(_case("select_dense/%s/tied_window" % f, "select", 12, 80, 960, (5, 15), 6, dist=10.0, dense=True, tuning=t, form=f,
                         kind="tied_window"))
        out.append(_case("select_dense/%s/empty_class" % f, "select", 4, 64, 256, (5, 16), 6, dist=1000.0, dense=True, tuning=t,
                         form=f, kind="empty_class"))
    # ---- the packing limits of (h << 16) | w: the last grid sizes admitted, centres at both ends; one more is refused
    for op, form in (("random", "g16u1"), ("select", "reg2/small")):
        out.append(_case("%s/pack/w65535" % op, op, 1, 65535, 5, (1, 5), 4, dist=1000.0, form=form, kind="pack"))
        out.append(_case("%s/pack/h32767" % op, op, 32767, 1, 5, (5, 1), 4, dist=1000.0, form=form, kind="pack"))
        for dense in (False, True):
            d = "_dense" if dense else ""
            out.append(_case("%s%s/pack/w65536" % (op, d), op, 1, 65536, 65536 if dense else 5, (1, 5), 4, dense=dense, refuse=ELO_ERR_LIMIT))
            out.append(_case("%s%s/pack/h32768" % (op, d), op, 32768, 1, 32768 if dense else 5, (5, 1), 4, dense=dense, refuse=ELO_ERR_LIMIT))
    return out


# ------------------------------------------------------------------------------------------------------------ (b) placed ties
def _offsets_by_norm(limit=6):
    table = {}
    r = range(-limit, limit + 1)
    for x in r:
        for y in r:
            for z in r:
                if x or y or z:
                    table.setdefault(x * x + y * y + z * z, []).append((x, y, z))
    return table


OFFSETS = _offsets_by_norm()
LADDER = [n for n in sorted(OFFSETS) if len(OFFSETS[n]) >= 3 and n < 56]       # 47 distinct exact squared distances below 7.5^2
LATTICE_CENTRE = (10.0, 10.0, 10.0)
TIE_FAMILIES = ("control", "tie_inside", "tie_swapped", "tie_Km1_K", "tie_K_Kp1", "triple_across", "two_at_centre", "exactly_K",
                "Km1_in_range", "none_in_range")
EDGE_FAMILIES = ("r2_edge", "r2_edge_tied", "eps_neighbour", "eps_centre_at", "eps_centre_above")
# the select-k forms of the general kernel the placed clouds run through: window, K
PLACED_FORMS = (("reg2/small", (5, 15), 6), ("reg2/mid", (5, 15), 12), ("reg3/small", (5, 35), 6), ("reg3/mid", (5, 35), 32),
                ("reg8/small", (11, 41), 6), ("reg8/rounds", (11, 41), 8), ("lds4", (5, 39), 9))


def sq3(v):
    """The kernels' squared norm in float32: (x*x + y*y) + z*z."""
    v = np.asarray(v, np.float32)
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


@functools.lru_cache(maxsize=None)
def eps_edge():
    """(at, above): a float32 point whose squared norm is EXACTLY the emptiness threshold 1e-10f (it counts as empty), and the
    point one float further out along x (it does not).  x is the largest float32 with x * x <= 1e-10f; its square falls one ulp
    short, and a small y makes up the difference."""
    x = np.float32(1e-5)
    while x * x <= EPS:
        x = np.nextafter(x, np.float32(1))
    while x * x > EPS:
        x = np.nextafter(x, np.float32(0))
    gap = float(EPS) - float(x * x)
    for k in range(0, 4000):
        at = np.array((x, np.sqrt(gap) * k / 1000, 0), np.float32)
        if sq3(at) == EPS:
            above = at.copy()
            above[0] = np.nextafter(x, np.float32(1))
            assert sq3(above) > EPS
            return at, above
    raise AssertionError("no float32 point with a squared norm of exactly 1e-10f")


def _family(fam, K, KT, rng, positions):
    """One designed centre: dict(centre, placed {visiting position: point}, rest ('near' in range / 'far' out of range / 'empty'),
    ties: tuples of ranks (among the in-range elements, by distance) that must share a distance, in_range: count or None)."""
    c = np.array(LATTICE_CENTRE, np.float32)
    M = K + 3                                                   # neighbours placed: ranks 0 .. K + 2
    norms = list(LADDER[:M])
    pick = [0] * M                                              # which offset of its norm rank r uses
    pos = list(positions[:M])
    rest, ties, in_range, marks = "near", [], None, {}

    def share(*ranks):                                          # these ranks take the distance of the first, distinct payloads
        for j, r in enumerate(ranks):
            norms[r], pick[r] = norms[ranks[0]], j
        ties.append(tuple(ranks))
    if fam == "tie_inside":
        share(K // 2, K // 2 + 1)
    elif fam == "tie_swapped":
        # rank 1 sits at array position 0, its twin (rank 2) at a later position, the nearest element later still: the reference's
        # first swap moves position 0 BEHIND the twin, so the twin comes first -- "lowest visiting position first" gets it wrong
        share(1, 2)
        later = sorted(pos[:3])
        pos[1], pos[2], pos[0] = 0, later[1], later[2]
        marks = dict(first=pos[2], second=0)
    elif fam == "tie_Km1_K":
        share(K - 1, K)
    elif fam == "tie_K_Kp1":
        share(K, K + 1)                                         # beyond the boundary: must not change the output
    elif fam == "triple_across":
        share(K - 2, K - 1, K)
    elif fam == "exactly_K":
        M, rest, in_range = K, "far", K
    elif fam == "Km1_in_range":
        M, rest, in_range = K - 1, "far", K - 1
    elif fam == "none_in_range":
        M, rest, in_range = 0, "far", 0
    placed = {pos[r]: c + np.array(OFFSETS[norms[r]][pick[r]], np.float32) for r in range(M)}
    if fam == "two_at_centre":                                  # both clamp to ELO_EPS: a tie at ranks 0 and 1
        placed[pos[0]], placed[pos[1]] = c.copy(), c.copy()
        ties.append((0, 1))
    return dict(centre=c, placed=placed, rest=rest, ties=ties, in_range=in_range, marks=marks, radius=(7.5, 9.9) if rest == "near" else (10.5, 13.0))


def _edge_family(fam, K, KT, rng, positions):
    """distance = 3 (r2 = 9, exact): a neighbour exactly AT the radius, its twin one float further out; a neighbour whose own
    squared norm is exactly the emptiness threshold 1e-10f, and one just above it; the same two as the centre."""
    at, above = eps_edge()
    c = np.array((1.0, 1.0, 1.0), np.float32)
    pos = list(positions)
    f32 = lambda *v: np.array(v, np.float32)
    out = dict(centre=c, rest="far", ties=[], in_range=None, radius=(4.0, 6.0), marks={})
    if fam in ("r2_edge", "r2_edge_tied"):
        twin = f32(np.nextafter(np.float32(4), np.float32(5)), 1, 1)         # (3 + 2^-21)^2 rounds above 9
        pts = [c + f32(1, 0, 0), c + f32(0, 1, 1), c + f32(2, 1, 0), c + f32(3, 0, 0), twin]
        out["marks"] = dict(edge=[pos[3]], twin=pos[4])
        if fam == "r2_edge_tied":
            pts.append(c + f32(1, 2, 2))                                      # a second neighbour at exactly 9: a tie at ranks 3, 4
            out["marks"]["edge"].append(pos[5])
            out["ties"] = [(3, 4)]
        out["in_range"] = len(pts) - 1
    elif fam == "eps_neighbour":
        pts = [above.copy(), at.copy(), c + f32(1, 0, 0), c + f32(0, 1, 1), c + f32(0, 2, 0)]
        out.update(rest="empty", in_range=4, marks=dict(above=pos[0], at=pos[1]))
    else:
        out["centre"] = (at if fam == "eps_centre_at" else above).copy()
        pts = [f32(1, 0, 0), f32(0, 2, 0), f32(0, 0, 1), f32(1, 1, 0)]
        out.update(rest="empty", in_range=4)       # (of the window; a centre that counts as empty is skipped whatever is in it)
    out["placed"] = {pos[r]: p for r, p in enumerate(pts)}
    return out


def _isolator_family(fam, K, KT, rng, positions):
    """(c): no two in-range distances equal, yet the rank form at hand gives up."""
    c = np.array(LATTICE_CENTRE, np.float32)
    if fam == "mid_over_64":
        # ranks 0..95 three per lane over lanes 0..31 (position j * 64 + lane), ranks 96..98 in lane 32: the 33rd smallest lane
        # minimum is rank 96, so select_mid_k's bound admits 97 candidates (> 64) and select_by_rank has to finish
        radii = 2.0 + 4.0 * (np.arange(99) + 0.5) / 99
        where = [(r % 3) * 64 + r // 3 for r in range(96)] + [32, 96, 160]
        return dict(centre=c, placed_radius=dict(zip(where, radii)), rest="near", ties=[], in_range=None, radius=(6.5, 9.9))
    # "small_no_bound": lane group 5 (lanes 40..47: visiting positions p with p % 64 // 8 == 5) holds no in-range slot, so the
    # largest of the eight group minima is "none" and every in-range slot (> 64 of them) is a candidate: the swap rounds run
    out_of_range = [p for p in range(KT) if p % 64 // 8 == 5]
    radii = 10.5 + 2.0 * (np.arange(len(out_of_range)) + 0.5) / len(out_of_range)
    return dict(centre=c, placed_radius=dict(zip(out_of_range, radii)), rest="near", ties=[], in_range=KT - len(out_of_range),
                radius=(2.0, 9.9))


def _placed_cases():
    out = []
    for form, win, K in PLACED_FORMS:
        tag = form.replace("/", "_")
        common = dict(kind="placed", B=None)
        out.append(_case("placed/%s/ties" % tag, "select", win[0], win[1], 3, win, K, dist=10.0, form=form, families=TIE_FAMILIES, **common))
        out.append(_case("placed/%s/edges" % tag, "select", win[0], win[1], 3, win, K, dist=3.0, form=form, families=EDGE_FAMILIES, **common))
    out.append(_case("isolator/reg3_mid/over_64_candidates", "select", 5, 35, 3, (5, 35), 32, dist=10.0, form="reg3/mid",
                     families=("mid_over_64",), kind="placed", B=None))
    for form, win in (("reg2/small", (8, 16)), ("reg8/small", (11, 41))):
        out.append(_case("isolator/%s/no_bound" % form.replace("/", "_"), "select", win[0], win[1], 3, win, 6, dist=10.0, form=form,
                         families=("small_no_bound",), kind="placed", B=None))
    return out


CASES = _boundary_cases() + _placed_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# (d): the clouds whose every pixel fused.cv_stage1 groups in-kernel (J = 2, 3, 8 at K = 6; J = 3 at K = 32 with fp16 storage)
IN_KERNEL = tuple(("placed/%s/%s" % (form, cloud), storage) for cloud in ("ties", "edges")
                  for form, storage in (("reg2_small", "f32"), ("reg3_small", "f32"), ("reg8_small", "f32"), ("reg3_mid", "f16")))


# ------------------------------------------------------------------------------------------------------------ input builders
def _unit(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _pixel_of(case, perm, hc, wc):
    """(h, w) of the pixel each visiting position of centre (hc, wc) probes (stride 1, window inside the grid: placed cases)."""
    kH, kW = case["kH"], case["kW"]
    p = perm.astype(np.int64)
    return hc + p // kW - kH // 2, wc + p % kW - kW // 2


def _placed_inputs(case):
    rng = _rng(case["name"])
    kH, kW, K = case["kH"], case["kW"], case["K"]
    H, W, KT = case["H"], case["W"], kH * kW
    hc, wc = kH // 2, kW // 2                                   # the grid IS the designed centre's window: no wrap, no padding
    perm = rng.permutation(KT).astype(np.int32)
    ph, pw = _pixel_of(case, perm, hc, wc)
    positions = [int(p) for p in rng.permutation(np.arange(K, KT))]     # placed neighbours sit behind the first K array positions
    fams = []
    B = len(case["families"])
    xyz1 = rng.normal(10.0, 1.5, (B, H, W, 3)).astype(np.float32)
    xyz2 = np.zeros((B, H, W, 3), np.float32)
    for b, fam in enumerate(case["families"]):
        maker = _family if fam in TIE_FAMILIES else _edge_family if fam in EDGE_FAMILIES else _isolator_family
        f = maker(fam, K, KT, rng, positions)
        f["name"] = fam
        c = f["centre"].astype(np.float64)
        pts = np.zeros((KT, 3), np.float64)                     # by visiting position
        placed = dict(f.get("placed", {}))
        for p, r in f.get("placed_radius", {}).items():
            placed[p] = c + _unit(rng, 1)[0] * r
        free = [p for p in range(KT) if p not in placed]
        if f["rest"] != "empty":
            lo, hi = f["radius"]
            radii = lo + (hi - lo) * (rng.permutation(len(free)) + 0.5) / len(free)
            pts[free] = c + _unit(rng, len(free)) * radii[:, None]
        for p, q in placed.items():
            pts[p] = q
        xyz2[b, ph, pw] = pts.astype(np.float32)
        xyz1[b, hc, wc] = f["centre"]
        fams.append(f)
    idx = np.empty((B, case["N"], 2), np.int32)
    idx[:, 0] = (hc, wc)
    idx[:, 1:, 0] = rng.integers(0, H, (B, case["N"] - 1))
    idx[:, 1:, 1] = rng.integers(0, W, (B, case["N"] - 1))
    return dict(xyz1=xyz1, xyz2=xyz2, idx=idx, perm=perm, families=fams)


def _cloud(rng, B, H, W, holes=0.1):
    x = rng.normal(0, 2.0, (B, H, W, 3))
    x[rng.random((B, H, W)) < holes] = 0
    return x.astype(np.float32)


def all_pixels(B, H, W):
    hh, ww = np.meshgrid(np.arange(H, dtype=np.int32), np.arange(W, dtype=np.int32), indexing="ij")
    return np.ascontiguousarray(np.broadcast_to(np.stack([hh, ww], -1).reshape(1, H * W, 2), (B, H * W, 2)))


def _cloud_inputs(case):
    rng = _rng(case["name"])
    B, H, W, N = case["B"], case["H"], case["W"], case["N"]
    H2, W2 = math.ceil(H / case["sh"]), math.ceil(W / case["sw"])
    KT = case["kH"] * case["kW"]
    xyz1, xyz2 = _cloud(rng, B, H, W), _cloud(rng, B, H2, W2)
    perm = rng.permutation(KT).astype(np.int32)
    if case["kind"] == "empty_class":
        # every window slot class of the dense select-k form is (raster slot % 8) = (column offset % 8) for a 16-wide window, so
        # emptying the columns = 3 (mod 8) of the queried grid leaves ONE class of every centre without a pixel: the bound is
        # "none", all 42 or 56 in-range neighbours (pairwise distinct distances) are candidates, the 32-entry list overflows
        xyz1, xyz2 = (rng.normal(0, 2.0, (B, H, W, 3)).astype(np.float32) for _ in range(2))
        xyz2[:, :, 3::8] = 0
    if case["kind"] == "tied_window":
        # placed ties for the centres of a dense call: all centres sit on one lattice point; every fifth column of the queried
        # grid holds a near neighbour at centre + an integer offset of norm LADDER[(3 * h + w // 5) % 14], so the 15 of them in a
        # 5x15 window inside the grid take 15 consecutive indices mod 14: ONE pair of equal distances at two pixels and nothing
        # else, at a rank that moves with the centre (among the nearest K + 1 for half of them, beyond for the rest); the other
        # pixels lie further out at pairwise distinct, inexact distances.  (A centre with several ties is redone as soon as
        # any of them shows; a single one must be seen wherever the two candidates land in the form's lists.)
        c = np.array(LATTICE_CENTRE, np.float64)
        radii = 7.5 + 2.4 * (rng.permutation(H * W) + 0.5) / (H * W)
        grid = (c + _unit(rng, H * W) * radii[:, None]).reshape(H, W, 3)
        for h in range(H):
            for m in range(0, W, 5):
                choices = OFFSETS[LADDER[(3 * h + m // 5) % 14]]
                grid[h, m] = c + np.array(choices[(h * 31 + m // 5) % len(choices)], np.float64)
        xyz2 = np.broadcast_to(grid.astype(np.float32), (B, H, W, 3)).copy()
        xyz1 = np.broadcast_to(c.astype(np.float32), (B, H, W, 3)).copy()
    if case["dense"]:
        idx = all_pixels(B, H, W)
    elif case["kind"] == "pack":
        far_h, far_w = H - 1, W - 1
        idx = np.array([[[0, 0], [far_h, far_w], [far_h // 2, far_w // 2], [far_h, far_w], [min(1, far_h), min(1, far_w)]]], np.int32)
        for h, w in idx[0]:                                    # the centres at both ends exist, and so do their neighbours
            xyz1[0, h, w] = rng.normal(0, 2.0, 3)
        xyz2[~xyz2.any(-1)] = 1.0
    else:
        idx = np.stack([rng.integers(0, H, (B, N)), rng.integers(0, W, (B, N))], -1).astype(np.int32)
    return dict(xyz1=xyz1, xyz2=xyz2, idx=idx, perm=perm)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = BY_NAME[name]
    return _placed_inputs(case) if case["kind"] == "placed" else _cloud_inputs(case)


def inputs(case):
    """The arrays of a case (cached; treat as read-only).  Refused cases have none: their sizes alone are refused."""
    assert case["refuse"] is None or isinstance(case["K"], str)
    return _inputs(case["name"])


def batch_of(case):
    return len(case["families"]) if case["kind"] == "placed" else case["B"]


def resolve_K(case, fits):
    """K of a case; "kmax" / "kmax+1": the largest K for which fits(kH, kW, K, sh, sw) (the library's own answer), and one more."""
    if not isinstance(case["K"], str):
        return case["K"]
    K = 1
    while fits(case["kH"], case["kW"], K + 1, case["sh"], case["sw"]):
        K += 1
    return K + (1 if case["K"].endswith("+1") else 0)


def oracle_args(case, K=None, all_centres=False):
    """The positional arguments (after the op) of oracle.grouping.fused_conv_*_k for a case."""
    a = inputs(case)
    idx = all_pixels(a["xyz1"].shape[0], case["H"], case["W"]) if all_centres else a["idx"]
    return (a["xyz1"], a["xyz2"], idx, a["perm"], case["H"], case["W"], idx.shape[1], case["kH"], case["kW"], K or case["K"], case["fc"],
            case["dist"], case["sh"], case["sw"])


# ------------------------------------------------------------------------------------------------------------ float32 restatements
def window_distances(case, b, n=0):
    """What the kernels see of centre n of batch element b, by visiting position, in float32 with the contract's operation
    order ((dx*dx + dy*dy) + dz*dz, no contraction): (d, valid, hit, hw) -- d clamped to 1e-10, hw = (h, w) of the probed pixel."""
    a = inputs(case)
    hc, wc = (int(v) for v in a["idx"][b, n])
    c = a["xyz1"][b, hc, wc]
    kH, kW = case["kH"], case["kW"]
    H2, W2 = a["xyz2"].shape[1:3]
    p = a["perm"].astype(np.int64)
    h = hc // case["sh"] + p // kW - kH // 2
    w = wc // case["sw"] + p % kW - kW // 2
    inside = (h >= 0) & (h < H2)
    w = np.where(w < 0, w + W2, w)
    w = np.where(w >= W2, w - W2, w)
    q = a["xyz2"][b, np.clip(h, 0, H2 - 1), w]
    valid = inside & ~(sq3(q) <= EPS)
    d = np.maximum(sq3((c[None, :] - q).astype(np.float32)), EPS).astype(np.float32)
    r2 = np.float32(case["dist"]) * np.float32(case["dist"])
    hit = valid & ~(d > r2)
    return d, valid, hit, np.stack([h, w], -1)


def small_k_bound_is_none(hit):
    """select_small_k's bound (the largest of the eight lane-group minima) is "none": a group of 8 lanes holds no in-range slot."""
    lanes = np.arange(hit.size) % 64 // 8
    return any(not hit[lanes == g].any() for g in range(8))


def mid_k_candidates(d, hit, K):
    """How many elements select_mid_k's bound admits: those not above the (K+1)-th smallest of the 64 per-lane minima."""
    dd = np.where(hit, d, np.float32(np.inf)).astype(np.float32)
    lane_min = np.full(64, np.inf, np.float32)
    np.minimum.at(lane_min, np.arange(dd.size) % 64, dd)
    return int((dd <= np.sort(lane_min)[K]).sum())

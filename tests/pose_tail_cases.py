"""ONE table of tiny cases for the pose tail -- the code that closes every pyramid level: softmax_valid_partial_kernel,
softmax_valid_merge_kernel, pose_head_kernel with its in-launch warp, scatter_min_kernel behind it, and mlp_sv_kernel -- each with
the form it must take (include/elo.h ELO_TAIL_FORM, spelled by _lib.tail_form_name).  Numpy only: tests/test_pose_tail_cpu.py asks the
library for the forms without a GPU and runs the float32 emulations, tests/test_pose_tail_gpu.py runs every case on the device.

Parts: (a) SV the stand-alone softmax_valid; (b) HEAD the pose head's own partial-sums launch; (c) MERGE hand-made partial sums into
the head's merge; (d) RIDE mlp_sv_kernel; (e) WARP the warp inside the head; (f) REFUSALS."""
from collections import namedtuple
import zlib

import numpy as np

F = np.float32
SV_MAX_PARTS = 512


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def sv_parts(N):
    """The slice count the table EXPECTS of a partial-sums launch (the library's answer is elo_softmax_valid_parts)."""
    return min(64, max(1, -(-N // 64)))


# ------------------------------------------------------------------------------------------------------------- validity patterns
def zero_points(rng, n):
    """n 'zero' points: every component +0.0 or -0.0"""
    return np.where(rng.random((n, 3)) < 0.5, F(0.0), F(-0.0)).astype(F)


def pattern_mask(pattern, N, rng):
    """(N,) bool validity of one batch element, or None where the cloud is too small for the pattern."""
    parts = sv_parts(N)
    per = -(-N // parts)
    ok = np.ones(N, bool)
    if pattern == "all":
        return ok
    if pattern == "random":                                     # ~30 % zero points
        return rng.random(N) >= 0.3 if N > 1 else ok
    if pattern == "none":
        return ~ok
    if pattern in ("one_first", "one_last", "one_boundary"):
        at = {"one_first": 0, "one_last": N - 1, "one_boundary": per if parts > 1 else None}[pattern]
        if at is None or N < 2:
            return None
        ok[:] = False
        ok[at] = True
        return ok
    if pattern == "slice_out":                                  # a whole slice invalid between valid ones
        if parts < 3:
            return None
        ok[per:2 * per] = False
        return ok
    if pattern in ("batch_out_first", "batch_out_last"):       # per slice: the rows of every wave's first 16-row batch (one trip =
        if per <= 64:                                           # 64 consecutive rows) invalid and the later ones valid / the reverse
            return None
        first = (np.arange(N) % per) < 64
        return ~first if pattern == "batch_out_first" else first
    raise KeyError(pattern)


PATTERNS = ("all", "random", "none", "one_first", "one_last", "one_boundary", "slice_out", "batch_out_first", "batch_out_last")


def cloud(name, B, N, pattern, none_element=None):
    """xyz (B,N,3) float32 with `pattern` in every batch element (`none_element`: that element has no valid point at all);
    zero points carry mixed signs of zero."""
    rng = rng_of("cloud|" + name)
    xyz = rng.normal(0, 5, (B, N, 3)).astype(F)
    xyz[np.all(xyz == 0, -1)] = 1.0
    some = rng.random((B, N)) < 0.15                            # VALID points with one or two components +-0: all three decide validity
    for k in rng.permutation(3)[:2]:
        hit = some & (rng.random((B, N)) < 0.6)
        xyz[..., k][hit] = np.where(rng.random(int(hit.sum())) < 0.5, F(0.0), F(-0.0))
    for b in range(B):
        ok = pattern_mask(pattern, N, rng) if b != none_element else np.zeros(N, bool)
        xyz[b][~ok] = zero_points(rng, int((~ok).sum()))
    return xyz


def logits_features(name, B, N, C, storage="f32", spread=3.0):
    """(feature, weight) (B,N,C) as STORED: float32, or float16 values for fp16 storage"""
    rng = rng_of("lf|" + name)
    f, w = rng.normal(0, 1, (B, N, C)), rng.normal(0, spread, (B, N, C))
    dt = np.float16 if storage == "f16" else F
    return f.astype(dt), w.astype(dt)


# ------------------------------------------------------------------------------------------------------------------ (a) SV
Sv = namedtuple("Sv", "name B N C pattern none_element")
SV_N = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 255, 257, 4095, 4096, 4097, 8193)
SV_C = (1, 3, 63, 64, 65, 130)


def _sv_cases():
    out = []
    add = lambda B, N, C, pattern, none=None: out.append(Sv("a_n%d_c%d_b%d_%s%s" % (N, C, B, pattern, "" if none is None else "_e%d" % none),
                                                            B, N, C, pattern, none))
    for N in SV_N:                                              # every N: random validity, C = 64
        add(1, N, 64, "random")
    for C in SV_C:                                              # every C on a subset of N (C > 64: more than one channel block)
        for N in (1, 17, 129) + ((4097,) if C <= 64 else ()):
            if C != 64:
                add(1, N, C, "random")
    for N, C in ((17, 64), (129, 65), (257, 3), (4097, 63)):    # B = 3, the last element without a valid point
        add(3 if N < 4097 else 2, N, C, "random", none=(2 if N < 4097 else 1))
    for pattern in PATTERNS:                                    # every pattern wherever the cloud is large enough for it
        if pattern == "random":
            continue
        for N in (1, 17, 129, 257, 4097, 8193):
            if pattern_mask(pattern, N, np.random.default_rng(0)) is not None and not (pattern == "all" and N in (1, 17)):
                add(1, N, 64 if N != 257 else 65, pattern)
    return out


SV = _sv_cases()

# ---------------------------------------------------------------------------------------------------------------- (b) HEAD
Head = namedtuple("Head", "name B N C hidden storage coarse pose7 pattern")
MODEL = (64, 256)
GENERIC = ((64, 128), (32, 256), (16, 64), (65, 256), (130, 40), (1, 1), (64, 300))
HEAD_N = (1, 17, 64, 65, 257, 4096, 4097, 8193)


def _head_cases():
    out = []

    def add(B, N, C, hidden, storage, coarse, pose7="none", pattern="random"):
        out.append(Head("b_n%d_c%d_h%d_%s_%s_%s_b%d_%s" % (N, C, hidden, storage, "coarse" if coarse else "l3", pose7, B, pattern),
                        B, N, C, hidden, storage, coarse, pose7, pattern))
    for i, N in enumerate(HEAD_N):                              # the model head over the N list, both storage types
        for storage in ("f32", "f16"):
            add(1 if N > 4096 else 2, N, 64, 256, storage, coarse=bool(i % 2) ^ (storage == "f16"))
    for i, (C, hidden) in enumerate(GENERIC):                   # the generic head, with and without the coarse pose
        for storage in ("f32", "f16"):
            for coarse in (False, True):
                add(2, (129, 17, 257)[i % 3], C, hidden, storage, coarse)
    add(2, 129, 64, 256, "f32", True, pose7="row")
    add(2, 129, 64, 256, "f16", False, pose7="ring")          # a PoseRing of 3 slots called 4 times: the cursor wraps
    add(2, 4097, 64, 256, "f32", False, pattern="batch_out_first")
    add(2, 4097, 65, 256, "f16", True, pattern="batch_out_last")
    add(3, 129, 130, 40, "f32", False, pattern="slice_out")
    return out


HEAD = _head_cases()


def head_weights(name, C, hidden):
    """Dense random weights (W_big, b_big, W_q, b_q, W_t, b_t), float32"""
    rng = rng_of("w|" + name)
    s = lambda *shape: rng.normal(0, 0.1, shape).astype(F)
    b_q = (np.array([1, 0, 0, 0], F) + s(4)).astype(F)          # (the model initialises near the identity)
    return s(C, hidden), s(hidden), s(hidden, 4), b_q, s(hidden, 3), s(3)


def integer_head(name, B, C, hidden):
    """The dense layers WITHOUT rounding: a cloud of ONE valid point per batch element (the softmax of one point is its feature, bit
    for bit: e^0 = 1, v / 1), integer features in -3..3 and integer weights in -2..2 -- every product and every partial sum of both
    layers is an integer below 2^24 (|big| <= 2 + 6 C <= 782, |raw| <= 2 + 2 hidden |big| < 2^19), so the head's raw output is exact in
    any summation order and the pose carries the composition's own roundings only.  Returns (feature (B,1,C), weights)."""
    rng = rng_of("int|" + name)
    i = lambda lo, hi, *shape: rng.integers(lo, hi + 1, shape).astype(F)
    b_q = i(-2, 2, 4)
    b_q[0] = 2                                                   # (not the zero quaternion)
    return i(-3, 3, B, 1, C), (i(-2, 2, C, hidden), i(-2, 2, hidden), i(-2, 2, hidden, 4), b_q, i(-2, 2, hidden, 3), i(-2, 2, 3))


def selection_weights(C, hidden, channels):
    """The head as a READ-OUT of up to three pooled channels: hidden unit k copies channel channels[k], W_t picks units 0..2, zero
    biases, q = (1, 0, 0, 0).  Every product is by 0 or 1 and every sum has one non-zero term: t[k] = pooled[channels[k]] bit for bit
    (hidden >= len(channels))."""
    W_big, W_t = np.zeros((C, hidden), F), np.zeros((hidden, 3), F)
    for k, c in enumerate(channels):
        W_big[c, k] = 1.0
        W_t[k, k] = 1.0
    return W_big, np.zeros(hidden, F), np.zeros((hidden, 4), F), np.array([1, 0, 0, 0], F), W_t, np.zeros(3, F)


def model_selection_weights(call):
    """The MODEL head's read-out of call `call` of 22: unit j copies channel j mod 64 and W_t selects units 3 call .. 3 call + 2."""
    W_big, W_t = np.zeros((64, 256), F), np.zeros((256, 3), F)
    W_big[np.arange(256) % 64, np.arange(256)] = 1.0
    chans = [c for c in range(3 * call, 3 * call + 3) if c < 64]
    for k, c in enumerate(chans):
        W_t[c, k] = 1.0
    return chans, (W_big, np.zeros(256, F), np.zeros((256, 4), F), np.array([1, 0, 0, 0], F), W_t, np.zeros(3, F))


def readout_channels(C, hidden):
    """Channel triples the (b) cases read out exactly: the first, the last, and the ones either side of the 64-channel block border."""
    k = min(3, hidden, C)
    want = [list(range(k)), list(range(C - k, C))]
    if C > 64:
        want.append([c for c in (63, 64, 65) if c < C][:k])
    return [w for i, w in enumerate(want) if w and w not in want[:i]]


def coarse_pose(name, B):
    rng = rng_of("coarse|" + name)
    q = rng.normal(0, 1, (B, 4))
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F), rng.normal(0, 1, (B, 3)).astype(F)


# --------------------------------------------------------------------------------------------------------------- (c) MERGE
Merge = namedtuple("Merge", "name parts top B first_live")
MERGE_PARTS = (1, 2, 4, 5, 63, 64, 65, 127, 128, 129, 257, 511, 512)
MERGE = [Merge("c_p%d_top_%s" % (p, top), p, top, 2, False) for p in MERGE_PARTS for top in ("last", "first")] + \
        [Merge("c_p%d_live0" % p, p, "last", 2, True) for p in (5, 65, 129, 257)]     # slice 0 live: the slot a clamped load reads


def merge_empty(parts, first_live=False):
    """The empty slices (denominator 0): first, last and every 4th (so thread group 2 of the in-head merge sees none) -- as far as
    one live slice remains; `first_live`: not the first."""
    empty = {0, parts - 1} | set(range(2, parts, 4))
    if parts <= 2:
        empty = {0} if parts == 2 else set()
    if len(empty) >= parts:
        empty.discard(1 if parts > 1 else 0)
    if first_live:
        empty.discard(0)
    return sorted(empty)


def merge_triples(case, C=64):
    """Hand-made (mx, den, acc), each (B, parts, C) float32: maxima spread over ~80 units (rescaling factors underflow) with the
    largest in the last / first LIVE slice; empty slices hold what the producers write there: -inf, 0, 0."""
    rng = rng_of("triples|" + case.name)
    B, parts = case.B, case.parts
    mx = rng.uniform(-80.0, 0.0, (B, parts, C)).astype(F)
    den = rng.uniform(1.0, 64.0, (B, parts, C)).astype(F)
    acc = (den * rng.normal(0, 1, (B, parts, C))).astype(F)
    empty = merge_empty(parts, case.first_live)
    live = [i for i in range(parts) if i not in empty]
    mx[:, live[-1] if case.top == "last" else live[0]] = F(1.5)
    mx[:, live[len(live) // 2], ::2] = F(-0.25)                 # (a close second on every other channel)
    mx[:, empty], den[:, empty], acc[:, empty] = -np.inf, 0.0, 0.0
    return mx, den, acc


# ---------------------------------------------------------------------------------------------------------------- (d) RIDE
Ride = namedtuple("Ride", "name B N tile storage pattern none_element pair")
RIDE_N = (1, 15, 16, 17, 31, 33, 100)


def _ride_cases():
    out = []

    def add(B, N, tile, storage, pattern="random", none=None, pair=False):
        out.append(Ride("d_n%d_t%d_%s_b%d_%s%s%s" % (N, tile, storage, B, pattern, "" if none is None else "_e%d" % none, "_pair" if pair else ""),
                        B, N, tile, storage, pattern, none, pair))
    for N in RIDE_N:
        for tile in (16, 32):
            for storage in ("f32", "f16"):
                add(1, N, tile, storage)
    add(1, 1025, 16, "f32")                                     # 65 tiles: the in-head merge takes trips of 32
    add(1, 2049, 16, "f16")                                     # 129 tiles: a second trip of 32
    add(1, 2049, 32, "f32")                                     # 65 tiles of 32 rows
    add(2, 100, 16, "f32", "tile_out", none=1)                 # one empty element, one all-invalid tile
    add(2, 100, 32, "f16", "tile_out", none=0)
    add(1, 100, 16, "f32", pair=True)                           # the paired form (job a the logits, job b the features, side by side)
    add(2, 57, 32, "f16", pair=True)
    return out


RIDE = _ride_cases()


def ride_cloud(case):
    if case.pattern != "tile_out":
        return cloud(case.name, case.B, case.N, case.pattern, case.none_element)
    xyz = cloud(case.name, case.B, case.N, "random", case.none_element)
    rng = rng_of("tile_out|" + case.name)
    for b in range(case.B):
        xyz[b, case.tile:2 * case.tile] = zero_points(rng, case.tile)      # tile 1: no valid row
    return xyz


def ride_inputs(case):
    """The MLP launch of a (d) case: sources x (B,N,64) as stored, one 64 -> 64 layer (W, b) without activation whose output are the
    logits (standard deviation ~3), and the features: an existing (B,N,64) tensor, or in the paired form job b's (x2, W2, b2)."""
    rng = rng_of("ride|" + case.name)
    dt = np.float16 if case.storage == "f16" else F
    shape = (case.B, case.N, 64)
    out = dict(x=rng.normal(0, 1, shape).astype(dt), W=rng.normal(0, 0.35, (64, 64)).astype(F), b=rng.normal(0, 0.5, 64).astype(F))
    if case.pair:
        out.update(x2=rng.normal(0, 1, shape).astype(dt), W2=rng.normal(0, 0.12, (64, 64)).astype(F), b2=rng.normal(0, 0.1, 64).astype(F))
    else:
        out.update(feature=rng.normal(0, 1, shape).astype(dt))
    return out


def tile_units(tile):
    """elo_tuning.small_tile_units that forces the tile height of a row-wise MLP launch"""
    return 1 << 40 if tile == 16 else 0


# ---------------------------------------------------------------------------------------------------------------- (e) WARP
Warp = namedtuple("Warp", "name B N H W C storage pose")
WARP = [Warp("e_n1_c0", 1, 1, 4, 57, 0, "f32", "general"),
        Warp("e_n255_c16_f16", 2, 255, 4, 57, 16, "f16", "general"),
        Warp("e_n256_c5", 1, 256, 4, 57, 5, "f32", "general"),
        Warp("e_n257_c0", 2, 257, 4, 57, 0, "f32", "general"),
        Warp("e_n600_c3", 2, 600, 4, 57, 3, "f32", "general"),
        Warp("e_n600_c4_f16", 1, 600, 4, 29, 4, "f16", "general2"),
        Warp("e_n257_c3_ties", 2, 257, 4, 57, 3, "f32", "identity"),         # exact pass-through: ties by construction
        Warp("e_n255_c2_f16_origin", 1, 255, 4, 57, 2, "f16", "shift")]      # identity rotation, t = -p0: a valid point lands on +0, +0, +0
# A zero point warps to (w + t) * 0 = the SIGNS of t (w = 0): 'general' t = (+, -, +) gives atan2f(-0, +0) = -0, zero cell kind 0;
# 'general2' t = (-, +, -) gives atan2f(+0, -0) = pi, kind 1; 'shift' t = (-, -, -) gives atan2f(-0, -0) = -pi, kind 2.
BORDER = 1e-3                                                    # cells are compared for points whose continuous row / column
EXCLUDED_CAP = 0.02                                              # coordinate is further than this from an integer; at most 2 % are not
ORIGIN_RANGE = 1e-6                                              # a point whose float64 range is below this is judged by the float32 warp
ORIGIN_NOTE = ("a valid point mapped onto the origin: found in float32 for the pattern (+0, +0, +0) -- identity rotation, t = -p, "
               "x + (-x) = +0 in round-to-nearest (tests/pose_tail_reference.py warp32 states it; in float64 the inverse's 1e-10 leaves "
               "the point 1e-10 beside the origin, so the cell comparison excludes it and the test asserts its bits).  None was found "
               "for a pattern with a -0 component: (w + t) * 1 is -0 only where w and t are both -0, and the identity rotation returns "
               "w = p, whose components are not all zero.")


def pose_weights(case, B):
    """Head weights that make the pose a CONSTANT of the case (W_q = W_t = 0: the pose is the biases): 'general' a rotation of a few
    degrees and a translation, 'identity' q = (1,0,0,0), t = 0 -- the warp then returns every point bit for bit -- and 'shift' the
    identity rotation with t = -(2, 4, 1)."""
    z = np.zeros
    if case.pose == "general":
        b_q, b_t = np.array([1.0, 0.02, -0.015, 0.03], F), np.array([0.4, -0.25, 0.1], F)
    elif case.pose == "general2":
        b_q, b_t = np.array([0.9, -0.03, 0.02, 0.01], F), np.array([-0.4, 0.25, -0.1], F)
    elif case.pose == "identity":
        b_q, b_t = np.array([1, 0, 0, 0], F), z(3, F)
    else:
        b_q, b_t = np.array([1, 0, 0, 0], F), np.array([-2.0, -4.0, -1.0], F)
    rng = rng_of("pw|" + case.name)
    return rng.normal(0, 0.1, (64, 256)).astype(F), rng.normal(0, 0.1, 256).astype(F), z((256, 4), F), b_q, z((256, 3), F), b_t


def warp_cloud(case, R):
    """The cloud the head warps, (B,N,3) float32: target points well inside their cells (0.2 .. 0.8 of a cell from its borders, as
    backward_check._boundary_safe_points draws them) carried back through the float64 inverse of the case's pose; ~10 % zero points
    with mixed signs of zero; the special points of the 'identity' and 'shift' cases.  Returns (xyz, dict of special indices)."""
    rng = rng_of("wc|" + case.name)
    B, N, H, W = case.B, case.N, case.H, case.W
    az, vres, voff = R.projection_constants(H, W)
    col = rng.integers(0, W, (B, N)) + rng.uniform(0.2, 0.8, (B, N))
    rowf = rng.integers(1, H, (B, N)) + rng.uniform(0.2, 0.8, (B, N))
    r = rng.uniform(3, 30, (B, N))
    if case.pose == "identity":                                 # the two tie pairs: their own cells, nearer than every other point
        col[:, 0], rowf[:, 0], r[:, 0] = 10.5, 1.5, 2.0
        col[:, 2], rowf[:, 2], r[:, 2] = 40.5, 2.5, 2.5
    a, beta = np.pi - col * az, (rowf - voff) * vres
    target = np.stack([r * np.cos(beta) * np.cos(a), r * np.cos(beta) * np.sin(a), r * np.sin(beta)], -1)
    _, _, _, b_q, _, b_t = pose_weights(case, B)
    q = R.normalise_q(np.asarray(b_q, np.float64)[None])[0]
    qi = R.inv_q(q[None])[0]
    back = target - np.asarray(b_t, np.float64)
    pq = np.concatenate([np.zeros((B, N, 1)), back], -1)
    xyz = R.hamilton(R.hamilton(qi, pq), R.inv_q(qi[None])[0])[..., 1:].astype(F)
    special = {}
    if N >= 20:
        zeros = rng.random((B, N)) < 0.1
        zeros[:, :13] = False
        if case.storage == "f16" and case.C:                    # fp16 features are summed with packed fp16 atomics: two zero points per
            zeros[:] = False                                    # image, so the zero cell's sum does not depend on the order of the adds
            zeros[:, 13:15] = True
        for b in range(B):
            xyz[b][zeros[b]] = zero_points(rng, int(zeros[b].sum()))
    if case.pose == "identity":
        xyz[:, 1] = xyz[:, 0]                                   # two points tied at the same range in one cell: the cell holds their sum
        xyz[:, 3] = xyz[:, 2]
        xyz[:, 4] = (F(0.0), F(-0.0), F(0.0))                   # zero points of three sign patterns
        xyz[:, 5] = (F(-0.0), F(0.0), F(-0.0))
        xyz[:, 6] = (F(-0.0), F(-0.0), F(0.0))
        special = {"ties": ((0, 1), (2, 3)), "zeros": (4, 5, 6)}
    if N >= 20:                                                 # valid points with zero components (a point is dropped only if ALL are zero)
        xyz[:, 10] = (F(0.0), F(3.1), F(-0.7))
        xyz[:, 11] = (F(2.2), F(-0.0), F(0.4))
        xyz[:, 12] = (F(-0.0), F(0.0), F(2.5))
        special = dict(special, axis=(10, 11, 12))
    if case.pose == "shift":
        xyz[:, 0] = (F(2.0), F(4.0), F(1.0))                    # + t = (+0, +0, +0): a VALID point of range 0
        special = dict(special, origin=0)
    return xyz, special


# ----------------------------------------------------------------------------------------------------------- (f) REFUSALS
Refusal = namedtuple("Refusal", "name status match fields warp")
ERR_ARG, ERR_LIMIT = -1, -2
REFUSALS = [
    Refusal("f_ready_parts_c32", ERR_ARG, "64 channels wide", dict(C=32, ready_parts=4), None),
    Refusal("f_ready_parts_513", ERR_ARG, "ready_parts is 0", dict(ready_parts=SV_MAX_PARTS + 1), None),
    Refusal("f_q_coarse_alone", ERR_ARG, "go together", dict(q_coarse=True, t_coarse=False), None),
    Refusal("f_f16_odd_clear_c", ERR_ARG, "even clear_C", dict(storage="f16", clear_C=3), None),
    Refusal("f_warp_other_buffers", ERR_ARG, "must be the ones this call clears", dict(), "other"),
    Refusal("f_lds_limit", ERR_LIMIT, "bytes of LDS", dict(C=64, hidden=15513), None),     # 64 + 15513 + 808 floats = 65540 bytes
]
LDS_FITS = dict(C=64, hidden=15512)                              # ... and one unit less is exactly 64 KiB: launched
RIDE_TOO_MANY_TILES = (8193, 16)                                 # 513 tiles of 16 rows: elo_mlp_sv_parts answers 0


# ------------------------------------------------------------------------------------------------------------ expected forms
def tail_form(partials, parts, C, hidden, warp=False):
    return "%sx%d/%s/%s%s%s" % (partials, parts, "trips16" if parts <= 64 else "trips32",
                                "model" if (C, hidden) == MODEL else "generic", "+wide" if C > 64 else "", "+warp" if warp else "")


def expected_form(case):
    if isinstance(case, Head):
        return tail_form(case.storage, sv_parts(case.N), case.C, case.hidden)
    if isinstance(case, Merge):
        return tail_form("ready", case.parts, 64, 256)
    if isinstance(case, Ride):
        return tail_form("ready", -(-case.N // case.tile), 64, 256)
    if isinstance(case, Warp):
        return tail_form(case.storage, 1, 64, 256, warp=True)
    raise TypeError(case)

"""TEST INFRASTRUCTURE of the fused-shape tests: ONE table of cases for the tile kernels of csrc/elo_fused.hip (setconv_kernel,
mlp_kernel, cv1_meta_kernel, cv2_kernel) with the form each must take, the seeded numpy inputs of a case, and the refusals.

A case is tiny (at most about 100 rows or centres).  It runs in fp32 and in fp16 storage, with split and with half products, and
the three cases per part named in CHECKED also on the range-checked instances.  tests/test_fused_shapes_cpu.py proves from the
table itself that it covers what the kernels can do differently (every (pairs, tail) class of the K loop, every column-block
count, both tile heights, every gather path, every pooling branch, every centre source, tile seams); tests/test_fused_shapes_gpu.py
runs it.  No GPU is touched here."""
import zlib
from collections import namedtuple

import numpy as np

STORAGES = ("f32", "f16")
PRODUCTS = ("split", "half")

# Part A: row-wise MLP.  srcs: source widths; layers: layer widths; tile: the forced tile height; pair: a paired launch;
# stage2: None or (w_before, w_after, second-stage layer widths); relu_last: ReLU on the last layer of each stage
MlpCase = namedtuple("MlpCase", "name srcs layers rows tile pair stage2 relu_last")
MLP = [
    MlpCase("a01", (1,), (1,), 1, 32, False, None, True),
    MlpCase("a02", (3,), (5,), 15, 16, False, None, False),
    MlpCase("a03", (7,), (16,), 16, 16, False, None, True),
    MlpCase("a04", (20,), (20,), 17, 16, False, None, True),
    MlpCase("a05", (33,), (40,), 33, 32, False, None, False),
    MlpCase("a06", (64, 6), (50,), 95, 32, False, None, True),
    MlpCase("a07", (8, 8, 8), (72,), 95, 16, False, None, True),
    MlpCase("a08", (40, 24, 12), (100,), 33, 16, False, None, False),
    MlpCase("a09", (128, 64), (128,), 17, 32, False, None, True),
    MlpCase("a10", (64, 64, 64), (90,), 16, 16, False, None, True),
    MlpCase("a11", (128, 40), (16,), 15, 32, False, None, True),
    MlpCase("a12", (20,), (20, 100), 33, 16, False, None, True),            # narrow -> wide: the K padding behind N = 20 is read
    MlpCase("a13", (33,), (50, 72), 17, 32, False, None, False),            # ... and behind N % 4 != 0
    MlpCase("a14", (7,), (5, 1), 16, 32, False, None, True),
    MlpCase("a15", (64, 6), (100, 40), 95, 16, False, None, True),
    MlpCase("a16", (8, 8, 8), (40, 128), 1, 16, False, None, True),
    MlpCase("a17", (3,), (16, 20, 50), 15, 32, False, None, True),
    MlpCase("a18", (40, 24, 12), (72, 100, 128), 33, 32, False, None, False),
    MlpCase("a19", (1,), (128, 5, 72), 17, 16, False, None, True),
    MlpCase("a20", (64, 64, 64), (128, 90, 128), 95, 32, False, None, True),
    MlpCase("a21", (20,), (40,), 17, 16, True, None, True),
    MlpCase("a22", (33,), (20, 100), 33, 32, True, None, False),
    MlpCase("a23", (64, 6), (50, 16, 90), 16, 16, True, None, True),
    MlpCase("a24", (8, 8, 8), (16,), 33, 32, False, (16, 64, (20, 40)), True),
    MlpCase("a25", (20,), (40, 128), 17, 16, False, (10, 0, (50,)), True),
    MlpCase("a26", (33,), (128,), 95, 32, False, (12, 20, (72, 16)), False),
    MlpCase("a27", (64, 6), (100, 128), 15, 16, False, (16, 64, (100,)), True),
    MlpCase("a28", (7,), (20,), 16, 32, False, (0, 7, (5,)), True),
    MlpCase("a29", (3,), (72,), 1, 32, False, (0, 0, (128, 1)), True),
    MlpCase("a30", (40, 24, 12), (40,), 17, 16, True, (12, 20, (90,)), True),
    MlpCase("a31", (128, 40), (20,), 33, 16, False, (10, 0, (16,)), False),  # 33 rows: the last 16-row tile clamps its before-rows
    MlpCase("a32", (1,), (100, 128), 33, 32, True, (16, 64, (128, 128, 128)), True),
    MlpCase("a33", (7,), (40,), 15, 32, False, (10, 0, (5,)), True),         # second-stage K = 50, 100, 120: the classes (2, -), (3, T),
    MlpCase("a34", (3,), (20,), 17, 16, False, (16, 64, (72,)), True),       # (4, -) of a layer fed by a gather
    MlpCase("a35", (33,), (40,), 16, 16, False, (16, 64, (16,)), False),
    MlpCase("a36", (33,), (128,), 17, 16, False, (12, 20, (16,)), True),     # ... and (5, -), (4, T), (3, -) at the tile height
    MlpCase("a37", (20,), (40, 128), 95, 32, False, (10, 0, (20,)), True),   # the cases above leave them out at
    MlpCase("a38", (8, 8, 8), (16,), 15, 16, False, (16, 64, (5,)), True),
]

# Part B: set-conv.  centre: "xyz" (centre_xyz), "hw" (centre_hw into a grid, new_xyz written) or "pixel" (every pixel, in-kernel
# grouping only); group: None = pre-grouped idx / mask, else (kernel_h, kernel_w, distance, stride_h, stride_w) of an in-kernel
# random-k over a 3 x 7 queried grid (n is then the centre count of a "hw" case, or 21 * stride_h * stride_w pixels)
SetconvCase = namedtuple("SetconvCase", "name B n K C layers tile centre group pair relu_last")
SETCONV = [
    SetconvCase("b01", 1, 1, 1, 0, (1,), 32, "xyz", None, False, True),
    SetconvCase("b02", 3, 7, 3, 3, (5,), 32, "xyz", None, False, True),
    SetconvCase("b03", 3, 7, 3, 4, (16,), 16, "hw", None, False, False),
    SetconvCase("b04", 1, 11, 5, 7, (20, 100), 32, "xyz", None, False, True),
    SetconvCase("b05", 3, 11, 5, 8, (40,), 16, "hw", None, False, True),
    SetconvCase("b06", 3, 7, 7, 12, (50, 72), 32, "hw", None, False, True),
    SetconvCase("b07", 1, 7, 7, 20, (72,), 16, "xyz", None, False, False),
    SetconvCase("b08", 3, 11, 8, 64, (100, 40), 32, "xyz", None, False, True),
    SetconvCase("b09", 1, 11, 8, 3, (128,), 16, "hw", None, False, True),
    SetconvCase("b10", 3, 7, 12, 4, (16, 20, 50), 32, "xyz", None, False, True),
    SetconvCase("b11", 1, 7, 12, 7, (90,), 16, "xyz", None, False, True),
    SetconvCase("b12", 3, 11, 16, 8, (5, 1), 32, "hw", None, False, False),
    SetconvCase("b13", 1, 11, 16, 12, (100,), 16, "xyz", None, False, True),
    SetconvCase("b14", 3, 7, 20, 20, (40, 128), 32, "xyz", None, False, True),
    SetconvCase("b15", 1, 7, 32, 64, (72, 100, 128), 32, "hw", None, False, True),
    SetconvCase("b16", 3, 11, 1, 7, (20,), 16, "xyz", None, False, True),
    SetconvCase("b17", 1, 11, 32, 0, (16,), 32, "xyz", None, False, True),
    SetconvCase("b18", 3, 7, 5, 3, (40, 16), 32, "xyz", None, True, True),
    SetconvCase("b19", 1, 11, 8, 8, (50,), 16, "hw", None, True, False),
    SetconvCase("b20", 1, 21, 5, 3, (20,), 32, "pixel", (3, 5, 3.0, 1, 1), False, True),
    SetconvCase("b21", 3, 21, 8, 64, (100, 40), 16, "pixel", (3, 5, 3.0, 1, 1), False, True),
    SetconvCase("b22", 3, 11, 12, 7, (50,), 32, "hw", (3, 5, 4.0, 2, 2), False, False),
    SetconvCase("b23", 1, 21, 3, 4, (16,), 16, "pixel", (3, 3, 2.5, 1, 1), True, True),
    SetconvCase("b24", 1, 7, 32, 12, (72,), 32, "hw", (3, 5, 1e3, 1, 2), False, True),   # 15 window slots, K = 32: zero-filled slots
    SetconvCase("b25", 3, 7, 20, 0, (5, 16), 32, "xyz", None, False, True),
    SetconvCase("b26", 1, 11, 3, 20, (128, 128), 16, "xyz", None, False, True),
]
GRID = (3, 7)                                            # the queried grid of parts B and C

# Part C: cost-volume stage 1 / stage 2, pre-grouped, on the 3 x 7 grid.  C: (fp32 storage, fp16 storage) channel counts;
# far: the valid logits lie at -3e10, below the -1e10 that stands for a clear slot (such a case pins the masked constant, not the
# arithmetic or the slot count: fp32 cannot resolve the logits' differences at that magnitude, and its clear rows are identical)
CvCase = namedtuple("CvCase", "name stage B K C tile far")
CV = [
    CvCase("c01", 1, 1, 1, (4, 8), 32, False),
    CvCase("c02", 1, 2, 3, (8, 8), 16, False),
    CvCase("c03", 1, 1, 5, (24, 24), 32, False),
    CvCase("c04", 1, 2, 8, (40, 40), 16, False),
    CvCase("c05", 1, 1, 12, (64, 64), 32, False),
    CvCase("c06", 1, 2, 20, (4, 24), 32, False),
    CvCase("c07", 1, 1, 32, (8, 8), 32, False),
    CvCase("c08", 1, 2, 4, (24, 40), 32, False),
    CvCase("c09", 1, 1, 6, (40, 64), 16, False),
    CvCase("c10", 1, 2, 8, (8, 8), 16, True),
    CvCase("c11", 1, 1, 16, (24, 24), 16, False),
    CvCase("c12", 2, 1, 1, (8, 8), 16, False),
    CvCase("c13", 2, 2, 3, (4, 24), 32, False),
    CvCase("c14", 2, 1, 5, (40, 40), 16, False),
    CvCase("c15", 2, 2, 8, (64, 64), 32, False),
    CvCase("c16", 2, 1, 12, (24, 24), 16, False),
    CvCase("c17", 2, 2, 20, (8, 8), 32, False),
    CvCase("c18", 2, 1, 32, (40, 64), 32, False),
    CvCase("c19", 2, 2, 4, (4, 8), 16, False),
    CvCase("c20", 2, 1, 6, (24, 24), 32, False),
    CvCase("c21", 2, 2, 8, (8, 40), 32, True),
    CvCase("c22", 2, 1, 16, (64, 64), 32, False),
]

CASES = {"mlp": MLP, "setconv": SETCONV, "cv": CV}
# three cases per part that also run on the range-checked instances
CHECKED = {"mlp": ("a06", "a18", "a27"), "setconv": ("b04", "b15", "b21"), "cv": ("c03", "c13", "c18")}


def runs(part):
    """(case, storage, products) of every run of a part: storages x {split, half}, and "checked" for the part's CHECKED cases"""
    out = [(c, s, p) for c in CASES[part] for s in STORAGES for p in PRODUCTS]
    return out + [(c, s, "checked") for c in CASES[part] if c.name in CHECKED[part] for s in STORAGES]


def run_id(run):
    return "%s-%s-%s" % (run[0].name, run[1], run[2])


def expected_form(case, products):
    return "tile%d/%s" % (case.tile, products)


def tile_units(tile):
    """elo_tuning.small_tile_units that forces a tile height (K <= 16; above that a point's rows only fit the 32-row tile)"""
    return 1 << 40 if tile == 16 else 0


def cv_channels(case, storage):
    return case.C[1] if storage == "f16" else case.C[0]


# ---------------------------------------------------------------------------- what a case exercises (read by the CPU test)
def k_loop_class(K):
    """(32-k pairs, 16-k tail) of a layer with K inputs: dense_impl's NP and KS & 1"""
    KS = (K + 15) // 16
    return KS // 2, bool(KS & 1)


def layer_inputs(case):
    """the K of every layer a case runs (first-stage chain, then the second stage's)"""
    if isinstance(case, MlpCase):
        ks = [sum(case.srcs)] + list(case.layers[:-1])
        if case.stage2:
            wb, wa, l2 = case.stage2
            ks += [wb + case.layers[-1] + wa] + list(l2[:-1])
        return ks
    if isinstance(case, SetconvCase):
        return [3 + case.C] + list(case.layers[:-1])
    return None


def layer_widths(case):
    if isinstance(case, MlpCase):
        return list(case.layers) + (list(case.stage2[2]) if case.stage2 else [])
    return list(case.layers)


def vector_path(width, storage):
    """seg_ok's width condition: whole 16-byte items (the test tensors are 16-byte aligned and the rows fit the segment budget)"""
    return width > 0 and width % (8 if storage == "f16" else 4) == 0


def pool_branch(K):
    return "k4" if K == 4 else "k6" if K == 6 else "mult8" if K % 8 == 0 else "other"


def tiles_of(points, K, tile):
    """(points per tile, tiles, points in the last tile) of a grouped kernel"""
    P = tile // K
    n = -(-points // P)
    return P, n, points - (n - 1) * P


# ---------------------------------------------------------------------------- seeded inputs
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def features(rng, shape, storage):
    """seeded normals as the product would hold them: fp16-representable values when the storage is fp16"""
    x = rng.normal(0, 1, shape).astype(np.float32)
    return x.astype(np.float16).astype(np.float32) if storage == "f16" else x


_LAYERS = {}


def deep_weights(rng, k, n):
    """Weights of a layer BEHIND another layer: per output column two strong entries (+-0.4 .. 0.8, at random rows) over a weak dense
    part (normal, column sum of magnitudes about 0.02), so that every weight is distinct and non-zero but sum_k |W_kn| stays near
    1.2.  A worst-case bound grows by that column sum per layer where rounding errors add like its root: with dense unit-variance
    columns (sum about 0.8 sqrt(k)) the bound of a three- or six-layer chain would sit hundreds of times above any real error and
    an arithmetic mistake of 2^-12 would pass.  The FIRST layer of every chain -- the one a gather feeds, whose K loop classes the
    table counts -- keeps dense weights of column norm 1."""
    W = rng.normal(0, 1, (k, n)) * (0.025 / k)
    for col in range(n):
        rows = rng.choice(k, size=min(2, k), replace=False)
        W[rows, col] = rng.uniform(0.4, 0.8, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    return W.astype(np.float32)


def make_layers(K, widths, relu_last=True, tag="", last_bias=None, deep_from=1):
    """[(W (K,N) float32, b (N,) float32, relu)] of a chain, in the reference's row order -- ONE draw per (K, widths, tag): cases that
    share a width set share their layers (and the GPU test packs them once).  Layers from index deep_from on take deep_weights."""
    key = (K, tuple(widths), relu_last, tag, last_bias, deep_from)
    hit = _LAYERS.get(key)
    if hit is None:
        rng = _rng("layers", K, tuple(widths), tag)
        hit, k = [], K
        for i, n in enumerate(widths):
            W = deep_weights(rng, k, n) if i >= deep_from else (rng.normal(0, 1, (k, n)) / np.sqrt(k)).astype(np.float32)
            b = (0.1 * rng.normal(0, 1, n)).astype(np.float32)
            last = i == len(widths) - 1
            if last and last_bias is not None:
                b = np.full(n, last_bias, np.float32)
            hit.append((W, b, relu_last or not last))
            k = n
        _LAYERS[key] = hit
    return hit


def mlp_inputs(case, storage, job=0):
    """dict: sources, layers, and (two-stage) before, after, layers2 -- numpy, reference order"""
    rng = _rng("mlp", case.name, job)
    tag = "job%d" % job
    out = {"sources": [features(rng, (case.rows, w), storage) for w in case.srcs],
           "layers": make_layers(sum(case.srcs), case.layers, case.relu_last or bool(case.stage2), tag)}
    if case.stage2:
        wb, wa, l2 = case.stage2
        out["before"] = features(rng, (case.rows, wb), storage) if wb else None
        out["after"] = features(rng, (case.rows, wa), storage) if wa else None
        out["layers2"] = make_layers(wb + case.layers[-1] + wa, l2, case.relu_last, tag + "s2")
    return out


def masks_and_slots(rng, B, n, K, H2, W2):
    """Pre-grouped slots: idx (B,n,K,3) int32, mask (B,n,K) float32 with, per batch element, point 0 all clear, point 1 one live
    slot (not the first where K > 1), point 2 all set and the rest random 0/1; clear slots point at cell (0, 0, 0) of batch 0."""
    mask = (rng.random((B, n, K)) < 0.6).astype(np.float32)
    for b in range(B):                                   # (the three points move with b: they meet different rows of a tile)
        if n >= 3:
            mask[b, b % n] = 0
            mask[b, (b + 1) % n] = 0
            mask[b, (b + 1) % n, K // 2] = 1
            mask[b, (b + 2) % n] = 1
        else:
            mask[b] = 1                                  # (a one-point case: all set)
    h, w = rng.integers(0, H2, (B, n, K)), rng.integers(0, W2, (B, n, K))
    idx = np.stack([np.broadcast_to(np.arange(B)[:, None, None], (B, n, K)), h, w], -1).astype(np.int32)
    idx[mask == 0] = 0
    return idx, mask


def setconv_inputs(case, storage, job=0):
    """dict of numpy inputs: src_xyz, src_feat, layers, and idx / mask / centre (pre-grouped) or the grouping's tensors"""
    rng = _rng("setconv", case.name, job)
    H2, W2 = GRID
    B, n, K, C = case.B, case.n, case.K, case.C
    out = {"layers": make_layers(3 + C, case.layers, case.relu_last, "sc%d" % job)}
    if case.group:
        kh, kw, dist, sh, sw = case.group
        H, W = H2 * sh - (sh - 1), W2 * sw - (sw - 1)     # the smallest centres' grid whose strided pixels cover the queried one
        grid = rng.normal(0, 1.5, (B, H, W, 3)).astype(np.float32)
        grid[:, 0, 0] = (0.5, -0.25, 1.0)
        grid[:, H - 1, W - 1] = 0.0                       # an invalid centre (all-zero xyz): no neighbours, every slot clear
        out["xyz1_grid"] = grid
        out["src_xyz"] = np.ascontiguousarray(grid[:, ::sh, ::sw]) if (sh, sw) != (1, 1) else grid
        assert out["src_xyz"].shape[1:3] == (H2, W2)
        out["order"] = rng.permutation(kh * kw).astype(np.int32)
        if case.centre == "hw":
            hw = np.stack([rng.integers(0, H, (B, n)), rng.integers(0, W, (B, n))], -1).astype(np.int32)
            hw[:, 0] = (H - 1, W - 1)
            out["centre_hw"] = hw
        else:
            assert n == H * W
    else:
        out["src_xyz"] = rng.normal(0, 5, (B, H2, W2, 3)).astype(np.float32)
        out["idx"], out["mask"] = masks_and_slots(rng, B, n, K, H2, W2)
        if case.centre == "hw":
            H, W = 5, 9
            out["xyz1_grid"] = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
            out["centre_hw"] = np.stack([rng.integers(0, H, (B, n)), rng.integers(0, W, (B, n))], -1).astype(np.int32)
        else:
            out["centre_xyz"] = rng.normal(0, 5, (B, n, 3)).astype(np.float32)
    out["src_feat"] = features(rng, (B, H2, W2, C), storage)
    assert np.abs(out["src_xyz"][0, 0, 0]).min() > 0 and (C == 0 or np.abs(out["src_feat"][0, 0, 0]).min() > 0)   # what a clear slot would gather
    return out


def setconv_centres(inp):
    """(B,n,3) centres of a case's inputs (the statement's `centre`; new_xyz where centre_hw is given)"""
    if "centre_xyz" in inp:
        return inp["centre_xyz"]
    g = inp["xyz1_grid"]
    B, H, W, _ = g.shape
    if "centre_hw" in inp:
        hw = inp["centre_hw"]
        return g[np.arange(B)[:, None], hw[..., 0], hw[..., 1]]
    return g.reshape(B, H * W, 3)


CV1_WIDTHS = {"cv0": 128, "cv1": 64, "cv2": 64, "cv_xyz": 64, "sum_cv0": 128, "sum_cv1": 64}
CV2_WIDTHS = {"xyz_enc": 64, "sum_cost0": 128, "sum_cost1": 64}
FAR_BIAS = -3e10


def cv_layers(stage, C, far):
    """dict name -> (W, b, relu) in the reference's row orders.  The logits layer has no ReLU in a `far` case (its bias is -3e10)."""
    if stage == 1:
        ins = {"cv0": 10 + 2 * C, "cv1": 128, "cv2": 64, "cv_xyz": 10, "sum_cv0": 128, "sum_cv1": 128}
        widths, last = CV1_WIDTHS, "sum_cv1"
    else:
        ins = {"xyz_enc": 10, "sum_cost0": 128 + C, "sum_cost1": 128}
        widths, last = CV2_WIDTHS, "sum_cost1"
    deep = ("cv1", "cv2", "sum_cv0", "sum_cv1", "sum_cost1")          # the layers another layer feeds (sum_cost0 reads two gathers)
    return {name: make_layers(ins[name], (widths[name],), not (far and name == last), "cv%d%s" % (stage, name),
                              FAR_BIAS if far and name == last else None, 0 if name in deep else 1)[0] for name in widths}


def cv_inputs(case, storage):
    rng = _rng("cv", case.name)
    H, W = GRID
    B, K, n, C = case.B, case.K, H * W, cv_channels(case, storage)
    idx, mask = masks_and_slots(rng, B, n, K, H, W)
    out = {"idx": idx, "mask": mask, "layers": cv_layers(case.stage, C, case.far), "C": C}
    if case.stage == 1:
        out["xyz1"] = rng.normal(0, 5, (B, n, 3)).astype(np.float32)
        out["feat1"] = features(rng, (B, n, C), storage)
        out["xyz2"] = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
        out["feat2"] = features(rng, (B, H, W, C), storage)
        first = (out["xyz2"], out["feat2"])
    else:
        out["xyz1"] = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
        out["feat1"] = features(rng, (B, H, W, C), storage)
        out["cost"] = features(rng, (B, H, W, 64), storage)
        first = (out["xyz1"], out["cost"])
    assert all(np.abs(a[0, 0, 0]).min() > 0 for a in first)
    return out


# ---------------------------------------------------------------------------- Part D: refusals (host only)
# what: the argument block's deviation from a healthy one (applied by the CPU test's builders); status: the elo_status; message:
# a fragment of elo_last_error()
Refusal = namedtuple("Refusal", "name op what status message")
ERR_ARG, ERR_LIMIT = -1, -2
REFUSALS = [
    Refusal("mlp_lds_32", "mlp", dict(srcs=(200, 200, 104), layers=(16,), rows=95, tile=32), ERR_LIMIT, "bytes of LDS"),
    Refusal("mlp_lds_16", "mlp", dict(srcs=(400, 400, 208), layers=(16,), rows=95, tile=16), ERR_LIMIT, "bytes of LDS"),
    Refusal("mlp_lds_pair", "mlp", dict(srcs=(200, 200, 104), layers=(16,), rows=95, tile=32, pair=True), ERR_LIMIT, "bytes of LDS"),
    Refusal("setconv_lds_pregrouped", "setconv", dict(C=501, K=8, layers=(16,), tile=32), ERR_LIMIT, "bytes of LDS"),
    Refusal("setconv_lds_pregrouped_pair", "setconv", dict(C=501, K=8, layers=(16,), tile=32, pair=True), ERR_LIMIT, "bytes of LDS"),
    Refusal("setconv_K33", "setconv", dict(C=8, K=33, layers=(16,), tile=32), ERR_LIMIT, "exceeds the 32-row tile"),
    Refusal("cv1_K33", "cv1", dict(C=8, K=33), ERR_LIMIT, "exceeds the 32-row tile"),
    Refusal("cv2_K33", "cv2", dict(C=8, K=33), ERR_LIMIT, "exceeds the 32-row tile"),
    Refusal("mlp_width_129", "mlp", dict(srcs=(8,), layers=(129,), rows=17, tile=32), ERR_LIMIT, "outside 1..128"),
    Refusal("setconv_width_129", "setconv", dict(C=8, K=8, layers=(16, 129), tile=32), ERR_LIMIT, "outside 1..128"),
    Refusal("mlp_mixed_products", "mlp", dict(srcs=(8,), layers=(16, 16), rows=17, tile=32, mixed=True), ERR_ARG, "share one products mode"),
    Refusal("mlp_pair_mixed_products", "mlp", dict(srcs=(8,), layers=(16,), rows=17, tile=32, pair=True, mixed=True), ERR_ARG, "share one products mode"),
    Refusal("setconv_mixed_products", "setconv", dict(C=8, K=8, layers=(16, 16), tile=32, mixed=True), ERR_ARG, "share one products mode"),
    Refusal("cv1_mixed_products", "cv1", dict(C=8, K=8, mixed=True), ERR_ARG, "share one products mode"),
    Refusal("mlp_stage2_behind_N50", "mlp", dict(srcs=(8,), layers=(50,), rows=17, tile=32, stage2=(0, 0, (16,))), ERR_ARG, "multiple of 4"),
    Refusal("cv1_f16_C12", "cv1", dict(C=12, K=8, f16=True), ERR_LIMIT, "multiple of 8"),
    Refusal("cv2_f16_C12", "cv2", dict(C=12, K=8, f16=True), ERR_LIMIT, "multiple of 8"),
    Refusal("cv1_C6", "cv1", dict(C=6, K=8), ERR_LIMIT, "multiple of 4"),
    Refusal("cv2_C72", "cv2", dict(C=72, K=8), ERR_LIMIT, "exceeds 64"),
]
# the widest concatenations the LDS limit still takes (include/elo.h "The LDS limit"): (srcs, tile) that must NOT be refused
WIDEST = [((200, 200, 96), 32), ((400, 400, 192), 16)]

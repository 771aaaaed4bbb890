"""TEST INFRASTRUCTURE of the chain-shape tests: ONE table of cases for the register-resident chain kernels of csrc/elo_fused.hip
(cv1_rr_kernel, cv2_rr_kernel, setconv_rr_kernel, mlp2_rr_kernel and cv1_setconv_rr_kernel, which runs two of them in one grid) -- the
kernels the library launches by default -- and the seeded numpy inputs of a case.  The generators, the float64 statements and the
bounds are those of the tile kernels' table (tests/fused_shapes_cases.py, fused_shapes_reference.py, fused_shapes_bounds.py).

A case is tiny (at most 17 workgroups of 128 rows).  It runs in fp32 and in fp16 storage, with split and with half products, under
CHAIN_TUNING, which sends any number of rows to the chain form.  tests/test_chain_shapes_cpu.py proves from the table itself that it
covers what the kernels can do differently (every chunking of the K rows of a point, dead rows, rows of a point across two waves,
both pools of the kernels that have two, the workgroup counts xcd_tile treats differently, windows below K, above a wave and at
the 512-slot limit); tests/test_chain_shapes_gpu.py runs it.  No GPU is touched here."""
from collections import namedtuple

import numpy as np

import fused_shapes_cases as table
from fused_shapes_cases import PRODUCTS, STORAGES, features, make_layers, masks_and_slots

ROWS = 128                                               # rows of a chain workgroup (RR_ROWS): P = ROWS // K points
CHAIN_TUNING = dict(chain_forms=1, setconv_chain_rows=0, mlp_chain_rows=0)
TILE_TUNING = dict(chain_forms=0, setconv_chain_rows=0, mlp_chain_rows=0)          # the tile twin of the same call
CV_CHANNELS = (16, 32, 64)
CV_K = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 20, 31, 32)

# Part A: cost-volume stage 1 / stage 2, pre-grouped.  n: centre points per batch element (stage 2: every pixel of `grid`, stage 1:
# any count); grid: the queried (H, W); relu_last: ReLU on the logits layer; far: the logits lie at -3e10 (no ReLU, see CvCase.far);
# draw: part of the seed -- what to change where a case's draw cannot show a dropped lo product (tests/test_chain_shapes_cpu.py)
CvCase = namedtuple("ChainCvCase", "name stage B n K C grid relu_last far draw")
CV = [
    CvCase("d01", 1, 1, 21, 6, 64, (3, 7), True, False, 0),       # P points, one workgroup, the K == 6 branch
    CvCase("d02", 1, 3, 24, 5, 16, (4, 5), True, False, 0),       # P - 1 per element: 3 workgroups, batch seams inside them
    CvCase("d03", 1, 1, 129, 1, 32, (3, 7), True, False, 0),      # P + 1: one point in the last workgroup
    CvCase("d04", 1, 1, 1, 31, 16, (2, 3), True, False, 0),       # one point; 4 dead rows behind 4 x 31
    CvCase("d05", 1, 3, 33, 9, 64, (3, 7), True, False, 0),       # 99 points at P = 14: 8 workgroups, one point in the last
    CvCase("d06", 1, 1, 70, 12, 32, (5, 5), True, False, 0),      # 7 workgroups
    CvCase("d07", 1, 1, 51, 20, 64, (3, 7), True, False, 0),      # 9 = 8 + 1 workgroups
    CvCase("d08", 1, 3, 225, 3, 16, (6, 9), True, False, 0),      # 17 = 2 * 8 + 1 workgroups
    CvCase("d09", 1, 1, 17, 8, 32, (3, 7), False, True, 0),       # far logits
    CvCase("e01", 2, 1, 32, 4, 16, (4, 8), True, False, 0),       # the in-wave pool of K == 4, P points
    CvCase("e02", 2, 3, 21, 4, 64, (3, 7), False, False, 0),      # K == 4 WITHOUT the ReLU, ordinary logits: the LDS pool
    CvCase("e03", 2, 1, 63, 2, 32, (7, 9), True, False, 0),       # P - 1
    CvCase("e04", 2, 1, 19, 7, 16, (1, 19), True, False, 0),      # P + 1
    CvCase("e05", 2, 3, 7, 16, 64, (1, 7), True, False, 0),       # 3 workgroups, batch seams inside them
    CvCase("e06", 2, 1, 33, 32, 32, (3, 11), True, False, 0),     # 9 workgroups, one point in the last
    CvCase("e07", 2, 1, 20, 6, 32, (4, 5), True, False, 0),       # the K == 6 branch, P - 1 (a ONE-pixel stage 2 pools one cell: no product in it)
    CvCase("e08", 2, 3, 5, 8, 16, (5, 1), False, True, 0),        # far logits, P - 1
    CvCase("e09", 2, 1, 28, 31, 64, (4, 7), True, False, 0),      # 7 workgroups
    CvCase("e10", 2, 1, 200, 5, 64, (10, 20), True, False, 0),    # 8 workgroups
    CvCase("e11", 2, 3, 55, 12, 32, (5, 11), True, False, 0),     # 17 workgroups
]

# Part B: set-conv with in-kernel random-k (C = 64).  centre: "hw" (a centre_hw list of n entries, new_xyz written) or "pixel" (every
# pixel of the centres' grid); grid: the queried (H2, W2); group: (kernel_h, kernel_w, distance, stride_h, stride_w)
SetconvCase = namedtuple("ChainSetconvCase", "name B n K layers centre grid group pair relu_last draw")
S1, S2, S3 = (128, 64), (64, 64, 128), (128, 64, 64)
SETCONV = [
    SetconvCase("f01", 1, 15, 8, S1, "pixel", (3, 5), (3, 5, 3.2, 1, 1), False, True, 0),     # P - 1; a radius that leaves windows short
    SetconvCase("f02", 3, 24, 16, S1, "hw", (4, 6), (5, 7, 3.2, 2, 2), True, False, 0),       # 9 workgroups
    SetconvCase("f03", 1, 4, 32, S1, "hw", (3, 7), (3, 5, 1e3, 1, 2), False, True, 0),        # P; 15 window slots below K = 32: zero fill
    SetconvCase("f04", 1, 17, 8, S2, "hw", (6, 10), (9, 9, 3.2, 1, 1), True, False, 0),       # P + 1; 81 slots: two wave steps
    SetconvCase("f05", 1, 9, 16, S2, "pixel", (2, 2), (3, 3, 1e3, 2, 2), False, True, 0),     # P + 1; 9 slots below K = 16
    SetconvCase("f06", 3, 11, 32, S2, "hw", (4, 32), (16, 32, 3.2, 1, 1), False, True, 0),    # 9 workgroups; exactly 512 slots
    SetconvCase("f07", 3, 5, 8, S3, "hw", (3, 7), (3, 5, 3.2, 1, 2), False, True, 0),         # P - 1, batch seams inside the workgroup
    SetconvCase("f08", 1, 9, 16, S3, "hw", (4, 6), (5, 7, 4.5, 1, 1), False, True, 0),        # P + 1; live slots in both halves of a point's 16 rows
    SetconvCase("f09", 1, 5, 32, S3, "hw", (3, 4), (5, 5, 3.2, 2, 2), True, False, 0),        # P + 1
    SetconvCase("f10", 3, 43, 8, S1, "hw", (3, 7), (3, 5, 3.2, 1, 1), False, False, 0),       # 129 points: 9 workgroups, one point in the last
]

# Part C: the two-stage MLP on the model's widths: [64 | C] -> 128 -> 64 = out, [C before | out | 64 after] -> 128 -> 64 = out2.
# relu_last: (ReLU on the last layer of stage 1, of stage 2); clear: the pair carries the clear_* side job
MlpCase = namedtuple("ChainMlpCase", "name C rows pair relu_last clear")
MLP = [
    MlpCase("g01", 16, 1, False, (True, True), False),
    MlpCase("g02", 32, 15, True, (True, False), False),
    MlpCase("g03", 64, 16, False, (False, True), False),
    MlpCase("g04", 16, 17, True, (False, False), False),
    MlpCase("g05", 32, 127, False, (True, True), False),
    MlpCase("g06", 64, 128, True, (True, True), True),
    MlpCase("g07", 16, 129, False, (True, False), False),
    MlpCase("g08", 32, 1025, True, (False, True), False),
]

# Part D: the heterogeneous launch: a pre-grouped stage 1 and two set-conv jobs of shape (128, 64) in one grid of n_cv + 2 n_sc workgroups
PairCase = namedtuple("ChainPairCase", "name cv sc")
PAIR = [
    PairCase("h01", CvCase("h01cv", 1, 1, 21, 6, 16, (3, 7), True, False, 0),
             SetconvCase("h01sc", 1, 16, 8, S1, "hw", (3, 7), (3, 5, 3.2, 1, 1), True, True, 0)),                  # (1, 1)
    PairCase("h02", CvCase("h02cv", 1, 3, 17, 5, 32, (4, 5), True, False, 0),
             SetconvCase("h02sc", 3, 13, 16, S1, "hw", (4, 6), (5, 7, 3.2, 2, 2), True, False, 0)),                # (3, 5)
    PairCase("h03", CvCase("h03cv", 1, 1, 33, 32, 64, (3, 7), True, False, 0),
             SetconvCase("h03sc", 1, 32, 32, S1, "hw", (3, 7), (3, 5, 1e3, 1, 2), True, True, 0)),                 # (9, 8)
]

CASES = {"cv": CV, "setconv": SETCONV, "mlp": MLP, "pair": PAIR}


def runs(part):
    """(case, storage, products) of every run of a part"""
    return [(c, s, p) for c in CASES[part] for s in STORAGES for p in PRODUCTS]


def run_id(run):
    return "%s-%s-%s" % (run[0].name, run[1], run[2])


# ---------------------------------------------------------------------------- what a case exercises (read by the CPU test)
def points_of(case):
    return case.B * case.n


def per_workgroup(K):
    return ROWS // K


def workgroups(case):
    """workgroups of a grouped case (per job), or of an MLP case's rows"""
    if isinstance(case, MlpCase):
        return -(-case.rows // ROWS)
    return -(-points_of(case) // per_workgroup(case.K))


def chunks(K):
    """(8-slot chunks of the generic pooling loop, slots of the last one)"""
    return -(-K // 8), K - (-(-K // 8) - 1) * 8


def cv_pool(case):
    """the pooling a cost-volume chain kernel takes"""
    if case.stage == 2 and case.K == 4 and case.relu_last:
        return "inwave4"
    return "k6" if case.K == 6 else "chunks"


def setconv_pool(case):
    return "inwave" if case.K in (8, 16) and case.relu_last else "lds"


def centres_grid(case):
    """(H, W) of a set-conv case's centres: the smallest grid whose strided pixels cover the queried one"""
    (H2, W2), (_kh, _kw, _d, sh, sw) = case.grid, case.group
    return H2 * sh - (sh - 1), W2 * sw - (sw - 1)


# ---------------------------------------------------------------------------- seeded inputs
_NO_RELU = {}


def cv_layers(case):
    """table.cv_layers; a case without the ReLU on its logits layer and with ordinary logits takes the same layer with the flag down
    (its own copy of the weights: the GPU test's packing cache keys on the array)"""
    L = table.cv_layers(case.stage, case.C, case.far)
    if case.far or case.relu_last:
        return L
    last = "sum_cv1" if case.stage == 1 else "sum_cost1"
    hit = _NO_RELU.get((case.stage, case.C))
    if hit is None:
        W, b, _relu = L[last]
        hit = _NO_RELU[(case.stage, case.C)] = (W.copy(), b.copy(), False)
    return dict(L, **{last: hit})


def cv_inputs(case, storage):
    rng = table._rng("chain-cv", case.name, case.draw)
    H, W = case.grid
    B, K, n, C = case.B, case.K, case.n, case.C
    idx, mask = masks_and_slots(rng, B, n, K, H, W)
    out = {"idx": idx, "mask": mask, "layers": cv_layers(case), "C": C}
    if case.stage == 1:
        out["xyz1"] = rng.normal(0, 5, (B, n, 3)).astype(np.float32)
        out["feat1"] = features(rng, (B, n, C), storage)
        out["xyz2"] = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
        out["feat2"] = features(rng, (B, H, W, C), storage)
        first = (out["xyz2"], out["feat2"])
    else:
        assert n == H * W
        out["xyz1"] = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
        out["feat1"] = features(rng, (B, H, W, C), storage)
        out["cost"] = features(rng, (B, H, W, 64), storage)
        first = (out["xyz1"], out["cost"])
    assert all(np.abs(a[0, 0, 0]).min() > 0 for a in first)               # what a clear slot gathers
    return out


FAR_CENTRE = (40.0, -40.0, 40.0)


def setconv_inputs(case, storage, job=0):
    """dict of numpy inputs of an in-kernel-grouping case.  The centres' grid holds an all-zero (invalid) centre in its last pixel
    and, at (0, W - 1), a centre some 70 away from every queried point (non-zero, finds no neighbour within a finite radius); a
    centre_hw list holds both, and repeats its third entry."""
    rng = table._rng("chain-setconv", case.name, job, case.draw)
    H2, W2 = case.grid
    _kh, _kw, _dist, sh, sw = case.group
    H, W = centres_grid(case)
    assert H >= 2 and W >= 2
    B, n = case.B, case.n
    grid = rng.normal(0, 1.5, (B, H, W, 3)).astype(np.float32)
    grid[:, 0, 0] = (0.5, -0.25, 1.0)
    grid[:, H - 1, W - 1] = 0.0
    src = np.ascontiguousarray(grid[:, ::sh, ::sw])
    assert src.shape[1:3] == (H2, W2)
    grid[:, 0, W - 1] = FAR_CENTRE
    out = {"layers": make_layers(3 + 64, case.layers, case.relu_last, "chain-sc%d" % job), "xyz1_grid": grid, "src_xyz": src,
           "order": rng.permutation(case.group[0] * case.group[1]).astype(np.int32)}
    if case.centre == "hw":
        hw = np.stack([rng.integers(0, H, (B, n)), rng.integers(0, W, (B, n))], -1).astype(np.int32)
        hw[:, 0] = (H - 1, W - 1)
        hw[:, 1] = (0, W - 1)
        hw[:, 3] = hw[:, 2]
        out["centre_hw"] = hw
    else:
        assert n == H * W
    out["src_feat"] = features(rng, (B, H2, W2, 64), storage)
    assert np.abs(src[0, 0, 0]).min() > 0 and np.abs(out["src_feat"][0, 0, 0]).min() > 0
    return out


setconv_centres = table.setconv_centres


def mlp_inputs(case, storage, job=0):
    """dict: sources, layers, before, after, layers2 -- numpy, reference order"""
    rng = table._rng("chain-mlp", case.name, job)
    C, rows, tag = case.C, case.rows, "chain-job%d" % job
    return {"sources": [features(rng, (rows, 64), storage), features(rng, (rows, C), storage)],
            "layers": make_layers(64 + C, (128, 64), case.relu_last[0], tag),
            "before": features(rng, (rows, C), storage), "after": features(rng, (rows, 64), storage),
            "layers2": make_layers(C + 64 + 64, (128, 64), case.relu_last[1], tag + "s2")}

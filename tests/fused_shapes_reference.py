"""TEST INFRASTRUCTURE of the fused-shape tests: plain numpy float64 statements of what elo_setconv_args, elo_mlp_args (one and two
stages), elo_cv1_args and elo_cv2_args ask for (include/elo.h "Fused inference kernels"; utils/pointnet_util.py:33-149, 153-175,
179-316), on explicit layers and pre-grouped idx / mask.

A layer is (W (K,N), b (N), relu) with W's rows in the REFERENCE's concat order ([xyz difference | features] for a set-conv,
[geometry | feat1 | feat2] for CV_0, [before | out | after] for the second stage of a row-wise MLP, ...): the kernels' own column
orders (fused.setconv_row_order, fused.cv0_row_order, fused.stage2_row_order) stay on the product side.

half=True states ELO_PRODUCTS_HALF: every operand of a product -- the layer's input and its weights -- is rounded to the nearest fp16
first (as tests/test_ops_gpu.py's half-products test does for one layer); bias, accumulation, ReLU and the poolings are exact here.
The values of a softmax pool are operands of the tile too (the kernel reads them from a layer's input region), so they are rounded
as well.

Every function returns a dict: "out" and the intermediates tests/fused_shapes_bounds.py carries its error bound through."""
import numpy as np

D = np.float64
MASKED_LOGIT = D(np.float32(-1e10))


def r16(x):
    """round to the nearest fp16 value (ties to even), as a float64 array"""
    return np.asarray(x, D).astype(np.float16).astype(D)


def dense(x, layer, half):
    """(x @ W + b, relu applied): the layer's output, and the operands as the products saw them"""
    W, b, relu = layer
    W, b = np.asarray(W, D), np.asarray(b, D)
    xo, Wo = (r16(x), r16(W)) if half else (np.asarray(x, D), W)
    y = xo @ Wo + b
    return (np.maximum(y, 0.0) if relu else y), xo, Wo


def chain(x, layers, half):
    """x through the layers; returns (output, [(operand input, operand W, b, relu) per layer])"""
    steps = []
    for layer in layers:
        y, xo, Wo = dense(x, layer, half)
        steps.append((xo, Wo, np.asarray(layer[1], D), bool(layer[2])))
        x = y
    return x, steps


def gather(grid, idx):
    """tf.gather_nd with (..., 3) (b, h, w) indices into a (B, H, W, C) tensor"""
    return np.asarray(grid, D)[idx[..., 0], idx[..., 1], idx[..., 2]]


def mlp(sources, layers, half=False):
    """elo_mlp_args, first stage: layers(concat(sources, -1)) on (rows, width) sources."""
    x = np.concatenate([np.asarray(s, D) for s in sources], -1)
    out, steps = chain(x, layers, half)
    return {"out": out, "input": x, "steps": steps}


def mlp_stage2(first_out, before, after, layers2, half=False):
    """elo_mlp_args, second stage: layers2(concat([before, first stage's output, after], -1)) -- the reference's order."""
    parts = ([np.asarray(before, D)] if before is not None else []) + [np.asarray(first_out, D)] + \
            ([np.asarray(after, D)] if after is not None else [])
    x = np.concatenate(parts, -1)
    out, steps = chain(x, layers2, half)
    return {"out": out, "input": x, "steps": steps}


def setconv(centre, src_xyz, src_feat, idx, mask, layers, half=False):
    """elo_setconv_args: concat([xyz[idx] * m - centre, feat[idx] * m]) -> layers -> * m -> max over K.
    centre (B,n,3), src_xyz (B,H2,W2,3), src_feat (B,H2,W2,C), idx (B,n,K,3), mask (B,n,K)."""
    m = np.asarray(mask, D)[..., None]
    diff = gather(src_xyz, idx) * m - np.asarray(centre, D)[:, :, None, :]
    x = np.concatenate([diff, gather(src_feat, idx) * m], -1)
    y, steps = chain(x, layers, half)
    return {"out": (y * m).max(axis=2), "input": x, "steps": steps, "rows": y, "diff": diff}


def geometry(p, g, m):
    """[p, g*m, g*m - p, |g*m - p|]: the 10 geometry columns of both cost-volume stages (p (B,n,3), g (B,n,K,3), m (B,n,K,1))"""
    pk = np.broadcast_to(np.asarray(p, D)[:, :, None, :], g.shape)
    gm = g * m
    diff = gm - pk
    euc = np.sqrt((diff * diff).sum(-1, keepdims=True) + D(np.float32(1e-20)))
    return np.concatenate([pk, gm, diff, euc], -1)


def softmax_pool(logits, values, mask):
    """sum_k softmax_k(mask == 1 ? logit : -1e10) * value: (B,n,K,64) x (B,n,K,64) x (B,n,K) -> out, weights, shifted logits"""
    l = np.where(np.asarray(mask)[..., None] == 1.0, logits, MASKED_LOGIT)
    x = l - l.max(axis=2, keepdims=True)
    e = np.exp(x)
    w = e / e.sum(axis=2, keepdims=True)
    return (w * values).sum(axis=2), w, x


def cv_stage1(xyz1, feat1, xyz2, feat2, idx, mask, layers, half=False):
    """elo_cv1_args.  layers: dict cv0, cv1, cv2, cv_xyz, sum_cv0, sum_cv1; CV_0 takes [geometry (10) | feat1 | feat2 grouped],
    sum_CV_0 takes [xyz encoding (64) | x (64)].  xyz1 (B,n,3), feat1 (B,n,C), xyz2 (B,H2,W2,3), feat2 (B,H2,W2,C)."""
    m = np.asarray(mask, D)[..., None]
    geo = geometry(xyz1, gather(xyz2, idx), m)
    f1 = np.broadcast_to(np.asarray(feat1, D)[:, :, None, :], idx.shape[:3] + (feat1.shape[-1],))
    cat = np.concatenate([geo, f1, gather(feat2, idx) * m], -1)
    x, steps_x = chain(cat, [layers["cv0"], layers["cv1"], layers["cv2"]], half)
    enc, steps_e = chain(geo, [layers["cv_xyz"]], half)
    both = np.concatenate([enc, x], -1)
    logits, steps_l = chain(both, [layers["sum_cv0"], layers["sum_cv1"]], half)
    values = r16(x) if half else x
    out, w, shifted = softmax_pool(logits, values, mask)
    return {"out": out, "geo": geo, "cat": cat, "steps_x": steps_x, "steps_e": steps_e, "steps_l": steps_l, "x": x, "enc": enc,
            "logits": logits, "values": values, "w": w, "shifted": shifted}


def cv_stage2(xyz1, feat1, cost, idx, mask, layers, half=False):
    """elo_cv2_args.  layers: dict xyz_enc, sum_cost0, sum_cost1; sum_cost_volume_0 takes [xyz encoding (64) | feat1 (C) |
    cost grouped (64)].  xyz1 (B,H,W,3), feat1 (B,H,W,C), cost (B,H,W,64); every pixel is a centre."""
    B, H, W, C = feat1.shape
    m = np.asarray(mask, D)[..., None]
    geo = geometry(np.asarray(xyz1, D).reshape(B, H * W, 3), gather(xyz1, idx), m)
    enc, steps_e = chain(geo, [layers["xyz_enc"]], half)
    f1 = np.broadcast_to(np.asarray(feat1, D).reshape(B, H * W, 1, C), idx.shape[:3] + (C,))
    grouped = gather(cost, idx) * m
    both = np.concatenate([enc, f1, grouped], -1)
    logits, steps_l = chain(both, [layers["sum_cost0"], layers["sum_cost1"]], half)
    values = r16(grouped) if half else grouped
    out, w, shifted = softmax_pool(logits, values, mask)
    return {"out": out, "geo": geo, "steps_e": steps_e, "steps_l": steps_l, "enc": enc, "both": both, "logits": logits,
            "values": values, "w": w, "shifted": shifted}

"""TEST INFRASTRUCTURE of the per-form kernel tests (tests/test_backward_forms_gpu.py, tests/test_forward_forms_gpu.py,
tests/test_forward_forms_cpu.py): numpy input generators with the edges where the feature kernels go wrong built in at FIXED
places, and tensors placed a few bytes off their buffer's alignment (the launchers pick a kernel by pointer alignment).  No GPU is
touched here: the callers move the arrays."""
import numpy as np
import torch

from conftest import expand_prefix


def at_offset(x, nbytes=4):
    """x's values in a contiguous tensor `nbytes` past a 16-byte boundary (differentiable)."""
    n, rem = divmod(nbytes, x.element_size())
    assert rem == 0 and 0 <= nbytes < 16
    if n == 0:
        return x
    y = torch.cat([x.new_zeros(n), x.reshape(-1)])[n:].view(x.shape)
    assert y.is_contiguous() and y.data_ptr() % 16 == nbytes
    return y


def counts(rng, B, N, K):
    """valid-slot counts of prefix-ones masks with the edges at fixed points: all masked, one valid slot, all valid."""
    c = rng.integers(0, K + 1, (B, N))
    c[:, 0], c[:, 1], c[:, 2] = 0, 1, K
    return c


def mask_of(cnt, K):
    return expand_prefix(cnt, K)[..., 0]                           # (B, N, K) of 0/1


def slots(rng, B, N, K, H2, W2, masked_at="origin"):
    """Synthetic neighbour slots [b, h, w] (B,N,K,3) int32 and a prefix-ones mask (B,N,K).  Half of the live slots go to 8 hot cells
    per image (their atomics pile up); a masked slot points at cell (0,0,0) as the grouping kernels leave it, or anywhere."""
    mask = mask_of(counts(rng, B, N, K), K)
    h, w = rng.integers(0, H2, (B, N, K)), rng.integers(0, W2, (B, N, K))
    hot = rng.random((B, N, K)) < 0.5
    j = rng.integers(0, 8, (B, N, K))
    hh, hw = rng.integers(0, H2, 8), rng.integers(0, W2, 8)
    h, w = np.where(hot, hh[j], h), np.where(hot, hw[j], w)
    idx = np.stack([np.broadcast_to(np.arange(B)[:, None, None], (B, N, K)), h, w], -1).astype(np.int32)
    off = mask == 0
    if masked_at == "origin":
        idx[off] = 0
    else:
        idx[off, 0] = rng.integers(0, B, int(off.sum()))
    return idx, mask.astype(np.float32)


def maxpool_inputs(rng, B, N, K, C):
    """Post-ReLU values (about half exact zeros) with ties built in, and a prefix-ones mask."""
    cnt = counts(rng, B, N, K)
    if K > 1:
        cnt[:, 3::7] = rng.integers(1, K, cnt[:, 3::7].shape)        # ... with at least one masked slot at these points:
    x = np.maximum(rng.normal(0, 1, (B, N, K, C)), 0).astype(np.float32)
    x[:, 3::7] = -np.abs(x[:, 3::7]) - 0.25                          # every valid product negative: the masked +-0 wins
    x[..., 1] = x[..., :1, 1]                                        # channel 1 equal on all K slots: a K-way (or masked) tie
    x[:, 5::9, -1] = x[:, 5::9, 0]                                   # a duplicated neighbour (flag_copy)
    return x, mask_of(cnt, K).astype(np.float32)


def softmax_pool_inputs(rng, B, N, K, C, width=None):
    """Logits with the edges: all-masked points (n = 0), a single valid slot (n = 1), masked logits above every valid one, and (every
    other point) logits spread over ~+-120 so that some exponentials underflow to 0.  Values `width` channels wide (the op reads C of
    them)."""
    cnt = counts(rng, B, N, K)
    m = mask_of(cnt, K)
    lg = rng.normal(0, 1, (B, N, K, C))
    lg[:, 1::2] *= 40.0
    lg = np.where((m[..., None] == 0) & (rng.random((B, N, 1, 1)) < 0.5), 1e3, lg)
    v = rng.normal(0, 1, (B, N, K, width or C))
    return lg.astype(np.float32), v.astype(np.float32), m.astype(np.float32)


def pool_forward_inputs(rng, B, N, K, C, width=None, f16=False):
    """softmax_pool_inputs for the forward tests, with one more edge in fp32: the valid logits of point 2 of batch element 0 (every slot
    valid) all lie BELOW the -1e10 that stands for a masked slot -- only a true -inf may stand for a slot that does not exist.  fp16
    storage cannot hold such a logit; there the logits and values are rounded to fp16-representable numbers instead."""
    lg, v, m = softmax_pool_inputs(rng, B, N, K, C, width)
    if f16:
        return as_half_values(lg), as_half_values(v), m
    assert m[0, 2].all()
    lg[0, 2] = -3e10
    return lg, v, m


def cv_encode1_inputs(rng, B, N, H, W, K, C, masked_at="origin"):
    """Centres anywhere (N of them), neighbours on the H x W grid; the first slot of every 5th centre sits ON the centre (d = 0: the
    norm is sqrt(1e-20) and its gradient 0 / 1e-10).  Returns xyz1, feat1, xyz2, feat2, idx, mask."""
    idx, m = slots(rng, B, N, K, H, W, masked_at)
    xyz1 = rng.normal(0, 5, (B, N, 3)).astype(np.float32)
    xyz2 = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
    for b in range(B):
        for n in range(4, N, 5):
            if m[b, n, 0] == 1:
                idx[b, n, 0] = (b, n % H, (n // H) % W)
                xyz2[b, n % H, (n // H) % W] = xyz1[b, n]
    f1 = rng.normal(0, 1, (B, N, C)).astype(np.float32)
    f2 = rng.normal(0, 1, (B, H, W, C)).astype(np.float32)
    return xyz1, f1, xyz2, f2, idx, m


def cv_encode2_inputs(rng, B, H, W, K, C, Cc=None, masked_at="origin"):
    """Centres are the grid's own pixels; the first slot of every 5th pixel is the pixel itself (d = 0).  Returns xyz, feat1, cost, idx,
    mask."""
    N = H * W
    idx, m = slots(rng, B, N, K, H, W, masked_at)
    for n in range(4, N, 5):
        live = m[:, n, 0] == 1
        idx[live, n, 0] = np.stack([np.arange(B), np.full(B, n // W), np.full(B, n % W)], -1)[live]
    xyz = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
    f1 = rng.normal(0, 1, (B, H, W, C)).astype(np.float32)
    cost = rng.normal(0, 1, (B, H, W, C if Cc is None else Cc)).astype(np.float32)
    return xyz, f1, cost, idx, m


def as_half_values(a):
    """a (float32) rounded to the nearest fp16-representable value, still float32: what fp16 storage can hold exactly."""
    return a.astype(np.float16).astype(np.float32)

"""fused_conv_random_k / fused_conv_select_k with the reference's signatures.

Drop-in for tf_ops/2d_conv_random_k/fused_conv_random_k.py:14-29 and
tf_ops/2d_conv_select_k/fused_conv_select_k.py:14-29: same positional /
keyword arguments, same four outputs (dtype, shape, order).  Tensors are torch
tensors on the GPU; the work is done by hand-written HIP kernels behind the C
ABI of include/elo.h (csrc/elo_grouping.hip).  The attribute and shape checks
of the TF op (fused_conv.cpp:78-123) are kept, plus the ones it forgot.

`random_hw` stays an input (the caller owns the randomness, e.g.
torch.randperm(KT, dtype=torch.int32)), so the op is a pure function.  It is
not differentiable: indices are integers and every caller wraps the mask in
stop_gradient (utils/pointnet_util.py:54-55,110-111,203-204,277-278).
"""
import ctypes
import math

import torch

from . import _lib


def _check(name, xyz1, xyz2, idx_n2, random_hw, npoints, kernel_size_H, kernel_size_W, K, flag_copy,
           distance, stride_h, stride_w):
    # attribute checks: fused_conv.cpp:78-100
    if npoints <= 0: raise ValueError("FusedConv expects positive npoints")
    if kernel_size_H <= 0: raise ValueError("FusedConv expects positive kernel_size_H")
    if kernel_size_W <= 0: raise ValueError("FusedConv expects positive kernel_size_W")
    if K <= 0: raise ValueError("FusedConv expects positive K")
    if flag_copy not in (0, 1): raise ValueError("FusedConv expects 0 OR 1 flag_copy")
    if not distance > 0: raise ValueError("FusedConv expects positive distance")
    if stride_h <= 0: raise ValueError("FusedConv expects positive stride_h")
    if stride_w <= 0: raise ValueError("FusedConv expects positive stride_w")
    # shape checks: fused_conv.cpp:107-123 (+ W2, channel, dtype, device, contiguity)
    _lib.require_gpu(xyz1, xyz2, idx_n2, random_hw)
    if xyz1.dim() != 4 or xyz1.shape[3] != 3:
        raise ValueError("%s expects (batch_size, H, W, 3) xyz1 shape." % name)
    B, H, W, _ = xyz1.shape
    H2, W2 = math.ceil(H / float(stride_h)), math.ceil(W / float(stride_w))
    if xyz2.dim() != 4 or tuple(xyz2.shape) != (B, H2, W2, 3):
        raise ValueError("%s expects (batch_size, H/stride_h, W/stride_w, 3) xyz2 shape." % name)
    if idx_n2.dim() != 3 or idx_n2.shape[0] != B or idx_n2.shape[1] != npoints or idx_n2.shape[2] != 2:
        raise ValueError("FusedConv expects (batch_size, npoints, 2) idx_n2 shape.")
    if random_hw.dim() != 1 or random_hw.shape[0] != kernel_size_H * kernel_size_W:
        raise ValueError("FusedConv expects (kernel_size_h * kernel_size_w) random_hw shape.")
    if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32:
        raise TypeError("xyz1/xyz2 must be float32")
    if idx_n2.dtype != torch.int32 or random_hw.dtype != torch.int32:
        raise TypeError("idx_n2/random_hw must be int32")
    if not (xyz1.device == xyz2.device == idx_n2.device == random_hw.device):
        raise ValueError("all inputs must live on the same device")
    return B, H, W, H2, W2


_DENSE_INDEX = {}        # data_ptr -> tensor: index tensors known to be "every pixel, row-major" (get_hw_idx's)


def register_dense_index(idx_n2):
    """Tell the wrappers that `idx_n2` (B, H*W, 2) lists every pixel in row-major order (pointnet_util.get_hw_idx builds
    and registers such tensors): random-k calls with it take the LDS-tiled kernel (elo_fused_conv_random_k_dense)."""
    if len(_DENSE_INDEX) >= 256:
        _DENSE_INDEX.clear()
    _DENSE_INDEX[idx_n2.data_ptr()] = idx_n2
    return idx_n2


_ALL_PIXELS = {}         # (B, H, W, device) -> the one cached "every pixel, row-major" tensor of that grid


def all_pixels(B, H, W, device):
    """(B, H*W, 2) int32, row-major (h, w) of every pixel (utils/pointnet_util.py:23-30): pointnet_util.get_hw_idx and the centre
    list of fused.group_prepass.  Cached, and registered as a dense index (random-k calls with it take the LDS-tiled kernel)."""
    key = (B, H, W, str(device))
    hit = _ALL_PIXELS.get(key)
    if hit is None:
        hh = torch.arange(H, dtype=torch.int32, device=device).view(1, H, 1, 1).expand(B, H, W, 1)
        ww = torch.arange(W, dtype=torch.int32, device=device).view(1, 1, W, 1).expand(B, H, W, 1)
        hit = torch.cat([hh, ww], -1).reshape(B, H * W, 2).contiguous()
        if hit.is_cuda and torch.cuda.is_current_stream_capturing():
            return hit                      # a tensor born inside a graph's private pool is never cached
        if len(_ALL_PIXELS) >= 256:
            _ALL_PIXELS.clear()
        _ALL_PIXELS[key] = register_dense_index(hit)
    return hit


def grouping_entry(kind, kH, kW, K, flag_copy, stride_h, stride_w, dense_ok):
    """Entry point of a grouping call (kind "random" / "select").  dense_ok is the caller's half of the choice: every pixel
    of xyz1 is a centre in row-major order (and whatever else it wants of the LDS-tiled form); whether the window fits
    that form's tile is the library's answer (include/elo.h elo_fused_conv_*_k_dense_fits)."""
    lib = _lib.lib()
    if kind == "select":
        fits = lib.elo_fused_conv_select_k_dense_fits(kH, kW, K, flag_copy, stride_h, stride_w)
    else:
        fits = lib.elo_fused_conv_random_k_dense_fits(kH, kW, K, stride_h, stride_w)
    return "elo_fused_conv_%s_k%s" % (kind, "_dense" if dense_ok and fits else "")


def grouping_form(kind, B, H, W, npoints, kernel_size_H, kernel_size_W, K, flag_copy=0, distance=1.0, stride_h=1, stride_w=1,
                  want_valid=True, dense=False):
    """The kernel form (as _lib.grouping_form_name spells it) that a "random" / "select" grouping call of these sizes takes
    through its general (dense=False) or LDS-tiled (dense=True) entry point, under the current tuning; raises _lib.EloError
    where that entry point would refuse the call.  Host only: the queries read no tensor, so the block carries placeholder
    addresses (want_valid says whether the two prefix masks are asked for, which the dense select-k form depends on)."""
    H2, W2 = -(-H // stride_h) if stride_h > 0 else 0, -(-W // stride_w) if stride_w > 0 else 0
    there = 1 << 12                                            # any non-NULL address: never read
    args = _lib.GroupArgs(B, H, W, H2, W2, npoints, kernel_size_H, kernel_size_W, K, flag_copy, float(distance), stride_h, stride_w,
                          there, there, there, there, there, there if want_valid else None, there if want_valid else None, there)
    return _lib.grouping_form("elo_fused_conv_%s_k%s_form" % (kind, "_dense" if dense else ""), args)


def _launch(kind, name, xyz1, xyz2, idx_n2, random_hw, H, W, npoints, kernel_size_H, kernel_size_W, K,
            flag_copy, distance, stride_h, stride_w, want_valid, dense=None):
    # H, W attributes are unused by the reference's Compute as well: the real
    # sizes come from the tensor (fused_conv.cpp:108-110).
    B, H, W, H2, W2 = _check(name, xyz1, xyz2, idx_n2, random_hw, npoints, kernel_size_H, kernel_size_W,
                             K, flag_copy, distance, stride_h, stride_w)
    xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
    idx_n2, random_hw = idx_n2.contiguous(), random_hw.contiguous()
    KT = kernel_size_H * kernel_size_W
    dev = xyz1.device
    if dense and npoints != H * W:
        raise ValueError("the dense form needs npoints == H*W (every pixel a centre)")
    all_pixels = npoints == H * W and (dense or (dense is None and _DENSE_INDEX.get(idx_n2.data_ptr()) is idx_n2))
    entry = grouping_entry(kind, kernel_size_H, kernel_size_W, K, flag_copy, stride_h, stride_w, all_pixels)
    if dense and not entry.endswith("_dense"):                # the caller insists on a form whose tile does not fit
        if kind == "select":
            raise ValueError("the dense select-k form takes K <= 7, flag_copy = 0 and a window of at most 512 slots")
        entry += "_dense"                                     # random-k: the launcher answers ELO_ERR_LIMIT
    sel = torch.empty((B, npoints, K, 3), dtype=torch.int32, device=dev)
    mask = torch.empty((B, npoints, K, 1), dtype=torch.float32, device=dev)
    if want_valid:
        valid = torch.empty((B, npoints, KT, 1), dtype=torch.float32, device=dev)
        indis = torch.empty((B, npoints, KT, 1), dtype=torch.float32, device=dev)
    else:
        valid = indis = None
    args = _lib.GroupArgs(B, H, W, H2, W2, npoints, kernel_size_H, kernel_size_W, K, flag_copy,
                          float(distance), stride_h, stride_w, xyz1.data_ptr(), xyz2.data_ptr(),
                          idx_n2.data_ptr(), random_hw.data_ptr(), sel.data_ptr(),
                          valid.data_ptr() if want_valid else None,
                          indis.data_ptr() if want_valid else None, mask.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), entry)(ctypes.byref(args), _lib.stream_ptr(xyz1)))
    return sel, valid, indis, mask


def fused_conv_random_k(xyz1, xyz2, idx_n2, random_hw, H, W, npoints, kernel_size_H, kernel_size_W, K,
                        flag_copy, distance, stride_h, stride_w, want_valid=True, dense=None):
    """First K in-range neighbours in the caller's visiting order.

    Returns (selected_bhw_idx i32 (B,N,K,3), valid_idx f32 (B,N,KT,1),
    valid_in_dis_idx f32 (B,N,KT,1), selected_mask f32 (B,N,K,1)).
    want_valid=False (an extension used by the model path) skips the two
    outputs no caller reads and returns None for them.
    dense (extension): True = the caller vouches that idx_n2 lists EVERY pixel in row-major order (get_hw_idx) and the
    LDS-tiled kernel is used; None = used automatically for index tensors registered with register_dense_index;
    False = always the general kernel.  Same outputs bit for bit either way.
    """
    return _launch("random", "FusedConvRandomK", xyz1, xyz2, idx_n2, random_hw, H, W,
                   npoints, kernel_size_H, kernel_size_W, K, flag_copy, distance, stride_h, stride_w,
                   want_valid, dense)


def fused_conv_select_k(xyz1, xyz2, idx_n2, random_hw, H, W, npoints, kernel_size_H, kernel_size_W, K,
                        flag_copy, distance, stride_h, stride_w, want_valid=True, dense=None):
    """K nearest in-range neighbours of the window (reference tie order).
    dense (extension, as for random-k): the LDS-tiled kernel for "every pixel a centre" with K <= 7 (the refinement cost
    volumes' call); None = automatically for registered index tensors.  Same outputs bit for bit."""
    return _launch("select", "FusedConvSelectK", xyz1, xyz2, idx_n2, random_hw, H, W,
                   npoints, kernel_size_H, kernel_size_W, K, flag_copy, distance, stride_h, stride_w,
                   want_valid, dense)

"""Thin torch-tensor front-ends of the feature kernels (include/elo.h, csrc/elo_features.hip) and of their hand-written
backward passes (csrc/elo_backward.hip).  Every public operator here is ONE implementation: the HIP kernel.  When an
input requires grad (training) the call goes through a torch.autograd.Function whose forward is that same kernel and
whose backward is the matching `elo_*_backward` kernel -- there is no second (torch) implementation to fall onto and
nothing here looks at the global autograd mode.  Shapes are validated in C as well.  No CPU fallback: CPU tensors raise."""
import collections
import ctypes
import math

import numpy as np

import torch

from . import _lib as L
from . import sensor as _sensor
from . import tuning
from .sensor import projection_constants          # (H, W, sensor=None) -> (az_res, vert_res, vert_off), python doubles


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


_ptr = lambda x: x.data_ptr() if x is not None else None


def _feature_dtype(*ts):
    """Feature tensors are stored as fp32 or fp16 (fp32 arithmetic either way): all feature tensors of a call share one
    of the two; returns (contiguous tensors, torch dtype, ELO_F32 / ELO_F16)."""
    dt = ts[0].dtype
    if dt not in (torch.float32, torch.float16) or any(t.dtype != dt for t in ts):
        raise TypeError("cost-volume feature tensors are all float32 or all float16 (got %s)" % [str(t.dtype) for t in ts])
    return [t.contiguous() for t in ts], dt, L.ELO_F16 if dt == torch.float16 else L.ELO_F32


def _f32(*ts):
    out = []
    for t in ts:
        if t.dtype != torch.float32:
            raise TypeError("feature-path tensors are float32 (got %s)" % t.dtype)
        out.append(t.contiguous())
    return out


class _GroupConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, centre_xyz, src_xyz, src_feat, idx, mask):
        ctx.save_for_backward(idx, mask)
        ctx.shapes = (centre_xyz.shape, src_xyz.shape, src_feat.shape)
        return _group_concat(centre_xyz, src_xyz, src_feat, idx, mask)

    @staticmethod
    def backward(ctx, grad):
        idx, mask = ctx.saved_tensors
        (cs, xs, fs), dev = ctx.shapes, grad.device
        (grad,) = _f32(grad)
        need = ctx.needs_input_grad
        g_c = torch.empty(cs, dtype=torch.float32, device=dev) if need[0] else None
        g_x = torch.zeros(xs, dtype=torch.float32, device=dev) if need[1] else None
        g_f = torch.zeros(fs, dtype=torch.float32, device=dev) if need[2] else None
        B, N, K, _ = idx.shape
        a = L.GroupConcatBwdArgs(B, N, K, fs[1], fs[2], fs[3], grad.data_ptr(), idx.data_ptr(), mask.data_ptr(),
                                 _ptr(g_c), _ptr(g_x), _ptr(g_f))
        L.call("elo_group_concat_backward", a, grad)
        return g_c, g_x, g_f, None, None


def group_concat(centre_xyz, src_xyz, src_feat, idx, mask):
    """[src_xyz[idx]*m - centre, src_feat[idx]*m] -> (B,N,K,3+C).  pointnet_util.py:203-213, :277-284."""
    if _wants_grad(centre_xyz, src_xyz, src_feat):
        return _GroupConcat.apply(centre_xyz, src_xyz, src_feat, idx.contiguous(), _f32(mask)[0])
    return _group_concat(centre_xyz, src_xyz, src_feat, idx, mask)


def _group_concat(centre_xyz, src_xyz, src_feat, idx, mask):
    L.require_gpu(centre_xyz, src_xyz, src_feat, idx, mask)
    centre_xyz, src_xyz, src_feat, mask = _f32(centre_xyz, src_xyz, src_feat, mask)
    idx = idx.contiguous()
    B, N, K, _ = idx.shape
    _, H2, W2, C = src_feat.shape
    out = torch.empty((B, N, K, 3 + C), dtype=torch.float32, device=idx.device)
    a = L.GroupConcatArgs(B, N, K, H2, W2, C, centre_xyz.data_ptr(), src_xyz.data_ptr(), src_feat.data_ptr(),
                          idx.data_ptr(), mask.data_ptr(), out.data_ptr())
    L.call("elo_group_concat", a, out)
    return out


class _MaskedMaxpool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(x, mask)
        return _masked_maxpool(x, mask)

    @staticmethod
    def backward(ctx, grad):
        x, mask = ctx.saved_tensors
        (grad,) = _f32(grad)
        B, N, K, C = x.shape
        g_x = torch.empty_like(x)
        L.call("elo_masked_maxpool_backward",
               L.MaskedMaxpoolBwdArgs(B, N, K, C, x.data_ptr(), mask.data_ptr(), grad.data_ptr(), g_x.data_ptr()), grad)
        return g_x, None


def masked_maxpool(x, mask):
    """max_k x*mask -> (B,N,C).  pointnet_util.py:224-230, :295-298."""
    if _wants_grad(x):
        return _MaskedMaxpool.apply(*_f32(x, mask))
    return _masked_maxpool(x, mask)


def _masked_maxpool(x, mask):
    L.require_gpu(x, mask)
    x, mask = _f32(x, mask)
    B, N, K, C = x.shape
    out = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
    L.call("elo_masked_maxpool", L.MaskedMaxpoolArgs(B, N, K, C, x.data_ptr(), mask.data_ptr(), out.data_ptr()), out)
    return out


class _CvEncode1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, feat1, xyz2_proj, feat2_proj, idx, mask):
        ctx.save_for_backward(xyz1, xyz2_proj, idx, mask)
        ctx.C = feat1.shape[-1]
        return _cv_encode1(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask)

    @staticmethod
    def backward(ctx, grad):
        xyz1, xyz2, idx, mask = ctx.saved_tensors
        (grad,) = _f32(grad)
        B, N, K, _ = idx.shape
        _, H2, W2, _ = xyz2.shape
        C, dev, need = ctx.C, grad.device, ctx.needs_input_grad
        new = lambda shape, zero: (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=dev)
        g_x1 = new((B, N, 3), False) if need[0] else None
        g_f1 = new((B, N, C), False) if need[1] else None
        g_x2 = new((B, H2, W2, 3), True) if need[2] else None
        g_f2 = new((B, H2, W2, C), True) if need[3] else None
        a = L.CvEncode1BwdArgs(B, N, K, H2, W2, C, xyz1.data_ptr(), xyz2.data_ptr(), idx.data_ptr(), mask.data_ptr(),
                               grad.data_ptr(), _ptr(g_x1), _ptr(g_f1), _ptr(g_x2), _ptr(g_f2))
        L.call("elo_cv_encode1_backward", a, grad)
        return g_x1, g_f1, g_x2, g_f2, None, None


def cv_encode1(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask):
    """(B,N,K,10+2C) = [p, q, q-p, |q-p|, feat1, feat2[idx]*m].  pointnet_util.py:54-66."""
    if _wants_grad(xyz1, feat1, xyz2_proj, feat2_proj):
        return _CvEncode1.apply(*_f32(xyz1, feat1, xyz2_proj, feat2_proj), idx.contiguous(), _f32(mask)[0])
    return _cv_encode1(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask)


def _cv_encode1_args(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask):
    """The call's argument block, its output and the (contiguous) tensors the block points into."""
    L.require_gpu(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask)
    xyz1, xyz2_proj, mask = _f32(xyz1, xyz2_proj, mask)
    (feat1, feat2_proj), dt, code = _feature_dtype(feat1, feat2_proj)
    idx = idx.contiguous()
    B, N, K, _ = idx.shape
    _, H2, W2, C = feat2_proj.shape
    out = torch.empty((B, N, K, 10 + 2 * C), dtype=dt, device=idx.device)
    a = L.CvEncode1Args(B, N, K, H2, W2, C, xyz1.data_ptr(), feat1.data_ptr(), xyz2_proj.data_ptr(),
                        feat2_proj.data_ptr(), idx.data_ptr(), mask.data_ptr(), out.data_ptr(), code)
    return a, out, (xyz1, feat1, xyz2_proj, feat2_proj, idx, mask)


def _cv_encode1(*tensors):
    a, out, _alive = _cv_encode1_args(*tensors)
    L.call("elo_cv_encode1", a, out)
    return out


def cv_encode1_form(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask):
    """Which kernel cv_encode1 launches for these tensors (include/elo.h: elo_cv_encode1_form; a name of _lib.ENCODE1_FORMS).
    Raises where the call would.  Launches nothing, but builds the call's argument block (its output tensor included) to ask.  The form
    depends on the tensors' addresses: the answer is the call's for tensors that are already contiguous -- of one that is not, the call
    reads a fresh (16-byte aligned) contiguous copy, and so does this query, each its own.  The same holds for the two queries below."""
    a, _out, _alive = _cv_encode1_args(xyz1, feat1, xyz2_proj, feat2_proj, idx, mask)
    return L.form("elo_cv_encode1_form", a)


class _CvEncode2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1_proj, feat1_proj, cost_proj, idx, mask):
        ctx.save_for_backward(xyz1_proj, idx, mask)
        ctx.widths = (feat1_proj.shape[-1], cost_proj.shape[-1])
        return _cv_encode2(xyz1_proj, feat1_proj, cost_proj, idx, mask)

    @staticmethod
    def backward(ctx, g_cat, g_rest):
        xyz1, idx, mask = ctx.saved_tensors
        B, H, W, _ = xyz1.shape
        K, (C, Cc), dev, need = idx.shape[2], ctx.widths, xyz1.device, ctx.needs_input_grad
        zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        g_cat = zeros(B, H * W, K, 10) if g_cat is None else _f32(g_cat)[0]
        g_rest = zeros(B, H * W, K, C + Cc) if g_rest is None else _f32(g_rest)[0]
        g_x = zeros(B, H, W, 3) if need[0] else None
        g_f = torch.empty((B, H, W, C), dtype=torch.float32, device=dev) if need[1] else None
        g_c = zeros(B, H, W, Cc) if need[2] else None
        a = L.CvEncode2BwdArgs(B, H * W, K, H, W, C, Cc, xyz1.data_ptr(), idx.data_ptr(), mask.data_ptr(), g_cat.data_ptr(),
                               g_rest.data_ptr(), _ptr(g_x), _ptr(g_f), _ptr(g_c))
        L.call("elo_cv_encode2_backward", a, xyz1)
        return g_x, g_f, g_c, None, None


def cv_encode2(xyz1_proj, feat1_proj, cost_proj, idx, mask):
    """xyz_cat (B,N,K,10) and rest (B,N,K,C+Cc) = [feat1, cost[idx]*m].  pointnet_util.py:110-129."""
    if _wants_grad(xyz1_proj, feat1_proj, cost_proj):
        return _CvEncode2.apply(*_f32(xyz1_proj, feat1_proj, cost_proj), idx.contiguous(), _f32(mask)[0])
    return _cv_encode2(xyz1_proj, feat1_proj, cost_proj, idx, mask)


def _cv_encode2_args(xyz1_proj, feat1_proj, cost_proj, idx, mask):
    L.require_gpu(xyz1_proj, feat1_proj, cost_proj, idx, mask)
    xyz1_proj, mask = _f32(xyz1_proj, mask)
    (feat1_proj, cost_proj), dt, code = _feature_dtype(feat1_proj, cost_proj)
    idx = idx.contiguous()
    B, N, K, _ = idx.shape
    _, H, W, C = feat1_proj.shape
    Cc = cost_proj.shape[-1]
    xyz_cat = torch.empty((B, N, K, 10), dtype=dt, device=idx.device)
    rest = torch.empty((B, N, K, C + Cc), dtype=dt, device=idx.device)
    a = L.CvEncode2Args(B, N, K, H, W, C, Cc, xyz1_proj.data_ptr(), feat1_proj.data_ptr(), cost_proj.data_ptr(),
                        idx.data_ptr(), mask.data_ptr(), xyz_cat.data_ptr(), rest.data_ptr(), code)
    return a, (xyz_cat, rest), (xyz1_proj, feat1_proj, cost_proj, idx, mask)


def _cv_encode2(*tensors):
    a, outs, _alive = _cv_encode2_args(*tensors)
    L.call("elo_cv_encode2", a, outs[1])
    return outs


def cv_encode2_form(xyz1_proj, feat1_proj, cost_proj, idx, mask):
    """Which kernel cv_encode2 launches for these tensors (elo_cv_encode2_form; a name of _lib.ENCODE2_FORMS).  Launches nothing."""
    a, _outs, _alive = _cv_encode2_args(xyz1_proj, feat1_proj, cost_proj, idx, mask)
    return L.form("elo_cv_encode2_form", a)


class _MaskedSoftmaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, mask):
        ctx.save_for_backward(logits, values, mask)
        return _masked_softmax_pool(logits, values, mask)

    @staticmethod
    def backward(ctx, grad):
        logits, values, mask = ctx.saved_tensors
        (grad,) = _f32(grad)
        B, N, K, C = logits.shape
        if values.stride(-1) != 1 or values.stride(1) != K * values.stride(2) or values.stride(0) != N * values.stride(1):
            values = values.contiguous()
        g_l, g_v = torch.empty_like(logits), torch.empty((B, N, K, C), dtype=torch.float32, device=grad.device)
        a = L.SoftmaxPoolBwdArgs(B, N, K, C, logits.data_ptr(), values.data_ptr(), values.stride(2), mask.data_ptr(),
                                 grad.data_ptr(), g_l.data_ptr(), g_v.data_ptr())
        L.call("elo_masked_softmax_pool_backward", a, grad)
        return g_l, g_v, None


def masked_softmax_pool(logits, values, mask):
    """sum_k softmax_k(where(mask==1, logits, -1e10)) * values -> (B,N,C).  pointnet_util.py:92-98, :137-146.
    `values` may be a last-dim slice of a wider contiguous tensor (no copy)."""
    if _wants_grad(logits, values):
        if logits.dtype != torch.float32 or values.dtype != torch.float32:
            raise TypeError("training stores its features in float32")
        return _MaskedSoftmaxPool.apply(logits.contiguous(), values, _f32(mask)[0])
    return _masked_softmax_pool(logits, values, mask)


def _masked_softmax_pool_args(logits, values, mask):
    L.require_gpu(logits, values, mask)
    (mask,) = _f32(mask)
    if logits.dtype not in (torch.float32, torch.float16):
        raise TypeError("logits are float32 or float16 (got %s)" % logits.dtype)
    logits = logits.contiguous()
    dt, code = logits.dtype, L.ELO_F16 if logits.dtype == torch.float16 else L.ELO_F32
    B, N, K, C = logits.shape
    if values.dtype != dt or values.shape != logits.shape:
        raise ValueError("values must have the dtype and shape of logits")
    if values.stride(-1) != 1 or values.stride(1) != K * values.stride(2) or values.stride(0) != N * values.stride(1):
        values = values.contiguous()
    out = torch.empty((B, N, C), dtype=dt, device=logits.device)
    a = L.SoftmaxPoolArgs(B, N, K, C, logits.data_ptr(), values.data_ptr(), values.stride(2), mask.data_ptr(),
                          out.data_ptr(), code)
    return a, out, (logits, values, mask)


def _masked_softmax_pool(*tensors):
    a, out, _alive = _masked_softmax_pool_args(*tensors)
    L.call("elo_masked_softmax_pool", a, out)
    return out


def masked_softmax_pool_form(logits, values, mask):
    """Which kernel masked_softmax_pool launches for these tensors under the current tuning (elo_masked_softmax_pool_form; a name of
    _lib.POOL_FORMS).  Launches nothing."""
    a, _out, _alive = _masked_softmax_pool_args(logits, values, mask)
    return L.form("elo_masked_softmax_pool_form", a)


class _SoftmaxValid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feature_bnc, weight_bnc, xyz_bn3):
        B, N, C = feature_bnc.shape
        stats = torch.empty((B, 2, C), dtype=torch.float32, device=feature_bnc.device)
        out = _softmax_valid(feature_bnc, weight_bnc, xyz_bn3, stats)
        ctx.save_for_backward(feature_bnc, weight_bnc, xyz_bn3, out, stats)
        return out

    @staticmethod
    def backward(ctx, grad):
        f, w, xyz, out, stats = ctx.saved_tensors
        (grad,) = _f32(grad)
        B, N, C = f.shape
        g_f, g_w = torch.empty_like(f), torch.empty_like(w)
        a = L.SoftmaxValidBwdArgs(B, N, C, f.data_ptr(), w.data_ptr(), xyz.data_ptr(), grad.data_ptr(), g_f.data_ptr(),
                                  g_w.data_ptr(), out.data_ptr(), stats.data_ptr())
        L.call("elo_softmax_valid_backward", a, grad)
        return g_f, g_w, None


def softmax_valid(feature_bnc, weight_bnc, xyz_bn3):
    """model_util.py:319-343 with mask_valid = any(xyz != 0) -> (B,1,C)."""
    if _wants_grad(feature_bnc, weight_bnc):
        return _SoftmaxValid.apply(*_f32(feature_bnc, weight_bnc, xyz_bn3.detach()))
    return _softmax_valid(feature_bnc, weight_bnc, xyz_bn3)


def _softmax_valid(feature_bnc, weight_bnc, xyz_bn3, stats=None):
    L.require_gpu(feature_bnc, weight_bnc, xyz_bn3)
    feature_bnc, weight_bnc, xyz_bn3 = _f32(feature_bnc, weight_bnc, xyz_bn3)
    B, N, C = feature_bnc.shape
    out = torch.empty((B, 1, C), dtype=torch.float32, device=feature_bnc.device)
    scratch = torch.empty((3 * B * L.SV_MAX_PARTS * C,), dtype=torch.float32, device=feature_bnc.device)
    a = L.SoftmaxValidArgs(B, N, C, feature_bnc.data_ptr(), weight_bnc.data_ptr(), xyz_bn3.data_ptr(), out.data_ptr(),
                           scratch.data_ptr(), stats.data_ptr() if stats is not None else None)
    L.call("elo_softmax_valid", a, out)
    return out


class _PoseCompose(torch.autograd.Function):
    """normalise -> compose with the coarse pose -> normalise (pwclo_model.py:197-208, :262-280) as ONE launch forward and ONE
    backward (elo_pose_compose); torch ran the same chain as ~60 + ~120 kernels of eight elements per level."""

    @staticmethod
    def forward(ctx, q_raw, t_det, q_coarse, t_coarse):
        B = q_raw.shape[0]
        q, t, q_norm = torch.empty_like(q_raw), torch.empty_like(t_det), torch.empty_like(q_raw)
        ptr = lambda x: x.data_ptr() if x is not None else None
        a = L.PoseComposeArgs(B, q_raw.data_ptr(), t_det.data_ptr(), ptr(q_coarse), ptr(t_coarse), q.data_ptr(), t.data_ptr(),
                              q_norm.data_ptr(), None, None, None, None, None, None, None)
        L.call("elo_pose_compose", a, q_raw)
        ctx.save_for_backward(q_raw, t_det, q_coarse, t_coarse)
        return q, t, q_norm

    @staticmethod
    def backward(ctx, gq, gt, gqn):
        q_raw, t_det, q_coarse, t_coarse = ctx.saved_tensors
        B = q_raw.shape[0]
        z = lambda g, like: torch.zeros_like(like) if g is None else g.contiguous()
        gq, gt, gqn = z(gq, q_raw), z(gt, t_det), z(gqn, q_raw)
        g_qr, g_td = torch.empty_like(q_raw), torch.empty_like(t_det)
        g_qc = torch.empty_like(q_coarse) if q_coarse is not None else None
        g_tc = torch.empty_like(t_coarse) if t_coarse is not None else None
        ptr = lambda x: x.data_ptr() if x is not None else None
        a = L.PoseComposeArgs(B, q_raw.data_ptr(), t_det.data_ptr(), ptr(q_coarse), ptr(t_coarse), None, None, None,
                              gq.data_ptr(), gt.data_ptr(), gqn.data_ptr(), g_qr.data_ptr(), g_td.data_ptr(), ptr(g_qc), ptr(g_tc))
        L.call("elo_pose_compose", a, q_raw)
        return g_qr, g_td, g_qc, g_tc


def pose_compose(q_raw, t_det, q_coarse=None, t_coarse=None):
    """(q (B,4), t (B,3), q_norm (B,4)) of a level from the head's raw quaternion and translation and the coarse pose
    (None at the coarsest level); differentiable (the training path's pose algebra in one launch each way)."""
    L.require_gpu(q_raw, t_det, q_coarse, t_coarse)
    B = q_raw.shape[0]
    f = lambda x, n: None if x is None else _f32(x.reshape(B, n))[0]
    return _PoseCompose.apply(f(q_raw, 4), f(t_det, 3), f(q_coarse, 4), f(t_coarse, 3))


class _PoseLoss(torch.autograd.Function):
    """get_loss (pwclo_model.py:437-481) over the four levels: one launch forward, one backward (elo_pose_loss)."""

    @staticmethod
    def forward(ctx, w_x, w_q, q_gt, t_gt, *poses):                # poses: l0_q, l0_t, l1_q, l1_t, l2_q, l2_t, l3_q, l3_t
        B = q_gt.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=q_gt.device)
        P4 = ctypes.c_void_p * 4
        a = L.PoseLossArgs(B, P4(*[poses[2 * i].data_ptr() for i in range(4)]), P4(*[poses[2 * i + 1].data_ptr() for i in range(4)]),
                           q_gt.data_ptr(), t_gt.data_ptr(), w_x.data_ptr(), w_q.data_ptr(), loss.data_ptr(), None, P4(), P4(), None, None)
        L.call("elo_pose_loss", a, q_gt)
        ctx.save_for_backward(w_x, w_q, q_gt, t_gt, *poses)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        w_x, w_q, q_gt, t_gt, *poses = ctx.saved_tensors
        B = q_gt.shape[0]
        grads = [torch.empty_like(x) for x in poses]
        g_wx, g_wq = torch.empty_like(w_x), torch.empty_like(w_q)
        go = grad_out.contiguous().float()
        P4 = ctypes.c_void_p * 4
        a = L.PoseLossArgs(B, P4(*[poses[2 * i].data_ptr() for i in range(4)]), P4(*[poses[2 * i + 1].data_ptr() for i in range(4)]),
                           q_gt.data_ptr(), t_gt.data_ptr(), w_x.data_ptr(), w_q.data_ptr(), None, go.data_ptr(),
                           P4(*[grads[2 * i].data_ptr() for i in range(4)]), P4(*[grads[2 * i + 1].data_ptr() for i in range(4)]),
                           g_wx.data_ptr(), g_wq.data_ptr())
        L.call("elo_pose_loss", a, q_gt)
        return (g_wx, g_wq, None, None) + tuple(grads)


def pose_loss(l0_q, l0_t, l1_q, l1_t, l2_q, l2_t, l3_q, l3_t, q_gt, t_gt, w_x, w_q):
    """get_loss's arithmetic on the device in one launch (arguments in get_loss's order)."""
    L.require_gpu(l0_q, q_gt, w_x)
    B = q_gt.shape[0]
    poses = [_f32(x.reshape(B, n))[0] for x, n in ((l0_q, 4), (l0_t, 3), (l1_q, 4), (l1_t, 3), (l2_q, 4), (l2_t, 3), (l3_q, 4), (l3_t, 3))]
    return _PoseLoss.apply(w_x, w_q, _f32(q_gt.reshape(B, 4))[0], _f32(t_gt.reshape(B, 3))[0], *poses)


class ProjectionBuffers:
    """Outputs + scratch of one warp_project call, allocated ahead of it so that the pose head that produces its
    (q, t) can clear them on the side (`pose_head(clear=...)`): the warp call then skips its init launch."""

    def __init__(self, B, N, H, W, C, device, dtype=torch.float32):
        self.shape = (B, N, H, W, C)
        self.out_xyz = torch.empty((B, H, W, 3), dtype=torch.float32, device=device)
        self.out_feat = torch.empty((B, H, W, C), dtype=dtype, device=device) if C else None
        self.scratch = torch.empty((B * H * W + 4 * B + 2 * B * N,), dtype=torch.int32, device=device)   # include/elo.h
        self.cleared = False
        self.result = None          # (warped, out_xyz, out_feat) once a pose head has run the projection itself


class SvPartials:
    """softmax_valid's partial sums as a hand-over: the launch that produces the pose head's inputs (fused.mlp2_pair / fused.mlp
    with sv=...) reduces each of its row tiles to a (maximum, denominator, weighted sum) triple per channel and leaves them in
    `scratch`; pose_head(partials=...) merges them instead of running its partial-sums launch (include/elo.h elo_mlp_args.sv_*,
    elo_pose_head_args.ready_parts).  `parts` = slices per batch element, 0 until (unless) a launch has taken the ride.
    xyz: (B,N,3) the cloud whose validity masks the softmax; feature: (B,N,64) for a SINGLE launch (whose output are the logits)."""

    def __init__(self, xyz_bn3, feature_bnc=None):
        (self.xyz,) = _f32(xyz_bn3)
        self.feature = feature_bnc
        self.scratch = torch.empty((3 * xyz_bn3.shape[0] * L.SV_MAX_PARTS * 64,), dtype=torch.float32, device=xyz_bn3.device)
        self.parts = 0


class PoseRing:
    """(slots, B, 7) rows [q_norm | t] + a per-batch-element cursor: the pose output of a launch that is REPLAYED from a
    captured graph.  Replay r writes slot cursor % slots and advances the cursor, so a stream of frame pairs needs no
    copy-out per pair (elo_pose_head_args.pose7_slots / pose7_cursor); drain with rows() every `slots` replays."""

    def __init__(self, slots, batch, device):
        if slots < 2:
            raise ValueError("a pose ring has at least 2 slots")
        self.rows = torch.zeros((slots, batch, 7), dtype=torch.float32, device=device)
        self.cursor = torch.zeros((batch,), dtype=torch.int32, device=device)
        self.slots = slots

    def reset(self):
        """Cursor back to slot 0 (on the current stream)."""
        self.cursor.zero_()


def pose_head(feature_bnc, weight_bnc, xyz_bn3, W_big, b_big, W_q, b_q, W_t, b_t, q_coarse=None, t_coarse=None, pose7=None,
              clear=None, warp=None, next_orders=None, partials=None, sensor=None, form_only=False):
    """softmax_valid -> conv1d(256) -> q,t heads -> normalise -> compose with the coarse pose, two launches.
    pwclo_model.py:194-208 / :262-280.  Returns (q (B,4), t (B,3), q_norm (B,4)); `pose7` (B,7), if given, also receives [q_norm | t].
    `next_orders`: an elo_perm_refresh_args (perm.PermSource.refresh_args): the next pooled set of visiting orders is
    loaded by this launch once the pose is written (the last launch of a captured forward).
    `partials`: an SvPartials a preceding launch has filled (partials.parts > 0): no partial-sums launch here; `clear` must
    then already have been cleared by that launch (fused.mlp(clear=...))).
    `clear`: ProjectionBuffers of the projection that will consume this pose (cleared on the side).
    `warp` = (xyz (B,N,3), feat (B,N,C) or None) with `clear`: that projection itself -- warp by this pose, spherical
    re-projection -- is run by this call (elo_pose_head_warp: 3 launches instead of 2 + 2); its result is left in
    `clear.result` for the warp_project call that follows.  `sensor`: whose field of view that projection uses (None: the
    reference's HDL-64E)."""
    L.require_gpu(feature_bnc, weight_bnc, xyz_bn3, W_big, W_q, W_t, q_coarse, t_coarse)
    xyz_bn3, W_big, b_big, W_q, b_q, W_t, b_t = _f32(xyz_bn3, W_big, b_big, W_q, b_q, W_t, b_t)
    (feature_bnc, weight_bnc), fdt, fcode = _feature_dtype(feature_bnc, weight_bnc)      # fp32 or fp16 storage
    B, N, C = feature_bnc.shape
    hidden = W_big.shape[1]
    dev = feature_bnc.device
    if q_coarse is not None:
        q_coarse, t_coarse = _f32(q_coarse.reshape(B, 4), t_coarse.reshape(B, 3))
    q = torch.empty((B, 4), dtype=torch.float32, device=dev)
    t = torch.empty((B, 3), dtype=torch.float32, device=dev)
    q_norm = torch.empty((B, 4), dtype=torch.float32, device=dev)
    ready = partials.parts if partials is not None else 0
    if ready and C != 64:
        raise ValueError("partials= goes with the 64-channel head")
    scratch = partials.scratch if ready else torch.empty((3 * B * L.SV_MAX_PARTS * C,), dtype=torch.float32, device=dev)
    ptr = lambda x: x.data_ptr() if x is not None else None
    ring = pose7 if isinstance(pose7, PoseRing) else None
    if ring is not None:
        if ring.rows.shape[1] != B:
            raise ValueError("pose ring of batch %d used with batch %d" % (ring.rows.shape[1], B))
        pose7 = ring.rows
    a = L.PoseHeadArgs(B, N, C, hidden, feature_bnc.data_ptr(), weight_bnc.data_ptr(), xyz_bn3.data_ptr(),
                       W_big.data_ptr(), b_big.data_ptr(), W_q.data_ptr(), b_q.data_ptr(), W_t.data_ptr(), b_t.data_ptr(),
                       ptr(q_coarse), ptr(t_coarse), q.data_ptr(), t.data_ptr(), q_norm.data_ptr(), scratch.data_ptr(),
                       ptr(pose7), *((clear.scratch.data_ptr(), clear.out_xyz.data_ptr(), ptr(clear.out_feat),
                                      clear.shape[0] * clear.shape[2] * clear.shape[3], clear.shape[4])
                                     if clear is not None else (None, None, None, 0, 0)), fcode,
                       ring.slots if ring is not None else 0, ring.cursor.data_ptr() if ring is not None else None,
                       next_orders if next_orders is not None else L.PermRefreshArgs(), ready)
    if ready and clear is not None and not clear.cleared:
        raise ValueError("partials=: the ProjectionBuffers must have been cleared by an earlier launch (fused.mlp(clear=...))")
    if clear is not None and clear.out_feat is not None and clear.out_feat.dtype != fdt:
        raise TypeError("the projection buffers and the pose head's features must share one storage dtype")
    if warp is not None:
        if clear is None:
            raise ValueError("warp= needs clear= (the ProjectionBuffers the projection writes)")
        xyz_w, feat_w = warp
        (xyz_w,) = _f32(xyz_w)
        Bw, Nw, Hw, Ww, Cw = clear.shape
        if xyz_w.shape != (Bw, Nw, 3) or (Cw and (feat_w is None or feat_w.shape != (Bw, Nw, Cw))):
            raise ValueError("warp inputs do not match the ProjectionBuffers %s" % (clear.shape,))
        if feat_w is not None:
            if feat_w.dtype != fdt:
                raise TypeError("the warped features and the pose head's features must share one storage dtype")
            feat_w = feat_w.contiguous()
        warped = torch.empty((Bw, Nw, 3), dtype=torch.float32, device=dev)
        az, vres, voff = projection_constants(Hw, Ww, sensor)
        w = L.WarpProjectArgs(Bw, Nw, Cw, Hw, Ww, az, vres, voff, xyz_w.data_ptr(), ptr(feat_w), None, None,
                              warped.data_ptr(), clear.out_xyz.data_ptr(), ptr(clear.out_feat), clear.scratch.data_ptr(), 1, fcode)
        if form_only:                                        # the argument blocks of the launch below, asked instead of launched
            return L.tail_form(a, w)
        L.call2("elo_pose_head_warp", a, w, q)
        clear.result = (warped, clear.out_xyz, clear.out_feat)
        return q, t, q_norm
    if form_only:
        return L.tail_form(a)
    L.call("elo_pose_head", a, q)
    if clear is not None:
        clear.cleared = True
    return q, t, q_norm


def pose_head_form(*args, **kwargs):
    """What pose_head with these arguments launches (elo_pose_head_form on pose_head's own argument blocks; _lib.tail_form_name:
    'f32x4/trips16/model', 'readyx129/trips32/model+warp', ...); raises where the call would be refused.  Launches nothing."""
    return pose_head(*args, form_only=True, **kwargs)


def softmax_valid_parts(npoints):
    """Slices per batch element of the partial-sums launch over `npoints` points (elo_softmax_valid_parts)."""
    return L.lib().elo_softmax_valid_parts(int(npoints))


def _aug_frame_dev(aug_frame, B, dev):
    """(B) int32 on `dev`: an int32 tensor that already lives there is passed through (same memory), anything array-like is
    built on the host and copied."""
    if isinstance(aug_frame, torch.Tensor) and aug_frame.dtype == torch.int32 and aug_frame.device == dev:
        if aug_frame.numel() != B or not aug_frame.is_contiguous():
            raise ValueError("a device aug_frame is a contiguous int32 tensor of one entry per batch element")
        return aug_frame.view(B)
    return torch.as_tensor(np.asarray(aug_frame).reshape(B), dtype=torch.int32).to(dev)


def preprocess_gt(T_gt, T_trans, T_trans_inv, aug_frame_dev):
    """elo_preprocess_gt: T_gt (B,4,4), T_trans / T_trans_inv (B,4,4) or both None, aug_frame_dev (B) int32 on the device
    (None without T_trans) -> (q_gt (B,4), t_gt (B,3)) in one launch."""
    L.require_gpu(T_gt, T_trans, T_trans_inv)
    B = T_gt.shape[0]
    (T_gt,) = _f32(T_gt.reshape(B, 4, 4))
    dev = T_gt.device
    if (T_trans is None) != (T_trans_inv is None):
        raise ValueError("T_trans and T_trans_inv come together")
    aug = None
    if T_trans is not None:
        T_trans, T_trans_inv = _f32(T_trans.reshape(B, 4, 4), T_trans_inv.reshape(B, 4, 4))
        if not isinstance(aug_frame_dev, torch.Tensor) or aug_frame_dev.dtype != torch.int32:
            raise TypeError("aug_frame_dev is an int32 tensor on the device (the launch reads it there)")
        L.require_gpu(aug_frame_dev)
        aug = _aug_frame_dev(aug_frame_dev, B, dev)
    q_gt = torch.empty((B, 4), dtype=torch.float32, device=dev)
    t_gt = torch.empty((B, 3), dtype=torch.float32, device=dev)
    a = L.PreprocessGtArgs(B, T_gt.data_ptr(), _ptr(T_trans), _ptr(T_trans_inv), _ptr(aug), q_gt.data_ptr(), t_gt.data_ptr())
    L.call("elo_preprocess_gt", a, q_gt)
    return q_gt, t_gt


def beam_table(table, H, device):
    """The (H) float32 device tensor elo_input_stage_beams reads (radians, row 0 = the highest beam) from a Sensor with a beam
    table or from a host array-like of radians.  Checked here, on the host, where the values can be seen: H finite, strictly
    descending float32 entries (EloError otherwise) -- the entry point itself cannot look into device memory.  The caller owns
    the tensor: a graph that records a launch reading it keeps its pointer (include/elo.h, LIFETIME)."""
    if isinstance(table, _sensor.Sensor):
        table = table.beam_elevations_rad()
        if table is None:
            raise L.EloError("this sensor has no beam table")
    if isinstance(table, torch.Tensor):
        table = table.detach().cpu().numpy()
    host = np.asarray(table, dtype=np.float64).astype(np.float32)
    if host.ndim != 1 or host.shape[0] != H:
        raise L.EloError("a beam table has one elevation per image row (got shape %s for H = %d)" % (host.shape, H))
    if not np.isfinite(host).all() or not (host[:-1] > host[1:]).all():
        raise L.EloError("beam elevations must be finite and strictly descending in float32 (row 0 is the highest beam)")
    return torch.from_numpy(host).to(device)


def _on_device(table):
    return isinstance(table, torch.Tensor) and table.is_cuda


def bind_sensor(sensor, device, beam_elev=None, H=None):
    """For whoever OWNS a beam table -- a net, a tracker, a trainer: (the resolved Sensor, its table as a float32 tensor on `device`
    or None).  `beam_elev` (None: the sensor's own table) and `H` (None: that table's length) as beam_table() takes them; a tensor
    that already lives on a GPU is handed back as it is.  The launches the owner issues read the table when they RUN, and a graph
    that records them holds its pointer: the owner keeps the tensor for as long as either can."""
    sensor = _sensor.resolve(sensor)
    if beam_elev is None and sensor.beam_elevations_deg is not None:
        beam_elev, H = sensor, len(sensor.beam_elevations_deg) if H is None else H
    if beam_elev is not None and not _on_device(beam_elev):
        beam_elev = beam_table(beam_elev, H, device)
    return sensor, beam_elev


CellRule = collections.namedtuple("CellRule", "az_res vert_res vert_off beam_elev sensor")


def cell_rule(H, W, device, sensor=None, beam_elev=None, whose="cloud's", max_beams=None, one_row=None):
    """The rule that gives a point its cell of an (H,W) image, resolved for ONE call: the three constants of the row formula
    (projection_constants) at the resolved `sensor`, and the beam table the launch reads -- a float32 tensor on `device` -- or None
    for the formula alone.  `beam_elev` None: the sensor's table, if it has one.  A tensor on a GPU is used as it is -- its owner
    (bind_sensor) validated its values and keeps it alive -- once its device (the `whose` device), dtype, layout and length are
    checked; anything else is validated and uploaded here, which a graph capture cannot record: refused while one is open.
    `max_beams`: an explicit table of more rows is refused here and not by the library; `one_row`: (vert_res, vert_off) of an
    image of ONE row, where the formula has no resolution."""
    sensor = _sensor.resolve(sensor)
    if isinstance(device, str):
        device = torch.device(device)
    if beam_elev is not None and max_beams is not None and H > max_beams:
        raise L.EloError("a beam table has at most %d beams (H = %d)" % (max_beams, H))
    if beam_elev is None and sensor.beam_elevations_deg is not None:
        beam_elev = sensor
    if _on_device(beam_elev):
        if beam_elev.device != device or beam_elev.dtype != torch.float32 or not beam_elev.is_contiguous() or beam_elev.numel() != H:
            raise L.EloError("a device beam table is a contiguous float32 tensor of H = %d entries on the %s device" % (H, whose))
    elif beam_elev is not None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise L.EloError("a graph capture needs the beam table as a device tensor its owner keeps (beam_elev=beam_table(...))")
        beam_elev = beam_table(beam_elev, H, device)
    if H == 1 and one_row is not None:
        return CellRule(projection_constants(2, W, sensor)[0], *one_row, beam_elev, sensor)
    return CellRule(*projection_constants(H, W, sensor), beam_elev, sensor)


def _check_tensors(given):
    """Each (name, tensor, dtype) of `given` is a tensor of that dtype (TypeError) that the launch can use in place (EloError)."""
    for name, t, dtype in given:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s is a tensor (got %r)" % (name, type(t).__name__))
        if t.dtype != dtype:
            raise TypeError("%s is %s (got %s)" % (name, str(dtype).replace("torch.", ""), t.dtype))
        if not t.is_contiguous():
            raise L.EloError("%s must be contiguous: the launch uses it in place" % name)


def _motion_dev(motion, B, dev, name):
    """(B,7) float32 on `dev`: a contiguous float32 tensor that already lives there is passed through (same memory: its pointer is
    what the launch -- and a graph that records it -- reads), anything else is converted and copied (not inside a capture)."""
    if isinstance(motion, torch.Tensor) and motion.is_cuda:
        if motion.device == dev and motion.dtype == torch.float32 and motion.is_contiguous() and tuple(motion.shape) == (B, 7):
            return motion
    if torch.cuda.is_current_stream_capturing():
        raise L.EloError("a graph capture needs `%s` as a contiguous float32 (B,7) tensor on the cloud's device" % name)
    if not isinstance(motion, torch.Tensor):
        motion = torch.from_numpy(np.ascontiguousarray(np.asarray(motion, dtype=np.float32)))
    if motion.numel() != B * 7:
        raise L.EloError("`%s` is one [q0 q1 q2 q3 | t0 t1 t2] row per batch element: (%d, 7) (got %s)" % (name, B, tuple(motion.shape)))
    return motion.to(device=dev, dtype=torch.float32).reshape(B, 7).contiguous()


def _check_sweep(sweep, motion, motion2, motion_is_pose, cloud):
    """input_stage's sweep and motion come together; the phase channel exists in the cloud; the batch fits the kernel's staging."""
    if sweep is None:
        if motion is not None or motion2 is not None or motion_is_pose:
            raise L.EloError("a motion without a sweep: pass sweep=Sweep(...) to say when each point was acquired")
        return
    if not isinstance(sweep, _sensor.Sweep):
        raise TypeError("sweep is a Sweep or None (got %r)" % (type(sweep).__name__,))
    if motion is None:
        raise L.EloError("a sweep without a motion: pass motion=(B,7) rows [q | t] (the identity row is 1 0 0 0 0 0 0)")
    if sweep.phase != "azimuth" and sweep.phase >= cloud.shape[-1]:
        raise L.EloError("the sweep's phase is channel %d, the cloud has %d floats per point" % (sweep.phase, cloud.shape[-1]))
    if cloud.shape[0] > L.DESKEW_MAX_BATCH:
        raise L.EloError("elo_input_stage_deskew stages the motions of at most %d batch elements (got %d)"
                         % (L.DESKEW_MAX_BATCH, cloud.shape[0]))


def input_stage(cloud, T_trans, aug_frame, H, W, crop_xy=None, sensor=None, beam_elev=None, sweep=None, motion=None, motion2=None,
                motion_is_pose=False):
    """elo_input_stage: cloud (B, 2N, S>=3) fp32, T_trans (B,4,4) or None, aug_frame (B) of 1/2 (array-like, or an int32
    tensor already on the cloud's device: its pointer is what the launch -- and a graph that records it -- reads) ->
    (points (2B,N,3), xyz_proj (2B,H,W,3)).
    `sensor` (None: the reference's HDL-64E) gives the field of view and, unless `crop_xy` is passed, the crop.  A sensor with
    a beam table -- or an explicit `beam_elev` -- takes elo_input_stage_beams: the row of a point is the beam nearest in
    elevation.  `beam_elev`: that table as a float32 tensor on the cloud's device (beam_table(); used as it is -- its owner
    validated it and keeps it alive for every graph that recorded this call), or a host array-like of radians (validated and
    uploaded here: not inside a graph capture).
    `sweep` (sensor.Sweep) with `motion`: the scan is NOT motion-compensated -- elo_input_stage_deskew first carries every point
    from its acquisition phase (sweep.phase: "azimuth", or the channel of the cloud that holds it) to sweep.phase_ref by the
    sensor's motion during the sweep, then does all of the above on the corrected cloud.  `motion`: (B,7) rows [q | t], the
    transform from the sensor frame at the END of the sweep to the one at its START, for both frames; `motion2`: frame 2's, if
    it differs.  `motion_is_pose`: the rows are the net's [q_norm | t] of the previous pair (frame 1 -> frame 2) and are inverted
    in the kernel.  A contiguous float32 tensor on the cloud's device is used as it is and read when the launch RUNS (a graph that
    records this call sees what it holds at every replay); anything else is uploaded here.  One without the other is an EloError;
    with neither this is exactly the calls above."""
    _check_sweep(sweep, motion, motion2, motion_is_pose, cloud)        # (what the host can refuse without a GPU, first)
    L.require_gpu(cloud, T_trans)
    (cloud,) = _f32(cloud)
    B, N2, S = cloud.shape
    if N2 % 2 or S < 3:
        raise ValueError("point_cloud must be (B, 2*N, >=3)")
    N, dev = N2 // 2, cloud.device
    if sweep is not None:
        motion = _motion_dev(motion, B, dev, "motion")
        if motion2 is not None:
            motion2 = _motion_dev(motion2, B, dev, "motion2")
    rule = cell_rule(H, W, dev, sensor, beam_elev)
    crop = float(rule.sensor.crop_xy if crop_xy is None else crop_xy)
    if T_trans is not None:
        (T_trans,) = _f32(T_trans.reshape(B, 4, 4))
        aug = _aug_frame_dev(aug_frame, B, dev)
    points = torch.empty((2 * B, N, 3), dtype=torch.float32, device=dev)
    out_xyz = torch.empty((2 * B, H, W, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty((2 * B * H * W + 4 * 2 * B + 2 * 2 * B * N,), dtype=torch.int32, device=dev)
    az, vres, voff, table = rule.az_res, rule.vert_res, rule.vert_off, _ptr(rule.beam_elev)
    tail = (cloud.data_ptr(), T_trans.data_ptr() if T_trans is not None else None,
            aug.data_ptr() if T_trans is not None else None, points.data_ptr(), out_xyz.data_ptr(), scratch.data_ptr())
    if sweep is not None:                                    # (with or without a table: the de-skewing entry takes both row rules)
        azimuth = sweep.phase == "azimuth"
        entry, a = "elo_input_stage_deskew", L.InputStageDeskewArgs(
            B, N, S, H, W, az, vres, voff, crop, *tail, table, motion.data_ptr(), _ptr(motion2), 1 if motion_is_pose else 0,
            L.PHASE_AZIMUTH if azimuth else L.PHASE_CHANNEL, 0 if azimuth else sweep.phase, sweep.phase_ref)
    elif table is None:
        entry, a = "elo_input_stage", L.InputStageArgs(B, N, S, H, W, az, vres, voff, crop, *tail)
    else:
        entry, a = "elo_input_stage_beams", L.InputStageBeamsArgs(B, N, S, H, W, az, crop, *tail, table)
    L.call(entry, a, out_xyz)
    return points, out_xyz


class PoseFitResult:
    """What elo_pose_fit wrote for a batch: pose (B,7) [q | t] -- the input pose, or the polished one --, info (B,6,6) = the
    normal matrix A at that pose (rotation first, then translation; left perturbation), grad (B,6) = b, and views of the (B,4)
    stats block: count (terms, an exact integer in float32), cost = sum w r^2, rms = sqrt(cost / sum w), status (0: fine; bits
    _lib.FIT_FEW / FIT_SINGULAR: a step was refused and the pose is the input's; FIT_FEW_FINAL: the reported evaluation has fewer
    than min_count terms).  The tensors are the launch's own outputs: valid once its stream has been synchronised or waited on."""
    __slots__ = ("pose", "info", "grad", "stats", "scratch", "keep")

    def __init__(self, pose, info, grad, stats, scratch=None, keep=None):
        self.pose, self.info, self.grad, self.stats, self.scratch = pose, info, grad, stats, scratch
        self.keep = keep                  # the beam table the launches read when they run: it lives as long as the result

    count = property(lambda self: self.stats[:, 0])
    cost = property(lambda self: self.stats[:, 1])
    rms = property(lambda self: self.stats[:, 2])
    status = property(lambda self: self.stats[:, 3])

    def covariance(self):
        """sigma^2 A^-1 with sigma^2 = cost / (count - 6), per image, (B,6,6) float64 on the host -- for reporting.  NaN rows
        where count <= 6 or A is singular."""
        A = self.info.detach().cpu().numpy().astype(np.float64)
        st = self.stats.detach().cpu().numpy().astype(np.float64)
        out = np.full(A.shape, np.nan)
        for b in range(A.shape[0]):
            if st[b, 0] > 6:
                try:
                    out[b] = st[b, 1] / (st[b, 0] - 6) * np.linalg.inv(A[b])
                except np.linalg.LinAlgError:
                    pass
        return out


def _check_pose_fit(xyz1, xyz2, pose7, fit):
    """What the host can refuse about a pose fit without a GPU or the library: the value, shapes, dtypes, layout, devices (the
    beam table: cell_rule)."""
    if not isinstance(fit, _sensor.PoseFit):
        raise TypeError("fit is a PoseFit (got %r)" % (type(fit).__name__,))
    _check_tensors((("xyz1", xyz1, torch.float32), ("xyz2", xyz2, torch.float32), ("pose7", pose7, torch.float32)))
    if xyz1.dim() != 4 or xyz1.shape[-1] != 3 or xyz1.shape != xyz2.shape:
        raise L.EloError("xyz1 / xyz2 are two (B,H,W,3) range images of one shape (got %s, %s)" % (tuple(xyz1.shape), tuple(xyz2.shape)))
    B, H, W, _ = xyz1.shape
    if H < 3:
        raise L.EloError("a normal needs three rows: H >= 3 (got %d)" % H)
    if tuple(pose7.shape) != (B, 7):
        raise L.EloError("pose7 is one [q0 q1 q2 q3 | t0 t1 t2] row per image: (%d, 7) (got %s)" % (B, tuple(pose7.shape)))
    if xyz2.device != xyz1.device or pose7.device != xyz1.device:
        raise L.EloError("xyz1, xyz2 and pose7 live on one device")


def pose_fit(xyz1, xyz2, pose7, fit, sensor=None, beam_elev=None):
    """elo_pose_fit: the point-to-plane fit of the poses `pose7` (B,7) [q | t] (frame 1 -> frame 2) on the range images xyz1 / xyz2
    (B,H,W,3) -> PoseFitResult.  `fit`: a sensor.PoseFit.  `sensor` (None: the reference's HDL-64E) gives the field of view of the
    cell rule; a sensor with a beam table -- or an explicit `beam_elev`, as input_stage takes it -- matches by the beam-table rows
    the input stage of such a sensor wrote the images with.  Inputs are float32, contiguous and used in place: pose7 is read when
    the launches RUN (a graph that records this call fits what the row holds at every replay).  Bad shapes, dtypes or layouts
    are refused here, before anything is launched."""
    _check_pose_fit(xyz1, xyz2, pose7, fit)
    B, H, W, _ = xyz1.shape
    dev = xyz1.device
    rule = cell_rule(H, W, dev, sensor, beam_elev, "images'", L.MAX_BEAMS)
    L.require_gpu(xyz1, xyz2, pose7)
    words = L.lib().elo_pose_fit_scratch_words(B, H, W)
    if words < 0:
        raise L.EloError("elo_pose_fit refuses a (%d,%d,%d) batch of images" % (B, H, W))
    res = PoseFitResult(torch.empty((B, 7), dtype=torch.float32, device=dev), torch.empty((B, 6, 6), dtype=torch.float32, device=dev),
                        torch.empty((B, 6), dtype=torch.float32, device=dev), torch.empty((B, 4), dtype=torch.float32, device=dev),
                        torch.empty((max(words, 1),), dtype=torch.int32, device=dev), keep=rule.beam_elev)
    a = L.PoseFitArgs(B, H, W, rule.az_res, rule.vert_res, rule.vert_off, xyz1.data_ptr(), xyz2.data_ptr(), pose7.data_ptr(),
                      _ptr(rule.beam_elev), fit.iters, fit.gate, fit.huber, fit.jump_rel, fit.min_count, fit.damping, res.pose.data_ptr(),
                      res.info.data_ptr(), res.grad.data_ptr(), res.stats.data_ptr(), res.scratch.data_ptr())
    L.call("elo_pose_fit", a, xyz1)
    return res


def _check_model_render(src, pose):
    """What the host can refuse about a model render without a GPU or the library: shapes, dtypes, layout, devices (the beam
    table: cell_rule)."""
    _check_tensors((("src", src, torch.float32), ("pose", pose, torch.float32)))
    if src.dim() != 5 or src.shape[-1] != 3:
        raise L.EloError("src is (B,K,H,W,3): K range images per batch element (got %s)" % (tuple(src.shape),))
    B, K, H, W, _ = src.shape
    if K < 1 or K > L.MODEL_MAX_SCANS:
        raise L.EloError("a model holds 1 .. %d scans (K = %d)" % (L.MODEL_MAX_SCANS, K))
    if H < 1 or W < 1:
        raise L.EloError("src has no cells: H, W >= 1 (got %d x %d)" % (H, W))
    if K * H * W >= 2 ** 31 or B * H * W >= 2 ** 31:
        raise L.EloError("K*H*W and B*H*W stay below 2^31 (got B, K, H, W = %d, %d, %d, %d)" % (B, K, H, W))
    if tuple(pose.shape) != (B, K, 7):
        raise L.EloError("pose is one [q0 q1 q2 q3 | t0 t1 t2] row per source: (%d, %d, 7) (got %s)" % (B, K, tuple(pose.shape)))
    if pose.device != src.device:
        raise L.EloError("src and pose live on one device")


def model_render(src, pose, sensor=None, beam_elev=None):
    """elo_model_render: the K range images src (B,K,H,W,3), each carried by its row of pose (B,K,7) [q | t] (source k -> the
    model's frame), rendered into one range image by nearest range -> (xyz (B,H,W,3) float32, src_idx (B,H,W) int32: (k*H + h)*W + w
    of the point each cell holds, -1 where it is empty).  `sensor` / `beam_elev`: the cell rule, as pose_fit takes them.  Inputs
    are float32, contiguous and used in place: both are read when the launches RUN (a graph that records this call renders what
    they hold at every replay).  Bad shapes, dtypes or layouts are refused here, before anything is launched."""
    _check_model_render(src, pose)
    B, K, H, W, _ = src.shape
    dev = src.device
    rule = cell_rule(H, W, dev, sensor, beam_elev, "images'", L.MAX_BEAMS, one_row=(1.0, 0.0))
    L.require_gpu(src, pose)
    words = L.lib().elo_model_render_scratch_words(B, H, W)
    if words < 0:
        raise L.EloError("elo_model_render refuses a (%d,%d,%d) batch of images" % (B, H, W))
    xyz = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    scratch = torch.empty((max(words, 2),), dtype=torch.int32, device=dev)
    a = L.ModelRenderArgs(B, K, H, W, rule.az_res, rule.vert_res, rule.vert_off, src.data_ptr(), pose.data_ptr(), _ptr(rule.beam_elev),
                          xyz.data_ptr(), idx.data_ptr(), scratch.data_ptr())
    L.call("elo_model_render", a, src)
    return xyz, idx


def _check_model_state(ring, state, image, name, poses64=None, poses32=None, T=None):
    """What the host can refuse about a tracker-state launch without a GPU or the library: types, dtypes, layout, shapes, devices."""
    given = [("ring", ring, torch.float32), ("state", state, torch.int32), (name, image, torch.float32)]
    if poses64 is not None or poses32 is not None or T is not None:
        given += [("poses64", poses64, torch.float64), ("poses32", poses32, torch.float32), ("T", T, torch.float32)]
    _check_tensors(given)
    if ring.dim() != 4 or ring.shape[-1] != 3:
        raise L.EloError("ring is (K,H,W,3): the K scans a model holds (got %s)" % (tuple(ring.shape),))
    K, H, W, _ = ring.shape
    if K < 1 or K > L.MODEL_MAX_SCANS:
        raise L.EloError("a model holds 1 .. %d scans (K = %d)" % (L.MODEL_MAX_SCANS, K))
    if H < 3 or W < 1:
        raise L.EloError("a pose fit needs H >= 3 and W >= 1 (got %d x %d)" % (H, W))
    if K * H * W >= 2 ** 31:
        raise L.EloError("K*H*W stays below 2^31 (got K, H, W = %d, %d, %d)" % (K, H, W))
    if tuple(state.shape) != (2,):
        raise L.EloError("state is the two int32 words {next, held} (got %s)" % (tuple(state.shape),))
    if tuple(image.shape) != (H, W, 3):
        raise L.EloError("%s is one (%d,%d,3) range image, as the ring's slots are (got %s)" % (name, H, W, tuple(image.shape)))
    if len(given) > 3:
        if tuple(poses64.shape) != (K, 7) or tuple(poses32.shape) != (K, 7):
            raise L.EloError("poses64 / poses32 are one [q | t] row per slot: (%d, 7) (got %s, %s)"
                             % (K, tuple(poses64.shape), tuple(poses32.shape)))
        if tuple(T.shape) not in ((7,), (1, 7)):
            raise L.EloError("T is one [q0 q1 q2 q3 | t0 t1 t2] row (got %s)" % (tuple(T.shape),))
    if any(t.device != ring.device for _w, t, _d in given):
        raise L.EloError("the tracker's state and its images live on one device")


def model_begin(ring, state, first):
    """elo_model_begin: where the tracker state `state` (int32[2] = {next, held}) says the model is empty, the image `first` (H,W,3)
    -- the pair's frame 2 -- enters slot 0 of `ring` (K,H,W,3); otherwise nothing is written.  One launch that takes its decision
    from device memory when it RUNS: no host synchronisation, capturable.  Bad types, shapes or layouts are refused here, before
    anything is launched."""
    _check_model_state(ring, state, first, "first")
    L.require_gpu(ring, state, first)
    K, H, W, _ = ring.shape
    L.call("elo_model_begin", L.ModelBeginArgs(K, H, W, ring.data_ptr(), state.data_ptr(), first.data_ptr()), ring)


def model_advance(ring, poses64, poses32, state, scan, T):
    """elo_model_advance: the image `scan` (H,W,3) enters the slot of `ring` (K,H,W,3) the state names; every row of `poses64` (K,7)
    double is re-based by T^-1 (`T`: (7) or (1,7) float32 [q | t], the fit's pose of `scan` against the model), the entered row becomes
    the identity, `poses32` (K,7) becomes poses64 rounded to float32 and `state` moves on.  Two launches that take their decisions
    from device memory when they RUN: no host synchronisation, capturable.  Refusals as model_begin."""
    _check_model_state(ring, state, scan, "scan", poses64, poses32, T)
    L.require_gpu(ring, state, scan, poses64, poses32, T)
    K, H, W, _ = ring.shape
    a = L.ModelAdvanceArgs(K, H, W, ring.data_ptr(), poses64.data_ptr(), poses32.data_ptr(), state.data_ptr(), scan.data_ptr(),
                           T.data_ptr())
    L.call("elo_model_advance", a, ring)


def _check_map(keys, acc, spec, stats=None):
    """What the host can refuse about a world map's buffers without a GPU or the library: the value, dtypes, layout, shapes, devices.
    The table's words are unsigned 64-bit on the device; torch holds them as int64 (counts and sums stay far below 2^63, and an empty
    key, all ones, reads -1)."""
    from .sensor import VoxelMap
    if not isinstance(spec, VoxelMap):
        raise TypeError("spec is a VoxelMap (got %r)" % (type(spec).__name__,))
    given = [("keys", keys, torch.int64), ("acc", acc, torch.int64)] + ([("stats", stats, torch.int64)] if stats is not None else [])
    _check_tensors(given)
    C = spec.capacity
    if tuple(keys.shape) != (C,) or tuple(acc.shape) != (C, 4):
        raise L.EloError("a map of log2_capacity %d has keys (%d,) and acc (%d, 4) (got %s, %s)"
                         % (spec.log2_capacity, C, C, tuple(keys.shape), tuple(acc.shape)))
    if stats is not None and tuple(stats.shape) != (8,):
        raise L.EloError("stats is eight 64-bit words (got %s)" % (tuple(stats.shape),))
    if any(t.device != keys.device for _w, t, _d in given):
        raise L.EloError("a map's buffers live on one device")


def map_insert(keys, acc, stats, xyz, pose64, spec):
    """elo_map_insert: the range images xyz (B,H,W,3) float32, each carried by its row of pose64 (B,7) float64 [q | t] (scan ->
    world), summed into the voxel map (keys (C,), acc (C,4), stats (8,), all int64, C = spec.capacity; spec: sensor.VoxelMap).  One
    launch on the current stream, no host synchronisation, capturable; inputs are contiguous and used in place.  Bad types, shapes or
    layouts are refused here, before anything is launched."""
    _check_map(keys, acc, spec, stats)
    _check_tensors((("xyz", xyz, torch.float32), ("pose64", pose64, torch.float64)))
    if xyz.dim() != 4 or xyz.shape[-1] != 3:
        raise L.EloError("xyz is (B,H,W,3): one range image per scan (got %s)" % (tuple(xyz.shape),))
    B, H, W, _ = xyz.shape
    if H < 1 or W < 1:
        raise L.EloError("xyz has no cells: H, W >= 1 (got %d x %d)" % (H, W))
    if B * H * W >= 2 ** 31:
        raise L.EloError("B*H*W stays below 2^31 (got B, H, W = %d, %d, %d)" % (B, H, W))
    if tuple(pose64.shape) != (B, 7):
        raise L.EloError("pose64 is one [q0 q1 q2 q3 | t0 t1 t2] row per scan: (%d, 7) (got %s)" % (B, tuple(pose64.shape)))
    if xyz.device != keys.device or pose64.device != keys.device:
        raise L.EloError("the map, the images and the poses live on one device")
    L.require_gpu(keys, acc, stats, xyz, pose64)
    a = L.MapInsertArgs(B, H, W, spec.voxel, spec.min_range, spec.max_range, spec.log2_capacity, xyz.data_ptr(), pose64.data_ptr(),
                        keys.data_ptr(), acc.data_ptr(), stats.data_ptr())
    L.call("elo_map_insert", a, keys)


def map_extract(keys, acc, spec, max_out):
    """elo_map_extract: the occupied slots of the map as rows in ARBITRARY order -> (key (max_out,) int64, count (max_out,) int64, xyz
    (max_out,3) float32 centroids, n: a 0-dim int64 device tensor, the number of occupied slots -- it may exceed max_out; only the
    first min(n, max_out) rows are written).  Two launches on the current stream, no host synchronisation, capturable."""
    _check_map(keys, acc, spec)
    if isinstance(max_out, bool) or not hasattr(max_out, "__index__") or max_out.__index__() < 0:
        raise L.EloError("max_out is a non-negative integer (got %r)" % (max_out,))
    max_out = max_out.__index__()
    L.require_gpu(keys, acc)
    dev = keys.device
    rows = max(max_out, 1)                                    # (an empty tensor has no address: with max_out = 0 the call still counts)
    key = torch.empty((rows,), dtype=torch.int64, device=dev)
    count = torch.empty((rows,), dtype=torch.int64, device=dev)
    xyz = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    n = torch.empty((), dtype=torch.int64, device=dev)
    a = L.MapExtractArgs(spec.voxel, spec.log2_capacity, max_out, keys.data_ptr(), acc.data_ptr(), key.data_ptr(), count.data_ptr(),
                         xyz.data_ptr(), n.data_ptr())
    L.call("elo_map_extract", a, keys)
    return key[:max_out], count[:max_out], xyz[:max_out], n


def _ranges_meet(a, b):
    """Two tensors' memory ranges share a byte (an empty tensor shares none)."""
    na, nb = a.numel() * a.element_size(), b.numel() * b.element_size()
    return na > 0 and nb > 0 and a.data_ptr() < b.data_ptr() + nb and b.data_ptr() < a.data_ptr() + na


def _check_map_merge(keys, acc, stats, src_keys, src_acc, spec, centre, radius, min_count):
    """What the host can refuse about a merge without a GPU or the library -> (radius as a float, min_count as an int)."""
    _check_map(keys, acc, spec, stats)
    _check_tensors((("src_keys", src_keys, torch.int64), ("src_acc", src_acc, torch.int64)))
    if src_keys.dim() != 1 or tuple(src_acc.shape) != (src_keys.shape[0], 4):
        raise L.EloError("source rows are src_keys (rows,) and src_acc (rows, 4) (got %s, %s)" % (tuple(src_keys.shape), tuple(src_acc.shape)))
    if src_keys.shape[0] >= 2 ** 31:
        raise L.EloError("rows stays below 2^31 (got %d)" % src_keys.shape[0])
    if src_keys.device != keys.device or src_acc.device != keys.device:
        raise L.EloError("the map and the source rows live on one device")
    if any(_ranges_meet(s, d) for s in (src_keys, src_acc) for d in (keys, acc)):
        raise L.EloError("the source rows overlap the destination table: a table is not merged into itself")
    if isinstance(min_count, bool) or not hasattr(min_count, "__index__") or not 1 <= min_count.__index__() < 2 ** 63:
        raise L.EloError("min_count is an integer >= 1 (got %r)" % (min_count,))
    if centre is None:
        if radius is not None:
            raise L.EloError("a radius needs the centre it is about")
        return 0.0, min_count.__index__()
    _check_tensors((("centre", centre, torch.float64),))
    if centre.numel() != 3:
        raise L.EloError("centre is 3 doubles x y z (got %s)" % (tuple(centre.shape),))
    if centre.device != keys.device:
        raise L.EloError("the map and the centre live on one device")
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not (math.isfinite(radius) and radius > 0):
        raise L.EloError("with a centre, radius is positive and finite (got %r)" % (radius,))
    return float(radius), min_count.__index__()


def map_merge(keys, acc, stats, src_keys, src_acc, spec, centre=None, radius=None, min_count=1):
    """elo_map_merge: the source rows src_keys (rows,), src_acc (rows,4) int64 -- another table's buffers, or the rows of a saved
    state; a key of -1 is an empty slot -- filtered and added into the voxel map (keys, acc, stats, spec as map_insert's) -> report,
    an (8,) int64 device tensor of L.MAP_REPORT.  centre: a contiguous float64 device tensor of 3 elements (a view such as
    world64[4:] qualifies), read when the launch RUNS, with radius (m): rows whose voxel centre lies outside the box are filtered;
    min_count: rows with fewer points are filtered.  One launch on the current stream, no host synchronisation, capturable.  Bad
    types, shapes, layouts, devices and overlap are refused here, before the library is touched."""
    radius, min_count = _check_map_merge(keys, acc, stats, src_keys, src_acc, spec, centre, radius, min_count)
    L.require_gpu(keys, acc, stats, src_keys, src_acc, centre)
    report = torch.zeros((8,), dtype=torch.int64, device=keys.device)
    rows = src_keys.shape[0]
    none = report.data_ptr()                                  # (an empty tensor has no address: rows = 0 reads nothing)
    a = L.MapMergeArgs(rows, src_keys.data_ptr() if rows else none, src_acc.data_ptr() if rows else none, spec.voxel,
                       spec.log2_capacity, keys.data_ptr(), acc.data_ptr(), stats.data_ptr(), _ptr(centre), radius, min_count,
                       report.data_ptr())
    L.call("elo_map_merge", a, keys)
    return report


class MapFitResult(PoseFitResult):
    """What elo_map_fit wrote for a batch: PoseFitResult's fields, with `pose` (B,7) FLOAT64 [q | t], scan -> world, `info` / `grad`
    for the perturbation about the sensor's position (rotation first, then translation), and `match` (B,H,W) int64 -- the key of
    the voxel each cell's term went to at `pose`, -1 where it gave none -- or None."""
    __slots__ = ("match",)

    def __init__(self, pose, info, grad, stats, scratch=None, match=None):
        PoseFitResult.__init__(self, pose, info, grad, stats, scratch)
        self.match = match


def map_fit(keys, acc, xyz, pose64, spec, fit, match=False):
    """elo_map_fit: the range images xyz (B,H,W,3) float32, each at its row of pose64 (B,7) float64 [q | t] (scan -> world), fitted
    against the voxel map (keys (C,), acc (C,4) int64, spec: sensor.VoxelMap; only read) -> MapFitResult.  `fit`: a sensor.MapFit
    (gate None: the map's voxel).  match=True: the per-cell association is written too.  2 (iters + 1) launches on the current
    stream, no host synchronisation, capturable; inputs are contiguous and used in place, and pose64 is read when the launches RUN.
    Bad types, shapes or layouts are refused here, before anything is launched."""
    _check_map(keys, acc, spec)
    if not isinstance(fit, _sensor.MapFit):
        raise TypeError("fit is a MapFit (got %r)" % (type(fit).__name__,))
    gate = fit.gate_for(spec)
    _check_tensors((("xyz", xyz, torch.float32), ("pose64", pose64, torch.float64)))
    if xyz.dim() != 4 or xyz.shape[-1] != 3:
        raise L.EloError("xyz is (B,H,W,3): one range image per scan (got %s)" % (tuple(xyz.shape),))
    B, H, W, _ = xyz.shape
    if H < 3 or W < 1:
        raise L.EloError("a normal needs three rows: H >= 3, W >= 1 (got %d x %d)" % (H, W))
    if B * H * W >= 2 ** 31:
        raise L.EloError("B*H*W stays below 2^31 (got B, H, W = %d, %d, %d)" % (B, H, W))
    if tuple(pose64.shape) != (B, 7):
        raise L.EloError("pose64 is one [q0 q1 q2 q3 | t0 t1 t2] row per scan: (%d, 7) (got %s)" % (B, tuple(pose64.shape)))
    if xyz.device != keys.device or pose64.device != keys.device:
        raise L.EloError("the map, the images and the poses live on one device")
    L.require_gpu(keys, acc, xyz, pose64)
    dev = xyz.device
    words = L.lib().elo_map_fit_scratch_words(B, H, W)
    if words < 0:
        raise L.EloError("elo_map_fit refuses a (%d,%d,%d) batch of images" % (B, H, W))
    res = MapFitResult(torch.empty((B, 7), dtype=torch.float64, device=dev), torch.empty((B, 6, 6), dtype=torch.float32, device=dev),
                       torch.empty((B, 6), dtype=torch.float32, device=dev), torch.empty((B, 4), dtype=torch.float32, device=dev),
                       torch.empty((max(words, 1),), dtype=torch.int32, device=dev),
                       torch.empty((B, H, W), dtype=torch.int64, device=dev) if match else None)
    a = L.MapFitArgs(B, H, W, spec.voxel, spec.log2_capacity, keys.data_ptr(), acc.data_ptr(), xyz.data_ptr(), pose64.data_ptr(),
                     fit.iters, gate, fit.huber, fit.jump_rel, fit.min_count, fit.damping, fit.min_points, res.pose.data_ptr(),
                     res.info.data_ptr(), res.grad.data_ptr(), res.stats.data_ptr(), _ptr(res.match), res.scratch.data_ptr())
    L.call("elo_map_fit", a, keys)
    return res


def _check_context(spec):
    if not isinstance(spec, _sensor.ScanContext):
        raise TypeError("spec is a ScanContext (got %r)" % (type(spec).__name__,))


def _check_descriptors(name, t, spec):
    _check_tensors(((name, t, torch.uint16),))
    if t.dim() != 3 or tuple(t.shape[1:]) != (spec.sectors, spec.rings):
        raise L.EloError("%s is (rows, %d, %d): sectors by rings, sector-major (got %s)" % (name, spec.sectors, spec.rings, tuple(t.shape)))


def scan_descriptor(xyz, spec, out=None):
    """elo_scan_descriptor: the range images xyz (n,H,W,3) float32, W >= spec.sectors -> their descriptors (n, sectors, rings)
    uint16 (spec: sensor.ScanContext), written into `out` where one is given.  One launch on the current stream, no host
    synchronisation, capturable; inputs are contiguous and used in place.  Bad types, shapes, layouts or devices are refused here,
    before the library is touched."""
    _check_context(spec)
    _check_tensors((("xyz", xyz, torch.float32),))
    if xyz.dim() != 4 or xyz.shape[-1] != 3:
        raise L.EloError("xyz is (n,H,W,3): one range image per scan (got %s)" % (tuple(xyz.shape),))
    n, H, W, _ = xyz.shape
    if H < 1 or W < spec.sectors:
        raise L.EloError("a sector needs a column: H >= 1, W >= sectors = %d (got %d x %d)" % (spec.sectors, H, W))
    if n * H * W >= 2 ** 31 or n > 65535:
        raise L.EloError("n*H*W stays below 2^31 and n below 65536 (got n, H, W = %d, %d, %d)" % (n, H, W))
    if out is not None:
        _check_descriptors("out", out, spec)
        if out.shape[0] != n:
            raise L.EloError("out holds one descriptor per image: (%d, %d, %d) (got %s)" % (n, spec.sectors, spec.rings, tuple(out.shape)))
        if out.device != xyz.device:
            raise L.EloError("the images and the descriptors live on one device")
    L.require_gpu(xyz, out)
    if out is None:
        out = torch.empty((n, spec.sectors, spec.rings), dtype=torch.uint16, device=xyz.device)
    if n == 0:
        return out
    edge2 = (ctypes.c_double * (L.PLACE_MAX_RINGS + 1))(*spec.edge2())
    a = L.ScanDescriptorArgs(n, H, W, spec.rings, spec.sectors, spec.z_min, spec.z_step, spec.min_range * spec.min_range, edge2,
                             xyz.data_ptr(), out.data_ptr())
    L.call("elo_scan_descriptor", a, xyz)
    return out


class PlaceSearchResult:
    """What elo_descriptor_search wrote for n queries: `entry` (n,k) int32, `shift` (n,k) int32, `dist` (n,k) float64 -- the k
    nearest entries by (dist, entry), padded with -1, -1, +inf beyond the entries searched -- and the profile they are taken
    from, `best_shift` (n,m) int32 and `best_dist` (n,m) float64: every entry's best shift and its distance."""
    __slots__ = ("entry", "shift", "dist", "best_shift", "best_dist")

    def __init__(self, entry, shift, dist, best_shift, best_dist):
        self.entry, self.shift, self.dist, self.best_shift, self.best_dist = entry, shift, dist, best_shift, best_dist


def descriptor_search(query, db, m, spec, k=1):
    """elo_descriptor_search: the descriptors query (n, sectors, rings) against the entries [0, m) of db (cap, sectors, rings), both
    uint16 (spec: sensor.ScanContext), over every entry and every column shift -> PlaceSearchResult.  m: a python integer in 0 ..
    cap (the caller counts its entries on the host); k: 1 .. 8.  Two launches on the current stream (one where m == 0), no host
    synchronisation, capturable.  Bad types, shapes, layouts, devices, m or k are refused here, before the library is touched."""
    _check_context(spec)
    _check_descriptors("query", query, spec)
    _check_descriptors("db", db, spec)
    if query.device != db.device:
        raise L.EloError("the queries and the database live on one device")
    if isinstance(m, bool) or not hasattr(m, "__index__") or not 0 <= m.__index__() <= db.shape[0] or m.__index__() >= 2 ** 31:
        raise L.EloError("m is an integer in 0 .. %d, the rows db holds (got %r)" % (db.shape[0], m))
    if isinstance(k, bool) or not hasattr(k, "__index__") or not 1 <= k.__index__() <= L.PLACE_MAX_K:
        raise L.EloError("k is an integer in 1 .. %d (got %r)" % (L.PLACE_MAX_K, k))
    m, k, n = m.__index__(), k.__index__(), query.shape[0]
    if n > 65535:
        raise L.EloError("n stays below 65536 (got %d)" % n)
    L.require_gpu(query, db)
    dev = query.device
    res = PlaceSearchResult(torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.int32, device=dev),
                            torch.empty((n, k), dtype=torch.float64, device=dev), torch.empty((n, m), dtype=torch.int32, device=dev),
                            torch.empty((n, m), dtype=torch.float64, device=dev))
    if n == 0:
        return res
    a = L.DescriptorSearchArgs(n, m, spec.rings, spec.sectors, k, query.data_ptr(), db.data_ptr() if m else query.data_ptr(),
                               res.entry.data_ptr(), res.shift.data_ptr(), res.dist.data_ptr(), res.best_shift.data_ptr() if m else None,
                               res.best_dist.data_ptr() if m else None)
    L.call("elo_descriptor_search", a, query)
    return res


class _WarpProject(torch.autograd.Function):
    """elo_warp_project / elo_warp_project_backward.  The forward's scratch (who won each cell) is kept for the backward."""

    @staticmethod
    def forward(ctx, xyz, feat, q, t, H, W, sensor=None):
        B, N, _ = xyz.shape
        C = 0 if feat is None else feat.shape[-1]
        buffers = ProjectionBuffers(B, N, H, W, C, xyz.device)
        warped, out_xyz, out_feat = _warp_project(xyz, feat, q, t, H, W, buffers, sensor)
        ctx.save_for_backward(xyz, q, t, buffers.scratch)
        ctx.dims = (B, N, C, H, W)
        ctx.sensor = sensor
        return warped, out_xyz, out_feat

    @staticmethod
    def backward(ctx, g_warped, g_xyz_proj, g_feat_proj):
        xyz, q, t, scratch = ctx.saved_tensors
        B, N, C, H, W = ctx.dims
        dev, need = xyz.device, ctx.needs_input_grad
        cont = lambda g: None if g is None else _f32(g)[0]
        g_warped, g_xyz_proj, g_feat_proj = cont(g_warped), cont(g_xyz_proj), cont(g_feat_proj)
        g_x = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if need[0] else None
        g_f = torch.empty((B, N, C), dtype=torch.float32, device=dev) if (need[1] and C) else None
        if g_f is not None and g_feat_proj is None:
            g_feat_proj = torch.zeros((B, H, W, C), dtype=torch.float32, device=dev)
        g_q = torch.zeros((B, 4), dtype=torch.float32, device=dev) if q is not None else None
        g_t = torch.zeros((B, 3), dtype=torch.float32, device=dev) if q is not None else None
        az, vres, voff = projection_constants(H, W, ctx.sensor)
        a = L.WarpProjectBwdArgs(B, N, C, H, W, az, vres, voff, xyz.data_ptr(), _ptr(q), _ptr(t), scratch.data_ptr(),
                                 _ptr(g_xyz_proj), _ptr(g_feat_proj), _ptr(g_warped), _ptr(g_x), _ptr(g_f), _ptr(g_q), _ptr(g_t))
        L.call("elo_warp_project_backward", a, xyz)
        return g_x, g_f, g_q, g_t, None, None, None


def warp_project(xyz, feat, q, t, H, W, buffers=None, sensor=None):
    """Optional quaternion warp (q,t: (B,4),(B,3) or None) + ProjectPC2SphericalRing.
    Returns (warped (B,N,3) or None, xyz_proj (B,H,W,3), feat_proj (B,H,W,C) or None).
    `buffers`: a ProjectionBuffers of this call's shape, used (and, if a pose head cleared it, not re-initialised).
    `sensor`: whose field of view the uniform row formula uses (None: the reference's HDL-64E), forward and backward."""
    if buffers is None and _wants_grad(xyz, feat, q, t):
        B = xyz.shape[0]
        if feat is not None and feat.dtype != torch.float32:
            raise TypeError("training stores its features in float32")
        return _WarpProject.apply(_f32(xyz)[0], None if feat is None else feat.contiguous(),
                                  None if q is None else _f32(q.reshape(B, 4))[0],
                                  None if q is None else _f32(t.reshape(B, 3))[0], H, W, sensor)
    return _warp_project(xyz, feat, q, t, H, W, buffers, sensor)


def _warp_project(xyz, feat, q, t, H, W, buffers=None, sensor=None):
    if buffers is not None and buffers.result is not None:   # the pose head that produced (q, t) already did it
        result, buffers.result = buffers.result, None
        return result
    L.require_gpu(xyz, feat, q, t)
    (xyz,) = _f32(xyz)
    B, N, _ = xyz.shape
    C = 0 if feat is None else feat.shape[-1]
    fdt, fcode = torch.float32, L.ELO_F32
    if feat is not None:
        (feat,), fdt, fcode = _feature_dtype(feat)
    if q is not None:
        q, t = _f32(q.reshape(B, 4), t.reshape(B, 3))
    dev = xyz.device
    warped = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if q is not None else None
    if buffers is not None and buffers.shape != (B, N, H, W, C):
        raise ValueError("ProjectionBuffers of shape %s given to a %s projection" % (buffers.shape, (B, N, H, W, C)))
    if buffers is None:
        buffers = ProjectionBuffers(B, N, H, W, C, dev, fdt)
    if buffers.out_feat is not None and buffers.out_feat.dtype != fdt:
        raise TypeError("ProjectionBuffers of dtype %s given to a projection of %s features" % (buffers.out_feat.dtype, fdt))
    out_xyz, out_feat, scratch = buffers.out_xyz, buffers.out_feat, buffers.scratch
    az, vres, voff = projection_constants(H, W, sensor)
    ptr = lambda x: x.data_ptr() if x is not None else None
    a = L.WarpProjectArgs(B, N, C, H, W, az, vres, voff, xyz.data_ptr(), ptr(feat), ptr(q), ptr(t), ptr(warped),
                          out_xyz.data_ptr(), ptr(out_feat), scratch.data_ptr(), 1 if buffers.cleared else 0, fcode)
    buffers.cleared = False                               # single use: the outputs now hold this call's result
    L.call("elo_warp_project", a, out_xyz)
    return warped, out_xyz, out_feat


# ---- training layer: conv2d -> batch norm (batch statistics) -> ReLU (utils/tf_util.py:120-185, :512-563) ----------
def dense_bn_supported(x2, cout):
    """The row-reduction kernels of csrc/elo_train.hip take fp32 (rows, C) matrices on the GPU with C a power of two in 4..256."""
    return x2.is_cuda and x2.dtype == torch.float32 and 4 <= cout <= 256 and cout & (cout - 1) == 0 and x2.shape[0] > 0


def _aligned16(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


def dense_rows_supported(x2, W):
    """elo_dense_rows takes fp32 (rows, Cin) x (Cin, Cout) on the GPU with Cout <= 192, W within 160 KB of LDS and x 16-byte aligned
    (a contiguous view at an offset is not: the library GEMM takes it)."""
    return (x2.is_cuda and x2.dtype == torch.float32 and W.dtype == torch.float32 and x2.shape[0] > 0 and _aligned16(x2)
            and bool(L.lib().elo_dense_rows_supported(x2.shape[0], W.shape[0], W.shape[1]))
            and bool(L.lib().elo_dense_rows_supported(x2.shape[0], W.shape[1], W.shape[0])))


def dense_rows(x2, W, bias=None, transposed=False, moments=None, bn_backward=None, groups=1):
    """x2 @ W + bias ((rows, Cin) x (Cin, Cout)), or x2 @ W.t() with transposed=True ((rows, Cout) x (Cin, Cout)^T), on
    csrc/elo_train_dense.hip.  moments = (eps, momentum, mean, invstd, running_mean, running_var): also the batch-norm moments of
    the result, written into mean / invstd (and the moving averages updated) -- what elo_bn_stats does in a second pass.
    bn_backward = (z, mean, invstd, gamma, beta, sums, relu, dz_out): x2 holds dy of a batch-normalised layer and the operand is that
    layer's dz, formed on the load from dy, z and the two sums of elo_bn_backward(dz=None) and written into dz_out on the way.
    groups > 1: the rows are that many equal blocks with their own batch statistics (mean, invstd (groups, C); sums (groups, 2C))."""
    L.require_gpu(x2, W)
    x2, Wc = x2.contiguous(), W.detach().contiguous()
    cin, cout = (Wc.shape[1], Wc.shape[0]) if transposed else (Wc.shape[0], Wc.shape[1])
    if x2.shape[1] != cin:
        raise ValueError("dense_rows: x is %s, W %s%s" % (tuple(x2.shape), tuple(W.shape), " (transposed)" if transposed else ""))
    out = torch.empty((x2.shape[0], cout), dtype=torch.float32, device=x2.device)
    bias_c = bias.detach().contiguous() if bias is not None else None
    head = (x2.shape[0], cin, cout, x2.data_ptr(), Wc.data_ptr(), 1 if transposed else 0, _ptr(bias_c), out.data_ptr())
    if moments is None:
        bn = (None,) * 6 + (0, None)
        if bn_backward is not None:
            z, mean, invstd, gamma, beta, sums, relu, dz_out = bn_backward
            bn = (z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sums.data_ptr(), 1 if relu else 0, dz_out.data_ptr())
        a = L.DenseRowsArgs(*head, None, 0.0, 0.0, None, None, None, None, *bn, groups)
        L.call("elo_dense_rows", a, x2)
        return out
    eps, momentum, mean, invstd, running_mean, running_var = moments
    scratch = torch.empty((L.lib().elo_dense_rows_scratch_floats(cout, groups),), dtype=torch.float32, device=x2.device)
    a = L.DenseRowsArgs(*head, scratch.data_ptr(), eps, momentum, mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean), _ptr(running_var),
                        None, None, None, None, None, None, 0, None, groups)
    L.call("elo_dense_rows", a, x2)
    return out


class _DenseBN(torch.autograd.Function):
    """y = act(batch_norm(x @ W + b)) with batch statistics.  The two dense products (forward, dx) run on elo_dense_rows where the layer
    has enough rows (tuning.train_dense*; the library GEMM below that); every pass OVER THE ROWS -- the batch moments (from the forward
    product's accumulators on the own kernel), the normalisation, the two sums of batch norm's backward, dz (on the dx kernel's operand
    load where that runs), the weight gradient x^T dz and the bias gradient -- is a hand-written kernel.  Saved for backward: x, W, the
    pre-normalisation z and the moments; the ReLU mask is recomputed from z.  The moving averages are updated in place exactly as
    F.batch_norm(training=True) does.  groups = G > 1: the rows are G equal blocks normalised with their OWN batch statistics (the
    reference calls the layer once per frame with shared variables, pwclo_model.py:117-143; one call on the 2B batch does the same
    arithmetic in half the launches): moments (G, C), moving averages updated G times in order."""

    @staticmethod
    def forward(ctx, x2, W, b, gamma, beta, running_mean, running_var, momentum, eps, relu, groups):
        x2 = x2.contiguous()
        M, C, G = x2.shape[0], W.shape[1], int(groups)
        dev = x2.device
        mean = torch.empty((G * C,), dtype=torch.float32, device=dev)
        invstd = torch.empty((G * C,), dtype=torch.float32, device=dev)
        g, bt = gamma.detach().contiguous(), beta.detach().contiguous()
        ctx.own_dense = bool(tuning.get("train_dense")) and dense_rows_supported(x2, W)
        wide_and_short = W.shape[0] > 128 and M < tuning.get("train_dense_dx_rows")
        if ctx.own_dense and M >= tuning.get("train_dense_rows") and not wide_and_short:
            # the product AND the batch moments in one pass over the rows
            z = dense_rows(x2, W, b, moments=(float(eps), float(momentum), mean, invstd, running_mean, running_var), groups=G)
        else:
            z = torch.addmm(b, x2, W)
            scratch = torch.empty((L.lib().elo_bn_scratch_floats(C, G),), dtype=torch.float32, device=dev)
            L.call("elo_bn_stats", L.BnStatsArgs(M, C, z.data_ptr(), scratch.data_ptr(), float(eps), float(momentum), mean.data_ptr(),
                                                 invstd.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), G), z)
        y = torch.empty_like(z)
        L.call("elo_bn_apply", L.BnApplyArgs(M, C, z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), bt.data_ptr(),
                                             1 if relu else 0, y.data_ptr(), G), z)
        ctx.save_for_backward(x2, W, z, mean, invstd, g, bt)
        ctx.relu = bool(relu)
        ctx.groups = G
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, W, z, mean, invstd, g, bt = ctx.saved_tensors
        (dy,) = _f32(dy)
        if not _aligned16(dy):                  # a contiguous view at an offset: elo_bn_backward (and the fused dx operand) read 16-byte vectors
            dy = dy.clone(memory_format=torch.contiguous_format)
        M, C = z.shape
        G = ctx.groups
        dev = z.device
        scratch = torch.empty((L.lib().elo_bn_scratch_floats(C, G),), dtype=torch.float32, device=dev)
        sums = torch.empty((G * 2 * C,), dtype=torch.float32, device=dev)
        dz = torch.empty_like(z)
        own_dx = ctx.needs_input_grad[0] and ctx.own_dense and M >= tuning.get("train_dense_dx_rows")
        fused = own_dx and tuning.get("train_dense_fused_dz") and _aligned16(mean, invstd, g, bt)
        # (fused: the reduction's two launches only -- dz is formed by the dx kernel on its operand load and written from there)
        L.call("elo_bn_backward", L.BnBackwardArgs(M, C, dy.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g.data_ptr(),
                                                   bt.data_ptr(), 1 if ctx.relu else 0, scratch.data_ptr(), sums.data_ptr(),
                                                   None if fused else dz.data_ptr(), G), z)
        total = sums if G == 1 else sums.view(G, 2 * C).sum(0)
        dbeta, dgamma = total[:C], total[C:]
        dx = None
        if fused:
            dx = dense_rows(dy, W, None, transposed=True, bn_backward=(z, mean, invstd, g, bt, sums, ctx.relu, dz), groups=G)
        elif ctx.needs_input_grad[0]:
            dx = dense_rows(dz, W, None, transposed=True) if own_dx else dz @ W.t()
        cin = W.shape[0]
        dW = torch.empty_like(W, memory_format=torch.contiguous_format)
        db = torch.empty((C,), dtype=torch.float32, device=dev)
        slices = L.lib().elo_weight_grad_slices(M, cin, C)
        wscratch = torch.empty((slices * (cin * C + C),), dtype=torch.float32, device=dev)
        L.call("elo_dense_weight_grad", L.WeightGradArgs(M, cin, C, x2.data_ptr(), dz.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                                         wscratch.data_ptr()), z)
        return dx, dW, db, dgamma, dbeta, None, None, None, None, None, None


def dense_bn(x2, W, b, gamma, beta, running_mean, running_var, momentum, eps, relu, groups=1):
    """(rows, Cin) -> (rows, Cout): the training layer on the kernels above (dense_bn_supported(x2, Cout) must hold).  groups: see _DenseBN."""
    L.require_gpu(x2, W, gamma, running_mean)
    if groups < 1 or x2.shape[0] % groups:
        raise ValueError("dense_bn: %d rows do not split into %d groups" % (x2.shape[0], groups))
    return _DenseBN.apply(x2, W, b, gamma, beta, running_mean, running_var, momentum, eps, relu, groups)

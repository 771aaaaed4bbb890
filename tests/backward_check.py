"""TEST INFRASTRUCTURE of the backward tests (tests/test_backward_gpu.py, tests/test_backward_forms_gpu.py): a hand-written
backward kernel, reached through its autograd Function in efficientlo-net_amd/_ops.py, against torch.autograd over the float64
restatement of tests/twins_torch.py; and cloud points that sit away from every cell border of a spherical range image."""
import numpy as np
import torch

from oracle import ops_np as O


def _check(fn_hip, fn_twin, inputs, wrt, seed=0, tol=1e-4):
    """inputs: list of fp32 tensors / non-tensors; wrt: indices of the tensors to differentiate.  The upstream gradient
    is random; every gradient is compared against the float64 autograd of the twin, relative to its own scale."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    a32 = [x.clone().requires_grad_(True) if i in wrt else x for i, x in enumerate(inputs)]
    a64 = [(x.double().clone().requires_grad_(True) if i in wrt else (x.double() if torch.is_tensor(x) and x.is_floating_point() else x))
           for i, x in enumerate(inputs)]
    out32, out64 = fn_hip(*a32), fn_twin(*a64)
    outs32 = [o for o in (out32 if isinstance(out32, (tuple, list)) else [out32]) if o is not None]
    outs64 = [o for o in (out64 if isinstance(out64, (tuple, list)) else [out64]) if o is not None]
    ups = [torch.randn(o.shape, generator=g).to(o.device) for o in outs32]
    for o32, o64 in zip(outs32, outs64):
        assert torch.allclose(o32.double(), o64, atol=1e-4, rtol=1e-4)
    # an output that depends on none of `wrt` (cv_encode2's xyz_cat when only features are wanted) gets no upstream gradient
    live = [j for j, o in enumerate(outs64) if o.requires_grad]
    g32 = torch.autograd.grad([outs32[j] for j in live], [a32[i] for i in wrt], [ups[j] for j in live], allow_unused=True)
    g64 = torch.autograd.grad([outs64[j] for j in live], [a64[i] for i in wrt], [ups[j].double() for j in live], allow_unused=True)
    for i, a, b in zip(wrt, g32, g64):
        assert (a is None) == (b is None), i
        if a is None:
            continue
        scale = float(b.abs().max()) + 1e-12
        err = float((a.double() - b).abs().max()) / scale
        assert err < tol, "input %d: max err %.3e of scale %.3e" % (i, err, scale)
        assert float(a.abs().max()) > 0, i                       # a real gradient, not zeros against zeros


def _boundary_safe_points(rng, B, N, H, W):
    az_res, vres, voff = (float(x) for x in O.projection_constants(H, W))
    col = rng.integers(0, W, (B, N)) + rng.uniform(0.3, 0.7, (B, N))
    rowf = rng.integers(1, H, (B, N)) + rng.uniform(0.3, 0.7, (B, N))
    az, beta, r = np.pi - col * az_res, (rowf - voff) * vres, rng.uniform(3, 30, (B, N))
    return np.stack([r * np.cos(beta) * np.cos(az), r * np.cos(beta) * np.sin(az), r * np.sin(beta)], -1).astype(np.float32)

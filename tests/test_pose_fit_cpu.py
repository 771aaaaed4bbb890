"""CPU: the float64 statement of the pose fit (tests/pose_fit_reference.py) against closed forms, the PoseFit value, the host's
refusals of _scan_ops.pose_fit (before the library is touched) and the scenes tests/test_pose_fit_gpu.py runs the kernel on: the share
of points the decision-margin filter removes, and the convergence the polish test relies on."""
import math

import numpy as np
import pytest
import torch

import pose_fit_reference as R
from conftest import load_pkg

TRUE = R.retract(np.array([1.0, 0, 0, 0, 0, 0, 0]), np.array([0.004, -0.003, 0.012, -0.7, 0.15, 0.03]))   # frame 1 -> frame 2


def _planes(H=24, W=96, pose=TRUE):
    """Float64 range images of planes -- the ground z = -1.7 seen by the rows below -6 degrees, a wall x = 12 seen above -3
    degrees within 60 degrees of straight ahead, a side wall y = 8 between 65 and 115 degrees (two planes leave the translation
    along their common line free; the third pins it), bands of empty cells between them -- from two sensor poses `pose` apart.
    Every frame-2 cell that has a normal has it from one plane; every frame-1 point lies on one of the planes."""
    q, Rm, t = R.split_pose(pose)
    planes2 = [(np.array([0.0, 0, 1]), -1.7), (np.array([1.0, 0, 0]), 12.0),
               (np.array([0.0, 1, 0]), 8.0)]                                               # n . x = d in frame 2
    planes1 = [(Rm.T @ n, d - n @ t) for n, d in planes2]                                  # n . (R x + t) = d
    step = 26.8 / (H - 1)
    el = np.deg2rad(2.0 + 1.5 * step - np.arange(H) * step)[:, None] * np.ones((1, W))     # mid-row beams (pose_fit_reference.scene)
    az = (math.pi - (np.arange(W) + 0.5) * (2 * math.pi / W))[None, :] * np.ones((H, 1))
    ray = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    pick = np.where(el < np.deg2rad(-6.0), 0, np.where((el > np.deg2rad(-3.0)) & (np.abs(az) < np.deg2rad(60.0)), 1,
                                                           np.where((el > np.deg2rad(-3.0)) & (np.abs(az - math.pi / 2) < np.deg2rad(25.0)), 2, -1)))
    out = []
    for planes in (planes1, planes2):
        img = np.zeros((H, W, 3))
        for k, (n, d) in enumerate(planes):
            with np.errstate(divide="ignore", invalid="ignore"):
                s = d / (ray @ n)
            hit = (pick == k) & (s > 0) & (s < 30.0)
            img[hit] = ray[hit] * s[hit, None]
        out.append(img)
    return out[0], out[1], R.constants(H, W)


def test_planes_have_no_residual_at_the_true_pose():
    x1, x2, c = _planes()
    ev = R.evaluate(x1, x2, TRUE, c, gate=3.0, jump_rel=0.5)
    assert ev["count"] > 300
    assert ev["cost"] < 1e-20 and np.abs(ev["b"]).max() < 1e-9
    assert np.allclose(ev["A"], ev["A"].T) and np.linalg.eigvalsh(ev["A"]).min() > 0      # three planes: all six directions
    off = R.retract(TRUE, np.array([0.002, 0.001, -0.003, 0.05, -0.02, 0.04]))
    assert R.evaluate(x1, x2, off, c, gate=3.0, jump_rel=0.5)["cost"] > 1e-3


def test_jacobian_is_the_derivative_of_the_residual():
    """b = sum J r is the gradient of cost / 2 = sum r^2 / 2 in the left perturbation (rotation first, then translation), with the
    Huber threshold out of reach.  On planes the residual of a point does not depend on WHICH cell of its plane it is matched with,
    so the cost is smooth in the pose and central differences see J alone."""
    x1, x2, c = _planes()
    kw = dict(gate=3.0, jump_rel=0.5, huber=1e9)
    at = R.retract(TRUE, np.array([0.003, -0.002, 0.004, 0.06, 0.03, -0.05]))
    ev = R.evaluate(x1, x2, at, c, **kw)
    h = 1e-6
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        up, down = R.evaluate(x1, x2, R.retract(at, d), c, **kw), R.evaluate(x1, x2, R.retract(at, -d), c, **kw)
        assert up["count"] == down["count"] == ev["count"]
        numeric = (up["cost"] - down["cost"]) / (4 * h)
        assert abs(numeric - ev["b"][i]) <= 1e-6 * max(1.0, ev["absb"][i]), (i, numeric, ev["b"][i])
    # ... and one Gauss-Newton step from there lands on the true pose (the problem is linear in the perturbation to first order)
    new = R.step(at, ev, min_count=10)
    assert R.pose_error(new, TRUE) < 1e-2 * R.pose_error(at, TRUE)


def test_normals_wrap_the_seam_and_skip_the_edge_rows():
    img = np.zeros((5, 8, 3))
    az = math.pi - (np.arange(8) + 0.5) * (2 * math.pi / 8)
    for h in range(5):
        img[h] = np.stack([10 * np.cos(az), 10 * np.sin(az), np.full(8, 1.0 - h)], -1)      # a cylinder of radius 10
    n, valid, _jm, _om = R.normals(img, 0.5)
    assert not valid[0].any() and not valid[4].any() and valid[1:4].all()                 # rows 0 and H-1: none; the seam columns: yes
    radial = img[..., :2] / 10.0
    assert np.allclose(n[1:4, :, :2], -radial[1:4], atol=1e-12) and np.allclose(n[1:4, :, 2], 0)     # inward: towards the sensor
    img[2, 0] = 0.0
    _n, valid, _jm, _om = R.normals(img, 0.5)
    assert not valid[2, 7] and not valid[2, 1] and not valid[1, 0] and not valid[3, 0] and not valid[2, 0]


def test_pose_fit_value():
    S = load_pkg("sensor")
    f = S.PoseFit()
    assert (f.iters, f.gate, f.huber, f.jump_rel, f.min_count, f.damping) == (0, 1.0, 0.1, 0.1, 50, 0.0)
    assert f == S.PoseFit(0, 1, 0.1, 0.1, 50, 0) and hash(f) == hash(S.PoseFit()) and f != S.PoseFit(iters=1)
    assert {f: 1}[S.PoseFit()] == 1 and "iters=0" in repr(f)
    with pytest.raises(AttributeError):
        f.iters = 2
    with pytest.raises(AttributeError):
        del f.gate
    for bad in (dict(iters=-1), dict(iters=1.5), dict(iters=True), dict(gate=0), dict(gate=float("nan")), dict(huber=-0.1),
                dict(huber=float("inf")), dict(jump_rel=-1), dict(min_count=-1), dict(min_count=2.0), dict(damping=-1e-3),
                dict(damping=float("nan"))):
        with pytest.raises(ValueError):
            S.PoseFit(**bad)


def test_host_refusals_come_before_the_library(monkeypatch):
    ops, L, S = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor")

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "lib", no_library)
    x, pose, fit = torch.zeros((2, 8, 16, 3)), torch.zeros((2, 7)), S.PoseFit()
    with pytest.raises(TypeError):
        ops.pose_fit(x, x, pose, None)
    with pytest.raises(TypeError):
        ops.pose_fit(x, x, pose, dict(iters=0))
    with pytest.raises(TypeError):
        ops.pose_fit(x.double(), x, pose, fit)
    with pytest.raises(TypeError):
        ops.pose_fit(x, x, pose.half(), fit)
    with pytest.raises(TypeError):
        ops.pose_fit(x.numpy(), x, pose, fit)
    with pytest.raises(L.EloError, match="contiguous"):
        ops.pose_fit(x.transpose(1, 2), x.transpose(1, 2), pose, fit)
    with pytest.raises(L.EloError, match="contiguous"):
        ops.pose_fit(x, x, torch.zeros((7, 2)).t(), fit)
    with pytest.raises(L.EloError, match="range images"):
        ops.pose_fit(x, x[:, :4].contiguous(), pose, fit)
    with pytest.raises(L.EloError, match="range images"):
        ops.pose_fit(x[..., 0].contiguous(), x[..., 0].contiguous(), pose, fit)
    with pytest.raises(L.EloError, match="H >= 3"):
        ops.pose_fit(x[:, :2].contiguous(), x[:, :2].contiguous(), pose, fit)
    with pytest.raises(L.EloError, match="row per image"):
        ops.pose_fit(x, x, torch.zeros((3, 7)), fit)
    with pytest.raises(L.EloError, match="row per image"):
        ops.pose_fit(x, x, torch.zeros((2, 4)), fit)
    with pytest.raises(TypeError):
        ops.pose_fit(x, x, pose, fit, sensor="hdl64")
    with pytest.raises(L.EloError, match="no CPU fallback"):                            # well-formed, but not on a GPU
        ops.pose_fit(x, x, pose, fit)


@pytest.mark.parametrize("case", range(len(R.SHAPES) + 1))
def test_the_gpu_scenes_lose_few_points_to_the_margin_filter(case):
    if case < len(R.SHAPES):
        B, H, W, starved = R.SHAPES[case]
        x1, x2, poses, c, beam, dropped = R.filtered_case(B, H, W, starved)
    else:
        B, H, W, starved = 2, 16, 128, False
        x1, x2, poses, c, beam, dropped = R.filtered_case(B, H, W, starved, R.BEAMS_DEG)
    assert max(dropped) <= R.DROP_CAP, dropped
    for b in range(B):
        ev = R.evaluate(x1[b], x2[b], poses[b], c, beam_elev=beam, **R.FIT)
        full = x1[b].any(-1)
        assert (ev["safe"] == full).all()                                  # what is left decides with room to spare
        if starved and b == B - 1:
            assert ev["count"] == 0
        else:
            assert ev["count"] >= 50 and ev["count"] >= 0.15 * full.sum()


def test_the_polish_scene_converges_as_the_gpu_test_needs():
    """tests/test_pose_fit_gpu.py asks the kernel after k steps to be no further from the reference's fixed point than the
    reference after k - 1: that leaves room for float32's association flips only if the reference's step k at least halves its
    error.  k = 2 at 32 x 256."""
    for b in range(2):
        fixed, start, errs = R.polish_case(b)
        assert errs[0] > 0.3                                               # 0.1 m + 0.76 degrees at the 20 m lever
        assert errs[R.POLISH_K] <= 0.5 * errs[R.POLISH_K - 1], errs
        assert errs[R.POLISH_K - 1] < 0.2 * errs[0], errs

"""GPU: elo_model_render (csrc/elo_model.hip) against the float64 statement of tests/local_model_reference.py, its decisions by
hand, its determinism and refusals, and the tracker built on it (local_model.ModelTracker; evaluate.predict_sequence(model=)).

The render cases are the ones tests/test_local_model_cpu.py vets: on every cell the reference does not call ambiguous the kernel
names the same winner, and its point lies within one float32 ulp of the point's largest component of the reference's unrounded
p' (the kernel rounds a double p' once: half an ulp of the component; its double arithmetic may differ from numpy's in the last
bits of the double, which can move that rounding by one float32 ulp, no more)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import local_model_reference as M
import pose_fit_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
bits = lambda x: x.contiguous().view(torch.int32)


def _sensor(beam):
    return None if beam is None else load_pkg("sensor").Sensor(beam_elevations_deg=R.BEAMS_DEG)


def _render(src, pose, beam=None):
    xyz, idx = load_pkg("_scan_ops").model_render(t(src), t(pose), sensor=_sensor(beam))
    torch.cuda.synchronize()
    return xyz.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("i", range(len(M.CASES)))
def test_render_against_float64(i):
    B, K, H, W, _beams = M.CASES[i]
    src, pose, _c, beam, want = M.rendered_case(i)
    xyz, idx = _render(src, pose, beam)
    assert np.isfinite(xyz).all() and ((idx >= -1) & (idx < K * H * W)).all()
    for b, w in enumerate(want):
        ok = ~w["ambiguous"]
        filled, empty = ok & (w["src_idx"] >= 0), ok & (w["src_idx"] < 0)
        err = np.abs(xyz[b][filled].astype(np.float64) - w["xyz"][filled]) / M.ulp_of_largest(w["xyz"][filled])
        print("case %d image %d: %d cells compared (%d filled), %d winners differ, worst point %.3f ulp of its largest component" % (
            i, b, ok.sum(), filled.sum(), (idx[b][ok] != w["src_idx"][ok]).sum(), err.max()))
        assert (idx[b][ok] == w["src_idx"][ok]).all()
        assert (err <= 1.0).all()
        assert (idx[b][empty] == -1).all() and not xyz[b][empty].view(np.int32).any()    # zeros, every bit
    if beam is not None:                                                                # the uniform formula puts these beams into other rows
        _xyz, plain = _render(src, pose)
        assert not np.array_equal(plain, idx)


def _cloud_images(H, W, n=4000, seed=11):
    """(2,H,W,3): the two range images _ops.input_stage writes from a random cloud of 2 n points inside the field of view."""
    rng = np.random.default_rng(seed)
    az, el = rng.uniform(-math.pi, math.pi, 2 * n), np.deg2rad(rng.uniform(-24.0, 1.5, 2 * n))
    r = rng.uniform(3.0, 30.0, 2 * n)
    cloud = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1).astype(np.float32)[None]
    _points, images = load_pkg("_ops").input_stage(t(cloud), None, None, H, W)
    torch.cuda.synchronize()
    return images


def test_identity_returns_the_image_bit_for_bit():
    H, W = 16, 128
    ops = load_pkg("_scan_ops")
    own = torch.arange(H * W, dtype=torch.int32, device=DEV).reshape(1, H, W)
    f1, _f2 = R.scene(1, H, W, seed=21)
    for name, images in (("input stage", _cloud_images(H, W)), ("scene", t(f1))):
        B = images.shape[0]
        full = (images != 0).any(-1)
        assert 0.3 < float(full.float().mean()) < 0.99, name
        xyz, idx = ops.model_render(images.reshape(B, 1, H, W, 3).contiguous(), t(np.tile(IDENTITY, (B, 1, 1))))
        torch.cuda.synchronize()
        assert torch.equal(bits(xyz), bits(images)), name
        assert torch.equal(idx, torch.where(full, own.expand(B, H, W), torch.full_like(idx, -1))), name


def _ray(h, w, H, W):
    """The unit vector through the middle of cell (h, w) of the uniform projection (pose_fit_reference.scene's beams)."""
    step = 26.8 / (H - 1)
    el, az = np.deg2rad(2.0 + 1.5 * step - h * step), math.pi - (w + 0.5) * (2 * math.pi / W)
    return np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])


@pytest.mark.parametrize("bad_q", (0.0, float("nan"), float("inf")))
def test_decisions_by_hand(bad_q):
    H, W, K = 8, 64, 5
    src = np.zeros((1, K, H, W, 3), np.float32)
    pose = np.tile(IDENTITY, (1, K, 1))
    far, near = (12.0 * _ray(3, 10, H, W)).astype(np.float32), (10.0 * _ray(3, 10, H, W)).astype(np.float32)
    same = (7.0 * _ray(5, 33, H, W)).astype(np.float32)
    src[0, 0, 3, 10], src[0, 1, 6, 20] = far, near            # two sources reach cell (3,10) at ranges 12 and 10: the nearer wins
    src[0, 0, 5, 33], src[0, 1, 1, 2] = same, same            # the same point in two sources: the lower k wins (not the lower cell)
    #                                                           source 2 is all zeros: it gives nothing
    src[0, 3, 4, 40] = (9.0 * _ray(4, 40, H, W)).astype(np.float32)
    pose[0, 3, :4] = bad_q                                    # a quaternion without a direction skips its source
    gone = (8.0 * _ray(2, 50, H, W)).astype(np.float32)
    src[0, 4, 2, 50] = gone
    pose[0, 4, 4:] = -gone                                    # t = -p under the identity rotation: the point lands on (0,0,0) and is dropped
    xyz, idx = _render(src, pose)
    assert np.isfinite(xyz).all()
    want_idx = np.full((H, W), -1, np.int32)
    want_xyz = np.zeros((H, W, 3), np.float32)
    want_idx[3, 10], want_xyz[3, 10] = (1 * H + 6) * W + 20, near
    want_idx[5, 33], want_xyz[5, 33] = (0 * H + 5) * W + 33, same
    assert np.array_equal(idx[0], want_idx)
    assert np.array_equal(xyz[0].view(np.int32), want_xyz.view(np.int32))
    xyz, idx = _render(np.zeros((2, 3, H, W, 3), np.float32), np.tile(IDENTITY, (2, 3, 1)))      # nothing at all
    assert (idx == -1).all() and not xyz.view(np.int32).any()


def test_two_calls_and_a_graph_replay_agree_bit_for_bit():
    ops = load_pkg("_scan_ops")
    src, pose, _c, _beam, _want = M.rendered_case(0)
    src_d, pose_d = t(src), t(pose)
    a, b = ops.model_render(src_d, pose_d), ops.model_render(src_d, pose_d)
    torch.cuda.synchronize()
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ops.model_render(src_d, pose_d)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        xyz, idx = ops.model_render(src_d, pose_d)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(xyz), bits(a[0])) and torch.equal(idx, a[1])
    moved = pose.copy()
    moved[..., 4:] += np.float32(0.25)
    moved[:, 0, :4] = R.retract(pose[0, 0].astype(np.float64), np.array([0.0, 0.0, 0.03, 0, 0, 0]))[:4]
    pose_d.copy_(t(moved))                                    # in place: the launches read the pose when they RUN
    g.replay()
    torch.cuda.synchronize()
    c = ops.model_render(src_d, t(moved))
    torch.cuda.synchronize()
    assert torch.equal(bits(xyz), bits(c[0])) and torch.equal(idx, c[1])
    assert not torch.equal(idx, a[1])


def test_abi_refusals_launch_nothing():
    L = load_pkg("_lib")
    lib = L.lib()
    B, K, H, W = 1, 2, 8, 64
    src = torch.ones((B, K, H, W, 3), device=DEV)
    pose = t(np.tile(IDENTITY, (B, K, 1)))
    beam = torch.linspace(0.1, -0.4, 300, device=DEV)
    out_xyz = torch.full((B, H, W, 3), -7.0, device=DEV)
    out_src = torch.full((B, H, W), -7, dtype=torch.int32, device=DEV)
    words = lib.elo_model_render_scratch_words(B, H, W)
    assert words >= 2 * B * H * W
    scratch = torch.full((words,), -7, dtype=torch.int32, device=DEV)
    az, vres, voff = R.constants(H, W)

    def args(**kw):
        a = L.ModelRenderArgs(B, K, H, W, az, vres, voff, src.data_ptr(), pose.data_ptr(), None, out_xyz.data_ptr(), out_src.data_ptr(),
                              scratch.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = L.stream_ptr(src)
    for bad in (dict(src=None), dict(pose=None), dict(out_xyz=None), dict(out_src=None), dict(scratch=None), dict(K=0), dict(K=17),
                dict(H=0), dict(W=0), dict(H=300, beam_elev=beam.data_ptr()), dict(K=16, H=1 << 14, W=1 << 13),
                dict(batch=16, K=1, H=1 << 14, W=1 << 13), dict(out_xyz=src.data_ptr()),
                dict(out_xyz=src.data_ptr() + 12 * H * W)):                             # (the second source: inside src)
        assert lib.elo_model_render(ctypes.byref(args(**bad)), stream) == -1, bad       # ELO_ERR_ARG
        assert b"elo_model_render" in lib.elo_last_error()
    torch.cuda.synchronize()
    assert (out_xyz == -7.0).all() and (out_src == -7).all() and (scratch == -7).all()  # nothing ran
    assert lib.elo_model_render_scratch_words(B, 0, W) < 0 and lib.elo_model_render_scratch_words(16, 1 << 14, 1 << 13) < 0
    assert lib.elo_model_render(ctypes.byref(args()), stream) == 0                      # the same block, mended, runs
    torch.cuda.synchronize()
    assert torch.isfinite(out_xyz).all() and not (out_xyz == -7.0).any() and not (out_src == -7).any()


def _same_result(a, b):
    return all(torch.equal(bits(u), bits(v)) for u, v in zip((a.pose, a.info, a.grad, a.stats), (b.pose, b.info, b.grad, b.stats)))


def test_tracker_on_the_box_scene():
    """Six half-empty scans of the box, PoseFit(iters=2), from the true poses rounded to float32.  scans=1 is the pair fit, bit for
    bit; scans=4 is a by-hand render + fit over the same ring, and from the third step on it has the terms the pair fit lacks."""
    ops, S, L, lm = load_pkg("_scan_ops"), load_pkg("sensor"), load_pkg("_lib"), load_pkg("local_model")
    fit = S.PoseFit(iters=2, **R.FIT)
    H, W = M.BOX_H, M.BOX_W
    pairs = [(t(x1[None]), t(x2[None]), t(p[None])) for x1, x2, p in M.box_pairs()]
    one, four = lm.ModelTracker(H, W, S.LocalModel(1), fit, device=DEV), lm.ModelTracker(H, W, S.LocalModel(4), fit, device=DEV)
    ring = torch.zeros((1, 4, H, W, 3), device=DEV)
    poses = torch.tensor(np.tile(IDENTITY, (4, 1)), dtype=torch.float64, device=DEV)
    poses_np = poses.cpu().numpy()
    ring[0, 0] = pairs[0][1][0]                               # the first frame 2 starts the model, at the identity
    entered = 1
    for n, (x1, x2, pose7) in enumerate(pairs):
        pair = ops.pose_fit(x1, x2, pose7, fit)
        r1, r4 = one.step(x1, x2, pose7), four.step(x1, x2, pose7)
        model, _src = ops.model_render(ring, poses.to(torch.float32).reshape(1, 4, 7).contiguous())
        hand = ops.pose_fit(x1, model, pose7, fit)
        torch.cuda.synchronize()
        assert _same_result(r1, pair), n
        assert _same_result(r4, hand), n
        c1, c4, s1, s4 = (int(v) for v in (r1.count[0], r4.count[0], r1.status[0], r4.status[0]))
        print("step %d: %d scans held; terms %d against the pair, %d against the model; status %d / %d" % (n, min(entered, 4), c1, c4, s1, s4))
        if n >= 2:
            assert c4 > c1 and s4 == 0 and (s1 & L.FIT_FEW)
        poses = lm.rebase(poses, hand.pose[0])                # float64, then scan n enters at the identity over the oldest
        poses_np = M.rebase(poses_np, hand.pose[0].cpu().numpy())
        ring[0, entered % 4] = x1[0]
        poses[entered % 4] = torch.tensor(IDENTITY, dtype=torch.float64, device=DEV)
        poses_np[entered % 4] = IDENTITY
        entered += 1
        assert np.abs(poses.cpu().numpy() - poses_np).max() <= 1e-12
        assert torch.equal(four.poses64, poses) and torch.equal(bits(four.ring), bits(ring[0]))
    four.reset()
    assert four.entered == 0 and not four.ring.any() and torch.equal(four.poses64[:, 0], torch.ones(4, dtype=torch.float64, device=DEV))
    again = four.step(*pairs[0])                              # after reset(): the first step again, every bit
    torch.cuda.synchronize()
    assert _same_result(again, ops.pose_fit(*pairs[0], fit))


def test_through_evaluate_one_scan_is_the_pair_fit(tmp_path):
    """predict_sequence(fit=, model=LocalModel(1)) gives the poses of fit= alone -- also across a gap in `frames`, where only a
    reset() keeps the model from being the wrong scan."""
    import kitti_tree
    model, ev, S = load_pkg("model"), load_pkg("evaluate"), load_pkg("sensor")
    H, W, n = 64, 900, 5
    T_diff = kitti_tree.write_sequence(str(tmp_path), "04", n, H, W)
    net = model.PWCLONet(DEV, seed=0)
    fit = S.PoseFit(iters=1)
    for frames in (None, [0, 1, 3, 4]):
        kw = dict(H_input=H, W_input=W, num_points=H * W, batch_size=2, frames=frames, fit=fit)
        q0, t0, f0 = ev.predict_sequence(net, str(tmp_path), "04", T_diff, **kw)
        q1, t1, f1 = ev.predict_sequence(net, str(tmp_path), "04", T_diff, model=S.LocalModel(1), **kw)
        assert q1.shape == q0.shape == (n if frames is None else len(frames), 4) and f1.shape == f0.shape
        assert np.array_equal(q1, q0) and np.array_equal(t1, t0) and np.array_equal(f1, f0)
        assert (f0[:, 0] >= 50).all()                                                   # (the fit did run: these scans are dense)

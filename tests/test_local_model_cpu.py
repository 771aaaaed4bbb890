"""CPU: the LocalModel value, the host's refusals of _scan_ops.model_render (before the library is touched), predict_sequence's argument
errors, local_model.rebase, and the scenes tests/test_local_model_gpu.py runs the kernel on -- the share of cells the float64
statement (tests/local_model_reference.py) calls ambiguous, and the box-scene term counts the tracker test relies on."""
import numpy as np
import pytest
import torch

import local_model_reference as M
import pose_fit_reference as R
from conftest import load_pkg


def test_local_model_value():
    S = load_pkg("sensor")
    m = S.LocalModel()
    assert m.scans == 4 and m == S.LocalModel(4) and hash(m) == hash(S.LocalModel(scans=4)) and m != S.LocalModel(3)
    assert {m: 1}[S.LocalModel()] == 1 and "scans=4" in repr(m) and m != S.PoseFit()
    assert S.LocalModel(np.int64(16)).scans == 16 and S.LocalModel(1).scans == 1
    with pytest.raises(AttributeError):
        m.scans = 2
    with pytest.raises(AttributeError):
        del m.scans
    for bad in (0, 17, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError):
            S.LocalModel(bad)


def test_host_refusals_come_before_the_library(monkeypatch):
    ops, L, S = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor")

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "lib", no_library)
    src, pose = torch.zeros((2, 3, 8, 16, 3)), torch.zeros((2, 3, 7))
    with pytest.raises(TypeError):
        ops.model_render(src.double(), pose)
    with pytest.raises(TypeError):
        ops.model_render(src, pose.half())
    with pytest.raises(TypeError):
        ops.model_render(src.numpy(), pose)
    with pytest.raises(L.EloError, match="contiguous"):
        ops.model_render(src.transpose(2, 3), pose)
    with pytest.raises(L.EloError, match="contiguous"):
        ops.model_render(src, torch.zeros((2, 7, 3)).transpose(1, 2))
    with pytest.raises(L.EloError, match="B,K,H,W,3"):
        ops.model_render(src[:, 0].contiguous(), pose)
    with pytest.raises(L.EloError, match="B,K,H,W,3"):
        ops.model_render(torch.zeros((2, 3, 8, 16, 4)), pose)
    with pytest.raises(L.EloError, match="1 .. 16 scans"):
        ops.model_render(torch.zeros((1, 17, 4, 4, 3)), torch.zeros((1, 17, 7)))
    with pytest.raises(L.EloError, match="1 .. 16 scans"):
        ops.model_render(torch.zeros((1, 0, 4, 4, 3)), torch.zeros((1, 0, 7)))
    with pytest.raises(L.EloError, match="no cells"):
        ops.model_render(torch.zeros((1, 2, 0, 4, 3)), torch.zeros((1, 2, 7)))
    with pytest.raises(L.EloError, match="row per source"):
        ops.model_render(src, torch.zeros((2, 7)))
    with pytest.raises(L.EloError, match="row per source"):
        ops.model_render(src, torch.zeros((2, 4, 7)))
    with pytest.raises(L.EloError, match="at most 256 beams"):
        ops.model_render(torch.zeros((1, 1, 300, 2, 3)), torch.zeros((1, 1, 7)), beam_elev=np.linspace(0.1, -0.4, 300))
    with pytest.raises(TypeError):
        ops.model_render(src, pose, sensor="hdl64")
    with pytest.raises(L.EloError, match="no CPU fallback"):                            # well-formed, but not on a GPU
        ops.model_render(src, pose)
    with pytest.raises(TypeError):                                                      # the tracker's values, before any tensor
        load_pkg("local_model").ModelTracker(8, 16, 4, S.PoseFit(), device="cpu")
    with pytest.raises(TypeError):
        load_pkg("local_model").ModelTracker(8, 16, S.LocalModel(), dict(iters=1), device="cpu")


def test_predict_sequence_argument_errors():
    ev, S = load_pkg("evaluate"), load_pkg("sensor")
    with pytest.raises(ValueError, match="fit"):
        ev.predict_sequence(None, "/nowhere", "00", None, model=S.LocalModel())
    with pytest.raises(NotImplementedError):
        ev.predict_sequence(None, "/nowhere", "00", None, fit=S.PoseFit(iters=1), model=S.LocalModel(), lanes=2)
    with pytest.raises(TypeError):
        ev.predict_sequence(None, "/nowhere", "00", None, fit=S.PoseFit(iters=1), model=4)


def test_rebase_carries_points_alike():
    """A point carried by the old P_j and then by T^-1 equals the point carried by the new P_j."""
    lm = load_pkg("local_model")
    rng = np.random.default_rng(3)
    poses = np.concatenate([rng.normal(size=(5, 4)), rng.normal(size=(5, 3)) * 3], 1)
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1, keepdims=True)
    poses[0] = (1, 0, 0, 0, 0, 0, 0)
    T = R.retract(np.array([1.0, 0, 0, 0, 0, 0, 0]), np.array([0.02, -0.01, 0.3, -0.8, 0.1, 0.02]))
    T[:4] *= 1.7                                                   # (a pose's quaternion is normalised where it is used)
    new = lm.rebase(torch.from_numpy(poses), torch.from_numpy(T.astype(np.float32)))
    assert new.dtype == torch.float64 and tuple(new.shape) == (5, 7)
    new = new.numpy()
    assert np.allclose(np.linalg.norm(new[:, :4], axis=1), 1.0, atol=1e-15)
    assert np.abs(new - M.rebase(poses, T.astype(np.float32))).max() <= 1e-12           # the numpy statement the GPU test rebases by
    _q, RT, tT = R.split_pose(T.astype(np.float32))
    pts = rng.normal(size=(40, 3)) * 10
    for j in range(5):
        _qo, Ro, to = R.split_pose(poses[j])
        _qn, Rn, tn = R.split_pose(new[j])
        old_then_back = ((pts @ Ro.T + to) - tT) @ RT                                   # T^-1 p = R^T (p - t)
        assert np.abs(old_then_back - (pts @ Rn.T + tn)).max() <= 1e-12
    assert np.abs(lm.rebase(poses, [1, 0, 0, 0, 0, 0, 0]).numpy() - poses).max() <= 1e-15   # array-likes, and the identity


@pytest.mark.parametrize("i", range(len(M.CASES)))
def test_the_gpu_render_cases_are_mostly_unambiguous(i):
    B, K, H, W, _beams = M.CASES[i]
    src, pose, _c, _beam, want = M.rendered_case(i)
    t = np.linalg.norm(pose[..., 4:], axis=-1)
    qn = pose[..., :4] / np.linalg.norm(pose[..., :4], axis=-1, keepdims=True)
    ang = 2 * np.arccos(np.minimum(np.abs(qn[..., 0]), 1.0))                            # (of q or -q)
    turned = np.zeros((B, K), bool)
    turned[:, K - 1] = K > 1
    assert (t <= 1.0).all() and (np.rad2deg(ang[~turned]) <= 3.0).all() and (np.rad2deg(ang[turned]) > 170.0).all()
    for b, w in enumerate(want):
        share = w["ambiguous"].mean()
        print("case %d image %d: %d points, %.1f %% of the cells filled, %.2f %% ambiguous" % (
            i, b, w["points"], 100 * (w["src_idx"] >= 0).mean(), 100 * share))
        assert share <= M.DROP_CAP
        assert (w["src_idx"] >= 0).mean() > 0.5
        if K > 1:                                                                      # every source wins somewhere
            assert set(np.unique(w["src_idx"][w["src_idx"] >= 0] // (H * W))) == set(range(K))


def test_a_turned_source_crosses_the_seam():
    """The source turned by ~180 degrees puts the points of its columns around W/2 into the columns at the seam."""
    B, K, H, W, _ = M.CASES[0]
    _src, _pose, _c, _beam, want = M.rendered_case(0)
    idx = want[0]["src_idx"]
    for col in (0, W - 1):
        from_turned = idx[:, col][idx[:, col] // (H * W) == K - 1] % W
        assert len(from_turned) and (np.abs(from_turned - W / 2) < W / 8).all()


def test_identity_keeps_every_cell_in_the_reference():
    f1, _f2 = R.scene(1, 16, 128, seed=21)
    got = M.render(f1, np.array([[1, 0, 0, 0, 0, 0, 0]], np.float32), R.constants(16, 128))
    own = np.where(f1[0].any(-1), np.arange(16 * 128).reshape(16, 128), -1)
    assert (got["src_idx"] == own).all() and not got["ambiguous"].any()
    assert np.array_equal(got["xyz"].astype(np.float32), f1[0])


def test_the_box_scene_counts_the_tracker_test_relies_on():
    """Half-empty scans: the pair fit finds fewer terms than min_count = 50 at every step; against four scans it finds >= 100 from
    the third step on.  (Measured with this generator: 20 - 24 for the pair fit; 293 with three scans held, 388 - 431 with four.)"""
    pairs = M.box_pairs()
    c = R.constants(M.BOX_H, M.BOX_W)
    for x1, _x2, _p in pairs:
        assert 0.4 < x1.any(-1).mean() < 0.6
    one, four = M.track_counts(pairs, 1, c), M.track_counts(pairs, 4, c)
    print("pair fit:", one, " four scans:", four)
    assert all(count < 50 for count, _held, _amb in one)
    assert [held for _c, held, _a in four] == [1, 2, 3, 4, 4]
    assert all(count >= 100 for count, _held, _amb in four[2:])
    assert all(amb <= M.DROP_CAP for _c, _h, amb in one + four)
    # pair n's frame 2 is pair n-1's frame 1: the direction the tracker assumes
    assert all(pairs[n][1] is pairs[n - 1][0] for n in range(1, len(pairs)))

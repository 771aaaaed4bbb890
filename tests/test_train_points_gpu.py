"""GPU: training from raw clouds -- elo_preprocess_gt against float64, the input stage reading a device aug_frame,
Trainer.step_points against Trainer.step, the captured step from clouds reading all five of its inputs, and
training.train_epoch over a synthetic KITTI tree."""
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_pkg
from kitti_tree import TR, write_sequence
from util_params import shuffle_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


def _gt_float64(T_gt, T_trans, T_trans_inv, aug):
    """model_util.py:403, :419, :427-445 in float64 numpy, on the float32 inputs the device sees:
    -> (q_gt (B,4), t_gt (B,3), cy (B))."""
    qs, ts, cys = [], [], []
    for b in range(len(T_gt)):
        G = T_gt[b].astype(np.float64)
        if aug[b] == 2:
            T = T_trans[b].astype(np.float64) @ G
        elif aug[b] == 1:
            T = G @ T_trans_inv[b].astype(np.float64)
        else:
            T = G
        cy = np.sqrt(T[2, 2] * T[2, 2] + T[1, 2] * T[1, 2])                       # mat2euler, :130-142
        z, y, x = np.arctan2(-T[0, 1], T[0, 0]) / 2, np.arctan2(T[0, 2], cy) / 2, np.arctan2(-T[1, 2], T[2, 2]) / 2
        cz, sz, cyh, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
        qs.append([cx * cyh * cz - sx * sy * sz, cx * sy * sz + cyh * cz * sx,     # euler2quat, :112-127
                   cx * cz * sy - sx * cyh * sz, cx * cyh * sz + sx * cz * sy])
        ts.append(T[:3, 3])
        cys.append(cy)
    return np.array(qs), np.array(ts), np.array(cys)


def _kitti_gt(B, start=40, stride=27):
    """B ground-truth transforms of KITTI sequence 04 in the LiDAR frame (kitti.ground_truth_transform of the golden
    frame-to-frame motions), fp32 as the step feeds them."""
    kitti = load_pkg("kitti")
    diff = np.load(os.path.join(GOLDEN, "kitti_seq04_gt.npz"))["diff"]
    return f32(np.stack([kitti.ground_truth_transform(diff[start + stride * i], TR) for i in range(B)]))


def _augmentations(B, seed):
    training = load_pkg("training")
    rng = np.random.default_rng(seed)
    T = np.stack([training.data_augmentation(rng) for _ in range(B)])
    return f32(T), f32(np.linalg.inv(T))


def test_preprocess_gt_kernel_against_float64():
    """elo_preprocess_gt (one launch) on B = 8 KITTI ground-truth motions with seeded data_augmentation matrices, the frame
    choice mixing 0 (T = T_gt), 1 (T_gt . T_trans_inv) and 2 (T_trans . T_gt), plus the call without matrices, against the
    same formulas in float64 numpy.  The bound is not a constant: the float32 torch chain model_util.preprocess_gt is measured
    against the same float64 values on the same inputs, and the kernel may be at most twice as far off, for q_gt and for t_gt.
    mat2euler has no gimbal branch here or in the reference (model_util.py:130-142: cy only feeds atan2), but the Euler round
    trip loses its meaning where cy -> 0; the inputs are asserted to sit far from there (cy > 0.9), so the comparison
    is of the regular case it claims to be.
    The kernel computes in double and rounds each output once, so its error is bounded by half an fp32 ulp of the output
    (2.98e-08 for |q| < 1).  The test prints the four errors before it asserts.
    Measured on an MI355X (max abs error against float64 over both calls): q_gt kernel 2.703e-08, torch fp32 chain 5.374e-08;
    t_gt kernel 9.757e-08, torch 9.757e-08 (the largest |t_gt| is 2.04: half an ulp there, for both)."""
    ops, mu = load_pkg("_ops"), load_pkg("model_util")
    B = 8
    T_gt = _kitti_gt(B)
    T_tr, T_inv = _augmentations(B, seed=11)
    aug = np.array([1, 2, 0, 2, 1, 0, 2, 1], np.int32)
    eye, zero = f32(np.tile(np.eye(4), (B, 1, 1))), np.zeros(B, np.int32)
    want_q, want_t, cy = _gt_float64(T_gt, T_tr, T_inv, aug)
    plain_q, plain_t, cy0 = _gt_float64(T_gt, eye, eye, zero)
    assert min(cy.min(), cy0.min()) > 0.9                                         # far from the degenerate Euler case
    assert np.abs(want_q - plain_q).max() > 1e-3 and np.abs(want_t - plain_t).max() > 1e-2    # the augmentation is in the answer
    got_q, got_t = ops.preprocess_gt(t(T_gt), t(T_tr), t(T_inv), t(aug))
    got_q0, got_t0 = ops.preprocess_gt(t(T_gt), None, None, None)
    assert got_q.shape == (B, 4) and got_t.shape == (B, 3) and got_q.dtype == got_t.dtype == torch.float32
    ref_q, ref_t = mu.preprocess_gt(t(T_gt), t(T_tr), t(T_inv), aug)
    ref_q0, ref_t0 = mu.preprocess_gt(t(T_gt), t(eye), t(eye), zero)
    err = lambda a, a0, w, w0: max(float(np.abs(a.double().cpu().numpy().reshape(w.shape) - w).max()),
                                   float(np.abs(a0.double().cpu().numpy().reshape(w0.shape) - w0).max()))
    kq, kt = err(got_q, got_q0, want_q, plain_q), err(got_t, got_t0, want_t, plain_t)
    tq, tt = err(ref_q, ref_q0, want_q, plain_q), err(ref_t, ref_t0, want_t, plain_t)
    print("elo_preprocess_gt against float64: q_gt %.3e (torch fp32 chain %.3e), t_gt %.3e (torch %.3e)" % (kq, tq, kt, tt))
    assert tq < 1e-5 and tt < 1e-5                                                # the yardstick itself is sane
    assert kq <= 2 * tq and kt <= 2 * tt
    # without matrices t_gt is T_gt's column, exactly
    assert np.array_equal(got_t0.cpu().numpy(), T_gt[:, :3, 3])


def _cloud(B, N, seed, stride=3):
    """(B, 2N, stride) LiDAR-like cloud: ranges to 60 m (the 35 m crop bites), 5 % zero padding."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, (B, 2 * N))
    el = np.deg2rad(rng.uniform(-24.8, 2.0, (B, 2 * N)))
    r = rng.uniform(2.0, 60.0, (B, 2 * N))
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.sin(az) * np.cos(el), r * np.sin(el)], -1)
    xyz[rng.random((B, 2 * N)) < 0.05] = 0
    out = np.zeros((B, 2 * N, stride), np.float32)
    out[..., :3] = xyz
    return out


def test_input_stage_reads_a_device_aug_frame():
    """_ops.input_stage with aug_frame as an int32 tensor on the cloud's device: bit-equal to the array-like path, points and
    projections, with frame 1 and frame 2 augmented in the same batch -- and the launch reads the tensor it was given (rewritten
    in place, the same call gives the other answer)."""
    ops = load_pkg("_ops")
    B, N, H, W = 4, 5000, 16, 225
    cloud = t(_cloud(B, N, seed=4, stride=4))
    T_tr, _ = _augmentations(B, seed=12)
    aug = np.array([1, 2, 2, 1], np.int32)
    want_pts, want_proj = ops.input_stage(cloud, t(T_tr), aug, H, W)
    aug_dev = t(aug)
    got_pts, got_proj = ops.input_stage(cloud, t(T_tr), aug_dev, H, W)
    assert torch.equal(got_pts, want_pts) and torch.equal(got_proj, want_proj)
    flipped_pts, flipped_proj = ops.input_stage(cloud, t(T_tr), 3 - aug, H, W)
    assert not torch.equal(flipped_pts, want_pts)
    aug_dev.copy_(t(3 - aug))
    got_pts, got_proj = ops.input_stage(cloud, t(T_tr), aug_dev, H, W)
    assert torch.equal(got_pts, flipped_pts) and torch.equal(got_proj, flipped_proj)
    with pytest.raises(ValueError):
        ops.input_stage(cloud, t(T_tr), t(np.ones(B + 1, np.int32)), H, W)


H_IN, W_IN, N_PTS = 64, 900, 64 * 900


def _scene(B, seed):
    """A fixed synthetic pair as raw clouds: the points of two range images of one scene 0.8 m apart (zero padded to
    N_PTS per frame), and the motion between them."""
    synth = load_pkg("synth")
    f1, f2 = synth.frame_pair(B, H_IN, W_IN, seed=seed)
    cloud = np.zeros((B, 2 * N_PTS, 3), np.float32)
    for b in range(B):
        for half, img in enumerate((f1[b], f2[b])):
            pts = img.reshape(-1, 3)
            pts = pts[np.any(pts != 0, -1)][:N_PTS]
            cloud[b, half * N_PTS:half * N_PTS + len(pts)] = pts
    T_gt = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T_gt[:, 0, 3] = 0.8
    c, s = np.cos(0.01), np.sin(0.01)
    T_gt[:, :2, :2] = np.array([[c, -s], [s, c]], np.float32)
    return cloud, T_gt


def _trainer(capturable=False):
    """Same seed, same visiting-order source (orders are a function of the operator, not of the draw count)."""
    model, training, perm = load_pkg("model"), load_pkg("training"), load_pkg("perm")
    return training.Trainer(model.PWCLONet(DEV, seed=3, perm_source=perm.PermSource(fn=shuffle_fn)), capturable=capturable)


def _same_loss(got, want, spread, what):
    """The rule of the step_points tests: bit-equal where the EXISTING path (Trainer.step) repeated itself bit for bit from
    identical state, else within four times the spread of that existing path."""
    print("%s: loss %.9g against %.9g (existing path's own spread %.3g)" % (what, got, want, spread))
    if spread == 0.0:
        assert got == want, (what, got, want)
    else:
        assert abs(got - want) <= 4 * spread, (what, got, want, spread)


def test_step_points_is_step_on_the_staged_tensors():
    """Trainer A: step_points(cloud, T_gt, T_trans, T_trans_inv, aug_frame).  Trainer B (same seed, same visiting-order
    source, same dropout seed): step() on what input_stage gives for that cloud and on q_gt / t_gt of _ops.preprocess_gt.
    B's path is first run twice from identical state.  If the loss of the existing step repeats itself bit for bit, A's loss
    must be bit-equal to B's; if not, A must agree with B within four times the spread of those two runs of the existing
    path.  The test prints the spread and so which case held.
    On an MI355X the first case held: spread 0, all three comparisons bit-equal (loss 39.6436386 with, 35.9696274 without
    augmentation)."""
    ops, mu = load_pkg("_ops"), load_pkg("model_util")
    B = 2
    cloud, T_gt = _scene(B, seed=20)
    T_tr, T_inv = _augmentations(B, seed=13)
    aug = np.array([2, 1], np.int32)

    def existing():
        tr = _trainer()
        _pts, staged = mu.input_stage(t(cloud), t(T_tr), aug, H_IN, W_IN)
        q_gt, t_gt = ops.preprocess_gt(t(T_gt), t(T_tr), t(T_inv), t(aug))
        torch.manual_seed(7)
        return float(tr.step(staged[:B], staged[B:], q_gt, t_gt)), tr

    (b1, _), (b2, trB) = existing(), existing()
    spread = abs(b1 - b2)
    trA = _trainer()
    torch.manual_seed(7)
    a = float(trA.step_points(cloud, T_gt, T_tr, T_inv, aug, H_input=H_IN, W_input=W_IN))
    assert np.isfinite(a) and trA.step_count == 1
    _same_loss(a, b1, spread, "step_points against step")
    # host arrays, device tensors and a device aug_frame are the same step
    trC = _trainer()
    torch.manual_seed(7)
    c = float(trC.step_points(t(cloud), t(T_gt), t(T_tr), t(T_inv), t(aug), H_input=H_IN, W_input=W_IN))
    _same_loss(c, b1, spread, "step_points on device tensors against step")
    # no matrices = no augmentation = the step on the unaugmented stage
    trD, trE = _trainer(), _trainer()
    _pts, staged = mu.input_stage(t(cloud), None, None, H_IN, W_IN)
    q_gt, t_gt = ops.preprocess_gt(t(T_gt), None, None, None)
    torch.manual_seed(7)
    want = float(trD.step(staged[:B], staged[B:], q_gt, t_gt))
    torch.manual_seed(7)
    got = float(trE.step_points(cloud, T_gt, H_input=H_IN, W_input=W_IN))
    _same_loss(got, want, spread, "step_points without augmentation against step")
    assert got != a
    with pytest.raises(ValueError):
        trE.step_points(cloud, T_gt, T_tr, None, aug, H_input=H_IN, W_input=W_IN)


def test_captured_step_from_clouds_trains_and_reads_all_five_inputs():
    """capture_points / step_graph_points: replays on a fixed synthetic pair with a fresh augmentation per replay lower the
    loss (the criterion of test_captured_training_step_trains: finite, and the best of the later steps below the first).
    Then ONE replay is fed a different cloud, a different T_gt, different T_trans / T_trans_inv and the flipped aug_frame, and
    its loss is compared with an eager step_points on a twin trainer in the same state (variables, moving statistics, Adam
    moments and step count through a checkpoint; same visiting orders; same dropout seed), under the rule of
    test_step_points_is_step_on_the_staged_tensors: the existing eager step is run twice from that state to see whether it repeats
    itself; bit-equal if it does, within four times its spread if not (printed).
    On an MI355X the first case held: spread 0, and the replay, the eager step_points and the existing step all gave
    4.43914461 bit for bit; the 32 replays took the loss from 32.19 to single digits."""
    training = load_pkg("training")
    B = 2
    cloud, T_gt = _scene(B, seed=20)
    rng = np.random.default_rng(5)

    def draw():
        T = np.stack([training.data_augmentation(rng) for _ in range(B)])
        return f32(T), f32(np.linalg.inv(T)), rng.choice([1, 2], size=B).astype(np.int32)

    tr = _trainer(capturable=True)
    torch.manual_seed(0)
    tr.capture_points(cloud, T_gt, *draw(), H_input=H_IN, W_input=W_IN)
    start = tr.step_count
    losses, last_aug = [], None
    for _ in range(32):
        T_tr, T_inv, last_aug = draw()
        losses.append(float(tr.step_graph_points(cloud, T_gt, T_tr, T_inv, last_aug, H_input=H_IN, W_input=W_IN)))
    print("captured step from clouds:", " ".join("%.4f" % v for v in losses))
    assert tr.step_count == start + 32 and tr.opt.t == tr.step_count
    assert all(np.isfinite(losses)) and min(losses[4:]) < losses[0], losses
    graph = tr._graph

    # the twins: the trainer's state through a checkpoint
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "state.npz")
        tr.save(path)
        twins = [_trainer().load(path) for _ in range(3)]
    assert all(other.step_count == tr.step_count and other.opt.t == tr.opt.t for other in twins)
    cloud2, T_gt2 = _scene(B, seed=31)
    T_gt2[:, 1, 3] = 0.05
    T_tr2, T_inv2 = _augmentations(B, seed=17)
    aug2 = (3 - last_aug).astype(np.int32)                    # flipped against what the previous replay left in the buffer
    assert (aug2 != last_aug).all() and torch.equal(tr._static[4].cpu(), torch.from_numpy(last_aug))
    assert not np.array_equal(cloud2, cloud)
    runs = []
    for other in twins[:2]:                                   # the existing path, twice from identical state
        mu, ops = load_pkg("model_util"), load_pkg("_ops")
        _pts, staged = mu.input_stage(t(cloud2), t(T_tr2), aug2, H_IN, W_IN)
        q_gt, t_gt = ops.preprocess_gt(t(T_gt2), t(T_tr2), t(T_inv2), t(aug2))
        torch.manual_seed(9)
        runs.append(float(other.step(staged[:B], staged[B:], q_gt, t_gt)))
    spread = abs(runs[0] - runs[1])
    torch.manual_seed(9)
    eager = float(twins[2].step_points(cloud2, T_gt2, T_tr2, T_inv2, aug2, H_input=H_IN, W_input=W_IN))
    _same_loss(eager, runs[0], spread, "eager step_points on the twin against step")
    torch.manual_seed(9)
    replay = float(tr.step_graph_points(cloud2, T_gt2, T_tr2, T_inv2, aug2, H_input=H_IN, W_input=W_IN))
    assert tr._graph is graph                                 # a replay, not a re-capture
    _same_loss(replay, eager, spread, "replay on new inputs against eager step_points")
    assert replay != losses[-1]
    with pytest.raises(RuntimeError, match="capturable"):
        _trainer().capture_points(cloud, T_gt, H_input=H_IN, W_input=W_IN)


def test_train_epoch_over_a_kitti_tree(tmp_path):
    """training.train_epoch over kitti_batches of a synthetic tree (7 scans in two sequences, batch 2, 57 600 points per scan,
    64 x 900 range images): samples // 2 steps, step_count advanced by as many, every parameter and the reported loss finite --
    through the captured step (the graph is recorded beforehand: its warm-up steps are optimisation steps of their own) and
    through the eager one on a fresh trainer."""
    training = load_pkg("training")
    root, N, H, W = str(tmp_path), 64 * 900, 64, 900
    seqs = ["04", "05"]
    T_diffs = {"04": write_sequence(root, "04", 4, H, W, seed=50), "05": write_sequence(root, "05", 3, H, W, seed=70)}
    samples = 7
    batches = lambda seed: training.kitti_batches(root, seqs, T_diffs, 2, np.random.default_rng(seed), num_points=N)
    for graph in (True, False):
        tr = _trainer(capturable=graph)
        if graph:
            tr.capture_points(*next(iter(batches(0))), H_input=H, W_input=W)
        before = tr.step_count
        loss, steps = training.train_epoch(tr, batches(1), graph=graph, H_input=H, W_input=W)
        assert steps == samples // 2 and tr.step_count == before + steps
        assert np.isfinite(loss)
        assert all(bool(torch.isfinite(p).all()) for p in tr.params)
        assert tr.opt.t == tr.step_count
    # a capturable trainer without a graph: the first batch records one, and the count returned is the real number of
    # optimisation steps (the three warm-up steps of the capture included), which is what step_count advanced by
    tr = _trainer(capturable=True)
    loss, steps = training.train_epoch(tr, batches(1), graph=True, H_input=H, W_input=W)
    assert steps == tr.step_count == samples // 2 + 3 and tr.opt.t == tr.step_count and np.isfinite(loss)
    # an empty epoch: no step, no loss
    loss, steps = training.train_epoch(tr, iter(()), graph=False, H_input=H, W_input=W)
    assert steps == 0 and np.isnan(loss)

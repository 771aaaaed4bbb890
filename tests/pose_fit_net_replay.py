"""The net half of tests/test_pose_fit_gpu.py, run as a program of its own: forward(fit=) against _scan_ops.pose_fit on the same pair and
pose, a lane captured with a fit against the eager result (and its other outputs against a capture without one), a graph replay of
the bare entry against its eager call, the refusals, and the sequence evaluation's fit file on both of its paths.
It is a program because capture() draws its streams from the process-wide pool and binds them to hardware queues: in the suite's
own process more captures move every later test's lanes to other queues (tests/test_sv_ride_gpu.py looks at exactly that)."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

import pose_fit_reference as R
from conftest import load_pkg
from test_evaluate_gpu import _write_sequence
from util_params import shuffle_fn

DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda x: x.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(u), bits(v)) for u, v in zip((a.pose, a.info, a.grad, a.stats), (b.pose, b.info, b.grad, b.stats)))


def main():
    model, S, perm, ops, ev = load_pkg("model"), load_pkg("sensor"), load_pkg("perm"), load_pkg("_scan_ops"), load_pkg("evaluate")
    H, W = 64, 900
    f1, f2 = R.scene(1, H, W, seed=21)
    a, b = t(f1), t(f2)
    fit = S.PoseFit(iters=1, gate=3.0, jump_rel=0.2, min_count=10)
    net = model.PWCLONet(DEV, seed=4, perm_source=perm.PermSource(fn=shuffle_fn))

    # eager: the extra entry is the entry's own result on the forward's pose; the other outputs do not move
    plain = [x.clone() for x in net.forward(a, b)]
    out = net.forward(a, b, fit=fit)
    assert len(out) == len(plain) + 1 and all(torch.equal(bits(g), bits(w)) for g, w in zip(out[:-1], plain))
    pose7 = torch.cat([out[0].reshape(1, 4), out[1].reshape(1, 3)], -1).contiguous()
    direct = ops.pose_fit(a, b, pose7, fit)
    torch.cuda.synchronize()
    want = ops.PoseFitResult(*(x.clone() for x in (direct.pose, direct.info, direct.grad, direct.stats)))
    assert same(out[-1], want) and torch.isfinite(want.info).all()
    print("net pose: count %d, rms %.4f, status %d" % (float(want.count[0]), float(want.rms[0]), float(want.status[0])))
    # ... and the pose head's own (B,7) row is that pose
    row = torch.zeros((1, 7), device=DEV)
    assert same(net.forward(a, b, pose_out=row, fit=fit)[-1], want) and torch.equal(bits(row), bits(pose7))

    # a graph replay of the bare entry reads the pose row when it RUNS
    side = torch.cuda.Stream(device=DEV)
    live = pose7.clone()
    with torch.cuda.stream(side):
        ops.pose_fit(a, b, live, fit)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with model.graph_capture(g):
        replayed = ops.pose_fit(a, b, live, fit)
    g.replay()
    torch.cuda.synchronize()
    assert same(replayed, want)
    other = t(R.GUESS[None])
    live.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    at_guess = ops.pose_fit(a, b, other, fit)
    torch.cuda.synchronize()
    assert same(replayed, at_guess) and not same(at_guess, want) and float(at_guess.count[0]) > 1000 and float(at_guess.status[0]) == 0

    # a lane with a fit: the eager result, from buffers the lane owns; every other output as a lane without one
    with pytest.raises(ValueError, match="pose_ring"):
        net.capture(1, H, W, pose_ring=4, fit=fit)
    with pytest.raises(TypeError):
        net.capture(1, H, W, fit=dict(iters=1))
    net.capture(1, H, W, fit=fit, check_every=2)
    pair = torch.cat([a, b], 0)
    for replay in range(2):                                            # the second one takes the checked graph
        rep = net.submit(0, pair)
        torch.cuda.synchronize()
        assert all(torch.equal(bits(r), bits(w)) for r, w in zip(rep, plain)) and same(net.lane_fit(0), want)
        assert torch.equal(bits(net.lane_pose(0)), bits(pose7))
    assert same(net.lane_fit(0, fit), want) and net.captured_fit == fit
    with pytest.raises(RuntimeError, match="keeps the fit of its capture"):
        net.lane_fit(0, S.PoseFit())
    net.capture(1, H, W, warmup=1)
    rep = net.submit(0, pair)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(r), bits(w)) for r, w in zip(rep, plain)) and net._lanes[0].fit is None and net.captured_fit is None
    with pytest.raises(RuntimeError, match="without a pose fit"):
        net.lane_fit(0)

    # raw clouds in: forward_points and the sequence evaluation, sequential and through lanes
    with tempfile.TemporaryDirectory() as root:
        n = 3
        _poses, T_diff = _write_sequence(root, "04", n, H, W)
        kw = dict(H_input=H, W_input=W, num_points=H * W)
        q0, t0 = ev.predict_sequence(net, root, "04", T_diff, **kw)
        measure = S.PoseFit(gate=3.0, jump_rel=0.2, min_count=10)
        q1, t1, rows1 = ev.predict_sequence(net, root, "04", T_diff, fit=measure, **kw)
        assert np.array_equal(q1, q0) and np.array_equal(t1, t0) and rows1.shape == (n, 24) and np.isfinite(rows1).all()
        q2, t2, rows2 = ev.predict_sequence(net, root, "04", T_diff, fit=measure, lanes=2, **kw)
        assert np.array_equal(q2, q0) and np.array_equal(t2, t0) and np.array_equal(rows2, rows1)
        rows, _score = ev.run_sequence(net, root, "04", T_diff, out_dir=os.path.join(root, "out"), fit=fit, **kw)
        back = np.loadtxt(os.path.join(root, "out", "04_fit.txt"))
        assert rows.shape == (n, 12) and back.shape == (n, 24) and np.isfinite(back).all() and (back[:, 0] == np.round(back[:, 0])).all()
        assert sorted(os.listdir(os.path.join(root, "out"))) == ["04_fit.txt", "04_pred.txt"]
        ev.run_sequence(net, root, "04", T_diff, out_dir=os.path.join(root, "plain"), **kw)
        assert os.listdir(os.path.join(root, "plain")) == ["04_pred.txt"]


if __name__ == "__main__":
    main()
    print("pose fit through the net: ok")

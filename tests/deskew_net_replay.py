"""The net half of tests/test_deskew_gpu.py, run as a program of its own: forward_points with a sweep against forward on the entry's
own images, a lane captured with a sweep fed through submit_points(motion=) and through lane_motion() -- bit for bit the eager
result, the motion row read at replay -- and a capture without a sweep having no motion buffer.
It is a program because capture() draws its streams from the process-wide pool and binds them to hardware queues: in the suite's
own process two more captures move every later test's lanes to other queues (tests/test_sv_ride_gpu.py looks at exactly that)."""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from util_params import shuffle_fn

DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def main():
    model, synth, S, perm, ops = load_pkg("model"), load_pkg("synth"), load_pkg("sensor"), load_pkg("perm"), load_pkg("_ops")
    sensor = S.Sensor(fov_up_deg=10.67, fov_down_deg=-30.67)
    H, W = 64, 900
    N = H * W
    f1, f2 = synth.frame_pair(1, H, W, seed=21, sensor=sensor)
    rng = np.random.default_rng(8)
    cloud = np.zeros((1, 2 * N, 4), np.float32)
    cloud[0, :N, :3], cloud[0, N:, :3] = f1.reshape(N, 3), f2.reshape(N, 3)
    cloud[..., 3] = rng.uniform(0, 1, (1, 2 * N))
    cloud = t(cloud)
    sweep = S.Sweep(3, 1.0)
    m1 = t(np.array([[0.999, 0.01, -0.02, 0.03, 1.0, -0.3, 0.05]], np.float32))
    m2 = t(np.array([[0.998, -0.03, 0.01, -0.04, -0.6, 0.8, -0.1]], np.float32))
    eye = torch.eye(4, device=DEV).repeat(1, 1, 1)
    mine = model.PWCLONet(DEV, seed=4, perm_source=perm.PermSource(fn=shuffle_fn), sensor=sensor)

    def eager(m):
        _pts, both = ops.input_stage(cloud, None, None, H, W, sensor=sensor, sweep=sweep, motion=m)
        return [x.clone() for x in mine.forward(both[:1], both[1:])]

    want1, want2 = eager(m1), eager(m2)
    plain = [x.clone() for x in mine.forward(*ops.input_stage(cloud, None, None, H, W, sensor=sensor)[1].split(1))]
    assert all(torch.isfinite(x).all() for x in want1) and not torch.equal(want1[0], want2[0]) and not torch.equal(want1[0], plain[0])
    got = mine.forward_points(cloud, H, W, eye, eye, eye, aug_frame=np.array([1]), sweep=sweep, motion=m1)
    assert all(torch.equal(g, w) for g, w in zip(got[:9], want1))
    mine.capture(1, H, W, num_points=N, point_stride=4, sweep=sweep)
    assert torch.equal(mine.lane_motion(0), t(np.array([[1, 0, 0, 0, 0, 0, 0]], np.float32)))
    rep = mine.submit_points(0, cloud, motion=m1)
    torch.cuda.synchronize()                                           # (the lane runs on its own stream: read its outputs after it)
    assert all(torch.equal(r, w) for r, w in zip(rep, want1))
    assert torch.equal(mine.lane_motion(0), m1)
    mine.lane_motion(0).copy_(m2)                                      # a device-side producer: the graph reads the row when it runs
    rep = mine.submit_points(0, cloud)
    torch.cuda.synchronize()
    assert all(torch.equal(r, w) for r, w in zip(rep, want2))
    with pytest.raises(RuntimeError, match="recorded"):
        mine.submit_points(0, cloud, motion_is_pose=True)
    # a capture without a sweep is today's: no motion buffer
    mine.capture(1, H, W, num_points=N, point_stride=4, warmup=1)
    assert mine._lanes[0].motion is None
    with pytest.raises(RuntimeError, match="without a sweep"):
        mine.lane_motion(0)
    with pytest.raises(RuntimeError, match="without a sweep"):
        mine.submit_points(0, cloud, motion=m1)
    rep = mine.submit_points(0, cloud)
    torch.cuda.synchronize()
    assert all(torch.equal(r, w) for r, w in zip(rep, plain))


if __name__ == "__main__":
    main()
    print("deskew through the net: ok")

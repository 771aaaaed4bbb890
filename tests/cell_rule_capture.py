"""The fixed calls of tests/test_cell_rule_gpu.py (build_calls) and, run as a program of its own, its capture half: inside an open
capture a host beam table is refused by _ops.input_stage, pose_fit and model_render with the one message, the capture then closes
cleanly and replays what it did record.
It is a program because a capture and its warm-up draw streams from the process-wide pool and bind them to hardware queues: in the
suite's own process they move every later test's lanes to other queues (tests/test_sv_ride_gpu.py looks at exactly that)."""
import numpy as np
import pytest
import torch

import deskew_reference as D
import pose_fit_reference as R
from conftest import load_pkg

DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
B, N, H, W, K = 2, 256, 8, 32, 2
RAD8 = [e * D.D2R for e in D.TABLE8]
IDENTITY = np.array([[1, 0, 0, 0, 0, 0, 0]], np.float32)
OPS = ("input_stage", "input_stage+sweep", "pose_fit/0", "pose_fit/2", "model_render")


def build_calls():
    """{name: f(**how) -> tuple of output tensors} on fixed device inputs; `how` is sensor= / beam_elev=."""
    ops, scan_ops, S, synth = load_pkg("_ops"), load_pkg("_scan_ops"), load_pkg("sensor"), load_pkg("synth")
    sensor = S.Sensor(beam_elevations_deg=D.TABLE8)
    rng = np.random.default_rng(8)
    cloud = np.zeros((B, 2 * N, 4), np.float32)
    cloud[..., :3] = D.target_cloud(rng, B, N, H, W, ops.projection_constants(H, W, sensor), table_deg=D.TABLE8)
    cloud[..., 3] = rng.uniform(0.0, 1.0, (B, 2 * N))                                   # the phase of every point
    cloud[rng.random((B, 2 * N)) < 0.05, :3] = 0.0
    cloud = t(cloud)
    motion = t(np.stack([D.motion_row(rng, scale=0.2) for _ in range(B)]))              # (B,7), used in place
    f1, f2 = synth.frame_pair(B, H, W, seed=4, sensor=sensor)
    x1, x2, pose7 = t(f1), t(f2), t(R.start_poses(B))
    src = torch.stack([x1, x2], 1).contiguous()                                         # (B,K,H,W,3)
    carry = t(np.stack([IDENTITY.repeat(B, 0), R.start_poses(B)], 1))                   # (B,K,7): scan 0 as it is, scan 1 by its pose
    # jump_rel = 0.5: eight beams 2 .. 5 degrees apart -- the reference counts 92 and 98 terms on these two images (47 and 51 at 0.2)
    fit = lambda iters: S.PoseFit(iters=iters, jump_rel=0.5, min_count=20)

    def fitted(iters, **how):
        res = scan_ops.pose_fit(x1, x2, pose7, fit(iters), **how)
        return res.pose, res.info, res.grad, res.stats

    return {"input_stage": lambda **how: ops.input_stage(cloud, None, None, H, W, **how),
            "input_stage+sweep": lambda **how: ops.input_stage(cloud, None, None, H, W, sweep=S.Sweep(phase=3), motion=motion, **how),
            "pose_fit/0": lambda **how: fitted(0, **how), "pose_fit/2": lambda **how: fitted(2, **how),
            "model_render": lambda **how: scan_ops.model_render(src, carry, **how)}


def same(a, b):
    torch.cuda.synchronize()
    return len(a) == len(b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def main():
    ops, L, S = load_pkg("_ops"), load_pkg("_lib"), load_pkg("sensor")
    calls = build_calls()
    sensor = S.Sensor(beam_elevations_deg=D.TABLE8)
    table = ops.beam_table(sensor, H, DEV)
    want = {op: [x.clone() for x in calls[op](sensor=sensor, beam_elev=table)] for op in OPS}
    on_host = table.cpu()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):                                                       # (allocations and code objects, before the capture)
        for op in OPS:
            calls[op](sensor=sensor, beam_elev=table)
    torch.cuda.synchronize()
    g, recorded = torch.cuda.CUDAGraph(), {}
    with torch.cuda.graph(g):
        for op in OPS:
            recorded[op] = calls[op](sensor=sensor, beam_elev=table)                    # the owner's tensor: recorded
            for how in (dict(sensor=sensor), dict(beam_elev=RAD8), dict(beam_elev=np.asarray(RAD8, np.float32)),
                        dict(beam_elev=on_host)):
                with pytest.raises(L.EloError, match="a graph capture needs the beam table as a device tensor its owner keeps"):
                    calls[op](**how)                                                    # a Python exception, before any launch
            assert torch.cuda.is_current_stream_capturing()
    assert not torch.cuda.is_current_stream_capturing()
    g.replay()
    for op in OPS:
        assert same(recorded[op], want[op])
        assert same(calls[op](sensor=sensor), want[op])                                 # outside the capture the same call uploads and runs


if __name__ == "__main__":
    main()
    print("host tables in a capture: ok")

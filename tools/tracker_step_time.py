"""Time of one step of the frame-to-model tracker on 64x1800 range images, half-empty scans ("kitti" profile of synth) a small motion
apart, K = 4, PoseFit(iters=2):
  (a) local_model.ModelTracker.step: the host's cursor, the re-basing as float64 torch operators, every launch issued from Python;
  (b) local_model.DeviceTracker.step, captured: three copies into the static inputs and ONE replay of the recorded step (begin,
      render, fit, advance: 6 + 2 (iters + 1) launches).
Host-clock time per step around a block of steps that ENDS in a synchronise (so the host's enqueue rate counts, as it does for a
caller); the two forms ALTERNATE in one process, the median block of each.  Both walk the same ring of consecutive pairs.
python tools/tracker_step_time.py [--scans 4] [--iters 2] [--out profiles/tracker_step.txt]"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=4)
ap.add_argument("--iters", type=int, default=2)
ap.add_argument("--reps", type=int, default=200, help="steps per timed block")
ap.add_argument("--rounds", type=int, default=15, help="alternating blocks per form")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tracker_step.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda:0")
S, synth, lm = pkg("sensor"), pkg("synth"), pkg("local_model")
H, W, N = 64, 1800, 8
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


scans = [torch.from_numpy(synth.range_image(H, W, seed=30 + k, yaw=0.01 * k, shift=(0.8 * k, 0.0, 0.0), profile="kitti", scene_seed=30)[None]).to(dev)
         for k in range(N + 1)]
# pair k = (scan k+1, scan k); the pose carries frame 1 into frame 2: the sensor moved 0.8 m forward and turned 0.01 rad
pose7 = torch.tensor([[math.cos(0.005), 0, 0, math.sin(0.005), 0.8, 0, 0]], dtype=torch.float32, device=dev)
pairs = [(scans[k + 1], scans[k], pose7) for k in range(N)]
fit, K = S.PoseFit(iters=args.iters), args.scans
host = lm.ModelTracker(H, W, S.LocalModel(K), fit, device=dev)
resident = lm.DeviceTracker(H, W, S.LocalModel(K, resident=True), fit, device=dev).capture()


def block(tracker, reps):
    """us per step: `reps` steps over the ring of pairs (the wrap from the last pair to the first is a jump the tracker is not told
    about: the fit then meets a model 6.4 m off and is flagged -- the launches are the same), ended by a synchronise."""
    tracker.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in range(reps):
        tracker.step(*pairs[n % N])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


for tr in (host, resident):
    block(tr, max(args.reps // 4, 3))
times = {"host": [], "resident": []}
for _ in range(args.rounds):
    times["host"].append(block(host, args.reps))
    times["resident"].append(block(resident, args.reps))
stat = lambda x: (float(np.median(x)), min(x), max(x))
(mh, lh, hh), (mr, lr, hr) = stat(times["host"]), stat(times["resident"])
filled = float(np.mean([float((s != 0).any(-1).float().mean()) for s in scans]))
say("one tracker step on %dx%d range images (%.0f %% of the cells filled), K = %d scans, PoseFit(iters=%d); host clock around blocks of "
    "%d steps ending in a synchronise, %d alternating blocks, median block (min .. max), us per step" % (
        H, W, 100 * filled, K, args.iters, args.reps, args.rounds))
say("(a) ModelTracker.step, host cursor + float64 torch re-basing, every launch from Python: %.1f us (%.1f .. %.1f)" % (mh, lh, hh))
say("(b) DeviceTracker.step, three copies + one replay of the recorded step (%d launches = 6 + 2 (iters + 1)): %.1f us (%.1f .. %.1f); "
    "(a)/(b) = %.2f" % (resident.launches(), mr, lr, hr, mh / mr))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

"""Time of elo_map_fit on ONE 64x1800 range image of the synthetic scene against a map of ~20 scans of the same place (voxel 0.5 m,
table 2^22 slots): (a) one evaluation (iters = 0: the evaluate launch and the report launch) and (b) a whole fit of iters = 2 (six
launches), and -- in the same run, as the yardstick -- elo_pose_fit at the same shape on the pair tools/pose_fit_time.py uses
(synth.frame_pair, its ego-motion as the guess), (c) one evaluation and (d) iters = 2.  Each form is recorded into a hipGraph of its
own (the device's time, not the host's enqueue rate), the graphs replayed ALTERNATING in one process, device events around blocks of
replays, the median block.  The map's scans are the scene
seen from sensor positions 0.8 m apart (synth.range_image subtracts `shift`), inserted at their true poses; the scan fitted is the
next one, its guess a few centimetres and milliradians off.  DESIGN.md gives ~4.7 us for a dependent launch on this machine.
python tools/map_fit_time.py [--scans 20] [--out profiles/map_fit.txt]"""
import argparse
import importlib
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=20, help="scans in the map")
ap.add_argument("--voxel", type=float, default=0.5)
ap.add_argument("--log2", type=int, default=22)
ap.add_argument("--reps", type=int, default=100, help="calls per timed block")
ap.add_argument("--rounds", type=int, default=11, help="alternating blocks per form")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "map_fit.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda:0")
ops, synth, sensor, world_map = pkg("_scan_ops"), pkg("synth"), pkg("sensor"), pkg("world_map")
H, W = 64, 1800
FLOOR_US = 4.7
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def recorded(fn):
    """fn's launches as a graph's replay; fn ran three times on a side stream first (allocations, code objects)."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    g.keep = keep
    return g.replay


n = args.scans
scans = np.stack([synth.range_image(H, W, seed=60 + k, shift=(0.8 * k, 0.0, 0.0)) for k in range(n + 1)])
poses = np.zeros((n + 1, 7))
poses[:, 0], poses[:, 4] = 1.0, 0.8 * np.arange(n + 1)
wm = world_map.WorldMap(sensor.VoxelMap(voxel=args.voxel, log2_capacity=args.log2), dev)
wm.insert(torch.from_numpy(scans[:n]).to(dev), torch.from_numpy(poses[:n]).to(dev))
xyz = torch.from_numpy(scans[n:]).to(dev)
f1, f2 = synth.frame_pair(1, H, W, seed=4)
pair1, pair2 = torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)
a = 0.004
guess = torch.tensor([[math.cos(a / 2), 0.0, 0.0, math.sin(a / 2), 0.8 * n + 0.05, -0.03, 0.01]], dtype=torch.float64, device=dev)
rel = torch.tensor([[math.cos(0.005), 0.0, 0.0, -math.sin(0.005), -0.8, 0.0, 0.0]], dtype=torch.float32, device=dev)
m0, m2 = sensor.MapFit(), sensor.MapFit(iters=2)
p0, p2 = sensor.PoseFit(), sensor.PoseFit(iters=2)
r0, r2 = wm.fit(xyz, guess, fit=m0), wm.fit(xyz, guess, fit=m2)
y0 = ops.pose_fit(pair1, pair2, rel, p0)
torch.cuda.synchronize()
s = wm.stats()
say("elo_map_fit on one %dx%d range image (%d points) against a map of %d scans: voxel %.2f m, 2^%d slots, %d voxels, %.1f points a "
    "voxel, dropped_full %d; gate = the voxel" % (H, W, int((xyz != 0).any(-1).sum()), n, args.voxel, args.log2, s["occupied"],
                                                 s["inserted"] / max(s["occupied"], 1), s["dropped_full"]))
say("terms: %d at the guess (rms %.4f m), %d after iters = 2 (rms %.4f m, status %d); the fitted pose lies %.4f m from the true "
    "translation (the guess: %.4f m); elo_pose_fit on its own pair: %d terms"
    % (int(r0.count[0]), float(r0.rms[0]), int(r2.count[0]), float(r2.rms[0]), int(r2.status[0]),
       float((r2.pose[0, 4:] - torch.tensor([0.8 * n, 0.0, 0.0], dtype=torch.float64, device=dev)).norm()),
       float((guess[0, 4:] - torch.tensor([0.8 * n, 0.0, 0.0], dtype=torch.float64, device=dev)).norm()), int(y0.count[0])))
forms = [recorded(fn) for fn in (lambda: wm.fit(xyz, guess, fit=m0), lambda: wm.fit(xyz, guess, fit=m2),
                                 lambda: ops.pose_fit(pair1, pair2, rel, p0), lambda: ops.pose_fit(pair1, pair2, rel, p2))]
for fn in forms:
    block(fn, max(args.reps // 4, 3))
times = [[] for _ in forms]
for _ in range(args.rounds):
    for k, fn in enumerate(forms):
        times[k].append(block(fn, args.reps))
med = [(float(np.median(x)), min(x), max(x)) for x in times]
say("%d alternating blocks of %d replays, median block (min .. max), us per call; a dependent launch costs ~%.1f us on this machine "
    "(DESIGN.md)" % (args.rounds, args.reps, FLOOR_US))
say("(a) elo_map_fit, one evaluation, 2 launches   %.1f us (%.1f .. %.1f)" % med[0])
say("(b) elo_map_fit, iters = 2, 6 launches        %.1f us (%.1f .. %.1f)" % med[1])
say("(c) elo_pose_fit, one evaluation, 2 launches  %.1f us (%.1f .. %.1f)   (a)/(c) = %.2f" % (med[2] + (med[0][0] / med[2][0],)))
say("(d) elo_pose_fit, iters = 2, 6 launches       %.1f us (%.1f .. %.1f)   (b)/(d) = %.2f" % (med[3] + (med[1][0] / med[3][0],)))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

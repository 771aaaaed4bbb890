"""Time of elo_model_render on 64x1800 range images, K = 1, 4, 8 half-empty scans ("kitti" profile of synth) a small motion apart:
each form recorded into a hipGraph of its own (so that the device's time is measured, not the host's enqueue rate), the graphs
replayed ALTERNATING in one process, device events around blocks of replays, the median block of each:
  (a) one call with K sources (three launches: clear, splat, resolve);
  (b) K calls of the same entry point with ONE source each (3 K launches; what rendering scan by scan would cost -- it is not a
      model: each call overwrites the last);
and the bytes (a) moves -- 12 per source cell read, per target cell 8 cleared, 8 read back, 16 written, 12 gathered for a winner --
against the cold streaming ceiling of this GPU (tools/micro/hbm_probe.hip: 0.81 of 8 TB/s).  The replays re-read the same ~5 MB,
which the caches hold: the ratio says how far the call is from being a streaming problem at all, not how well it streams.
DESIGN.md gives ~4.7 us for a dependent launch on this machine whatever it does.
python tools/model_render_time.py [--scans 1 4 8] [--out profiles/model_render.txt]"""
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
ap.add_argument("--scans", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--reps", type=int, default=200, help="calls per timed block")
ap.add_argument("--rounds", type=int, default=15, help="alternating blocks per form")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "model_render.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda:0")
ops, synth = pkg("_scan_ops"), pkg("synth")
H, W = 64, 1800
FLOOR_US, CEILING = 4.7, 0.81 * 8e12
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


def alternate(forms, reps):
    forms = [recorded(fn) for fn in forms]
    for fn in forms:
        block(fn, max(reps // 4, 3))
    times = [[] for _ in forms]
    for _ in range(args.rounds):
        for k, fn in enumerate(forms):
            times[k].append(block(fn, reps))
    return [(float(np.median(x)), min(x), max(x)) for x in times]


say("elo_model_render on %dx%d range images, %d alternating blocks of %d replays, median block (min .. max), us per call; a dependent "
    "launch costs ~%.1f us on this machine (DESIGN.md)" % (H, W, args.rounds, args.reps, FLOOR_US))
for K in args.scans:
    scans = np.stack([synth.range_image(H, W, seed=30 + k, yaw=0.01 * k, shift=(0.8 * k, 0.0, 0.0), profile="kitti", scene_seed=30)
                      for k in range(K)])
    pose = np.array([[math.cos(0.005 * k), 0, 0, math.sin(0.005 * k), 0.8 * k, 0, 0] for k in range(K)], np.float32)   # scan k -> scan 0
    src, poses = torch.from_numpy(scans[None]).to(dev), torch.from_numpy(pose[None]).to(dev)
    singles = [(src[:, k:k + 1].contiguous(), poses[:, k:k + 1].contiguous()) for k in range(K)]
    xyz, idx = ops.model_render(src, poses)
    torch.cuda.synchronize()
    filled = int((idx >= 0).sum())
    points = int((src != 0).any(-1).sum())
    moved = 12 * K * H * W + (8 + 8 + 16) * H * W + 12 * filled
    (ma, la, ha), (mb, lb, hb) = alternate([lambda: ops.model_render(src, poses),
                                            lambda: [ops.model_render(s, p) for s, p in singles]], args.reps)
    say("K = %d: %d points in, %d of %d cells filled (one scan fills %d); (a) one call, 3 launches %.1f us (%.1f .. %.1f) = %.1f us per "
        "launch   (b) %d single-source calls, %d launches %.1f us (%.1f .. %.1f); (b)/(a) = %.2f" % (
            K, points, filled, H * W, int((src[0, 0] != 0).any(-1).sum()), ma, la, ha, ma / 3, K, 3 * K, mb, lb, hb, mb / ma))
    say("K = %d: (a) moves %.2f MB = %.0f GB/s, %.3f of the cold streaming ceiling (%.2f TB/s); three launches at the floor would be "
        "%.1f us: the call is %.2f of that" % (K, moved / 1e6, moved / ma / 1e3, moved / (ma * 1e-6) / CEILING, CEILING / 1e12,
                                                3 * FLOOR_US, ma / (3 * FLOOR_US)))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

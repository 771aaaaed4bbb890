"""Time of elo_map_merge and of what WorldMap builds on it, on the 20-scan synthetic map of tools/map_fit_time.py (64x1800 scans of one
place from sensor positions 0.8 m apart) in a table of 2^22 slots, at voxel 0.5 m and 0.1 m:
(a) elo_map_merge of the whole table (2^22 source rows, most of them empty slots) into a second table -- WARM (the replays merge the
    same table again: every key is found) as a hipGraph, and COLD (the destination just reset: every key is claimed) as one eager
    call after a reset outside the events -- with elo_map_extract on the same table in the same run as the yardstick: it reads the
    same keys and the same occupied acc rows;
(b) a whole WorldMap.rebuild(), fills of the fresh table included, and the fills alone;
(c) the per-scan time of a tracked add() (MapFit(iters=2)) of the 20-scan drive with MapWindow(every=10) against the same drive
    without a window -- eager, host enqueue included, since add() is host code around the launches.
The graphs are replayed ALTERNATING in one process, device events around blocks of replays, the median block.
python tools/map_merge_time.py [--out profiles/map_merge.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=20)
ap.add_argument("--voxels", type=float, nargs="+", default=[0.5, 0.1])
ap.add_argument("--log2", type=int, default=22)
ap.add_argument("--reps", type=int, default=20, help="calls per timed block")
ap.add_argument("--rounds", type=int, default=9, help="alternating blocks per form")
ap.add_argument("--drives", type=int, default=5, help="repetitions of the tracked drive")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "map_merge.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda:0")
ops, synth, sensor, world_map = pkg("_scan_ops"), pkg("synth"), pkg("sensor"), pkg("world_map")
H, W = 64, 1800
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


def alternating(forms):
    for fn in forms:
        block(fn, 3)
    times = [[] for _ in forms]
    for _ in range(args.rounds):
        for k, fn in enumerate(forms):
            times[k].append(block(fn, args.reps))
    return [(float(np.median(x)), min(x), max(x)) for x in times]


n = args.scans
scans = np.stack([synth.range_image(H, W, seed=60 + k, shift=(0.8 * k, 0.0, 0.0)) for k in range(n)])
poses = np.zeros((n, 7))
poses[:, 0], poses[:, 4] = 1.0, 0.8 * np.arange(n)
X, P = torch.from_numpy(scans).to(dev), torch.from_numpy(poses).to(dev)
C = 1 << args.log2
say("elo_map_merge: a table of 2^%d slots holding %d scans of %dx%d; %d alternating blocks of %d replays, median block (min .. max), us"
    % (args.log2, n, H, W, args.rounds, args.reps))
for voxel in args.voxels:
    spec = sensor.VoxelMap(voxel=voxel, log2_capacity=args.log2)
    wm = world_map.WorldMap(spec, dev)
    wm.insert(X, P)
    s = wm.stats()
    dk = torch.full((C,), -1, dtype=torch.int64, device=dev)
    da = torch.zeros((C, 4), dtype=torch.int64, device=dev)
    ds = torch.zeros((8,), dtype=torch.int64, device=dev)
    centre = torch.tensor([0.8 * (n - 1), 0.0, 0.0], dtype=torch.float64, device=dev)
    wm.rebuild()                                     # (the spare buffers exist from here on)

    def rebuild():
        was = (wm.keys, wm.acc, wm._spare, wm._rebuilds)
        rep = wm.rebuild(centre=centre, radius=40.0)
        wm.keys, wm.acc, wm._spare, wm._rebuilds = was      # (the graph rebuilds the same table into the same spare every replay)
        return rep

    def fills():
        wm._spare[0].fill_(-1)
        wm._spare[1].zero_()

    forms = [recorded(lambda: ops.map_merge(dk, da, ds, wm.keys, wm.acc, spec)),
             recorded(lambda: ops.map_merge(dk, da, ds, wm.keys, wm.acc, spec, centre, 40.0)),
             recorded(lambda: ops.map_extract(wm.keys, wm.acc, spec, s["occupied"])), recorded(rebuild), recorded(fills)]
    med = alternating(forms)
    cold = []
    for _ in range(args.rounds):
        dk.fill_(-1)
        da.zero_()
        ds.zero_()
        torch.cuda.synchronize()
        cold.append(block(lambda: ops.map_merge(dk, da, ds, wm.keys, wm.acc, spec), 1))
    kept = int(ops.map_merge(dk, da, ds, wm.keys, wm.acc, spec, centre, 40.0)[0])
    say("voxel %.2f m: %d voxels (load %.3f), %.1f points a voxel, dropped_full %d" % (voxel, s["occupied"], s["occupied"] / C,
                                                                                     s["inserted"] / max(s["occupied"], 1), s["dropped_full"]))
    say("  (a) merge, warm, 1 launch                      %8.1f us (%.1f .. %.1f)   = %.2f of the extract" % (med[0] + (med[0][0] / med[2][0],)))
    say("      merge under a 40 m window (%6d voxels kept) %6.1f us (%.1f .. %.1f)" % ((kept,) + med[1]))
    say("      merge, cold (eager, one call after a reset, host enqueue included) %.1f us" % float(np.median(cold)))
    say("      yardstick: elo_map_extract, 2 launches     %8.1f us (%.1f .. %.1f)" % med[2])
    say("  (b) rebuild() under the window, fills included %8.1f us (%.1f .. %.1f); the fills alone (%d MB) %.1f us (%.1f .. %.1f)"
        % (med[3] + (C * 40 // 1000000,) + med[4]))
    del wm, dk, da, forms
    torch.cuda.empty_cache()

# (c) the tracked drive
rel = np.zeros((n, 7), np.float32)
rel[:, 0], rel[1:, 4] = 1.0, 0.8
R = torch.from_numpy(rel).to(dev)
fit = sensor.MapFit(iters=2)
spec = sensor.VoxelMap(voxel=0.5, log2_capacity=args.log2)
per_scan = []
for window in (None, sensor.MapWindow(radius=40.0, every=10)):
    wm = world_map.WorldMap(spec, dev, fit=fit, window=window)
    t = []
    for _ in range(args.drives + 1):
        wm.reset()
        torch.cuda.synchronize()
        t.append(block(lambda: [wm.add(X[j:j + 1], R[j:j + 1]) for j in range(n)], 1) / n)
    per_scan.append((float(np.median(t[1:])), min(t[1:]), max(t[1:]), wm.window_stats(), wm.stats()))
    del wm
    torch.cuda.empty_cache()
say("(c) tracked add() (MapFit(iters=2), voxel 0.5 m), one scan a call, eager, the %d-scan drive %d times, us per scan, median (min .. max):"
    % (n, args.drives))
say("    without a window (the add() as it was)   %8.1f us (%.1f .. %.1f)" % per_scan[0][:3])
say("    MapWindow(radius=40, every=10)           %8.1f us (%.1f .. %.1f)   = %.3f of it; %d rebuilds, %d voxels evicted, %d occupied"
    % (per_scan[1][:3] + (per_scan[1][0] / per_scan[0][0], per_scan[1][3]["rebuilds"], per_scan[1][3]["evicted_voxels"],
                         per_scan[1][4]["occupied"])))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

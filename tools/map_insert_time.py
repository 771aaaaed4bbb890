"""Time of elo_map_insert on ONE 64x1800 range image of the synthetic scene ("kitti" profile of synth: half of the cells empty) at
voxel 0.5 m and 0.1 m, and -- in the same run, as the yardstick -- of elo_model_render with K = 1 on the same image: the same bytes
read, one 64-bit integer atomic per point, three launches.  Each form is recorded into a hipGraph of its own (the device's time, not
the host's enqueue rate), the graphs replayed ALTERNATING in one process, device events around blocks of replays, the median block.
The map is WARM in the timed blocks (replays insert the same scan again: every key is found, nothing is claimed) -- what a drive does
to the part of the map it keeps looking at; a COLD insert (the table just reset: every voxel is claimed) is timed on its own, reset
outside the events.  DESIGN.md gives ~4.7 us for a dependent launch on this machine whatever it does.
python tools/map_insert_time.py [--out profiles/map_insert.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--voxels", type=float, nargs="+", default=[0.5, 0.1])
ap.add_argument("--reps", type=int, default=200, help="calls per timed block")
ap.add_argument("--rounds", type=int, default=15, help="alternating blocks per form")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "map_insert.txt"))
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


scan = synth.range_image(H, W, seed=30, yaw=0.0, shift=(0.0, 0.0, 0.0), profile="kitti", scene_seed=30)
xyz = torch.from_numpy(scan[None]).to(dev)
pose64 = torch.tensor([[0.9998, 0.0, 0.0, 0.02, 12.5, -3.25, 0.4]], dtype=torch.float64, device=dev)
pose32 = pose64.float().reshape(1, 1, 7).contiguous()
src = xyz.reshape(1, 1, H, W, 3)
points = int((xyz != 0).any(-1).sum())
maps = [world_map.WorldMap(sensor.VoxelMap(voxel=v), dev) for v in args.voxels]
for m in maps:
    m.insert(xyz, pose64)
torch.cuda.synchronize()
forms = [recorded(lambda: ops.model_render(src, pose32))] + [recorded(lambda m=m: m.insert(xyz, pose64)) for m in maps]
for m in maps:                                     # (the recording's warm-up inserted too: start over, one scan in)
    m.reset()
    m.insert(xyz, pose64)
voxels = [m.stats()["occupied"] for m in maps]
for fn in forms:
    block(fn, max(args.reps // 4, 3))
times = [[] for _ in forms]
for _ in range(args.rounds):
    for k, fn in enumerate(forms):
        times[k].append(block(fn, args.reps))
med = [(float(np.median(x)), min(x), max(x)) for x in times]
cold = []
for m in maps:
    t = []
    for _ in range(args.rounds):
        m.reset()
        torch.cuda.synchronize()
        t.append(block(lambda m=m: m.insert(xyz, pose64), 1))
    cold.append(float(np.median(t)))
say("elo_map_insert on one %dx%d range image, %d points, table 2^%d slots; %d alternating blocks of %d replays, median block (min .. "
    "max), us per call; a dependent launch costs ~%.1f us on this machine (DESIGN.md)" % (H, W, points, maps[0].spec.log2_capacity,
                                                                                          args.rounds, args.reps, FLOOR_US))
say("yardstick: elo_model_render, K = 1, the same image (3 launches: clear, splat, resolve)   %.1f us (%.1f .. %.1f)" % med[0])
for v, n, (t, lo, hi), c, m in zip(args.voxels, voxels, med[1:], cold, maps):
    s = m.stats()
    say("voxel %.2f m: %d voxels, %.1f points per voxel; warm insert (1 launch) %.1f us (%.1f .. %.1f) = %.2f of the render; cold insert "
        "(eager, one call after a reset, host enqueue included) %.1f us; dropped_full %d"
        % (v, n, points / max(n, 1), t, lo, hi, t / med[0][0], c, s["dropped_full"]))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

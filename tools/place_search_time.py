"""Time of elo_scan_descriptor and elo_descriptor_search at the default ScanContext (60 sectors x 20 rings):
(a) the descriptor of one 64x1800 scan, one launch;
(b) the search of one query over m = 256 and m = 4096 entries, k = 1: both launches (every entry and every shift, then the ranking)
    as one hipGraph; the ranking's share is not taken apart;
(c) the yardstick, in the same run: elo_map_fit, ONE evaluation (iters = 0) of the same scan against a map of 20 such scans at voxel
    0.5 m.
The database is random levels (the search's work does not depend on the values, only on which columns are empty: a tenth are).
Each form is a hipGraph; the graphs are replayed ALTERNATING in one process, device events around blocks of replays; the median
block with its range.  python tools/place_search_time.py [--out profiles/place_search.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--entries", type=int, nargs="+", default=[256, 4096])
ap.add_argument("--scans", type=int, default=20, help="scans in the yardstick's map")
ap.add_argument("--reps", type=int, default=50, help="replays per timed block")
ap.add_argument("--rounds", type=int, default=9, help="alternating blocks per form")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "place_search.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda:0")
ops, synth, sensor, world_map, model = pkg("_scan_ops"), pkg("synth"), pkg("sensor"), pkg("world_map"), pkg("model")
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
    with model.graph_capture(g):
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


spec = sensor.ScanContext()
n = args.scans
scans = np.stack([synth.range_image(H, W, seed=60 + k, shift=(0.8 * k, 0.0, 0.0)) for k in range(n)])
poses = np.zeros((n, 7))
poses[:, 0], poses[:, 4] = 1.0, 0.8 * np.arange(n)
X, P = torch.from_numpy(scans).to(dev), torch.from_numpy(poses).to(dev)
wm = world_map.WorldMap(sensor.VoxelMap(voxel=0.5, log2_capacity=22), dev, fit=sensor.MapFit(iters=0))
wm.insert(X, P)
rng = np.random.default_rng(5)
cap = max(args.entries)
levels = rng.integers(1, sensor.ScanContext.LEVELS + 1, (cap, spec.sectors, spec.rings))
levels[rng.random((cap, spec.sectors)) < 0.1] = 0
db = torch.from_numpy(levels.astype(np.uint16)).to(dev)
out = torch.zeros((1, spec.sectors, spec.rings), dtype=torch.uint16, device=dev)
query = ops.scan_descriptor(X[:1], spec)
forms = [recorded(lambda: ops.scan_descriptor(X[:1], spec, out=out))]
forms += [recorded(lambda m=m: ops.descriptor_search(query, db, m, spec, 1)) for m in args.entries]
forms += [recorded(lambda: wm.fit(X[:1], P[:1]))]
med = alternating(forms)
props = torch.cuda.get_device_properties(dev)
say("place recognition at %d sectors x %d rings on %s (%d CUs); each form a hipGraph, %d alternating blocks of %d replays, median block "
    "(min .. max), us" % (spec.sectors, spec.rings, props.name, props.multi_processor_count, args.rounds, args.reps))
say("  (a) elo_scan_descriptor, one %dx%d scan, 1 launch              %8.1f us (%.1f .. %.1f)" % ((H, W) + med[0]))
for m, t in zip(args.entries, med[1:]):
    work = m * spec.sectors * spec.sectors * spec.rings
    say("  (b) elo_descriptor_search, 1 query, m = %5d, k = 1, 2 launches %8.1f us (%.1f .. %.1f)   = %.1f G integer multiply-adds / s, "
        "%.1f MB of entries" % ((m,) + t + (work / t[0] * 1e-3, m * spec.sectors * spec.rings * 2e-6)))
say("  (c) yardstick: elo_map_fit, one evaluation of the same scan, 2 launches %6.1f us (%.1f .. %.1f)" % med[-1])
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

"""Time of elo_input_stage_beams (rows by a calibrated beam table) against elo_input_stage (the uniform row formula) on the
same clouds: 2 x 150 000 points -> two 64x1800 range images, the two entries ALTERNATING in one process, device events around
blocks of calls, the median block of each.   python tools/input_stage_beams_time.py [--batch 1 8] [--out FILE]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
ap.add_argument("--points", type=int, default=150000)
ap.add_argument("--reps", type=int, default=50, help="calls per timed block")
ap.add_argument("--rounds", type=int, default=21, help="alternating blocks per entry")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda")
ops, S = pkg("_ops"), pkg("sensor")
H, W, N = 64, 1800, args.points
# the HDL-64E as built: 32 beams at 1/3 degree from +2.0, 32 at 1/2 degree from -8.83
sensor = S.Sensor(2.0, -24.8, beam_elevations_deg=[2.0 - i / 3.0 for i in range(32)] + [-8.83 - 0.5 * i for i in range(32)])
table = ops.beam_table(sensor, H, dev)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / args.reps


say("elo_input_stage_beams against elo_input_stage, 2 x %d points -> 2 x %dx%d, %d alternating blocks of %d calls, median block" % (N, H, W, args.rounds, args.reps))
for B in args.batch:
    rng = np.random.default_rng(B)
    az = rng.uniform(-np.pi, np.pi, (B, 2 * N))
    el = np.deg2rad(rng.uniform(-24.8, 2.0, (B, 2 * N)))
    r = rng.uniform(2.0, 60.0, (B, 2 * N))
    cloud = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1).astype(np.float32)
    cloud[rng.random((B, 2 * N)) < 0.05] = 0
    cloud = torch.from_numpy(cloud).to(dev)
    eye = torch.eye(4, device=dev).repeat(B, 1, 1)
    aug = torch.ones(B, dtype=torch.int32, device=dev)
    formula = lambda: ops.input_stage(cloud, eye, aug, H, W)
    beams = lambda: ops.input_stage(cloud, eye, aug, H, W, sensor=sensor, beam_elev=table)
    rows = lambda img: int((img[1] != 0).any(-1).any(-1)[0].sum())
    say("batch %d: rows of frame 1 with a return: formula %d, beam table %d" % (B, rows(formula()), rows(beams())))
    for fn in (formula, beams):
        block(fn)
    tf, tb = [], []
    for _ in range(args.rounds):
        tf.append(block(formula))
        tb.append(block(beams))
    mf, mb = float(np.median(tf)), float(np.median(tb))
    say("batch %d: elo_input_stage %.4f ms (blocks %.4f .. %.4f)   elo_input_stage_beams %.4f ms (blocks %.4f .. %.4f)   ratio %.3f"
        % (B, mf, min(tf), max(tf), mb, min(tb), max(tb), mb / mf))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

"""Time of elo_input_stage_deskew (the input stage on a scan that is not motion-compensated) on 2 x 150 000 points -> two 64x1800
range images, against the two things it can be compared with, the three forms ALTERNATING in one process, device events around
blocks of calls, the median block of each:
  (a) elo_input_stage on the same cloud (no correction: what the stage costs without it);
  (b) elo_input_stage_deskew (phase in channel 3, one motion row per batch element);
  (c) the same correction written in torch in front of elo_input_stage -- the only way to get (b)'s result without the entry.
python tools/input_stage_deskew_time.py [--batch 1 8] [--out FILE]"""
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
ap.add_argument("--rounds", type=int, default=21, help="alternating blocks per form")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda")
ops, S = pkg("_ops"), pkg("sensor")
H, W, N = 64, 1800, args.points
sweep = S.Sweep(3, 1.0)
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


def torch_deskew(cloud, motion, phase_ref):
    """The entry's correction in eager torch, fp32: (B, 2N, 4) with the phase in channel 3, motion (B,7) -> (B, 2N, 3)."""
    q = motion[:, :4] / motion[:, :4].norm(dim=1, keepdim=True)
    q = torch.where(q[:, :1] < 0, -q, q)
    vn = q[:, 1:].norm(dim=1, keepdim=True)
    u = torch.where(vn > 0, q[:, 1:] / vn, torch.zeros_like(q[:, 1:]))[:, None, :]          # (B,1,3)
    theta = 2 * torch.atan2(vn, q[:, :1])                                                   # (B,1)
    p = cloud[..., :3]
    a = cloud[..., 3] - phase_ref                                                           # (B,2N)
    half = 0.5 * (a * theta)
    w = torch.sin(half)[..., None] * u
    c = torch.cross(w, p, dim=-1)
    out = p + 2 * torch.cos(half)[..., None] * c + 2 * torch.cross(w, c, dim=-1) + a[..., None] * motion[:, None, 4:]
    return torch.where((p != 0).any(-1, keepdim=True), out, p)


say("elo_input_stage_deskew, 2 x %d points -> 2 x %dx%d, %d alternating blocks of %d calls, median block; (a) elo_input_stage, "
    "(b) elo_input_stage_deskew, (c) the correction in torch + elo_input_stage" % (N, H, W, args.rounds, args.reps))
for B in args.batch:
    rng = np.random.default_rng(B)
    az = rng.uniform(-np.pi, np.pi, (B, 2 * N))
    el = np.deg2rad(rng.uniform(-24.8, 2.0, (B, 2 * N)))
    r = rng.uniform(2.0, 60.0, (B, 2 * N))
    cloud = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), (np.pi - az) / (2 * np.pi)], -1).astype(np.float32)
    cloud[rng.random((B, 2 * N)) < 0.05, :3] = 0
    cloud = torch.from_numpy(cloud).to(dev)
    motion = np.tile(np.array([0.9990482, 0.0, 0.0, 0.0436194, 1.5, 0.1, 0.0], np.float32), (B, 1))       # 5 degrees of yaw, 1.5 m
    motion = torch.from_numpy(motion).to(dev)
    eye = torch.eye(4, device=dev).repeat(B, 1, 1)
    aug = torch.ones(B, dtype=torch.int32, device=dev)
    plain = lambda: ops.input_stage(cloud, eye, aug, H, W)
    entry = lambda: ops.input_stage(cloud, eye, aug, H, W, sweep=sweep, motion=motion)
    eager = lambda: ops.input_stage(torch_deskew(cloud, motion, sweep.phase_ref), eye, aug, H, W)
    pb, pc = entry()[0], eager()[0]
    both = (pb != 0).any(-1) & (pc != 0).any(-1)                        # (the crop may decide differently on a point at 35 m)
    say("batch %d: (b) and (c) agree within %.3g m on the %d points neither crops (of %d); the correction moves a point by up to %.2f m"
        % (B, float((pb - pc)[both].abs().max()), int(both.sum()), both.numel(), float((pb - plain()[0]).abs().max())))
    for fn in (plain, entry, eager):
        block(fn)
    ta, tb, tc = [], [], []
    for _ in range(args.rounds):
        ta.append(block(plain))
        tb.append(block(entry))
        tc.append(block(eager))
    ma, mb, mc = (float(np.median(x)) for x in (ta, tb, tc))
    say("batch %d: (a) %.4f ms (blocks %.4f .. %.4f)   (b) %.4f ms (blocks %.4f .. %.4f)   (c) %.4f ms (blocks %.4f .. %.4f)   "
        "(b)/(a) %.3f   (b)/(c) %.3f" % (B, ma, min(ta), max(ta), mb, min(tb), max(tb), mc, min(tc), max(tc), mb / ma, mb / mc))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

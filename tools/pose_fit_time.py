"""Time of elo_pose_fit on 64x1800 range images: each form recorded into a hipGraph of its own (so that the device's time is
measured, not the host's enqueue rate), the graphs replayed ALTERNATING in one process, device events around blocks of replays,
the median block of each:
  (a) one evaluation (iters = 0: the evaluate launch and the report launch);
  (b) one evaluation + solve + the evaluation at the new pose (iters = 1: four launches);
  (c) the same evaluation written in torch on the same tensors (float32, gather + elementwise + sums) -- what a user has today;
and a lane replay recorded with fit=None, fit=PoseFit() and fit=PoseFit(iters=2), replayed in turn.
DESIGN.md gives ~4.7 us for a dependent launch on this machine whatever it does; the images are L2-resident and tiny, so each of the
fit's launches is expected near that floor: the record says whether it held.
python tools/pose_fit_time.py [--batch 1 8] [--out profiles/pose_fit.txt]"""
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
ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
ap.add_argument("--reps", type=int, default=200, help="calls per timed block")
ap.add_argument("--rounds", type=int, default=15, help="alternating blocks per form")
ap.add_argument("--no-net", action="store_true", help="skip the lane replays")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "pose_fit.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("this measurement needs the GPU")
dev = torch.device("cuda:0")
ops, S, synth, model = pkg("_scan_ops"), pkg("sensor"), pkg("synth"), pkg("model")
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


def alternate(forms, reps):
    forms = [recorded(fn) for fn in forms]
    for fn in forms:
        block(fn, max(reps // 4, 3))
    times = [[] for _ in forms]
    for _ in range(args.rounds):
        for k, fn in enumerate(forms):
            times[k].append(block(fn, reps))
    return [(float(np.median(x)), min(x), max(x)) for x in times]


def torch_evaluation(x1, x2, pose, fit, consts):
    """One evaluation of the fit (uniform row formula) in eager torch, float32: the sums (A (B,6,6), b (B,6), cost, count)."""
    az_res, vert_res, vert_off = consts
    B = x1.shape[0]
    q = pose[:, :4] / pose[:, :4].norm(dim=1, keepdim=True)
    q0, q1, q2, q3 = q.unbind(1)
    Rm = torch.stack([1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2),
                      2 * (q1 * q2 + q0 * q3), 1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 - q0 * q1),
                      2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 1 - 2 * (q1 * q1 + q2 * q2)], 1).reshape(B, 3, 3)
    # the normals of frame 2
    left, right, up, down = x2.roll(1, 2), x2.roll(-1, 2), x2.roll(1, 1), x2.roll(-1, 1)
    r2 = x2.norm(dim=-1)
    ok = (x2 != 0).any(-1)
    for nb in (left, right, up, down):
        ok = ok & (nb != 0).any(-1) & ((nb.norm(dim=-1) - r2).abs() <= fit.jump_rel * r2)
    ok[:, 0] = False
    ok[:, -1] = False
    n = torch.cross(right - left, down - up, dim=-1)
    length = n.norm(dim=-1, keepdim=True)
    ok = ok & (length[..., 0] > 0)
    n = n / length.clamp_min(1e-30)
    n = torch.where(((n * x2).sum(-1, keepdim=True) > 0), -n, n)
    # the terms of frame 1
    p1 = x1.reshape(B, -1, 3)
    p = p1 @ Rm.transpose(1, 2) + pose[:, None, 4:]
    rr = p.norm(dim=-1)
    col = ((math.pi - torch.atan2(p[..., 1], p[..., 0])) / az_res).to(torch.int64).clamp(0, W - 1)
    row = (H - (torch.asin(p[..., 2] / rr) / vert_res + vert_off).nan_to_num(0.0).to(torch.int64)).clamp(0, H - 1)
    cell = (row * W + col)[..., None].expand(-1, -1, 3)
    p2 = x2.reshape(B, -1, 3).gather(1, cell)
    nn = n.reshape(B, -1, 3).gather(1, cell)
    use = (p1 != 0).any(-1) & ok.reshape(B, -1).gather(1, cell[..., 0]) & ((p - p2).norm(dim=-1) <= fit.gate)
    res = (nn * (p - p2)).sum(-1)
    J = torch.cat([torch.cross(p, nn, dim=-1), nn], -1)
    w = torch.where(res.abs() <= fit.huber, torch.ones_like(res), fit.huber / res.abs().clamp_min(1e-30)) * use
    A = torch.einsum("bn,bni,bnj->bij", w, J, J)
    b = torch.einsum("bn,bni,bn->bi", w, J, res)
    return A, b, (w * res * res).sum(1), use.sum(1)


say("elo_pose_fit on %dx%d range images, %d alternating blocks, median block (min .. max), us per call; a dependent launch costs "
    "~%.1f us on this machine (DESIGN.md)" % (H, W, args.rounds, FLOOR_US))
consts = S.projection_constants(H, W)
guess = np.array([math.cos(0.005), 0, 0, -math.sin(0.005), -0.8, 0, 0], np.float32)
for B in args.batch:
    f1, f2 = synth.frame_pair(B, H, W, seed=4)
    x1, x2 = torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)
    pose = torch.from_numpy(np.tile(guess, (B, 1))).to(dev)
    one, two = S.PoseFit(), S.PoseFit(iters=1)
    got = ops.pose_fit(x1, x2, pose, one)
    A, b, cost, count = torch_evaluation(x1, x2, pose, one, consts)
    torch.cuda.synchronize()
    say("batch %d: %d terms per image; the torch statement (float32, its own cell decisions) counts %d; info agrees within %.2g relative"
        % (B, int(got.count[0]), int(count[0]), float(((A - got.info).abs().max() / got.info.abs().max()))))
    (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = alternate(
        [lambda: ops.pose_fit(x1, x2, pose, one), lambda: ops.pose_fit(x1, x2, pose, two),
         lambda: torch_evaluation(x1, x2, pose, one, consts)], args.reps)
    say("batch %d: (a) evaluation, 2 launches %.1f us (%.1f .. %.1f)   (b) evaluation + solve + evaluation, 4 launches %.1f us "
        "(%.1f .. %.1f)   (c) torch %.1f us (%.1f .. %.1f)" % (B, ma, la, ha, mb, lb, hb, mc, lc, hc))
    say("batch %d: per launch %.1f us in (a), an evaluate + solve pair adds %.1f us in (b): %s the %.1f us floor; (c)/(a) = %.1f"
        % (B, ma / 2, mb - ma, "near" if (mb - ma) / 2 <= 1.5 * FLOOR_US else "ABOVE", FLOOR_US, mc / ma))

if not args.no_net:
    for B in args.batch:
        f1, f2 = synth.frame_pair(B, H, W, seed=4)
        pair = torch.from_numpy(np.concatenate([f1, f2], 0)).to(dev)
        nets = []
        for fit in (None, S.PoseFit(), S.PoseFit(iters=2)):
            net = model.PWCLONet(dev, seed=0)
            net.capture(B, H, W, fit=fit)
            net.lane_input(0).copy_(pair)
            nets.append(net)
        torch.cuda.synchronize()

        def timed(net, reps):
            s = net.lane_stream(0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record()
                for _ in range(reps):
                    net._lanes[0].graph.replay()
                b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / reps

        reps = max(args.reps // 4, 10)
        for net in nets:
            timed(net, 5)
        times = [[] for _ in nets]
        for _ in range(args.rounds):
            for k, net in enumerate(nets):
                times[k].append(timed(net, reps))
        med = [float(np.median(x)) for x in times]
        say("batch %d lane replay (one lane, back to back): fit=None %.1f us (%.1f .. %.1f)   PoseFit() %.1f us (%.1f .. %.1f), +%.1f us"
            "   PoseFit(iters=2) %.1f us (%.1f .. %.1f), +%.1f us"
            % (B, med[0], min(times[0]), max(times[0]), med[1], min(times[1]), max(times[1]), med[1] - med[0],
               med[2], min(times[2]), max(times[2]), med[2] - med[0]))
        del nets
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

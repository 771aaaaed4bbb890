"""Time of the captured training step FROM CLOUDS (Trainer.step_graph_points: input stage + elo_preprocess_gt + the step in
one hipGraph) next to its three parts as they were before it existed: the captured step from projections
(Trainer.step_graph), one eager elo_input_stage and the torch preprocess_gt.  On a tree without step_graph_points the
three parts are timed alone.

    python tools/train_points_timer.py [--batch 8] [--points 150000] [--reps 30] [--out FILE.json]

Times are device times (events around `reps` back-to-back calls after a warm-up), inputs resident on the device."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pkg = lambda m: importlib.import_module("efficientlo-net_amd" + ("." + m if m else ""))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--points", type=int, default=150000)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
model, training, mu = pkg("model"), pkg("training"), pkg("model_util")
B, N, H, W = args.batch, args.points, 64, 1800

rng = np.random.default_rng(0)
az = rng.uniform(-np.pi, np.pi, (B, 2 * N))
el = np.deg2rad(rng.uniform(-24.8, 2.0, (B, 2 * N)))
r = rng.uniform(2.0, 60.0, (B, 2 * N))
cloud = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1).astype(np.float32)
cloud[rng.random((B, 2 * N)) < 0.05] = 0
cloud = torch.from_numpy(cloud).to(dev)
T_aug = np.stack([training.data_augmentation(rng) for _ in range(B)])
T_trans = torch.from_numpy(T_aug.astype(np.float32)).to(dev)
T_trans_inv = torch.from_numpy(np.linalg.inv(T_aug).astype(np.float32)).to(dev)
T_gt = torch.eye(4, device=dev).repeat(B, 1, 1)
T_gt[:, 0, 3] = 0.8
aug = rng.choice([1, 2], size=B).astype(np.int32)
aug_dev = torch.from_numpy(aug).to(dev)


def timed(fn, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / args.reps


res = {"batch": B, "points": N, "H": H, "W": W, "reps": args.reps}
with torch.no_grad():
    _pts, staged = mu.input_stage(cloud, T_trans, aug, H, W)
    q_gt, t_gt = mu.preprocess_gt(T_gt, T_trans, T_trans_inv, aug)
res["input_stage_eager_ms"] = timed(lambda: mu.input_stage(cloud, T_trans, aug, H, W))
res["preprocess_gt_torch_ms"] = timed(lambda: mu.preprocess_gt(T_gt, T_trans, T_trans_inv, aug))
f1, f2 = staged[:B].clone(), staged[B:].clone()
tr = training.Trainer(model.PWCLONet(dev, seed=0), capturable=True).capture(f1, f2, q_gt, t_gt)
res["step_graph_projections_ms"] = timed(lambda: tr.step_graph(f1, f2, q_gt, t_gt))
res["sum_of_parts_ms"] = res["input_stage_eager_ms"] + res["preprocess_gt_torch_ms"] + res["step_graph_projections_ms"]
del tr
if hasattr(training.Trainer, "step_graph_points"):
    _ops = pkg("_ops")
    res["preprocess_gt_kernel_ms"] = timed(lambda: _ops.preprocess_gt(T_gt, T_trans, T_trans_inv, aug_dev))
    tp = training.Trainer(model.PWCLONet(dev, seed=0), capturable=True).capture_points(
        cloud, T_gt, T_trans, T_trans_inv, aug_dev, H_input=H, W_input=W)
    res["step_graph_points_ms"] = timed(lambda: tp.step_graph_points(cloud, T_gt, T_trans, T_trans_inv, aug_dev, H_input=H, W_input=W))
for k, v in res.items():
    print("%-28s %s" % (k, "%.3f" % v if isinstance(v, float) else v))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)

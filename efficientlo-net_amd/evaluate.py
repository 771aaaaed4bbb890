"""Sequence evaluation: KITTI scans in, `NN_pred.txt` and the KITTI relative errors out -- what
main.py:459-600 `eval_one_epoch` does around the hot path, without the TF session and the subprocess call to
kitti_evaluation.py.

    rows, (t_rel, r_rel) = run_sequence(net, root, "04", T_diff, out_dir="results")

Per sample i of a sequence the dataset hands over (scan i, scan i-1) -- sample 0 pairs scan 0 with itself
(kitti_dataset.py:66-70) -- and the network predicts the motion of the pair in the LiDAR frame; the trajectory is
the running product of  Tr . [R(q)|t] . Tr^-1  (camera frame), ONE row per sample: row 0 is sample 0's own
(near-identity) prediction, not a prepended identity (main.py:557-572).
"""
import os

import numpy as np
import torch

from . import kitti, pwclo_model
from ._check import is_a
from .local_model import DeviceTracker, ModelTracker
from .distributed import quat2mat
from .sensor import LocalModel, VoxelMap
from .world_map import WorldMap


def pose_rows(q_n4, t_n3, Tr):
    """main.py:537-572: (n,4) quaternions + (n,3) translations (LiDAR frame) -> (n,12) chained camera-frame poses."""
    Tr = np.asarray(Tr, dtype=np.float64)
    if Tr.shape != (4, 4):
        Tr = kitti.to_4x4(Tr.reshape(12))
    Tr_inv = np.linalg.inv(Tr)
    T_final, rows = None, []
    for q, t in zip(np.asarray(q_n4, dtype=np.float64), np.asarray(t_n3, dtype=np.float64)):
        TT = np.eye(4)
        TT[:3, :3] = quat2mat(q.reshape(4))
        TT[:3, 3] = t.reshape(3)
        TT = Tr @ TT @ Tr_inv
        T_final = TT if T_final is None else T_final @ TT
        rows.append(T_final[:3, :].reshape(12).copy())
    return np.stack(rows) if rows else np.zeros((0, 12))


def predict_sequence(net, root, seq, T_diff, H_input=64, W_input=1800, batch_size=1, num_points=150000, frames=None,
                     lanes=0, sensor=None, sweep=None, fit=None, model=None, world_map=None):
    """Run the network over samples `frames` (default: all scans found) of sequence `seq`; returns (q (n,4), t (n,3))
    = the l0 pose of every sample, in sample order.  Batches are padded by repeating the last sample
    (main.py:497-509 keeps stale rows instead; either way the padding rows are dropped).
    `lanes` > 0: through `lanes` hipGraphs recorded from the raw clouds on (`PWCLONet.capture(num_points=...)`: input
    stage + pyramid in one replay, several batches in flight while the host reads the next scans) instead of the eager
    `forward_points`; same results (no augmentation in evaluation: the identity T_trans of the eager call is a no-op).
    `sensor`: the LiDAR the scans come from.  A net projects with the sensor it was built with (`PWCLONet(sensor=...)`, fixed for
    its life and baked into its graphs), so this is a check that the caller and the net agree: None, or the net's.
    `sweep` (sensor.Sweep): the scans are NOT motion-compensated; the input stage de-skews both scans of every pair with a
    constant-velocity guess -- the l0 pose of the previous chunk's last pair, handed over on the device as a pose
    (`motion_is_pose`), the identity for the first chunk.  Sequential path only: with `lanes` the pairs in flight do not wait for
    one another's poses (NotImplementedError).
    `fit` (sensor.PoseFit): every l0 pose is also fitted on its pair's range images (elo_pose_fit) and the returned poses are the
    fit's `pose_out` -- the net's own with iters = 0, the polished ones otherwise (a flagged sample keeps the net's); a third
    value comes back, (n,24) float64 rows [count, rms, status, the 21 entries of the upper triangle of info, row-major].  On both
    paths.  Without it: the two values of before.
    `model` (sensor.LocalModel; needs `fit`): the fit of every sample runs against the last `model.scans` scans rendered into one
    range image (local_model.ModelTracker) instead of against the pair's frame 2.  The net runs per chunk as before; its samples
    then go through ONE tracker in order, which is reset wherever `frames` does not continue by one.  Sample i is (frame 1, frame
    2) = (scan i, scan i-1) (kitti.load_pair), so a sample's frame 2 is the frame 1 of the sample before it: what the tracker
    assumes.  The three return values are those of `fit`.  The host-driven tracker is for the sequential path only: it takes the
    samples one after the other (NotImplementedError with `lanes`).  `model.resident`: the tracker's state machine lives on the
    device (local_model.DeviceTracker) and a sample is one replay of its recorded step -- on the sequential path, and with `lanes`:
    the lanes are then captured WITHOUT a fit, chunks are collected in order as before, and every sample of a collected chunk steps
    the one tracker on the range images of the lane's clouds and the lane's pose row; its result is on the host before the lane is
    submitted again.  Without `model` nothing changes.
    `world_map` (world_map.WorldMap): every sample's frame-1 range image -- the one the net saw: with `sweep` the de-skewed one -- is
    added to the map at the pose RETURNED for that sample (the net's, the fit's or the tracker's), in sample order (WorldMap.add:
    the poses are composed onto the map's running world pose, which the caller resets between drives).  The images come from the
    input stage run once more on the chunk's clouds -- the same launches on the same bytes, as the resident tracker's branch gets
    them; the forward itself is untouched, so the return values are those of a run without the argument, bit for bit.  On the
    sequential path and with `lanes` (inside the in-order collection; the lane is not written again before the insert has read its
    clouds)."""
    is_a("world_map", world_map, WorldMap, or_none=True)
    if is_a("model", model, LocalModel, or_none=True) is not None:
        if fit is None:
            raise ValueError("a local model is what a pose fit runs against: pass fit=PoseFit(...) with model=")
        if lanes > 0 and not model.resident:
            raise NotImplementedError("the host-driven local model takes the samples in order, each after the one before: the lanes run "
                                      "chunks concurrently -- LocalModel(resident=True) steps a device tracker behind them")
    if sweep is not None and lanes > 0:
        raise NotImplementedError("de-skewing feeds each chunk the previous chunk's pose: the lanes run chunks concurrently")
    if sensor is not None and sensor != net.sensor:
        raise ValueError("this net was built for %r, the sequence is said to come from %r: build PWCLONet(sensor=...) for it"
                         % (net.sensor, sensor))
    seq_dir = os.path.join(root, seq)
    if frames is None:
        frames = range(len([f for f in os.listdir(os.path.join(seq_dir, "velodyne")) if f.endswith(".bin")]))
    frames = list(frames)
    dev = net.device
    if lanes > 0:
        return _predict_sequence_lanes(net, root, seq, T_diff, H_input, W_input, batch_size, num_points, frames, lanes, fit, model,
                                       world_map)
    eye = torch.eye(4, dtype=torch.float32, device=dev).repeat(batch_size, 1, 1)      # main.py:308-309: no augmentation
    qs, ts, fits, tracker = [], [], [], None
    skew = {} if fit is None else {"fit": fit}
    if sweep is not None:
        identity = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], device=dev).repeat(batch_size, 1)
        skew.update(sweep=sweep, motion=identity, motion_is_pose=True)
    for start in range(0, len(frames), batch_size):
        chunk = frames[start:start + batch_size]
        cloud = np.zeros((batch_size, 2 * num_points, 3), np.float32)
        T_gt = np.zeros((batch_size, 4, 4), np.float32)
        for j in range(batch_size):
            pos2, pos1, _n2, _n1, T = kitti.load_pair(root, seq, chunk[min(j, len(chunk) - 1)], T_diff, num_points)
            cloud[j, :num_points], cloud[j, num_points:], T_gt[j] = pos2, pos1, T     # main.py:316-320
        motion = {k: v for k, v in skew.items() if k != "fit"}       # (this chunk's: skew moves on below)
        if model is not None:
            if tracker is None:
                tracker = _tracker(net, H_input, W_input, model, fit)
            with torch.no_grad():                            # forward_points(fit=)'s own first half: the range images stay at hand
                _pts, both = pwclo_model.input_stage(torch.from_numpy(cloud).to(dev), eye, np.ones(batch_size, np.int64), H_input,
                                                     W_input, sensor=net.sensor, beam_elev=net.beam_elev, **motion)
            out = net.forward(both[:batch_size], both[batch_size:], False)
            pose7 = torch.cat([out[0].detach().reshape(-1, 4), out[1].detach().reshape(-1, 3)], -1).contiguous()
            if sweep is not None:
                last = len(chunk) - 1
                skew["motion"] = pose7[last].repeat(batch_size, 1).contiguous()
            pose, rows = _track(tracker, frames, start, both, pose7, len(chunk))
            qs.append(pose[:, :4].copy())
            ts.append(pose[:, 4:].copy())
            fits.append(rows)
            if world_map is not None:
                world_map.add(both[:len(chunk)], pose)
            continue
        cloud_dev = torch.from_numpy(cloud).to(dev)
        out = net.forward_points(cloud_dev, H_input, W_input, torch.from_numpy(T_gt).to(dev),
                                 eye, eye, is_training=False, aug_frame=np.ones(batch_size, np.int64), **skew)
        if sweep is not None:                                # [q_norm | t] of this chunk's last pair, for every pair of the next
            last = len(chunk) - 1
            skew["motion"] = torch.cat([out[0][last].reshape(4), out[1][last].reshape(3)]).repeat(batch_size, 1).contiguous()
        if fit is not None:
            pose = out[-1].pose[:len(chunk)].cpu().numpy()
            qs.append(pose[:, :4].copy())
            ts.append(pose[:, 4:].copy())
            fits.append(fit_rows(out[-1], len(chunk)))
        else:
            qs.append(out[0][:len(chunk)].reshape(-1, 4).cpu().numpy())
            ts.append(out[1][:len(chunk)].reshape(-1, 3).cpu().numpy())
        if world_map is not None:
            with torch.no_grad():
                _pts, both = pwclo_model.input_stage(cloud_dev, eye, np.ones(batch_size, np.int64), H_input, W_input, sensor=net.sensor,
                                                     beam_elev=net.beam_elev, **motion)
            world_map.add(both[:len(chunk)], np.concatenate([qs[-1], ts[-1]], 1))
    return _stacked(qs, ts, fits, fit)


_TRIU = np.triu_indices(6)


def fit_rows(result, n):
    """(n,24) float64: [count, rms, status | the upper triangle of info, row-major] of the first n images of a PoseFitResult."""
    stats = result.stats[:n].cpu().numpy().astype(np.float64)
    info = result.info[:n].cpu().numpy().astype(np.float64)
    return np.concatenate([stats[:, [0, 2, 3]], info[:, _TRIU[0], _TRIU[1]]], 1)


def _stacked(qs, ts, fits, fit):
    """predict_sequence's return from the per-chunk pieces: (q, t), and the fit rows where a fit was asked for."""
    q_t = (np.concatenate(qs), np.concatenate(ts))
    return q_t if fit is None else q_t + (np.concatenate(fits),)


def _track(tracker, frames, first, both, pose7, n):
    """The first `n` samples of a chunk -- samples first .. first + n - 1 of `frames` -- through the tracker, in order: `both`
    (2B,H,W,3) the chunk's stacked range images (frame 1 of sample j at j, its frame 2 at B + j), `pose7` (B,7) its pose rows ->
    (poses (n,7), fit_rows (n,24)).  The tracker is reset wherever `frames` does not continue by one, and every result is on the
    host (.cpu()) before the next step overwrites it."""
    B = both.shape[0] // 2
    poses, rows = [], []
    for j in range(n):
        i = first + j
        if i > 0 and frames[i] != frames[i - 1] + 1:
            tracker.reset()
        res = tracker.step(both[j:j + 1], both[B + j:B + j + 1], pose7[j:j + 1])
        poses.append(res.pose.cpu().numpy())
        rows.append(fit_rows(res, 1))
    return np.concatenate(poses), np.concatenate(rows)


def _tracker(net, H_input, W_input, model, fit):
    """The tracker `model` asks for: the host-driven one, or the device's with its step recorded."""
    kw = dict(sensor=net.sensor, beam_elev=net.beam_elev, device=net.device)
    if model.resident:
        return DeviceTracker(H_input, W_input, model, fit, **kw).capture()
    return ModelTracker(H_input, W_input, model, fit, **kw)


def _predict_sequence_lanes(net, root, seq, T_diff, H_input, W_input, batch_size, num_points, frames, lanes, fit=None, model=None,
                            world_map=None):
    dev = net.device
    net.capture(batch_size, H_input, W_input, lanes=lanes, num_points=num_points, fit=fit if model is None else None)
    tracker = None if model is None else _tracker(net, H_input, W_input, model, fit)      # (recorded while no lane is in flight)
    chunks = [frames[s:s + batch_size] for s in range(0, len(frames), batch_size)]
    qs, ts, fits = [None] * len(chunks), [None] * len(chunks), [None] * len(chunks)
    pinned = [torch.empty((batch_size, 2 * num_points, 3), dtype=torch.float32).pin_memory() for _ in range(lanes)]

    def collect(ci):                                         # the lane's stream has finished chunk ci
        lane = ci % lanes
        net.lane_stream(lane).synchronize()
        both = None
        if tracker is not None:
            # the range images of the lane's clouds: a lane that starts from raw clouds keeps them inside its graph (lane_input() is
            # the buffer of a lane fed with range images), so the input stage runs once more on the cloud buffer -- the same launches on
            # the same bytes.  Every result is on the host (_track) before the lane's buffers are written again.
            with torch.no_grad():
                _pts, both = pwclo_model.input_stage(net.lane_cloud(lane), None, None, H_input, W_input, sensor=net.sensor,
                                                     beam_elev=net.beam_elev)
            pose, fits[ci] = _track(tracker, frames, ci * batch_size, both, net.lane_pose(lane), len(chunks[ci]))
        elif fit is not None:
            res = net.lane_fit(lane, fit)
            pose, fits[ci] = res.pose[:len(chunks[ci])].cpu().numpy(), fit_rows(res, len(chunks[ci]))
        else:
            pose = net.lane_pose(lane)[:len(chunks[ci])].cpu().numpy()    # (b,7) = [q_norm | t] of l0
        qs[ci], ts[ci] = pose[:, :4].copy(), pose[:, 4:].copy()
        if world_map is not None:
            if both is None:
                with torch.no_grad():
                    _pts, both = pwclo_model.input_stage(net.lane_cloud(lane), None, None, H_input, W_input, sensor=net.sensor,
                                                         beam_elev=net.beam_elev)
            world_map.add(both[:len(chunks[ci])], pose)
            net.lane_stream(lane).wait_stream(torch.cuda.current_stream(dev))    # the next submit writes the clouds the stage reads

    for ci, chunk in enumerate(chunks):
        lane = ci % lanes
        if ci >= lanes:
            collect(ci - lanes)                              # frees the lane (and its pinned staging buffer)
        cloud = pinned[lane].numpy()
        for j in range(batch_size):
            pos2, pos1, _n2, _n1, _T = kitti.load_pair(root, seq, chunk[min(j, len(chunk) - 1)], T_diff, num_points)
            cloud[j, :num_points], cloud[j, num_points:] = pos2, pos1                      # main.py:316-320
        net.submit_points(lane, pinned[lane])                # async H2D into the lane's cloud buffer + one replay
    for ci in range(max(0, len(chunks) - lanes), len(chunks)):
        collect(ci)
    return _stacked(qs, ts, fits, fit)


def run_sequence(net, root, seq, T_diff, poses_gt=None, out_dir=None, **kw):
    """predict_sequence -> pose_rows -> `<out_dir>/<seq>_pred.txt` (main.py:574-583) -> KITTI errors against
    `poses_gt` ((n,12) absolute camera poses, e.g. ground_truth_pose/<seq>.txt) if given.
    Returns (rows (n,12), (t_rel %, r_rel deg/100m) or None).
    `fit=PoseFit(...)` (predict_sequence): the trajectory is built from the fit's poses and `<out_dir>/<seq>_fit.txt` holds one row
    per sample: count, rms, status and the 21 unique entries of the information matrix.
    `world_map=` a sensor.VoxelMap (a WorldMap is built for it on the net's device) or a world_map.WorldMap (used as it stands: reset
    it between drives): the scans are added to it at the poses of the trajectory (predict_sequence) and `<out_dir>/<seq>_map.bin`
    holds its voxels, float32 rows x y z count in the frame the first sample's pose leads to (WorldMap.save).
    `map_fit=MapFit(...)` with `world_map=VoxelMap(...)`: the map TRACKS -- every scan's composed pose is fitted against the map
    before the scan goes in (WorldMap(fit=)).  What predict_sequence returns does not change; `<out_dir>/<seq>_map_poses.txt`, beside
    the map, holds one row per sample: the world pose q t the scan was inserted at, then count, rms and status of its fit.
    `map_window=MapWindow(...)` with `world_map=VoxelMap(...)`: the map follows the vehicle (WorldMap(window=)).  With a map,
    `<out_dir>/<seq>_map_state.npz` holds its state (WorldMap.save_state): WorldMap.load_state continues from it.
    `places=Places(...)` with `world_map=VoxelMap(...)`: the map keeps an index of scan descriptors and looks every few scans up in
    it (WorldMap(places=)); `<out_dir>/<seq>_revisits.txt` holds one row per lookup: scan, entry, entry_scan, shift, dist."""
    wmap, map_fit, map_window = kw.get("world_map"), kw.pop("map_fit", None), kw.pop("map_window", None)
    places = kw.pop("places", None)
    if places is not None and not isinstance(wmap, VoxelMap):
        raise ValueError("places= builds the map with its index itself: pass world_map=VoxelMap(...) with it")
    if map_fit is not None and not isinstance(wmap, VoxelMap):
        raise ValueError("map_fit= builds the tracking map itself: pass world_map=VoxelMap(...) with it")
    if map_window is not None and not isinstance(wmap, VoxelMap):
        raise ValueError("map_window= builds the windowed map itself: pass world_map=VoxelMap(...) with it")
    if isinstance(wmap, VoxelMap):
        wmap = kw["world_map"] = WorldMap(wmap, device=net.device, fit=map_fit, window=map_window, places=places)
    q, t, *fit_out = predict_sequence(net, root, seq, T_diff, **kw)
    Tr = kitti.read_calib(os.path.join(root, seq, "calib.txt"))["Tr"]
    rows = pose_rows(q, t, Tr)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        kitti.write_pred_txt(os.path.join(out_dir, "%s_pred.txt" % seq), rows)
        if fit_out:
            np.savetxt(os.path.join(out_dir, "%s_fit.txt" % seq), fit_out[0], fmt="%.9e")
        if wmap is not None:
            wmap.save(os.path.join(out_dir, "%s_map.bin" % seq))
            wmap.save_state(os.path.join(out_dir, "%s_map_state.npz" % seq))
            if map_fit is not None:
                log = wmap.fit_log().cpu().numpy().astype(np.float64)
                table = np.concatenate([wmap.trajectory().cpu().numpy(), log[:, (0, 2, 3)]], 1)
                np.savetxt(os.path.join(out_dir, "%s_map_poses.txt" % seq), table, fmt="%.17g")
            if places is not None:
                np.savetxt(os.path.join(out_dir, "%s_revisits.txt" % seq), wmap.revisits().cpu().numpy(), fmt="%.17g")
    score = None
    if poses_gt is not None:
        score = kitti.overall(kitti.sequence_errors(np.asarray(poses_gt)[:len(rows)], rows))
    return rows, score

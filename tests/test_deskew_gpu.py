"""GPU: elo_input_stage_deskew -- the raw-scan input stage on a scan that is not motion-compensated.  Against a float64 restatement
(tests/deskew_reference.py) with the phase in a channel, for both row rules; bit for bit against the plain entries fed the entry's
own points, and where the correction is a no-op; `invert`; the azimuth phase; with augmentation on top; bad arguments; through the
net, eager and replayed, the motion row read at replay.

Tolerance: 2e-4 m absolute on `points`, the project's own for the point half of the input stage; a
float32 evaluation of the formula stays within 1e-5 m of float64 at these ranges."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import deskew_reference as R
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
TOL = 2e-4
SHAPES = {"formula": (2, 3000, 8, 32), "table8": (2, 3000, 8, 32), "table128": (1, 20000, 128, 64)}
TABLES = {"formula": None, "table8": R.TABLE8, "table128": R.TABLE128}
_scenes = {}


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sensor(rows):
    S = load_pkg("sensor")
    return S.Sensor() if TABLES[rows] is None else S.Sensor(beam_elevations_deg=TABLES[rows])


def _scene(rows, phase_ref, second=False):
    """(raw stride-4 cloud, motion, motion2, target, the entry's two outputs as numpy), built and run once per parametrisation."""
    key = (rows, phase_ref, second)
    if key not in _scenes:
        ops, S = load_pkg("_ops"), load_pkg("sensor")
        B, N, H, W = SHAPES[rows]
        rng = np.random.default_rng([len(rows), int(phase_ref * 2), int(second)])
        sensor = _sensor(rows)
        target = R.target_cloud(rng, B, N, H, W, ops.projection_constants(H, W, sensor), TABLES[rows])
        motion = np.stack([R.motion_row(rng, q0_negative=(b == 0), scale=(1.0 if b else 1.7)) for b in range(B)])
        motion2 = np.stack([R.motion_row(rng) for b in range(B)]) if second else None
        cloud = R.raw_scan(rng, target, motion, motion2, phase_ref)
        pts, proj = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor, sweep=S.Sweep(3, phase_ref), motion=t(motion),
                                    motion2=None if motion2 is None else t(motion2))
        _scenes[key] = (cloud, motion, motion2, target, pts, proj)
    return _scenes[key]


def _reference_points(cloud, motion, motion2, phase_ref, b, f, N, phase=None, invert=False):
    sl = slice(f * N, (f + 1) * N)
    raw = cloud[b, sl, :3].astype(np.float64)
    s = cloud[b, sl, 3].astype(np.float64) if phase is None else phase
    row = (motion2 if f and motion2 is not None else motion)[b]
    return R.deskew(raw, s, row, phase_ref, invert)


# ---- 1. against float64, the phase in a channel -------------------------------------------------------------------------
@pytest.mark.parametrize("rows,phase_ref,second", [(r, p, False) for r in SHAPES for p in (0.0, 0.5, 1.0)] + [("table8", 1.0, True)])
def test_channel_phase_against_float64(rows, phase_ref, second):
    ops = load_pkg("_ops")
    B, N, H, W = SHAPES[rows]
    cloud, motion, motion2, target, pts, proj = _scene(rows, phase_ref, second)
    pts, proj = pts.cpu().numpy(), proj.cpu().numpy()
    sensor = _sensor(rows)
    az_res, vres, voff = ops.projection_constants(H, W, sensor)
    row_of = R.formula_rows(H, vres, voff) if TABLES[rows] is None else R.nearest_beam(sensor.beam_elevations_rad())
    assert motion[0, 0] < 0 and abs(np.linalg.norm(motion[0, :4]) - 1.7) < 1e-3
    worst, duplicates, moved = 0.0, 0, 0.0
    for b in range(B):
        for f in range(2):
            img = f * B + b
            fixed = _reference_points(cloud, motion, motion2, phase_ref, b, f, N)
            live = (cloud[b, f * N:(f + 1) * N, :3] != 0).any(-1)
            assert np.abs(fixed - target[b, f * N:(f + 1) * N])[live].max() < 2e-5          # the raw cloud is the target's, to fp32 rounding
            moved = max(moved, np.abs(fixed - cloud[b, f * N:(f + 1) * N, :3])[live].max())
            want_pts = R.point_half(fixed, 35.0)
            worst = max(worst, float(np.abs(pts[img] - want_pts).max()))
            assert np.abs(pts[img] - want_pts).max() <= TOL
            assert (want_pts[~live] == 0).all() and (pts[img][~live] == 0).all()
            assert ((want_pts == 0).all(-1) & live).mean() > 0.02                          # the crop bites
            want, count = R.project(want_pts, H, W, az_res, row_of)
            assert np.array_equal((proj[img] != 0).any(-1), count > 0)                      # the same cells, none excluded
            assert (proj[img][count == 0] == 0).all()                                       # empty and blanked cells: exactly 0
            assert (np.abs(proj[img] - want) <= np.maximum(count, 1)[..., None] * TOL).all()
            assert (count == 1).sum() > 20
            duplicates += int((count > 1).sum())
            assert (count > 0).any(1).sum() >= H - 1                                        # every row the cloud reaches is occupied
    assert duplicates > 5 and moved > 0.5                                                   # sums were checked; the motion is no detail
    print("%s phase_ref %.1f: points within %.3g m of float64 (moved by up to %.2f m)" % (rows, phase_ref, worst, moved))


# ---- 2. the image is the plain entry's image of the entry's own points -----------------------------------------------
def _image_of_own_points(rows, pts, proj, B, H, W):
    ops = load_pkg("_ops")
    back = t(R.restack(pts.cpu().numpy(), B))
    again_pts, again = ops.input_stage(back, None, None, H, W, sensor=_sensor(rows))
    return _same_bits(again_pts, pts) and _same_bits(again, proj)


@pytest.mark.parametrize("rows", list(SHAPES))
def test_image_is_the_plain_entrys_image_of_its_own_points(rows):
    B, N, H, W = SHAPES[rows]
    _cloud, _m, _m2, _target, pts, proj = _scene(rows, 1.0)
    assert float(proj.abs().max()) > 0
    assert _image_of_own_points(rows, pts, proj, B, H, W)


# ---- 3. the identity and the other no-ops ------------------------------------------------------------------------------
def _formula_centres_deg(H, up=2.0, down=-24.8):
    dv = (up - down) / (H - 1)
    return [down + (H - r + 0.5) * dv for r in range(H)]


def _agreeing_cloud(rng, B, N, H, W, signed_zero_padding=False):
    """(B, 2N, 3): points at any azimuth, 0.1 .. 0.9 rows into the uniform formula's bands from below the image to above it, out to
    60 m (the crop bites), many per cell, exact duplicates, 5 % zero padding -- of every combination of +0 / -0 if asked."""
    dv = (2.0 + 24.8) / (H - 1)
    beta = (-24.8 + (rng.integers(-2, H + 2, (B, 2 * N)) + rng.uniform(0.1, 0.9, (B, 2 * N))) * dv) * R.D2R
    cloud = R.xyz(beta, rng.uniform(-np.pi, np.pi, (B, 2 * N)), rng.uniform(2.0, 60.0, (B, 2 * N))).astype(np.float32)
    for b in range(B):
        for f in range(2):
            cloud[b, rng.integers(0, N, N // 20) + f * N] = cloud[b, rng.integers(0, N, N // 20) + f * N]
    pad = rng.random((B, 2 * N)) < 0.05
    cloud[pad] = 0.0
    if signed_zero_padding:
        signs = np.array([[sx, sy, sz] for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (0.0, -0.0)], np.float32)
        cloud[pad] = signs[rng.integers(0, 8, int(pad.sum()))]
    live = ~pad
    assert not (np.signbit(cloud[live]) & (cloud[live] == 0)).any()     # no -0 component in a non-zero point
    return cloud


@pytest.mark.parametrize("rows", ["formula", "table"])
def test_identity_and_constant_phase_are_the_plain_entry(rows):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    rng = np.random.default_rng(31)
    B, N, H, W = 2, 3000, 8, 32
    sensor = S.Sensor() if rows == "formula" else S.Sensor(2.0, -24.8, beam_elevations_deg=_formula_centres_deg(H))
    cloud = np.zeros((B, 2 * N, 4), np.float32)
    cloud[..., :3] = _agreeing_cloud(rng, B, N, H, W, signed_zero_padding=True)
    cloud[..., 3] = 0.25
    identity = np.tile(np.array([1, 0, 0, 0, 0, 0, 0], np.float32), (B, 1))
    motion = np.stack([R.motion_row(rng, q0_negative=(b == 0)) for b in range(B)])
    want = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor)
    assert float(want[1].abs().max()) > 0
    calls = {"identity, channel phase": dict(sweep=S.Sweep(3, 1.0), motion=identity),
             "identity, azimuth phase": dict(sweep=S.Sweep("azimuth", 0.0), motion=identity),
             "identity as a pose": dict(sweep=S.Sweep(3, 1.0), motion=identity, motion_is_pose=True),
             "identity for frame 2 too": dict(sweep=S.Sweep(3, 0.5), motion=identity, motion2=identity),
             "phase_ref is the constant phase": dict(sweep=S.Sweep(3, 0.25), motion=motion)}
    for name, kw in calls.items():
        got = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor, **kw)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), name
    # with augmentation on top
    T_tr = np.stack([load_pkg("training").data_augmentation(np.random.default_rng(3)) for _ in range(B)]).astype(np.float32)
    aug = np.array([1, 2], np.int32)
    want = ops.input_stage(t(cloud), t(T_tr), aug, H, W, sensor=sensor)
    got = ops.input_stage(t(cloud), t(T_tr), aug, H, W, sensor=sensor, sweep=S.Sweep(3, 0.25), motion=motion)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    # a real correction leaves the paddings' bits alone, moves the rest, and blanks the same three cells
    got = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor, sweep=S.Sweep(3, 1.0), motion=motion)
    plain = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor)
    pad = t(R.stack_frames((cloud[..., :3] == 0).all(-1)))
    assert _same_bits(got[0][pad], plain[0][pad]) and bool(torch.signbit(got[0][pad]).any())
    assert float((got[0][~pad] - plain[0][~pad]).abs().max()) > 0.5
    bottom = got[1][:, H - 1]
    zero_cols = (R.zero_cell(H, W, ops.projection_constants(H, W)[0]) - (H - 1) * W, 0, W - 1)      # atan2 = +-0, pi, -pi
    for col in zero_cols:
        assert float(bottom[:, col].abs().max()) == 0
    assert (bottom != 0).any(-1).float().mean() > 0.5


# ---- 4. invert --------------------------------------------------------------------------------------------------------
def test_a_pose_row_inverted_in_the_kernel_is_its_float64_inverse():
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    B, N, H, W = SHAPES["formula"]
    cloud, motion, _m2, _target, _pts, _proj = _scene("formula", 1.0)
    inverse = np.stack([R.inverse_row(row) for row in motion]).astype(np.float32)
    a = ops.input_stage(t(cloud), None, None, H, W, sweep=S.Sweep(3, 1.0), motion=t(motion), motion_is_pose=True)[0].cpu().numpy()
    b = ops.input_stage(t(cloud), None, None, H, W, sweep=S.Sweep(3, 1.0), motion=t(inverse))[0].cpu().numpy()
    assert np.abs(a - b).max() <= TOL
    for bi in range(B):                                                # ... and both are the float64 statement of `invert`
        for f in range(2):
            want = R.point_half(_reference_points(cloud, motion, None, 1.0, bi, f, N, invert=True), 35.0)
            near = np.abs(np.hypot(want[:, 0], want[:, 1]) - 35.0) < 0.01          # (this cloud was not kept clear of the crop)
            assert np.abs(a[f * B + bi] - want)[~near].max() <= TOL
    forward = ops.input_stage(t(cloud), None, None, H, W, sweep=S.Sweep(3, 1.0), motion=t(motion))[0].cpu().numpy()
    assert np.abs(a - forward).max() > 0.5


# ---- 5. the azimuth phase -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["formula", "table8"])
def test_azimuth_phase_is_the_channel_phase_of_the_raw_azimuths(rows):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    B, N, H, W = SHAPES[rows]
    sensor = _sensor(rows)
    rng = np.random.default_rng(50 + len(rows))
    target = R.target_cloud(rng, B, N, H, W, ops.projection_constants(H, W, sensor), TABLES[rows])
    motion = np.stack([R.motion_row(rng, q0_negative=(b == 0)) for b in range(B)])
    bare = R.raw_scan_azimuth(rng, target, motion, 1.0)                 # (B, 2N, 3): no channel to look at, none needed
    host = np.zeros((B, 2 * N, 4), np.float32)
    host[..., :3] = bare
    host[..., 3] = R.azimuth_phase(bare.reshape(-1, 3).astype(np.float64)).reshape(B, 2 * N)       # s from the raw azimuths, on the host
    want = ops.input_stage(t(host), None, None, H, W, sensor=sensor, sweep=S.Sweep(3, 1.0), motion=t(motion))[0]
    pts, proj = ops.input_stage(t(bare), None, None, H, W, sensor=sensor, sweep=S.Sweep("azimuth", 1.0), motion=t(motion))
    assert float((pts - want).abs().max()) <= TOL
    assert float((pts - t(R.stack_frames(bare))).abs().max()) > 0.5     # the correction is no detail
    assert _image_of_own_points(rows, pts, proj, B, H, W)
    again = ops.input_stage(t(host), None, None, H, W, sensor=sensor, sweep=S.Sweep("azimuth", 1.0), motion=t(motion))
    assert _same_bits(again[0], pts) and _same_bits(again[1], proj)    # the stride is no part of it
    # ... and against float64, phase and all
    pts = pts.cpu().numpy()
    for b in range(B):
        for f in range(2):
            raw = bare[b, f * N:(f + 1) * N].astype(np.float64)
            fixed = R.deskew(raw, R.azimuth_phase(raw), motion[b], 1.0)
            live = (raw != 0).any(-1)
            assert np.abs(fixed - target[b, f * N:(f + 1) * N])[live].max() < 2e-5
            assert np.abs(pts[f * B + b] - R.point_half(fixed, 35.0)).max() <= TOL


# ---- 6. with augmentation on top ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["formula", "table8"])
def test_augmentation_comes_on_top_of_the_correction(rows):
    ops, S, training = load_pkg("_ops"), load_pkg("sensor"), load_pkg("training")
    B, N, H, W = SHAPES[rows]
    cloud, motion, _m2, _target, _pts, _proj = _scene(rows, 0.5)
    rng = np.random.default_rng(3)
    T_tr = np.stack([training.data_augmentation(rng) for _ in range(B)]).astype(np.float32)
    aug = np.array([1, 2], np.int32)
    pts, proj = ops.input_stage(t(cloud), t(T_tr), aug, H, W, sensor=_sensor(rows), sweep=S.Sweep(3, 0.5), motion=t(motion))
    pts = pts.cpu().numpy()
    changed = 0.0
    for b in range(B):
        for f in range(2):
            fixed = _reference_points(cloud, motion, None, 0.5, b, f, N)
            want = R.point_half(fixed, 35.0, T_tr[b] if aug[b] == f + 1 else None)
            assert np.abs(pts[f * B + b] - want).max() <= TOL
            changed = max(changed, float(np.abs(want - R.point_half(fixed, 35.0)).max()))
    assert changed > 0.1                                               # the augmentation is no identity
    # the image is the plain entry's image of these points (they are past crop and augmentation: fed back with neither)
    back = t(R.restack(pts, B))
    again = ops.input_stage(back, None, None, H, W, sensor=_sensor(rows), crop_xy=1e30)
    assert _same_bits(again[1], proj)


# ---- 7. bad arguments --------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_launch_nothing():
    ops, S, L = load_pkg("_ops"), load_pkg("sensor"), load_pkg("_lib")
    B, N, H, W = SHAPES["formula"]
    cloud, motion, _m2, _target, want_pts, want_proj = _scene("formula", 1.0)
    cloud_d, motion_d = t(cloud), t(motion)
    pts = torch.full((2 * B, N, 3), 5.0, device=DEV)
    out = torch.full((2 * B, H, W, 3), 5.0, device=DEV)
    scratch = torch.zeros((2 * B * H * W + 8 * B + 4 * B * N,), dtype=torch.int32, device=DEV)
    az, vres, voff = ops.projection_constants(H, W)

    def args(motion=motion_d.data_ptr(), mode=L.PHASE_CHANNEL, channel=3, ref=1.0, batch=B, beams=None, rows=H):
        return L.InputStageDeskewArgs(batch, N, 4, rows, W, az, vres, voff, 35.0, cloud_d.data_ptr(), None, None, pts.data_ptr(), out.data_ptr(),
                                      scratch.data_ptr(), beams, motion, None, 0, mode, channel, ref)

    table = ops.beam_table(S.Sensor(beam_elevations_deg=R.TABLE8), 8, DEV)
    for bad, message in ((args(motion=None), "null motion"), (args(channel=4), "phase_channel"), (args(channel=2), "phase_channel"),
                         (args(mode=7), "phase_mode"), (args(ref=float("nan")), "phase_ref"), (args(ref=float("inf")), "phase_ref"),
                         (args(batch=L.DESKEW_MAX_BATCH + 1), "ELO_DESKEW_MAX_BATCH"),
                         (args(beams=table.data_ptr(), rows=L.MAX_BEAMS + 1), "ELO_MAX_BEAMS")):
        with pytest.raises(L.EloError, match=message):
            L.call("elo_input_stage_deskew", bad, out)
    torch.cuda.synchronize()
    assert float((pts - 5.0).abs().max()) == 0 and float((out - 5.0).abs().max()) == 0 and int(scratch.abs().max()) == 0   # nothing ran
    # the host refuses what it can see
    with pytest.raises(L.EloError, match="without a motion"):
        ops.input_stage(cloud_d, None, None, H, W, sweep=S.Sweep(3, 1.0))
    with pytest.raises(L.EloError, match="without a sweep"):
        ops.input_stage(cloud_d, None, None, H, W, motion=motion_d)
    with pytest.raises(L.EloError, match="channel 4"):
        ops.input_stage(cloud_d, None, None, H, W, sweep=S.Sweep(4, 1.0), motion=motion_d)
    with pytest.raises(L.EloError, match="channel 3"):
        ops.input_stage(cloud_d[..., :3], None, None, H, W, sweep=S.Sweep(3, 1.0), motion=motion_d)
    with pytest.raises(L.EloError):
        ops.input_stage(cloud_d, None, None, H, W, sweep=S.Sweep(3, 1.0), motion=motion_d[:1])
    # the same argument block, valid, is right
    L.call("elo_input_stage_deskew", args(), out)
    assert _same_bits(pts, want_pts) and _same_bits(out, want_proj)


# ---- 8. through the net ------------------------------------------------------------------------------------------------
def test_a_net_deskews_eager_and_replayed_and_reads_the_motion_at_replay():
    """tests/deskew_net_replay.py in a child process: its two captures take streams from the process-wide pool and bind hardware
    queues, which in this process would move the lanes of every later test of the suite."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deskew_net_replay.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "deskew through the net: ok" in out.stdout

"""GPU: the sensor as a value.  The default sensor is today's behaviour bit for bit; elo_input_stage_beams (the row of a point =
the beam nearest in elevation) against elo_input_stage where both rules agree, against a float64 restatement on a non-uniform
table, on zero points and on bad arguments; a non-default field of view reaching every projection of the model (warp_project
forward and backward, the projection inside pose_head, the net eager and replayed); the trainer's step from clouds."""
import math
import os
import tempfile

import numpy as np
import pytest
import torch

import twins_torch as twin
from backward_check import _check
from conftest import load_pkg
from util_params import shuffle_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
D2R = math.pi / 180

TABLE8 = (1.5, -0.5, -2.5, -4.5, -9.5, -14.0, -19.0, -23.5)            # two blocks: 2 degree and ~4.5-5 degree spacing


def _xyz(beta, az, r):
    return np.stack([r * np.cos(beta) * np.cos(az), r * np.cos(beta) * np.sin(az), r * np.sin(beta)], -1).astype(np.float32)


def _distinct_ranges(rng, shape, lo=3.0, step=0.01):
    """Ranges on a 1 cm grid, every one used once: the nearest point of a cell is the same point in float32 and in float64."""
    n = int(np.prod(shape))
    return (lo + step * rng.permutation(n)).reshape(shape)


def _formula_centres_deg(H, up=2.0, down=-24.8):
    """beta_r = down + (H - r + 0.5) dv: the middle of the band the uniform formula sends to row r, so that the midpoints of
    consecutive entries are the formula's own borders."""
    dv = (up - down) / (H - 1)
    return [down + (H - r + 0.5) * dv for r in range(H)]


def _agreeing_cloud(rng, B, N, H, W, signed_zero_padding=False):
    """(B, 2N, 3) whose points sit at (beta - down) / dv = k + [0.1, 0.9] for k from below the image to above it, at any
    azimuth, with zero padding, points beyond the 35 m crop, many points per cell and exact duplicates."""
    dv = (2.0 + 24.8) / (H - 1)
    rowf = rng.integers(-2, H + 2, (B, 2 * N)) + rng.uniform(0.1, 0.9, (B, 2 * N))
    beta = (-24.8 + rowf * dv) * D2R
    az = rng.uniform(-np.pi, np.pi, (B, 2 * N))
    r = rng.uniform(2.0, 60.0, (B, 2 * N))                             # 60 m: the crop bites
    cloud = _xyz(beta, az, r)
    for b in range(B):
        for f in range(2):                                             # exact duplicates inside a frame
            src = rng.integers(0, N, N // 20) + f * N
            dst = rng.integers(0, N, N // 20) + f * N
            cloud[b, dst] = cloud[b, src]
    pad = rng.random((B, 2 * N)) < 0.05
    cloud[pad] = 0.0
    if signed_zero_padding:                                            # every combination of +0 / -0
        signs = np.array([[sx, sy, sz] for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (0.0, -0.0)], np.float32)
        cloud[pad] = signs[rng.integers(0, 8, int(pad.sum()))]
    assert (np.hypot(cloud[..., 0], cloud[..., 1]) > 35.0).mean() > 0.1
    return cloud


def _augmentation(B, seed):
    training = load_pkg("training")
    rng = np.random.default_rng(seed)
    return np.stack([training.data_augmentation(rng) for _ in range(B)]).astype(np.float32)


# ---- 1. defaults are today's ---------------------------------------------------------------------------------------
def test_the_default_sensor_is_todays_behaviour():
    ops, S, model, synth = load_pkg("_ops"), load_pkg("sensor"), load_pkg("model"), load_pkg("synth")
    rng = np.random.default_rng(1)
    B, N, H, W = 2, 3000, 8, 32
    cloud = np.zeros((B, 2 * N, 4), np.float32)                        # stride 4
    cloud[..., :3] = _agreeing_cloud(rng, B, N, H, W)
    cloud[..., 3] = 7.0
    T_tr, aug = _augmentation(B, 3), np.array([1, 2], np.int32)
    want = ops.input_stage(t(cloud), t(T_tr), aug, H, W)
    got = ops.input_stage(t(cloud), t(T_tr), aug, H, W, sensor=S.KITTI_HDL64)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and float(want[1].abs().max()) > 0
    # one forward from clouds
    f1, f2 = synth.frame_pair(1, 64, 900, seed=11)
    pts = np.concatenate([f1.reshape(1, -1, 3), f2.reshape(1, -1, 3)], 1)
    eye = torch.eye(4, device=DEV).repeat(1, 1, 1)
    net = lambda **kw: model.PWCLONet(DEV, seed=2, perm_source=load_pkg("perm").PermSource(fn=shuffle_fn), **kw)
    a = net().forward_points(t(pts), 64, 900, eye, eye, eye, aug_frame=np.array([1]))
    b = net(sensor=S.KITTI_HDL64).forward_points(t(pts), 64, 900, eye, eye, eye, aug_frame=np.array([1]))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 2. the table entry equals the formula entry where both rules agree -------------------------------------------
@pytest.mark.parametrize("B,N,H,W", [(2, 3000, 8, 32), (1, 20000, 128, 64)])
def test_beam_table_of_the_formulas_row_centres_is_the_formula(B, N, H, W):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    rng = np.random.default_rng(H)
    cloud = t(_agreeing_cloud(rng, B, N, H, W))
    sensor = S.Sensor(2.0, -24.8, beam_elevations_deg=_formula_centres_deg(H))
    want_pts, want_proj = ops.input_stage(cloud, None, None, H, W)
    got_pts, got_proj = ops.input_stage(cloud, None, None, H, W, sensor=sensor)
    assert torch.equal(got_pts, want_pts)
    assert torch.equal(got_proj, want_proj)                            # every cell of every image: no point is left out
    filled = (want_proj != 0).any(-1)
    assert filled[:, 0].any() and filled[:, H - 1].any() and filled.float().mean() > 0.5       # both clipped ends are in play
    # a table the net keeps on the device is the same call
    table = ops.beam_table(sensor, H, DEV)
    again = ops.input_stage(cloud, None, None, H, W, sensor=sensor, beam_elev=table)
    assert torch.equal(again[1], want_proj)


# ---- 3. a non-uniform table against a float64 restatement ----------------------------------------------------------
def _zero_cell(H, W, az_res):
    """The cell of a (+0, +0, +0) point: row H-1, column int((pi - atan2(+0, +0)) / az_res) as the kernels evaluate it, in fp32."""
    return (H - 1) * W + min(int(np.float32(np.pi) / np.float32(az_res)), W - 1)


def _restate(points, H, W, az_res, row_of, crop=None):
    """float64: (M,3) fp32 points of ONE image -> (cropped points (M,3) fp32, image (H,W,3) float64 = the sum of the points
    of minimum range per cell, how many were summed (H,W), the cell of every point).  `row_of(beta)`: the row rule.  The crop and the
    range that orders a cell's points are evaluated as the kernel does (fp32, no FMA); the caller keeps its points clear of
    both thresholds, so that this only fixes which of two equal-to-float32 ranges is "the" minimum: both."""
    F = np.float32
    pts = points.copy()
    if crop is not None:
        xy = np.sqrt((pts[:, 0] * pts[:, 0]).astype(F) + (pts[:, 1] * pts[:, 1]).astype(F)).astype(F)
        pts[xy > F(crop)] = 0.0
    x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
    r = np.sqrt(x * x + y * y + z * z)
    live = r > 0
    col = np.clip(np.trunc((np.pi - np.arctan2(y, x)) / az_res), 0, W - 1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        row = np.clip(row_of(np.arcsin(z / r)), 0, H - 1).astype(np.int64)
    cell = row * W + col
    r32 = np.sqrt(((pts[:, 0] * pts[:, 0]).astype(F) + (pts[:, 1] * pts[:, 1]).astype(F)).astype(F) + (pts[:, 2] * pts[:, 2]).astype(F)).astype(F)
    img, count = np.zeros((H * W, 3)), np.zeros(H * W, np.int64)
    best = np.full(H * W, np.inf)
    np.minimum.at(best, cell[live], r32[live].astype(np.float64))
    win = live & (r32 == best[cell])
    np.add.at(img, cell[win], pts[win].astype(np.float64))
    np.add.at(count, cell[win], 1)
    if not live.all():                                                 # zero points (+0, +0, +0 here) win their cell and blank it (SURVEY a-10)
        img[_zero_cell(H, W, az_res)], count[_zero_cell(H, W, az_res)] = 0.0, 0
    return pts, img.reshape(H, W, 3), count.reshape(H, W), np.where(live, cell, -1)


def _nearest_beam(table_rad):
    table = np.asarray(table_rad, np.float64)
    mids = 0.5 * (table[:-1] + table[1:])
    return lambda beta: (beta[:, None] < mids[None, :]).sum(1)         # the number of midpoints above beta


def test_non_uniform_table_against_float64():
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    rng = np.random.default_rng(3)
    B, N, H, W = 2, 3000, 8, 32
    table = np.asarray(TABLE8)
    # every point at a beam's elevation +- 0.1 degree: <= 0.3 of the smaller neighbouring gap (2 degrees), so none is near a midpoint
    # -- and small enough that the SAME cloud stays >= 0.06 rows clear of the uniform formula's borders below
    beam = rng.integers(0, H, (B, 2 * N))
    beta = (table[beam] + rng.uniform(-0.1, 0.1, (B, 2 * N))) * D2R
    az = np.pi - (rng.integers(0, W, (B, 2 * N)) + rng.uniform(0.3, 0.7, (B, 2 * N))) * (2 * np.pi / W)
    r = _distinct_ranges(rng, (B, 2 * N), step=0.005)                  # 3 .. 63 m; the crop bites from 35 m / cos(beta) on
    xy = r * np.cos(beta)
    r = np.where(np.abs(xy - 35.0) < 0.5, r + 2.0025, r)                # nobody within 0.5 m of the crop radius
    cloud = _xyz(beta, az, r)
    for b in range(B):
        for f in range(2):
            src, dst = rng.integers(0, N, 150) + f * N, rng.integers(0, N, 150) + f * N
            cloud[b, dst] = cloud[b, src]                              # exact duplicates: summed
    cloud[rng.random((B, 2 * N)) < 0.05] = 0.0
    sensor = S.Sensor(beam_elevations_deg=TABLE8)
    pts, proj = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor)
    pts, proj = pts.cpu().numpy(), proj.cpu().numpy()
    az_res = ops.projection_constants(H, W, sensor)[0]
    duplicates = 0
    for b in range(B):
        for f in range(2):
            img = f * B + b
            want_pts, want, count, _cell = _restate(cloud[b, f * N:(f + 1) * N], H, W, az_res, _nearest_beam(sensor.beam_elevations_rad()), crop=35.0)
            assert np.array_equal(pts[img], want_pts)
            one = count <= 1
            assert np.array_equal(proj[img][one], want[one].astype(np.float32))         # the winner's xyz, bit for bit (empty cells: 0)
            many = ~one
            duplicates += int(many.sum())
            ulp = np.spacing(np.abs(want[many]).astype(np.float32)).astype(np.float64)
            assert (np.abs(proj[img][many] - want[many]) <= count[many][:, None] * ulp).all()   # 1 ulp per addend
            assert (count > 0).any(1).all()                                              # all 8 rows are occupied
            assert ((proj[img] != 0).any(-1)).any(1).all()
    assert duplicates > 20
    # the same cloud through the uniform formula at (2, -24) degrees: the eight beams fall in rows 2, 2, 3, 3, 5, 6, 7, 7
    _pts, uniform = ops.input_stage(t(cloud), None, None, H, W, sensor=S.Sensor(fov_up_deg=2, fov_down_deg=-24))
    occupied = (uniform != 0).any(-1).any(-1).cpu().numpy()             # (2B, H)
    for img in range(2 * B):
        assert set(np.nonzero(~occupied[img])[0].tolist()) == {0, 1, 4}


# ---- 4. zero points -------------------------------------------------------------------------------------------------
def test_signed_zero_points_blank_the_same_cells():
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    rng = np.random.default_rng(4)
    B, N, H, W = 2, 3000, 8, 32
    sensor = S.Sensor(2.0, -24.8, beam_elevations_deg=_formula_centres_deg(H))
    # paddings only: every combination of +0 / -0, nothing else
    signs = np.array([[sx, sy, sz] for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (0.0, -0.0)], np.float32)
    zeros = signs[rng.integers(0, 8, (B, 2 * N))]
    a, b = ops.input_stage(t(zeros), None, None, H, W), ops.input_stage(t(zeros), None, None, H, W, sensor=sensor)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(b[1].abs().max()) == 0
    # ... and among real points, which also fall in the bottom row: the three cells the zero points win stay blank in both
    cloud = _agreeing_cloud(rng, B, N, H, W, signed_zero_padding=True)
    a, b = ops.input_stage(t(cloud), None, None, H, W), ops.input_stage(t(cloud), None, None, H, W, sensor=sensor)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    bottom = b[1][:, H - 1]                                            # (2B, W, 3)
    zero_cols = (_zero_cell(H, W, ops.projection_constants(H, W)[0]) - (H - 1) * W, 0, W - 1)     # atan2 = +-0, pi, -pi (SURVEY a-10)
    for col in zero_cols:
        assert float(bottom[:, col].abs().max()) == 0
    assert (bottom != 0).any(-1).float().mean() > 0.5                  # the rest of that row is filled
    # without the paddings those cells are not blank: it is the zero points that blank them
    live = cloud.copy()
    live[(cloud == 0).all(-1)] = (9.0, 3.0, -1.5)
    live[np.hypot(live[..., 0], live[..., 1]) > 34.0] *= 0.4          # (a cropped point is a zero point too)
    c = ops.input_stage(t(live), None, None, H, W, sensor=sensor)[1][:, H - 1]
    assert all(float(c[:, col].abs().max()) > 0 for col in zero_cols)


# ---- 5. bad arguments -----------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_launch_nothing():
    ops, S, L = load_pkg("_ops"), load_pkg("sensor"), load_pkg("_lib")
    rng = np.random.default_rng(5)
    B, N, H, W = 1, 3000, 8, 32
    cloud = t(_agreeing_cloud(rng, B, N, H, W))
    sensor = S.Sensor(beam_elevations_deg=TABLE8)
    want = [x.clone() for x in ops.input_stage(cloud, None, None, H, W, sensor=sensor)]
    with pytest.raises(L.EloError, match="ELO_MAX_BEAMS"):             # H = 257
        ops.input_stage(cloud, None, None, 257, W, sensor=S.Sensor(beam_elevations_deg=np.linspace(15.0, -25.0, 257)))
    # a null table, straight at the entry point
    pts = torch.full((2 * B, N, 3), 5.0, device=DEV)
    out = torch.full((2 * B, H, W, 3), 5.0, device=DEV)
    scratch = torch.zeros((2 * B * H * W + 8 * B + 4 * B * N,), dtype=torch.int32, device=DEV)
    az = ops.projection_constants(H, W, sensor)[0]
    args = L.InputStageBeamsArgs(B, N, 3, H, W, az, 35.0, cloud.data_ptr(), None, None, pts.data_ptr(), out.data_ptr(), scratch.data_ptr(), None)
    with pytest.raises(L.EloError, match="null beam table"):
        L.call("elo_input_stage_beams", args, out)
    torch.cuda.synchronize()
    assert float((pts - 5.0).abs().max()) == 0 and float((out - 5.0).abs().max()) == 0 and int(scratch.abs().max()) == 0   # nothing ran
    # an ascending table: the host refuses it where it can see the values
    with pytest.raises(L.EloError, match="descending"):
        ops.input_stage(cloud, None, None, H, W, beam_elev=np.asarray(TABLE8[::-1]) * D2R)
    with pytest.raises(L.EloError, match="descending"):
        ops.beam_table(np.asarray(TABLE8[::-1]) * D2R, H, DEV)
    with pytest.raises(L.EloError):                                    # 8 beams, 16 rows
        ops.input_stage(cloud, None, None, 16, W, sensor=sensor)
    # a valid call after them gives the right image
    got = ops.input_stage(cloud, None, None, H, W, sensor=sensor)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = ops.input_stage(cloud, None, None, H, W, beam_elev=np.asarray(TABLE8) * D2R)
    assert torch.equal(got[1], want[1])


# ---- 6. a non-default uniform field of view reaches every projection ----------------------------------------------
HDL32 = dict(fov_up_deg=10.67, fov_down_deg=-30.67)


def _safe_points(rng, B, N, H, W, consts, r_lo=10.0, r_hi=30.0):
    """tests/backward_check._boundary_safe_points at the sensor's constants: every point 0.3 cells or more from a border, so the
    float64 restatement excludes none (the cap is 1 %)."""
    az_res, vres, voff = consts
    col = rng.integers(0, W, (B, N)) + rng.uniform(0.3, 0.7, (B, N))
    rowf = rng.integers(1, H, (B, N)) + rng.uniform(0.3, 0.7, (B, N))
    return np.pi - col * az_res, (rowf - voff) * vres, rng.uniform(r_lo, r_hi, (B, N))


def test_a_field_of_view_reaches_warp_project_and_its_backward(monkeypatch):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    sensor = S.Sensor(**HDL32)
    rng = np.random.default_rng(6)
    B, H, W, C = 2, 32, 64, 16
    N = H * W
    consts = ops.projection_constants(H, W, sensor)
    az, beta, _r = _safe_points(rng, B, N, H, W, consts)
    pc = _xyz(beta, az, _distinct_ranges(rng, (B, N), lo=10.0))
    _w, proj, _f = ops.warp_project(t(pc), None, None, None, H, W, sensor=sensor)
    proj = proj.cpu().numpy()
    az_res, vres, voff = consts
    formula = lambda beta: H - np.trunc(beta / vres + voff)
    moved = 0
    for b in range(B):
        _p, want, count, cell = _restate(pc[b], H, W, az_res, formula)
        assert count.max() == 1 and np.array_equal(proj[b], want.astype(np.float32))        # no point excluded
        d = ops.projection_constants(H, W)
        _p, _i, _c, cell_default = _restate(pc[b], H, W, d[0], lambda beta: H - np.trunc(beta / d[1] + d[2]))
        moved += int((cell != cell_default).sum())
    assert moved > N                                                    # these constants are not the default's
    assert not torch.equal(ops.warp_project(t(pc), None, None, None, H, W)[1], t(proj))
    # backward: float64 autograd of the restatement (tests/twins_torch.warp_project) at the sensor's constants
    monkeypatch.setattr(twin, "projection_constants", lambda H_, W_: ops.projection_constants(H_, W_, sensor))
    az, beta, r = _safe_points(rng, B, N, H, W, consts)
    pc = _xyz(beta, az, r)
    pc[rng.random((B, N)) < 0.1] = 0
    feat = rng.normal(0, 1, (B, N, C)).astype(np.float32)
    q = np.array([[1.0, 2e-4, -1e-4, 3e-4], [1.0, -2e-4, 1e-4, 2e-4]], np.float32)
    tt = np.array([[0.02, 0.005, -0.002], [-0.01, 0.01, 0.001]], np.float32)
    hip = lambda x, f, q_, t_: ops.warp_project(x, f, q_, t_, H, W, sensor=sensor)
    ref = lambda x, f, q_, t_: twin.warp_project(x, f, q_, t_, H, W)
    _check(hip, ref, [t(pc), t(feat), t(q), t(tt)], wrt=[0, 1, 2, 3], tol=2e-4)
    az, beta, r = _safe_points(rng, B, N, H, W, consts)
    _check(lambda x, f: ops.warp_project(x, f, None, None, H, W, sensor=sensor), lambda x, f: twin.warp_project(x, f, None, None, H, W),
           [t(_xyz(beta, az, r)), t(feat)], wrt=[0, 1])


def test_a_field_of_view_reaches_the_projection_inside_pose_head():
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    sensor = S.Sensor(**HDL32)
    rng = np.random.default_rng(7)
    B, H, W, C = 2, 32, 64, 16
    N = H * W
    az, beta, r = _safe_points(rng, B, N, H, W, ops.projection_constants(H, W, sensor))
    pc = _xyz(beta, az, r)
    pc[rng.random((B, N)) < 0.1] = 0
    feat = t(rng.normal(0, 1, (B, N, C)).astype(np.float32))
    f, w = (t(rng.normal(0, 1, (B, 116, 64)).astype(np.float32)) for _ in range(2))
    xyz_small = t(rng.normal(0, 5, (B, 116, 3)).astype(np.float32))
    head = (t(rng.normal(0, .1, (64, 256)).astype(np.float32)), t(rng.normal(0, .1, (256,)).astype(np.float32)),
            t(rng.normal(0, .1, (256, 4)).astype(np.float32)), t(np.array([1, 0, 0, 0], np.float32)),
            t(rng.normal(0, .1, (256, 3)).astype(np.float32)), t(np.zeros(3, np.float32)))
    buf = ops.ProjectionBuffers(B, N, H, W, C, DEV)
    buf.out_xyz.fill_(float("nan")); buf.out_feat.fill_(-3.0); buf.scratch.fill_(5)
    q, tt, _qn = ops.pose_head(f, w, xyz_small, *head, clear=buf, warp=(t(pc), feat), sensor=sensor)
    assert buf.result is not None
    got = ops.warp_project(t(pc), feat, q, tt, H, W, buffers=buf, sensor=sensor)          # hands the stored result over
    want = ops.warp_project(t(pc), feat, q, tt, H, W, sensor=sensor)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.allclose(got[2], want[2], atol=1e-4)
    assert not torch.equal(got[1], ops.warp_project(t(pc), feat, q, tt, H, W)[1])


def test_a_net_projects_with_its_sensor_eager_and_replayed():
    model, synth, S, perm = load_pkg("model"), load_pkg("synth"), load_pkg("sensor"), load_pkg("perm")
    sensor = S.Sensor(**HDL32)
    f1, f2 = synth.frame_pair(1, 64, 900, seed=21, sensor=sensor)
    both = torch.from_numpy(np.concatenate([f1, f2], 0)).to(DEV)
    net = lambda **kw: model.PWCLONet(DEV, seed=4, perm_source=perm.PermSource(fn=shuffle_fn), **kw)
    mine = net(sensor=sensor)
    eager = [x.clone() for x in mine.forward(both[:1], both[1:])]
    default = net().forward(both[:1], both[1:])
    assert all(torch.isfinite(x).all() for x in eager)
    for i in range(6):                                                 # l0, l1, l2 (q, t): behind a re-projection each
        assert not torch.equal(eager[i], default[i]), i
    assert torch.equal(eager[6], default[6]) and torch.equal(eager[7], default[7])      # l3: no projection in front of it
    mine.capture(1, 64, 900)
    rep = mine(both[:1], both[1:])
    torch.cuda.synchronize()
    assert all(torch.equal(e, r) for e, r in zip(eager, rep))


# ---- 7. the trainer ------------------------------------------------------------------------------------------------
def _table64():
    """A two-block 64-beam table: 32 beams at 1/3 degree from +2.0, 32 at 1/2 degree from -8.83."""
    return [2.0 - i / 3.0 for i in range(32)] + [-8.83 - 0.5 * i for i in range(32)]


def test_trainer_steps_from_clouds_with_a_beam_table():
    """One eager step_points and one captured replay with a table sensor, from the same state (a checkpoint), same visiting
    orders, same dropout seed.  The rule of tests/test_train_points_gpu.py: the eager step is run twice from that state; if it
    repeats itself bit for bit the replay's loss is bit-equal to it, else within four times that spread (printed)."""
    model, training, perm, synth, S = load_pkg("model"), load_pkg("training"), load_pkg("perm"), load_pkg("synth"), load_pkg("sensor")
    sensor = S.Sensor(beam_elevations_deg=_table64())
    H, W, N = 64, 900, 64 * 900

    def scene(seed):
        f1, f2 = synth.frame_pair(1, H, W, seed=seed, sensor=sensor)
        cloud = np.zeros((1, 2 * N, 3), np.float32)
        for half, img in enumerate((f1[0], f2[0])):
            p = img.reshape(-1, 3)
            p = p[np.any(p != 0, -1)]
            cloud[0, half * N:half * N + len(p)] = p
        T_gt = np.eye(4, dtype=np.float32)[None].copy()
        T_gt[:, 0, 3] = 0.8
        return cloud, T_gt

    trainer = lambda capturable=False: training.Trainer(
        model.PWCLONet(DEV, seed=3, perm_source=perm.PermSource(fn=shuffle_fn), sensor=sensor), capturable=capturable)
    cloud, T_gt = scene(20)
    # the table entry fills what the uniform formula leaves empty on this sensor
    ops = load_pkg("_ops")
    by_table = ops.input_stage(t(cloud), None, None, H, W, sensor=sensor)[1]
    by_formula = ops.input_stage(t(cloud), None, None, H, W, sensor=S.Sensor(sensor.fov_up_deg, sensor.fov_down_deg))[1]
    rows = lambda img: int((img != 0).any(-1).any(-1)[0].sum())
    assert rows(by_table) == 64 > rows(by_formula)
    tr = trainer(capturable=True)
    torch.manual_seed(0)
    tr.capture_points(cloud, T_gt, H_input=H, W_input=W, warmup=1)
    graph = tr._graph
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "state.npz")
        tr.save(path)
        twins = [trainer().load(path) for _ in range(2)]
    cloud2, T_gt2 = scene(31)
    runs = []
    for other in twins:
        torch.manual_seed(9)
        runs.append(float(other.step_points(cloud2, T_gt2, H_input=H, W_input=W)))
    spread = abs(runs[0] - runs[1])
    torch.manual_seed(9)
    replay = float(tr.step_graph_points(cloud2, T_gt2, H_input=H, W_input=W))
    assert tr._graph is graph and np.isfinite(replay)
    print("table sensor: replay %.9g, eager step_points %.9g (its own spread %.3g)" % (replay, runs[0], spread))
    if spread == 0.0:
        assert replay == runs[0]
    else:
        assert abs(replay - runs[0]) <= 4 * spread

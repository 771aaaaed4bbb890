"""GPU: the scan-level kernels at the cases of tests/scan_shapes_cases.py, which tests/test_scan_shapes_cpu.py vets on the CPU.

A. fit_solve_kernel (csrc/elo_fit_device.h), through _scan_ops.pose_fit and WorldMap.fit: one step against its float64 restatement
   from the sums the kernel itself reports, at dampings 0, 1e-3 and 1, under the perturbation bound scan_shapes_cases derives; two
   steps against one step fed its own result; a step of exactly zero; an exactly singular matrix; dead pose rows.
B. elo_pose_fit on images that are no multiple of its 512-cell tile, and on images of one and two columns.
C. The beam-table row rule at every length class of its padded table: the input stage plain and de-skewed, the pose-fit evaluation
   and the model render -- the render also where its loads go one float at a time.

The sums of an evaluation are compared under tests/test_pose_fit_gpu.py's bound, (n + 16) 2^-24 sum |terms|, counts exactly."""
import math
import types

import numpy as np
import pytest
import torch

import deskew_reference as D
import local_model_reference as LM
import map_fit_reference as F
import pose_fit_reference as R
import scan_shapes_cases as C
import test_map_fit_gpu as TM
import test_pose_fit_gpu as TP
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
TOL_POINTS = 2e-4                                                  # metres: tests/test_deskew_gpu.py's, of the input stage's point half


def _table_sensor(H):
    return load_pkg("sensor").Sensor(beam_elevations_deg=C.table_deg(H))


def _pose_fit(x1, x2, poses, sensor=None, **kw):
    S = load_pkg("sensor")
    poses = poses if isinstance(poses, torch.Tensor) else t(poses)
    res = load_pkg("_scan_ops").pose_fit(t(x1), t(x2), poses, S.PoseFit(**dict(R.FIT, **kw)), sensor=sensor)
    torch.cuda.synchronize()
    return res


def _bits(res):
    wide = torch.int64 if res.pose.dtype == torch.float64 else torch.int32
    return [res.pose.view(wide), res.info.view(torch.int32), res.grad.view(torch.int32), res.stats.view(torch.int32)]


def _same(a, b, rows=slice(None)):
    return all(torch.equal(u[rows], v[rows]) for u, v in zip(_bits(a), _bits(b)))


def _np64(x):
    return x.cpu().numpy().astype(np.float64)


# ---- A. the solve step ---------------------------------------------------------------------------------------------------------------
def _check_step(kind, run, starts, min_count, label, dampings=C.DAMPINGS):
    """run(iters, damping) -> the result of the fit at `starts` (B,7).  One step of every image against float64."""
    for damping in dampings:
        at, moved = run(0, damping), run(1, damping)
        assert not moved.status.any() and not at.status.any()
        info, grad, count, pose = _np64(at.info), _np64(at.grad), _np64(at.count), _np64(moved.pose)
        for b in range(len(starts)):
            want = C.reference_step(kind, starts[b], info[b], grad[b], count[b], damping, min_count)
            assert want is not None and count[b] >= min_count
            share_q, share_t = C.step_shares(kind, pose[b], want, starts[b], info[b], grad[b], damping)
            tol_q, tol_t = C.step_tolerances(kind, starts[b], info[b], grad[b], damping)
            print("%s image %d, damping %g: count %d; worst share of the bound: q %.3g, t %.3g (bounds %.3g, %.3g m)" % (
                label, b, damping, count[b], share_q, share_t, tol_q, tol_t))
            assert share_q <= 1.0 and share_t <= 1.0
            assert np.abs(pose[b] - np.asarray(starts[b], np.float64)).max() > 100 * max(tol_q, tol_t)      # it moved


@pytest.mark.parametrize("turned", [False, True])
def test_one_pose_fit_step_against_float64(turned):
    x1, x2, start, _c = C.pose_solve_case(turned)
    _check_step("turned" if turned else "pose", lambda iters, damping: _pose_fit(x1, x2, start, iters=iters, damping=damping), start, 50,
                "pose fit (turned)" if turned else "pose fit")


def _map_solve():
    wm, _table, _scans, _guess = TM._filled(0)
    scan, start, _t = C.map_solve_case()
    X = TM.dev(scan)

    def run(iters, damping, at=None):
        res = wm.fit(X, TM.dev(start) if at is None else at, fit=TM._fit(iters=iters, damping=damping))
        torch.cuda.synchronize()
        return res

    return run, start


def test_one_map_fit_step_against_float64():
    run, start = _map_solve()
    _check_step("map", run, start, F.MIN_COUNT, "map fit")


def test_two_steps_are_one_step_fed_its_own_result():
    x1, x2, start, _c = C.pose_solve_case()
    map_run, _start = _map_solve()
    for damping in (0.0, 1e-3):
        for name, run in (("pose", lambda iters, at=None: _pose_fit(x1, x2, start if at is None else at, iters=iters, damping=damping)),
                          ("map", lambda iters, at=None: map_run(iters, damping, at))):
            two, one = run(2), run(1)
            again = run(1, one.pose.clone())
            assert not two.status.any() and not torch.equal(_bits(two)[0], _bits(one)[0]), name
            assert _same(two, again), name                          # pose, info, grad and stats -- count, cost, rms, status -- bit for bit


def test_a_step_of_exactly_zero():
    x, pose = C.zero_step_case()
    res = _pose_fit(x, x, pose, iters=1)
    assert float(res.status[0]) == 0 and float(res.count[0]) == 84 and float(res.cost[0]) == 0 and float(res.rms[0]) == 0
    assert not res.grad.any()                                       # b = 0 exactly: d = 0, the series branch of the exponential
    assert np.array_equal(res.pose.cpu().numpy(), [[1.0, 0, 0, 0, 0, 0, 0]])
    assert torch.isfinite(res.info).all() and float(res.info[0].diagonal().min()) > 0


def test_an_exactly_singular_matrix_is_flagged_and_nothing_else():
    L = load_pkg("_lib")
    x1, x2, poses, _c = C.wall_case()
    P = t(poses)
    for iters, damping in ((1, 0.0), (2, 0.0), (1, 1.0)):
        res = _pose_fit(x1, x2, P, iters=iters, damping=damping)
        status = res.status.cpu().numpy().astype(np.int64)
        assert status.tolist() == [L.FIT_SINGULAR, 0], (iters, damping)
        assert torch.equal(res.pose[0].view(torch.int32), P[0].view(torch.int32))           # left exactly as it came
        assert not torch.equal(res.pose[1], P[1])                                           # its healthy neighbour moved
        assert all(torch.isfinite(v).all() for v in (res.pose, res.info, res.grad, res.stats))
        assert float(res.count[0]) == 84 and not res.info[0, 0].any() and not res.info[0, :, 0].any() and res.info[0, 3:, 3:].any()
        assert float(res.grad[0, 0]) == 0 and res.grad[0, 3:].any()
    alone, both = _pose_fit(x1[1:], x2[1:], poses[1:], iters=1), _pose_fit(x1, x2, P, iters=1)
    assert all(torch.equal(u[0], v[1]) for u, v in zip(_bits(alone), _bits(both)))          # ... as it moves on its own


def test_dead_pose_rows_in_the_pose_fit():
    L = load_pkg("_lib")
    x1, x2, good, dead, c, _dropped = C.dead_rows_case()
    H, W = x1.shape[1:3]
    G, Dd = t(good), t(dead)
    want = [R.evaluate(x1[b], x2[b], good[b], c, **R.FIT) for b in (1, 2)]
    for iters, flag in ((0, L.FIT_FEW_FINAL), (1, L.FIT_FEW | L.FIT_FEW_FINAL)):
        ok, res = _pose_fit(x1, x2, G, iters=iters), _pose_fit(x1, x2, Dd, iters=iters)
        assert res.status.cpu().numpy().astype(np.int64).tolist() == [flag, 0, 0] and not ok.status.any()
        assert torch.equal(res.pose[0].view(torch.int32), Dd[0].view(torch.int32))          # a NaN translation: back bit for bit, NaN included
        assert float(res.count[0]) == 0 and not res.info[0].any() and not res.grad[0].any() and float(res.cost[0]) == 0
        assert all(torch.isfinite(v).all() for v in (res.pose[1:], res.info, res.grad, res.stats))
        assert _same(res, ok, slice(1, 2))                                                  # the neighbour is untouched
        assert all(torch.equal(u[2], v[2]) for u, v in zip(_bits(res)[1:], _bits(ok)[1:]))  # a zero quaternion is the identity
        if iters == 0:
            assert torch.equal(res.pose[2].view(torch.int32), Dd[2].view(torch.int32))      # no step: the row as it came, zeros
            TP._compare(types.SimpleNamespace(info=res.info[1:], grad=res.grad[1:], stats=res.stats[1:]), want, H, W)
            at = res
        else:
            assert torch.equal(res.pose[2].view(torch.int32), ok.pose[2].view(torch.int32))  # ... and steps from the identity
            one = types.SimpleNamespace(info=at.info[2:], grad=at.grad[2:], count=at.count[2:], status=at.status[2:], pose=at.pose[2:])
            step = types.SimpleNamespace(info=res.info[2:], grad=res.grad[2:], count=res.count[2:], status=res.status[2:], pose=res.pose[2:])
            _check_step("pose", lambda it, damping: one if it == 0 else step, good[2:], 50, "zero quaternion", dampings=(0.0,))


# ---- B. ragged and narrow images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.RAGGED)))
def test_pose_fit_on_a_ragged_image(i):
    B, H, W = C.RAGGED[i]
    x1, x2, poses, c, _beam, _dropped = C.ragged_case(i)
    _n, parts = TP._chain(H, W)
    assert parts == math.ceil(H * W / C.FIT_TILE)
    want = [R.evaluate(x1[b], x2[b], poses[b], c, **R.FIT) for b in range(B)]
    assert tuple(ev["count"] for ev in want) == C.RAGGED_COUNTS[i]
    res = _pose_fit(x1, x2, poses, min_count=C.MIN_COUNT)
    TP._compare(res, want, H, W)
    assert not res.status.any() and torch.equal(res.pose.view(torch.int32), t(poses).view(torch.int32))
    if i in C.RAGGED_STEPS:
        _check_step("pose", lambda iters, damping: _pose_fit(x1, x2, poses, iters=iters, damping=damping, min_count=C.MIN_COUNT), poses,
                    C.MIN_COUNT, "ragged %s" % (C.RAGGED[i],), dampings=(0.0,))


@pytest.mark.parametrize("W", [1, 2])
def test_pose_fit_on_one_and_two_columns(W):
    L = load_pkg("_lib")
    x, pose, _c = C.narrow_case(W)
    P = t(pose)
    for iters, flag in ((0, L.FIT_FEW_FINAL), (1, L.FIT_FEW | L.FIT_FEW_FINAL)):
        res = _pose_fit(x, x, P, iters=iters)
        assert all(torch.isfinite(v).all() for v in (res.pose, res.info, res.grad, res.stats))
        assert float(res.count[0]) == 0 and int(res.status[0]) == flag and not res.info.any() and not res.grad.any()
        assert torch.equal(res.pose.view(torch.int32), P.view(torch.int32))


# ---- C. beam tables of every length class -------------------------------------------------------------------------------------------
def _check_image(proj, points, H):
    """One image of the input stage against the float64 projection of `points` (N,3) under the nearest-beam rule -> cells that sum."""
    want, count = C.project(points, H)
    one = count <= 1
    assert np.array_equal(proj[one], want[one].astype(np.float32))                          # the winner's xyz, bit for bit (empty cells: 0)
    many = ~one
    ulp = np.spacing(np.abs(want[many]).astype(np.float32)).astype(np.float64)
    assert (np.abs(proj[many] - want[many]) <= count[many][:, None] * ulp).all()            # 1 ulp per addend
    assert (count > 0).any(1).all() and (proj != 0).any(-1).any(1).all()                    # every row is occupied
    blank = D.zero_cells(np.asarray(points, np.float64), H, C.BEAM_W, R.constants(H, C.BEAM_W)[0])
    assert len(blank) == 3 and (blank // C.BEAM_W == H - 1).all() and not proj.reshape(-1, 3)[blank].any()
    return int(many.sum()), count


@pytest.mark.parametrize("H", C.BEAM_H)
def test_input_stage_beam_table_of_any_length(H):
    ops = load_pkg("_ops")
    W, N = C.BEAM_W, C.BEAM_N
    cloud = C.plain_cloud(H)
    pts, proj = ops.input_stage(t(cloud), None, None, H, W, sensor=_table_sensor(H))
    pts, proj = pts.cpu().numpy(), proj.cpu().numpy()
    assert abs(ops.projection_constants(H, W, _table_sensor(H))[0] - R.constants(H, W)[0]) < 1e-8
    sums = 0
    for f in range(2):
        assert np.array_equal(pts[f], cloud[0, f * N:(f + 1) * N])                          # nothing is cropped
        sums += _check_image(proj[f], cloud[0, f * N:(f + 1) * N], H)[0]
    assert sums > min(40, H * W // 3)
    print("H = %d (%d padding entries): %d cells are sums" % (H, C.padded_entries(H), sums))


@pytest.mark.parametrize("H", C.BEAM_H)
def test_deskewed_input_stage_beam_table_of_any_length(H):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    W, N = C.BEAM_W, C.BEAM_N
    raw, motion = C.skewed_cloud(H)
    target, zero, _beam, _copies = C.beam_cloud(H)
    pts, proj = ops.input_stage(t(raw), None, None, H, W, sensor=_table_sensor(H), sweep=S.Sweep(3, C.DESKEW_PHASE_REF), motion=t(motion))
    pts, proj = pts.cpu().numpy(), proj.cpu().numpy()
    worst, moved = 0.0, 0.0
    for f in range(2):
        sl = slice(f * N, (f + 1) * N)
        fixed = D.point_half(D.deskew(raw[0, sl, :3].astype(np.float64), raw[0, sl, 3].astype(np.float64), motion[0], C.DESKEW_PHASE_REF), 35.0)
        live = ~zero[0, sl]
        assert np.abs(fixed - target[0, sl])[live].max() < 2e-5                             # the raw cloud is the target's, to fp32 rounding
        worst = max(worst, float(np.abs(pts[f] - fixed).max()))
        moved = max(moved, float(np.abs(fixed - raw[0, sl, :3])[live].max()))
        assert (pts[f][~live] == 0).all() and (pts[f][live] != 0).any(-1).all()
        _sums, count = _check_image(proj[f], pts[f], H)                                     # the image of the entry's own points
        assert np.array_equal(count, C.project(target[0, sl] * live[:, None], H)[1])        # ... which fill the cells they were made for
    assert worst <= TOL_POINTS and moved > 0.5
    print("H = %d: points within %.3g m of float64 (moved by up to %.2f m)" % (H, worst, moved))


@pytest.mark.parametrize("i", range(len(C.BEAM_FIT)))
def test_pose_fit_beam_table_of_any_length(i):
    B, H, W = C.BEAM_FIT[i]
    x1, x2, poses, c, beam, _dropped = C.beam_fit_case(i)
    want = [R.evaluate(x1[b], x2[b], poses[b], c, beam_elev=beam, **R.FIT) for b in range(B)]
    assert tuple(ev["count"] for ev in want) == C.BEAM_FIT_COUNTS[i]
    res = _pose_fit(x1, x2, poses, sensor=_table_sensor(H), min_count=C.MIN_COUNT)
    TP._compare(res, want, H, W)
    assert not res.status.any()
    plain = _pose_fit(x1, x2, poses, min_count=C.MIN_COUNT)                                 # the uniform formula puts these beams into other rows
    assert not torch.equal(plain.info, res.info)


def _check_render(xyz, idx, want, K, H, W, label):
    assert np.isfinite(xyz).all() and ((idx >= -1) & (idx < K * H * W)).all()
    for b, w in enumerate(want):
        ok = ~w["ambiguous"]
        filled, empty = ok & (w["src_idx"] >= 0), ok & (w["src_idx"] < 0)
        err = np.abs(xyz[b][filled].astype(np.float64) - w["xyz"][filled]) / LM.ulp_of_largest(w["xyz"][filled])
        print("%s image %d: %d cells compared (%d filled), %d winners differ, worst point %.3f ulp of its largest component" % (
            label, b, ok.sum(), filled.sum(), (idx[b][ok] != w["src_idx"][ok]).sum(), err.max()))
        assert (idx[b][ok] == w["src_idx"][ok]).all()
        assert (err <= 1.0).all()
        assert (idx[b][empty] == -1).all() and not xyz[b][empty].view(np.int32).any()


def _render(src, pose, sensor=None):
    src = src if isinstance(src, torch.Tensor) else t(src)
    xyz, idx = load_pkg("_scan_ops").model_render(src, t(pose), sensor=sensor)
    torch.cuda.synchronize()
    return xyz.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("i", range(len(C.RENDERS)))
def test_model_render_table_and_scalar_loads(i):
    B, K, H, W, beams, _why = C.RENDERS[i]
    src, pose, _c, _beam, want = C.rendered(i)
    xyz, idx = _render(src, pose, _table_sensor(beams) if beams else None)
    _check_render(xyz, idx, want, K, H, W, "render %d" % i)
    if beams:                                                                              # the uniform formula puts these beams into other rows
        assert not np.array_equal(_render(src, pose)[1], idx)


def test_model_render_from_an_unaligned_view():
    B, K, H, W, _beams = LM.CASES[0]
    src, pose, _c, _beam, want = LM.rendered_case(0)
    room = torch.zeros((src.size + 1,), dtype=torch.float32, device=DEV)
    room[1:] = t(src).reshape(-1)
    view = room[1:].view(B, K, H, W, 3)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and (H * W) % 4 == 0          # only the address keeps it off the 16-byte loads
    xyz, idx = _render(view, pose)
    _check_render(xyz, idx, want, K, H, W, "unaligned")
    aligned = _render(src, pose)
    assert np.array_equal(xyz.view(np.int32), aligned[0].view(np.int32)) and np.array_equal(idx, aligned[1])

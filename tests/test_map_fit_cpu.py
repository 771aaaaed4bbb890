"""CPU: the float64 statement of the scan-to-map fit (tests/map_fit_reference.py) against cases made by hand and against finite
differences of its own residual, the MapFit value, the host's refusals of _scan_ops.map_fit (before the library is touched) and the cases
tests/test_map_fit_gpu.py runs the kernel on: the share of points the vetting removes, the terms every case gives, the convergence
the polish test relies on and the small synthetic drive."""
import math

import numpy as np
import pytest
import torch

import map_fit_reference as F
import world_map_reference as M
from conftest import load_pkg

EYE = np.array([1.0, 0, 0, 0, 0, 0, 0])


def test_map_fit_is_a_validated_frozen_value():
    S = load_pkg("sensor")
    f = S.MapFit()
    p = S.PoseFit()
    assert (f.iters, f.huber, f.jump_rel, f.min_count, f.damping) == (p.iters, p.huber, p.jump_rel, p.min_count, p.damping)
    assert f.gate is None and f.min_points == 1
    g = S.MapFit(iters=2, gate=0.25, huber=0.05, jump_rel=0.2, min_count=10, damping=1e-3, min_points=3)
    assert eval(repr(g), {"MapFit": S.MapFit}) == g and eval(repr(f), {"MapFit": S.MapFit}) == f
    assert hash(g) == hash(S.MapFit(2, 0.25, 0.05, 0.2, 10, 1e-3, 3)) and g != f and len({f, g, S.MapFit()}) == 2
    with pytest.raises(AttributeError):
        g.iters = 3
    for kw in (dict(iters=-1), dict(iters=1.5), dict(iters=True), dict(gate=0.0), dict(gate=-1.0), dict(gate=math.inf), dict(gate=math.nan),
               dict(huber=0.0), dict(jump_rel=-0.1), dict(damping=math.nan), dict(min_count=-1), dict(min_points=0), dict(min_points=1.5),
               dict(min_points=True)):
        with pytest.raises(ValueError):
            S.MapFit(**kw)
    # the gate against a map: the value's own, or the voxel; never beyond the voxel
    assert f.gate_for(S.VoxelMap(voxel=0.5)) == 0.5 and g.gate_for(S.VoxelMap(voxel=0.5)) == 0.25
    with pytest.raises(ValueError):
        S.MapFit(gate=0.75).gate_for(S.VoxelMap(voxel=0.5))


def test_the_host_refuses_before_the_library_is_touched():
    ops, S, L = load_pkg("_scan_ops"), load_pkg("sensor"), load_pkg("_lib")
    spec = S.VoxelMap(voxel=0.5, log2_capacity=10)
    keys, acc = torch.full((1024,), -1, dtype=torch.int64), torch.zeros((1024, 4), dtype=torch.int64)
    x, pose = torch.zeros((2, 4, 8, 3)), torch.zeros((2, 7), dtype=torch.float64)
    fit = S.MapFit()
    for call in (lambda: ops.map_fit(keys, acc, x, pose, spec, S.PoseFit()), lambda: ops.map_fit(keys, acc, x, pose, "spec", fit),
                 lambda: ops.map_fit(keys, acc, x, pose.float(), spec, fit), lambda: ops.map_fit(keys, acc, x.double(), pose, spec, fit),
                 lambda: ops.map_fit(keys.int(), acc, x, pose, spec, fit)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: ops.map_fit(keys, acc, x[:, :2], pose, spec, fit), lambda: ops.map_fit(keys, acc, x, pose[:1], spec, fit),
                 lambda: ops.map_fit(keys[:-1], acc, x, pose, spec, fit), lambda: ops.map_fit(keys, acc, x[..., :2], pose, spec, fit),
                 lambda: ops.map_fit(keys, acc, x, pose, spec, fit)):                       # (the last: CPU tensors, no fall-back)
        with pytest.raises(L.EloError):
            call()
    with pytest.raises(ValueError):
        ops.map_fit(keys, acc, x, pose, spec, S.MapFit(gate=0.75))
    W = load_pkg("world_map")
    with pytest.raises(TypeError):
        W.WorldMap(spec, "cpu", fit=S.PoseFit())
    with pytest.raises(ValueError):
        W.WorldMap(spec, "cpu", fit=S.MapFit(gate=0.75))


def _plane_table(voxel=1.0, z=0.25, n=9):
    """A table by hand: one plane of n x n voxels (ix, iy, 0), ix, iy in 0 .. n-1, one point each at the voxel's centre in x, y and
    at height z -- inserted through the reference's own rule from a one-row scan at the identity."""
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pts = np.stack([ix + 0.5, iy + 0.5, np.full(ix.shape, z)], -1).reshape(1, 1, -1, 3).astype(np.float32) * np.float32(voxel)
    return F.table_of(pts, EYE[None], voxel), pts.reshape(-1, 3)


def _patch(centre, tilt=(0.0, 0.0)):
    """A 3 x 3 scan whose middle cell is `centre`, its neighbours 0.1 m away on the plane through it with slopes `tilt` in x and
    y; the corners are empty, so the middle cell alone has a normal (columns wrap: a full row of three would have three)."""
    x = np.zeros((3, 3, 3), np.float32)
    for h in range(3):
        for w in range(3):
            dx, dy = 0.1 * (h - 1), 0.1 * (w - 1)
            if h != 1 and w != 1:
                continue
            x[h, w] = (centre[0] + dx, centre[1] + dy, centre[2] + tilt[0] * dx + tilt[1] * dy)
    return x


def test_one_point_above_a_plane_of_voxels_by_hand():
    table, pts = _plane_table()
    c = np.array([4.5, 4.5, 0.25], np.float32).astype(np.float64)
    assert np.abs(table["xyz"].astype(np.float64) - pts).max() < 1e-4                       # a single point is its voxel's centroid (to g's grid)
    cen = table["xyz"][np.searchsorted(table["key"], int(M.pack([4], [4], [0])[0]))].astype(np.float64)
    t = np.array([0.3, -0.2, 0.1])
    x = _patch((4.4 - t[0], 4.7 - t[1], 0.75 - t[2]))                                       # carried to (4.4, 4.7, 0.75): voxel (4, 4, 0)
    pose = np.concatenate([[1.0, 0, 0, 0], t])
    ev = F.evaluate(x, pose, table, 1.0, gate=1.0, huber=10.0, jump_rel=0.5)
    assert ev["count"] == 1 and ev["match"][1, 1] == int(M.pack([4], [4], [0])[0]) and (np.delete(ev["match"].reshape(-1), 4) == -1).all()
    p = x[1, 1].astype(np.float64) + t
    n = np.array([0.0, 0.0, 1.0])                                                           # a level patch seen from above: towards the sensor
    n = n if n @ x[1, 1] <= 0 else -n
    assert abs(ev["r"][0] - n @ (p - cen)) < 1e-12 and abs(abs(ev["r"][0]) - 0.5) < 1e-3
    assert np.allclose(ev["J"][0], np.concatenate([np.cross(cen - t, n), n]), atol=1e-12)
    assert np.allclose(ev["A"], np.outer(ev["J"][0], ev["J"][0])) and np.allclose(ev["b"], ev["J"][0] * ev["r"][0])
    # beyond the gate: no term; a voxel of too few points: no candidate
    assert F.evaluate(x, pose, table, 1.0, gate=0.4, huber=10.0, jump_rel=0.5)["count"] == 0
    assert F.evaluate(x, pose, table, 1.0, gate=1.0, huber=10.0, jump_rel=0.5, min_points=2)["count"] == 0
    # a pose without direction, a non-finite t: nothing
    for bad in (np.concatenate([[0.0, 0, 0, 0], t]), np.concatenate([[1.0, 0, 0, 0], [np.nan, 0, 0]])):
        e = F.evaluate(x, bad, table, 1.0, gate=1.0)
        assert e["count"] == 0 and (e["match"] == -1).all()


def test_the_nearest_centroid_may_sit_in_a_corner_neighbour():
    # two voxels only: the point's own voxel (0,0,0) holds a point in its far corner, the diagonal neighbour (1,1,1) one just across
    pts = np.array([[[[0.05, 0.05, 0.05], [1.05, 1.05, 1.05]]]], np.float32)
    table = F.table_of(pts, EYE[None], 1.0)
    assert len(table["key"]) == 2
    x = _patch((0.9, 0.9, 0.9))
    ev = F.evaluate(x, EYE, table, 1.0, gate=1.0, huber=10.0, jump_rel=0.5)
    assert ev["count"] == 1 and ev["match"][1, 1] == int(M.pack([1], [1], [1])[0])
    far = F.evaluate(_patch((0.3, 0.3, 0.3)), EYE, table, 1.0, gate=1.0, huber=10.0, jump_rel=0.5)
    assert far["count"] == 1 and far["match"][1, 1] == int(M.pack([0], [0], [0])[0])


def _walls():
    """Three planes of voxels' worth of points as a table (x = 12, y = 8, z = -1.7, seen from near the origin) and a scan of the
    same planes from the pose TRUE: every scan point lies on one plane, and so does every centroid."""
    import test_pose_fit_cpu as T
    x1, x2, _c = T._planes(24, 96)
    world = np.array([math.cos(0.2), 0, 0, math.sin(0.2), 400.0, -300.0, 5.0])
    table = F.table_of(x2[None].astype(np.float32), world[None], 1.0)
    return x1.astype(np.float32), F.compose(world, T.TRUE), table


def test_jacobian_is_the_derivative_of_the_residual_about_the_sensor():
    """r(d) of every term, its target held, under the reference's own retraction: central differences give J = [(c - t) x n | n].
    The sensor sits 500 m from the world's origin: about the origin the rotation columns would be ~500 times these."""
    x, pose, table = _walls()
    kw = dict(gate=1.0, jump_rel=0.5, huber=1e9)
    at = F.retract(pose, np.array([0.003, -0.002, 0.004, 0.06, 0.03, -0.05]))
    ev = F.evaluate(x, at, table, 1.0, **kw)
    assert ev["count"] > 200
    cen = dict(zip(table["key"].tolist(), table["xyz"].astype(np.float64)))
    c = np.stack([cen[k] for k in ev["match"].reshape(-1)[ev["cell"]]])
    ns = F.P.normals(x, 0.5)[0].reshape(-1, 3)[ev["cell"]]
    pts = x.reshape(-1, 3)[ev["cell"]].astype(np.float64)

    def residual(p7):
        Rm, t = M.rotation(p7)
        return ((ns @ Rm.T) * (pts @ Rm.T + t - c)).sum(-1)

    assert np.allclose(residual(at), ev["r"], atol=1e-9)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        num = (residual(F.retract(at, d)) - residual(F.retract(at, -d))) / (2 * h)
        assert np.abs(num - ev["J"][:, k]).max() < 1e-6
    assert np.abs(ev["J"][:, :3]).max() < 40.0                                              # sensor-relative: the scene's own extent


def test_a_step_at_least_halves_the_error_from_the_planted_start():
    _x, _table, _fixed, _start, errs = F.polish_case()
    print("error to the fixed point after 0 .. %d steps: %s" % (F.POLISH_K, errs))
    assert errs[0] > 0.1
    for k in range(F.POLISH_K):
        assert errs[k + 1] <= 0.5 * errs[k]


@pytest.mark.parametrize("i", range(len(F.SHAPES)))
def test_the_vetting_keeps_the_gpu_cases_whole(i):
    B, H, W, starved = F.SHAPES[i]
    _f2, _poses, table, scans, guess, dropped = F.case(i)
    print("case %d: %d voxels, %.2f points a voxel, dropped %s" % (i, len(table["key"]), table["acc"][:, 0].mean(), dropped))
    assert max(dropped) <= F.DROP_CAP
    assert (table["acc"][:, 0] >= 2).sum() >= 40 and len(table["key"]) < 0.5 * (1 << F.LOG2)       # voxels of several points
    for b in range(B):
        ev = F.evaluate(scans[b], guess[b], table, F.VOXEL, **F.FIT)
        assert ev["safe"][scans[b].any(-1)].all()                                            # vetted once is vetted
        if starved and b == B - 1:
            assert ev["count"] == 0
        else:
            assert ev["count"] >= F.MIN_COUNT


def test_tracking_the_small_drive_beats_dead_reckoning():
    # observed: dead reckoning ends 0.60 m (lever 20 m) from the truth, the tracked pose 0.011 m: a ratio of 0.019
    scans, _rel, biased, worlds = F.drive()
    tracked, reckoned = F.track(scans, biased.astype(np.float64), **F.FIT)
    et, ed = F.pose_error(tracked[-1], worlds[-1]), F.pose_error(reckoned[-1], worlds[-1])
    print("end pose error: tracked %.4f m, dead-reckoned %.4f m, ratio %.3f" % (et, ed, et / ed))
    assert ed > 0.2 and et < ed

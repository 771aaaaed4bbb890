"""CPU: the cases of tests/test_scan_shapes_gpu.py (tests/scan_shapes_cases.py) vetted with the float64 statements alone -- that the
solve-step check tells a wrong step from a right one, that the singular and the zero-step scenes are exact, that the ragged and the
beam-table scenes lose few points to the margin filter and give the counts they were chosen for, that every beam-table cloud reaches
every row and every kind of zero cell, and that the new render cases are mostly unambiguous."""
import math

import numpy as np
import pytest

import deskew_reference as D
import local_model_reference as LM
import map_fit_reference as F
import pose_fit_reference as R
import scan_shapes_cases as C


# ---- A. the solve step ---------------------------------------------------------------------------------------------------------------
def _sums(kind):
    """(start pose (7), reference evaluation there, min_count) of the solve case of `kind`."""
    if kind != "map":
        x1, x2, start, c = C.pose_solve_case(kind == "turned")
        return start[0], R.evaluate(x1[0], x2[0], start[0], c, **R.FIT), 50
    scan, start, table = C.map_solve_case()
    return start[0], F.evaluate(scan[0], start[0], table, F.VOXEL, **F.FIT), F.MIN_COUNT


@pytest.mark.parametrize("kind", ["pose", "turned", "map"])
def test_the_step_check_tells_a_wrong_step_from_a_right_one(kind):
    """Every deliberately wrong step lands at least OUTSIDE = 5 tolerances from the right one, at every damping it differs at --
    and the right one, restated here term by term, is the references' own.
    Measured (worst component, in tolerances; dampings 0 / 1e-3 / 1):
      pose fit   t about the sensor 1.2e3 / 1.2e3 / 1.4e3;  t + omega x t 15 / 15 / 5.6;  damping * I 71 / 8.3e4;  damping dropped
                 71 / 8.5e4;  q (x) dq 1.0 / 1.0 / 16 -- excused at the first two (scan_shapes_cases.EXCUSED says why)
      turned     as the pose fit, but q (x) dq 251 / 251 / 304
      map fit    t about the origin 9.2e5 / 9.2e5 / 1.2e6;  q (x) dq 37 / 37 / 115;  damping * I 97 / 1.2e5;  damping dropped
                 98 / 1.3e5.  (With the lever term dd (1 + |t|), |t| = 278 m, the two damping mutants would sit 0.35 tolerances
                 away in t and 3.8 in q at damping 1e-3: the start needs no enlarging once the term that does not arise is gone.)"""
    start, ev, min_count = _sums(kind)
    assert ev["count"] >= 800
    A32, b32 = ev["A"].astype(np.float32).astype(np.float64), ev["b"].astype(np.float32).astype(np.float64)
    for damping in C.DAMPINGS:
        want = C.reference_step(kind, start, A32, b32, ev["count"], damping, min_count)
        own = C.advance(start, C.solve(A32, b32, damping), kind == "map")
        assert np.abs(own - want).max() <= 1e-13                                        # the rule as advance() states it
        tol_q, tol_t = C.step_tolerances(kind, start, A32, b32, damping)
        d = C.solve(A32, b32, damping)
        print("%s fit, damping %g: |d| = %.3g, tolerances %.3g (q) %.3g (t)" % (kind, damping, np.linalg.norm(d), tol_q, tol_t))
        # the step from the unrounded sums is inside: what the bound is for
        exact = C.reference_step(kind, start, ev["A"], ev["b"], ev["count"], damping, min_count)
        assert max(C.step_shares(kind, exact, want, start, A32, b32, damping)) <= 1.0
        for name, (kinds, dampings, wrong) in C.MUTANTS.items():
            if kind not in kinds or damping not in dampings:
                continue
            far = max(C.step_shares(kind, wrong(kind, start, A32, b32, damping), want, start, A32, b32, damping))
            print("    %-20s %.3g tolerances away" % (name, far))
            assert far >= C.OUTSIDE or (kind, name, damping) in C.EXCUSED, (name, damping, far)


def test_the_zero_step_scene_is_exact():
    x, pose = C.zero_step_case()
    ev = R.evaluate(x[0], x[0], pose[0], R.constants(8, 64), **R.FIT)
    assert ev["count"] == 84 and not ev["b"].any() and ev["cost"] == 0.0
    assert np.linalg.eigvalsh(ev["A"]).min() > 0.1                                      # the solve runs; d = 0
    new = R.step(pose[0], ev)
    assert np.array_equal(new, [1.0, 0, 0, 0, 0, 0, 0])


def test_the_wall_is_exactly_singular_and_its_neighbour_healthy():
    x1, x2, poses, c = C.wall_case()
    H, W = x1.shape[1:3]
    wall = x1[0]
    assert (wall[wall.any(-1)][:, 0] == np.float32(C.WALL_X)).all() and wall.any(-1).all(0).sum() == 16
    own = np.flatnonzero(wall.any(-1).reshape(-1))
    for pose in (np.array([1.0, 0, 0, 0, 0, 0, 0]), poses[0]):                          # every point falls in its own cell, slid or not
        _q, Rm, t = R.split_pose(pose)
        row, col, margin = R.cells(wall.reshape(-1, 3)[own].astype(np.float64) @ Rm.T + t, H, W, c)
        assert np.array_equal(row * W + col, own) and margin.min() > 0.4
    n, valid, _jm, _om = R.normals(wall, R.FIT["jump_rel"])
    assert valid.sum() == 84 and (n[valid] == (-1.0, 0.0, 0.0)).all()
    ev = R.evaluate(x1[0], x2[0], poses[0], c, **R.FIT)
    assert ev["count"] == 84 and not ev["A"][0].any() and not ev["A"][:, 0].any() and ev["b"][0] == 0 and ev["b"][3:].any()
    assert ev["safe"][wall.any(-1)].all()                                               # no decision of it is near its threshold
    for damping in (0.0, 1.0):
        assert R.step(poses[0], ev, damping) is None                                    # damping multiplies a zero diagonal
    healthy = R.evaluate(x1[1], x2[1], poses[1], c, **R.FIT)
    assert healthy["count"] >= 50 and R.step(poses[1], healthy) is not None


def test_the_dead_rows_scene():
    x1, x2, good, dead, c, dropped = C.dead_rows_case()
    print("dropped %s" % dropped)
    assert max(dropped) <= R.DROP_CAP
    assert np.isnan(dead[0, 5]) and not dead[2, :4].any() and np.array_equal(dead[1], good[1]) and np.array_equal(dead[2, 4:], good[2, 4:])
    assert np.array_equal(good[2, :4], [1, 0, 0, 0])
    for b in range(3):
        ev = R.evaluate(x1[b], x2[b], good[b], c, **R.FIT)
        assert (ev["safe"] == x1[b].any(-1)).all() and ev["count"] >= 50


# ---- B. ragged and narrow images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(C.RAGGED)))
def test_the_ragged_scenes(i):
    B, H, W = C.RAGGED[i]
    x1, x2, poses, c, beam, dropped = C.ragged_case(i)
    counts = []
    for b in range(B):
        ev = R.evaluate(x1[b], x2[b], poses[b], c, **R.FIT)
        assert (ev["safe"] == x1[b].any(-1)).all()
        counts.append(ev["count"])
    print("%s: dropped %s, counts %s" % (C.RAGGED[i], ["%.2f %%" % (100 * d) for d in dropped], counts))
    assert beam is None and max(dropped) <= R.DROP_CAP
    assert tuple(counts) == C.RAGGED_COUNTS[i] and min(counts) > C.MIN_COUNT
    assert (H * W) % C.FIT_TILE != 0


def test_the_ragged_shapes_reach_the_paths_they_are_for():
    tail = {(H, W): (H * W) % C.FIT_TILE for _B, H, W in C.RAGGED}
    parts = {(H, W): math.ceil(H * W / C.FIT_TILE) for _B, H, W in C.RAGGED}
    assert parts[(5, 100)] == 1 and tail[(5, 100)] == 500                               # one ragged workgroup
    assert parts[(3, 171)] == 2 and tail[(3, 171)] == 1                                 # the last workgroup holds one cell
    assert parts[(9, 120)] == 3 and tail[(9, 120)] == 56                                # less than a wave: three waves hold no cell
    assert parts[(12, 200)] == 5 and 256 < tail[(12, 200)] < 512 and tail[(12, 200)] % 64  # the second strip ends mid-wave
    assert parts[(17, 250)] == 9 > C.FIT_SOLVE_LANES and tail[(17, 250)] == 154         # the solve's second trip round its loop


@pytest.mark.parametrize("W", [1, 2])
def test_a_narrow_image_has_no_normal(W):
    x, pose, c = C.narrow_case(W)
    assert x.any(-1).all()
    assert not R.normals(x[0], R.FIT["jump_rel"])[1].any()                              # np.roll's neighbours coincide
    assert R.evaluate(x[0], x[0], pose[0], c, **R.FIT)["count"] == 0


# ---- C. beam tables -------------------------------------------------------------------------------------------------------------------
def test_the_table_lengths_cover_every_class():
    pad = {H: C.padded_entries(H) for H in C.BEAM_H}
    assert pad == {2: 0, 3: 1, 5: 3, 6: 2, 9: 7, 17: 15, 40: 24, 129: 127, 255: 1, 256: 0}
    assert all(np.all(np.diff(np.asarray(C.table_deg(H), np.float64).astype(np.float32)) < 0) for H in C.BEAM_H)
    assert np.allclose(C.table_deg(16), R.BEAMS_DEG, rtol=0, atol=1e-12)


@pytest.mark.parametrize("H", C.BEAM_H)
def test_the_beam_clouds(H):
    W, N = C.BEAM_W, C.BEAM_N
    target, zero, beam, copies = C.beam_cloud(H)
    cloud = C.plain_cloud(H)
    rad = np.asarray(C.table_deg(H)) * (math.pi / 180)
    row_of = D.nearest_beam(rad.astype(np.float32).astype(np.float64))
    live = ~zero[0]
    p = cloud[0].astype(np.float64)
    beta = np.arcsin(p[live, 2] / np.linalg.norm(p[live], axis=-1))
    assert np.array_equal(np.clip(row_of(beta), 0, H - 1), beam[0, live])              # each point in the row it was made for
    mids = 0.5 * (rad[:-1] + rad[1:])
    clear = np.abs(beta[:, None] - mids[None, :]).min(1) / np.abs(np.diff(rad)).min()
    assert clear.min() > 0.25                                                           # ... 0.3 gaps from every midpoint, less rounding
    assert (beta > rad[0] + 0.005).sum() >= 100 and (beta < rad[-1] - 0.005).sum() >= 100       # beyond both ends
    assert (np.hypot(p[:, 0], p[:, 1]) < 34.0).all()
    ranges = np.sort(np.linalg.norm(np.unique(target[0], axis=0), axis=-1))
    assert len(ranges) < 2 * N - 200 and np.diff(ranges).min() > 0.004                  # exact duplicates; every other range is its own
    az_res = R.constants(H, W)[0]
    for f in range(2):
        pts = cloud[0, f * N:(f + 1) * N]
        dead = pts[(pts == 0).all(-1)]
        assert len({tuple(np.signbit(z)) for z in dead}) == 8                           # every combination of +0 / -0
        blank = D.zero_cells(pts.astype(np.float64), H, W, az_res)
        assert len(blank) == 3 and (blank // W == H - 1).all()
        img, count = C.project(pts, H)
        assert (count > 0).any(1).all()                                                 # every row is occupied
        assert min((count > 1).sum(), (count == 1).sum()) > min(20, H * W // 6)          # cells of one point, cells that are sums
        assert not count.reshape(-1)[blank].any()


@pytest.mark.parametrize("i", range(len(C.BEAM_FIT)))
def test_the_beam_table_fits(i):
    B, H, W = C.BEAM_FIT[i]
    x1, x2, poses, c, beam, dropped = C.beam_fit_case(i)
    counts, differs = [], False
    for b in range(B):
        ev = R.evaluate(x1[b], x2[b], poses[b], c, beam_elev=beam, **R.FIT)
        assert (ev["safe"] == x1[b].any(-1)).all()
        counts.append(ev["count"])
        plain = R.evaluate(x1[b], x2[b], poses[b], c, **R.FIT)
        differs |= plain["count"] != ev["count"] or not np.array_equal(plain["A"], ev["A"])
    print("%s: dropped %s, counts %s" % (C.BEAM_FIT[i], ["%.2f %%" % (100 * d) for d in dropped], counts))
    assert len(beam) == H and max(dropped) <= 0.009 <= R.DROP_CAP
    assert tuple(counts) == C.BEAM_FIT_COUNTS[i] and min(counts) > C.MIN_COUNT
    assert differs                                                                      # the uniform formula puts these beams into other rows


@pytest.mark.parametrize("i", range(len(C.RENDERS)))
def test_the_new_render_cases_are_mostly_unambiguous(i):
    """Measured: the 40-beam case 0.78 % ambiguous at 87 % of the cells filled; the 17 x 67 case 1.14 % at 87 %."""
    B, K, H, W, beams, _why = C.RENDERS[i]
    src, pose, _c, beam, want = C.rendered(i)
    assert (beam is None) == (beams == 0) and ((H * W) % 4 != 0) == (beams == 0)
    for b, w in enumerate(want):
        share = w["ambiguous"].mean()
        print("render %d image %d: %d points, %.1f %% of the cells filled, %.2f %% ambiguous" % (
            i, b, w["points"], 100 * (w["src_idx"] >= 0).mean(), 100 * share))
        assert share <= LM.DROP_CAP and (w["src_idx"] >= 0).mean() > 0.5
        assert set(np.unique(w["src_idx"][w["src_idx"] >= 0] // (H * W))) == set(range(K))
        if beams:
            assert (w["src_idx"] >= 0).any(1).all()                                     # every row of the table is reached

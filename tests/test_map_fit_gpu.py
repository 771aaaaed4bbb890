"""GPU: elo_map_fit (csrc/elo_mapfit.hip), world_map.WorldMap(fit=) and evaluate.run_sequence(map_fit=) against the float64 statement
of tests/map_fit_reference.py.

The cases are the ones tests/test_map_fit_cpu.py vets: every scan point whose discrete decisions (the normal's range test and
orientation, the gate, the choice between two centroids, the float32 rounding of the carried point) could flip under last-bit
differences was removed, so kernel and reference compare the SAME terms: `count` and `match` are equal exactly.

The bound on a sum is tests/test_pose_fit_gpu.py's: every product of a term is formed in double and rounded to float32 once; the
float32 additions that follow are a thread over its strip (ceil(H W / parts / 256) cells, parts = elo_map_fit_parts(H, W)), a wave
by DPP (6 steps) and the waves of a workgroup (3 additions); the partial rows are added in double.  n = strip + 6 + 3, and
|error| <= (n + 16) 2^-24 sum |terms|."""
import math
import os

import numpy as np
import pytest
import torch

import map_fit_reference as F
import test_world_map_gpu as TW
import world_map_reference as M
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dev = TW.dev
same_bits = TW.same_bits


def _fit(**kw):
    return load_pkg("sensor").MapFit(**dict(dict(F.FIT, min_count=F.MIN_COUNT), **kw))


def new_map(voxel=F.VOXEL, log2_capacity=F.LOG2, fit=None):
    return load_pkg("world_map").WorldMap(load_pkg("sensor").VoxelMap(voxel, log2_capacity), DEV, fit=fit)


def _chain(H, W):
    parts = load_pkg("_lib").lib().elo_map_fit_parts(H, W)
    assert parts == math.ceil(H * W / 256)
    return math.ceil(H * W / parts / 256) + 6 + 3, parts


def _filled(i):
    """The map of case i on the device, checked against the reference's table."""
    f2, poses, table, scans, guess, _d = F.case(i)
    wm = new_map()
    wm.insert(dev(f2), dev(poses))
    key, acc = TW.table(wm)
    assert np.array_equal(key, table["key"]) and np.array_equal(acc, table["acc"])
    return wm, table, scans, guess


def _table_of(wm):
    """The device table read back as the reference's content(): keys sorted, acc, float32 centroids by the reference's rule."""
    key, acc = TW.table(wm)
    return {"key": key, "acc": acc, "xyz": M.centroids(key, acc, wm.spec.voxel)}


def _compare(res, want, H, W):
    n, _parts = _chain(H, W)
    eps = (n + 16) * 2.0 ** -24
    info, grad, stats = (x.cpu().numpy().astype(np.float64) for x in (res.info, res.grad, res.stats))
    match = res.match.cpu().numpy()
    for b, ev in enumerate(want):
        dA, db, dc = np.abs(info[b] - ev["A"]), np.abs(grad[b] - ev["b"]), abs(stats[b, 1] - ev["cost"])
        print("image %d: count %d (reference %d); worst share of the bound: A %.3g, b %.3g; cost off by %.3g, bound %.3g" % (
            b, stats[b, 0], ev["count"], (dA / np.maximum(eps * ev["absA"], 1e-300)).max(),
            (db / np.maximum(eps * ev["absb"], 1e-300)).max(), dc, eps * ev["abscost"]))
        assert stats[b, 0] == ev["count"]
        assert np.array_equal(match[b], ev["match"])
        assert (dA <= eps * ev["absA"]).all() and (db <= eps * ev["absb"]).all() and dc <= eps * ev["abscost"]
        assert np.array_equal(info[b], info[b].T)
        rms = math.sqrt(ev["cost"] / ev["sw"]) if ev["sw"] > 0 else 0.0
        assert abs(stats[b, 2] - rms) <= 1e-5 * rms


@pytest.mark.parametrize("i", range(len(F.SHAPES)))
def test_one_evaluation_against_float64(i):
    B, H, W, starved = F.SHAPES[i]
    wm, table, scans, guess = _filled(i)
    _n, parts = _chain(H, W)
    assert parts > 1 or i == 2
    assert (H * W) % 256 != 0 or i != 3                                                  # the ragged case ends in a partial workgroup
    before = (wm.keys.clone(), wm.acc.clone(), wm.stat_words.clone())
    G = dev(guess)
    res = wm.fit(dev(scans), G, match=True, fit=_fit())
    torch.cuda.synchronize()
    want = [F.evaluate(scans[b], guess[b], table, F.VOXEL, **F.FIT) for b in range(B)]
    _compare(res, want, H, W)
    assert res.pose.dtype == torch.float64 and torch.equal(res.pose.view(torch.int64), G.view(torch.int64))     # iters = 0: bits
    status = res.status.cpu().numpy()
    assert (status[:B - 1] == 0).all() and status[B - 1] == (4 if starved else 0)
    for was, now in zip(before, (wm.keys, wm.acc, wm.stat_words)):                      # the table is only read
        assert torch.equal(was, now)
    res2 = wm.fit(dev(scans), G, match=True, fit=_fit(iters=2))
    torch.cuda.synchronize()
    for was, now in zip(before, (wm.keys, wm.acc, wm.stat_words)):
        assert torch.equal(was, now)
    assert np.isfinite(res2.covariance()[0]).all()


def _brute(wm, scan, pose, gate, jump_rel, min_points=1):
    """(H,W) int64: nearest centroid of wm.points() within the gate for every cell that has a normal, ties by key; -1 elsewhere.
    This statement knows nothing of voxels' neighbourhoods or of the hash."""
    xyz, count, key = (v.cpu().numpy() for v in wm.points())
    H, W, _ = scan.shape
    valid = F.P.normals(scan, jump_rel)[1].reshape(-1)
    out = np.full(H * W, -1, np.int64)
    if F.live_pose(pose) is None or not len(key):
        return out.reshape(H, W)
    keep = count >= min_points
    cen, key = xyz[keep].astype(np.float64), key[keep]                                  # (sorted by key: argmin takes the smaller key)
    p = M.carry(scan.reshape(-1, 3), pose)
    for c in np.flatnonzero(valid):
        e = p[c] - cen
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        j = int(np.argmin(d2)) if len(d2) else -1
        if j >= 0 and math.sqrt(d2[j]) <= gate:
            out[c] = key[j]
    return out.reshape(H, W)


def test_match_is_the_nearest_centroid_of_the_whole_map():
    wm, _table, scans, guess = _filled(0)
    res = wm.fit(dev(scans), dev(guess), match=True, fit=_fit())
    match = res.match.cpu().numpy()
    for b in range(len(scans)):
        want = _brute(wm, scans[b], guess[b], F.FIT["gate"], F.FIT["jump_rel"])
        assert (want >= 0).sum() >= F.MIN_COUNT and np.array_equal(match[b], want)


# ---- scans made of crosses: one cell with a normal per query point -----------------------------------------------------------------
T_OFF = np.array([-100.0, -50.0, -30.0])                          # the sensor's world position: integers, so x + t is exact in double
EYE_AT = np.concatenate([[2.0, 0.0, 0.0, 0.0], T_OFF])            # un-normalised; R = I exactly


def _crosses(world_points, t=T_OFF):
    """(3, 3n, 3) float32: query k is the middle cell of columns 3k .. 3k+2, its four neighbours 0.1 m off, the corners empty -- the
    middle cells alone have normals.  In the scan's frame: world - t."""
    n = len(world_points)
    x = np.zeros((3, 3 * n, 3), np.float64)
    c = np.asarray(world_points, np.float64) - t
    for h, w, off in ((1, 1, (0, 0, 0)), (0, 1, (-0.1, 0, 0.02)), (2, 1, (0.1, 0, -0.02)), (1, 0, (0, -0.1, 0.01)), (1, 2, (0, 0.1, -0.01))):
        x[h, w::3] = c + off
    return x.astype(np.float32)


def _query(wm, world_points, pose=EYE_AT, t=T_OFF, **kw):
    """The kernel's match of every query point (n,), checked against the reference on the table read back AND against brute force."""
    scan = _crosses(world_points, t)
    fit = _fit(min_count=0, jump_rel=0.5, **kw)
    res = wm.fit(dev(scan[None]), dev(pose[None]), match=True, fit=fit)
    torch.cuda.synchronize()
    got = res.match[0].cpu().numpy()
    gate = fit.gate_for(wm.spec)
    ev = F.evaluate(scan, pose, _table_of(wm), wm.spec.voxel, gate=gate, huber=fit.huber, jump_rel=0.5, min_points=fit.min_points)
    unsafe = scan.any(-1) & ~ev["safe"]                      # only: two centroids equally near, both beyond the gate -- decides nothing
    assert (ev["margins"]["tie"][unsafe] < F.TIE_REL).all() and (ev["match"][unsafe] == -1).all()
    assert (ev["margins"]["gate"][unsafe] >= F.MARGIN * gate).all()
    assert np.array_equal(got, ev["match"])
    assert np.array_equal(got, _brute(wm, scan, pose, gate, 0.5, fit.min_points))
    assert float(res.count[0]) == ev["count"] and all(torch.isfinite(v).all() for v in (res.pose, res.info, res.grad, res.stats))
    assert (np.delete(got, np.s_[1::3], 1) == -1).all() and (got[0] == -1).all() and (got[2] == -1).all()
    return got[1, 1::3]


def test_lookups_that_share_a_home_slot_and_wrap_around_the_table():
    voxels = TW._voxels_at_home((1023, 0), 5)
    rng = np.random.default_rng(21)
    pts = TW._in_voxels(np.array(voxels), rng)
    wm = new_map(0.5, 10)
    wm.insert(dev(pts.reshape(1, 1, -1, 3)), dev(TW.IDENTITY))
    xyz, _count, key = (v.cpu().numpy() for v in wm.points())
    assert len(key) == 10 and wm.stats()["dropped_full"] == 0
    slots = np.flatnonzero(wm.keys.cpu().numpy() != -1)
    assert slots.min() < 10 and slots.max() == 1023                                     # the probe sequences wrapped
    got = _query(wm, xyz.astype(np.float64), gate=0.5)
    assert np.array_equal(got, key)                                                     # every stored voxel is found, at its own centroid


def test_lookups_in_a_table_loaded_to_nine_tenths():
    a, b = np.meshgrid(np.arange(-15, 15), np.arange(-15, 16), indexing="ij")          # 930 voxels into 1024 slots
    pts = np.stack([0.75 * a + 0.05, 0.75 * b + 0.05, 0.0 * a + 0.3], -1).reshape(1, 1, -1, 3).astype(np.float32)
    wm = new_map(0.5, 10)
    wm.insert(dev(pts), dev(TW.IDENTITY))
    xyz, _count, key = (v.cpu().numpy() for v in wm.points())
    assert len(key) >= 0.85 * 1024
    got = _query(wm, xyz.astype(np.float64), gate=0.5)
    assert np.array_equal(got, key)


def test_a_full_table_finds_what_it_stored_and_nothing_else():
    a, b = np.meshgrid(np.arange(-32, 32), np.arange(-32, 32), indexing="ij")
    pts = np.stack([0.75 * a + 0.05, 0.75 * b + 0.05, 0.0 * a + 0.3], -1).reshape(1, 4, 1024, 3).astype(np.float32)
    wm = new_map(0.5, 10)
    wm.insert(dev(pts), dev(TW.IDENTITY))
    s = wm.stats()
    assert s["dropped_full"] > 0
    _xyz, _count, key = (v.cpu().numpy() for v in wm.points())
    flat = pts.reshape(-1, 3)
    want = M.classify(pts, TW.IDENTITY, 0.5)["key"].astype(np.int64)
    got = _query(wm, flat.astype(np.float64), gate=0.5)
    stored = np.isin(want, key)
    assert stored.sum() == len(key) and np.array_equal(got[stored], want[stored]) and (got[~stored] == -1).all()


def test_neighbourhood_diagonal_negative_and_the_last_index():
    # a target in a diagonal neighbour voxel, on the negative side
    wm = new_map(1.0, 10)
    pts = np.array([[-3.95, -6.95, -0.95], [-4.95, -7.95, -1.95], [5.5, 5.5, 5.5], [5.6, 5.4, 5.5], [7.5, 7.5, 7.5]], np.float32)
    wm.insert(dev(pts.reshape(1, 1, -1, 3)), dev(TW.IDENTITY))
    k = lambda *v: int(M.pack([v[0]], [v[1]], [v[2]])[0])
    got = _query(wm, np.array([[-4.1, -7.1, -1.1], [-4.7, -7.7, -1.7], [5.4, 5.6, 5.5], [7.4, 7.4, 7.6]]), gate=1.0)
    assert got.tolist() == [k(-4, -7, -1), k(-5, -8, -2), k(5, 5, 5), k(7, 7, 7)]        # the first: its own voxel (-5,-8,-2) holds a point too, further off
    # min_points = 2: the singletons are no targets
    got = _query(wm, np.array([[-4.1, -7.1, -1.1], [5.4, 5.6, 5.5], [7.4, 7.4, 7.6]]), gate=1.0, min_points=2)
    assert got.tolist() == [-1, k(5, 5, 5), -1]
    # voxel index 2^20 - 1 (voxel 1.0): the +1 neighbours along x are out of range and skipped
    wm = new_map(1.0, 10)
    edge = np.array([[1048575.25, 3.25, -2.25], [1048574.5, 3.5, -2.5]], np.float32)
    wm.insert(dev(edge.reshape(1, 1, -1, 3)), dev(TW.IDENTITY))
    assert wm.stats()["inserted"] == 2
    zero = np.zeros(3)
    got = _query(wm, np.array([[1048575.5, 3.5, -2.0]]), pose=np.array([2.0, 0, 0, 0, 0, 0, 0]), t=zero, gate=1.0)
    assert got.tolist() == [k(1048575, 3, -3)]


def test_flags_an_empty_map_and_dead_pose_rows():
    L = load_pkg("_lib")
    wm, _table, scans, guess = _filled(1)
    X = dev(scans)
    empty = new_map()
    for iters, flag in ((0, L.FIT_FEW_FINAL), (2, L.FIT_FEW | L.FIT_FEW_FINAL)):
        G = dev(guess)
        res = empty.fit(X, G, match=True, fit=_fit(iters=iters))
        assert (res.count == 0).all() and (res.status == flag).all() and (res.match == -1).all()
        assert torch.equal(res.pose.view(torch.int64), G.view(torch.int64))
        for bad in ((0, slice(0, 4), 0.0), (0, 5, math.nan)):
            g = guess.copy()
            g[bad[0], bad[1]] = bad[2]
            G = dev(g)
            res = wm.fit(X, G, match=True, fit=_fit(iters=iters))
            status = res.status.cpu().numpy().astype(np.int64)
            assert status.tolist() == [flag, 0, flag] and float(res.count[0]) == 0 and (res.match[0] == -1).all()
            assert torch.equal(res.pose[0].view(torch.int64), G[0].view(torch.int64))   # left exactly as it came, NaN and all
            assert torch.equal(res.pose[2].view(torch.int64), G[2].view(torch.int64))   # (the starved image)
            if iters:
                assert not torch.equal(res.pose[1], G[1])                              # the others move
            for v in (res.pose[1:], res.info, res.grad, res.stats):
                assert torch.isfinite(v).all()


def _bits(res):
    return [v.clone() for v in (res.pose.view(torch.int64), res.info.view(torch.int32), res.grad.view(torch.int32),
                                res.stats.view(torch.int32), res.match)]


def test_two_runs_and_a_graph_replay_agree_bit_for_bit():
    model = load_pkg("model")
    wm, _table, scans, guess = _filled(1)
    X, G = dev(scans), dev(guess)
    for iters in (0, 2):
        fit = _fit(iters=iters)
        first = _bits(wm.fit(X, G, match=True, fit=fit))
        again = _bits(wm.fit(X, G, match=True, fit=fit))
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            wm.fit(X, G, match=True, fit=fit)
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with model.graph_capture(graph):
            res = wm.fit(X, G, match=True, fit=fit)
        for v in (res.pose, res.info, res.grad, res.stats, res.match):
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, _bits(res)))


def test_polish_follows_the_reference_and_reports_the_pose_it_returns():
    x, table, fixed, start, errs = F.polish_case()
    wm = new_map()
    f2, poses = F.case(1)[:2]
    wm.insert(dev(f2), dev(poses))
    X, S = dev(x[None]), dev(start[None])
    for k in range(1, F.POLISH_K + 1):
        res = wm.fit(X, S, fit=_fit(iters=k))
        err = F.pose_error(res.pose[0].cpu().numpy(), fixed)
        print("after %d steps: kernel %.3g, reference %.3g (after %d: %.3g)" % (k, err, errs[k], k - 1, errs[k - 1]))
        assert float(res.status[0]) == 0 and err <= errs[k - 1]
    fresh = wm.fit(X, res.pose.clone(), match=True, fit=_fit())
    polished = wm.fit(X, S, match=True, fit=_fit(iters=F.POLISH_K))
    assert all(torch.equal(a, b) for a, b in zip(_bits(fresh), _bits(polished)))


def test_refusals_launch_nothing():
    L = load_pkg("_lib")
    wm, _table, scans, guess = _filled(2)
    B, H, W, _ = F.SHAPES[2]
    X, G = dev(scans), dev(guess)
    out = {"pose_out": torch.full((B, 7), -7.0, dtype=torch.float64, device=DEV), "info": torch.full((B, 36), -7.0, device=DEV),
           "grad": torch.full((B, 6), -7.0, device=DEV), "stats": torch.full((B, 4), -7.0, device=DEV),
           "match": torch.full((B, H, W), -7, dtype=torch.int64, device=DEV)}
    scratch = torch.zeros((L.lib().elo_map_fit_scratch_words(B, H, W),), dtype=torch.int32, device=DEV)
    before = (wm.keys.clone(), wm.acc.clone(), wm.stat_words.clone())

    def args(**kw):
        base = dict(batch=B, H=H, W=W, voxel=F.VOXEL, log2_capacity=F.LOG2, keys=wm.keys.data_ptr(), acc=wm.acc.data_ptr(),
                    xyz=X.data_ptr(), pose_in=G.data_ptr(), iters=1, gate=1.0, huber=0.1, jump_rel=0.2, min_count=30, damping=0.0,
                    min_points=1, scratch=scratch.data_ptr(), **{k: v.data_ptr() for k, v in out.items()})
        base.update(kw)
        return L.MapFitArgs(**base)

    L.call("elo_map_fit", args(batch=0), wm.keys)                                        # an empty batch is fine and does nothing
    inf, nan = math.inf, math.nan
    bad = [dict(keys=None), dict(acc=None), dict(xyz=None), dict(pose_in=None), dict(pose_out=None), dict(info=None), dict(grad=None),
           dict(stats=None), dict(scratch=None), dict(H=2), dict(W=0), dict(batch=-1), dict(batch=2 ** 15, H=2 ** 8, W=2 ** 8),
           dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=inf), dict(voxel=nan), dict(log2_capacity=9), dict(log2_capacity=29),
           dict(gate=0.0), dict(gate=-1.0), dict(gate=nan), dict(gate=2.5), dict(gate=inf), dict(huber=0.0), dict(huber=nan),
           dict(jump_rel=-0.1), dict(jump_rel=nan), dict(damping=-1.0), dict(damping=nan), dict(iters=-1), dict(min_points=0),
           dict(pose_out=G.data_ptr()), dict(keys=wm.keys.data_ptr() + 4), dict(acc=wm.acc.data_ptr() + 4),
           dict(pose_in=G.data_ptr() + 4), dict(pose_out=out["pose_out"].data_ptr() + 4), dict(match=out["match"].data_ptr() + 4)]
    for kw in bad:
        with pytest.raises(L.EloError):
            L.call("elo_map_fit", args(**kw), wm.keys)
    assert L.lib().elo_map_fit(None, None) == -1
    assert L.lib().elo_map_fit_scratch_words(1, 2, 8) < 0 and L.lib().elo_map_fit_parts(2, 8) < 0
    torch.cuda.synchronize()
    for was, now in zip(before, (wm.keys, wm.acc, wm.stat_words)):
        assert torch.equal(was, now)
    assert all((v == -7).all() for v in out.values()) and not scratch.any()
    L.call("elo_map_fit", args(match=None), wm.keys)                                     # match is optional
    torch.cuda.synchronize()
    assert (out["match"] == -7).all() and (out["stats"][:, 0] >= F.MIN_COUNT).all()


def test_world_map_tracks_by_compose_fit_insert():
    W = load_pkg("world_map")
    scans, _rel, biased, _worlds = F.drive()
    X, P = dev(scans[:3]), dev(biased[:3])
    fit = _fit(iters=2)
    one = new_map(fit=fit)
    one.add(X, P)
    three = new_map(fit=fit)
    for j in range(3):
        three.add(X[j:j + 1], P[j:j + 1])
    hand = new_map(fit=fit)
    world, rows = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device=DEV), []
    for j in range(3):
        guess = W.compose(world, P[j]).reshape(1, 7).contiguous()
        res = hand.fit(X[j:j + 1], guess)
        hand.insert(X[j:j + 1], res.pose)
        world = res.pose[0]
        rows.append(res.pose)
        if j == 0:                                                                       # against an empty map: flagged, in at its guess
            assert int(res.status[0]) == 1 | 4 and torch.equal(res.pose.view(torch.int64), guess.view(torch.int64))
        else:
            assert int(res.status[0]) == 0 and not torch.equal(res.pose, guess)
    rows = torch.cat(rows)
    snap = TW.snapshot(hand)
    for wm in (one, three):
        assert TW.same_snapshot(TW.snapshot(wm), snap)
        assert torch.equal(wm.world64.view(torch.int64), world.view(torch.int64))
        assert torch.equal(wm.trajectory().view(torch.int64), rows.view(torch.int64))
    assert one.last_fit.pose.shape == (3, 7) and one.last_fit.status.tolist() == [5.0, 0.0, 0.0] and three.last_fit.pose.shape == (1, 7)
    assert one.fit_log().shape == (3, 4) and torch.equal(one.fit_log(), three.fit_log())
    one.reset()
    assert one.trajectory().shape == (0, 7) and one.last_fit is None
    # fit=None: today's map, launch for launch
    plain, old = new_map(), TW.new_map(F.VOXEL, F.LOG2)
    plain.add(X, P)
    old.add(X, P)
    assert TW.same_snapshot(TW.snapshot(plain), TW.snapshot(old)) and torch.equal(plain.world64, old.world64)
    assert torch.equal(plain.trajectory()[-1], plain.world64) and plain.last_fit is None


def test_tracking_the_small_drive_beats_dead_reckoning():
    scans, _rel, biased, worlds = F.drive()
    tracked, reckoned = new_map(fit=_fit(iters=2)), new_map()
    tracked.add(dev(scans), dev(biased))
    reckoned.add(dev(scans), dev(biased))
    et = F.pose_error(tracked.world64.cpu().numpy(), worlds[-1])
    ed = F.pose_error(reckoned.world64.cpu().numpy(), worlds[-1])
    print("end pose error: tracked %.4f m, dead-reckoned %.4f m" % (et, ed))
    assert tracked.last_fit.status.tolist() == [5.0, 0.0, 0.0, 0.0, 0.0]
    assert ed > 0.2 and et < ed


def test_run_sequence_writes_the_tracked_poses(tmp_path):
    model, ev, sensor = load_pkg("model"), load_pkg("evaluate"), load_pkg("sensor")
    from kitti_tree import write_sequence
    root = str(tmp_path / "drive")
    T_diff = write_sequence(root, "04", TW.SEQ_N, TW.SEQ_H, TW.SEQ_W)
    kw = dict(H_input=TW.SEQ_H, W_input=TW.SEQ_W, num_points=TW.SEQ_H * TW.SEQ_W, batch_size=1, lanes=0)
    net = model.PWCLONet(DEV, seed=0)
    spec = sensor.VoxelMap(0.5, 18)
    rows0, _ = ev.run_sequence(net, root, "04", T_diff, out_dir=str(tmp_path / "a"), world_map=spec, **kw)
    rows1, _ = ev.run_sequence(net, root, "04", T_diff, out_dir=str(tmp_path / "b"), world_map=spec, map_fit=sensor.MapFit(iters=2), **kw)
    assert same_bits(rows0, rows1)                                                       # what the net returns does not change
    q0, t0 = ev.predict_sequence(net, root, "04", T_diff, **kw)[:2]
    wm = load_pkg("world_map").WorldMap(spec, DEV, fit=sensor.MapFit(iters=2))
    q1, t1 = ev.predict_sequence(net, root, "04", T_diff, world_map=wm, **kw)[:2]
    assert same_bits(q0, q1) and same_bits(t0, t1)
    table = np.loadtxt(os.path.join(str(tmp_path / "b"), "04_map_poses.txt"))
    assert table.shape == (TW.SEQ_N, 10) and np.isfinite(table).all()
    assert table[0, 7] == 0 and int(table[0, 9]) == 1 | 4                                # row 0: an empty map, flagged
    assert np.array_equal(table[:, :7], wm.trajectory().cpu().numpy())
    assert os.path.exists(os.path.join(str(tmp_path / "b"), "04_map.bin")) and not os.path.exists(os.path.join(str(tmp_path / "a"), "04_map_poses.txt"))
    with pytest.raises(ValueError):
        ev.run_sequence(net, root, "04", T_diff, map_fit=sensor.MapFit(), **kw)

"""GPU: elo_map_merge and what the host builds on it (WorldMap.merge / rebuild / window= / state, evaluate.run_sequence(map_window=))
against the numpy restatement of its rule (tests/map_merge_reference.py).  Every comparison is EXACT and on CONTENT (rows sorted by
key) -- keys, counts, sums, stats, the report, the bits of the float32 centroids --, never on where a key sits in the table."""
import os

import numpy as np
import pytest
import torch

import map_fit_reference as F
import map_merge_reference as R
import test_world_map_gpu as TW
import world_map_reference as M
from conftest import load_pkg
from kitti_tree import write_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dev, same_bits, new_map, table, check = TW.dev, TW.same_bits, TW.new_map, TW.table, TW.check


def key_of(ix, iy, iz):
    return int(M.pack([ix], [iy], [iz])[0])


def report_of(rep):
    return dict(zip(R.REPORT, (int(v) for v in rep.cpu())))


def source(key, acc, offset=False):
    """The rows on the device; offset: the keys start one word into their buffer, so they are 8- but not 16-byte aligned."""
    key, acc = np.asarray(key, np.int64), np.asarray(acc, np.int64).reshape(-1, 4)
    if not offset:
        return dev(key), dev(acc)
    buf = torch.empty((len(key) + 1,), dtype=torch.int64, device=DEV)
    buf[1:] = dev(key)
    assert buf.data_ptr() % 16 == 0 and (len(key) == 0 or buf[1:].data_ptr() % 16 == 8)
    return buf[1:], dev(acc)


def distinct_keys(rng, n, reach=40):
    """n different keys of voxels with indices of both signs within `reach`."""
    idx = np.unique(rng.integers(-reach, reach, (4 * n + 8, 3)), axis=0)
    assert len(idx) >= n
    idx = idx[rng.permutation(len(idx))[:n]]
    return M.pack(idx[:, 0], idx[:, 1], idx[:, 2]).astype(np.int64)


def rows_for(rng, n, pool):
    """n source rows over the keys `pool`: a fifth of them empty slots, duplicates where n outgrows the pool, sums within 65535 n --
    and, from 63 rows on, one row of every malformed kind."""
    key = pool[rng.integers(0, len(pool), n)].copy()
    count = rng.integers(1, 6, n)
    acc = np.concatenate([count[:, None], (rng.random((n, 3)) * (65535 * count[:, None] + 1)).astype(np.int64)], 1)
    key[rng.random(n) < 0.2] = -1
    if n >= 63:
        key[5] = pool[3] | -(1 << 63)
        acc[11] = (0, 0, 0, 0)
        acc[17] = (1 << 40, 0, 0, 0)
        acc[23] = (2, 0, 2 * 65535 + 1, 0)
        key[[11, 17, 23]] = pool[:3]
    return key, acc


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 257])
def test_merge_matches_the_reference_exactly(rows, offset):
    rng = np.random.default_rng(600 + rows)
    pool = distinct_keys(rng, 90)
    wm = new_map(0.5, 12)
    # first into the empty table, unfiltered; then more rows into the table as it stands, under a window and a least count
    key, acc = rows_for(rng, rows, pool)
    rep = wm.merge(source(key, acc, offset))
    want, want_rep = R.merge(None, key, acc, 0.5)
    assert report_of(rep) == want_rep
    check(wm, want)
    key2, acc2 = rows_for(rng, rows, pool)
    centre = np.array([2.25, -3.0, 0.75])
    rep = wm.merge(source(key2, acc2, offset), centre=dev(centre), radius=12.0, min_count=2)
    want, want_rep = R.merge(want, key2, acc2, 0.5, centre, 12.0, 2)
    assert report_of(rep) == want_rep
    if rows >= 63:
        assert want_rep["voxels_filtered"] > 0 and want_rep["voxels_rejected"] == 4 and want_rep["voxels_merged"] > 0
    check(wm, want)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("log2", [10, 13])                  # 1024 rows: one wave's eight steps; 8192: two workgroups
def test_merge_of_a_whole_table(log2, offset):
    xyz, pose, _share = M.exact_case(3)
    src = new_map(0.5, log2)
    src.insert(dev(xyz), dev(pose))
    want = M.exact_content(3, 0.5)
    assert src.stats()["dropped_full"] == 0 and 0 < len(want["key"]) < 1024
    wm = new_map(0.5, 13)
    if offset:
        buf = torch.empty(((1 << log2) + 1,), dtype=torch.int64, device=DEV)
        buf[1:] = src.keys
        rep = wm.merge((buf[1:], src.acc))
    else:
        rep = wm.merge(src)
    assert report_of(rep) == dict(voxels_merged=len(want["key"]), voxels_filtered=0, voxels_rejected=0, voxels_dropped=0,
                                  points_merged=want["stats"]["inserted"], points_filtered=0, points_dropped=0, claimed=len(want["key"]))
    check(wm, want)


def test_find_against_claim():
    rng = np.random.default_rng(610)
    K = distinct_keys(rng, 300)
    acc = np.concatenate([rng.integers(1, 9, (300, 1)), rng.integers(0, 65536, (300, 3))], 1)
    # a source sharing half its keys with a table that is not empty
    wm = new_map(0.5, 11)
    wm.merge(source(K[:100], acc[:100]))
    want, _ = R.merge(None, K[:100], acc[:100], 0.5)
    rep = wm.merge(source(K[50:150], acc[50:150]))
    want, want_rep = R.merge(want, K[50:150], acc[50:150], 0.5)
    assert want_rep["claimed"] == 50 and want_rep["voxels_merged"] == 100 and report_of(rep) == want_rep
    check(wm, want)
    # 64 and 65 rows of ONE key: a wave's lanes, and one more, race for one slot
    for n in (64, 65):
        wm = new_map(0.5, 10)
        one = rng.integers(0, 65536, (n, 4))
        one[:, 0] = rng.integers(1, 4, n)
        rep = report_of(wm.merge(source(np.full(n, K[0]), one)))
        key, got = table(wm)
        assert key.tolist() == [K[0]] and got.tolist() == [one.sum(0).tolist()]
        assert rep["claimed"] == 1 and rep["voxels_merged"] == n and rep["points_merged"] == int(one[:, 0].sum())
        assert wm.stats() == dict(inserted=int(one[:, 0].sum()), filtered=0, rejected=0, dropped_full=0, occupied=1)
    # every row its own key
    wm = new_map(0.5, 11)
    rep = wm.merge(source(K[:257], acc[:257]))
    want, want_rep = R.merge(None, K[:257], acc[:257], 0.5)
    assert want_rep["claimed"] == 257 and report_of(rep) == want_rep
    check(wm, want)


def _consistent(wm, key, acc, rep, before=0):
    """What must hold of a merge of rows with DISTINCT keys whatever was dropped: every row merged or dropped, the points add up, no
    key twice, every stored row the source's."""
    got_key, got_acc = table(wm)
    s = wm.stats()
    assert rep["voxels_merged"] + rep["voxels_dropped"] == len(key) and rep["voxels_filtered"] == rep["voxels_rejected"] == 0
    assert rep["points_merged"] + rep["points_dropped"] == int(acc[:, 0].sum())
    assert len(np.unique(got_key)) == len(got_key) == s["occupied"] and np.isin(got_key, key).all()
    order = np.argsort(key)
    where = order[np.searchsorted(key[order], got_key)]
    assert np.array_equal(got_acc, acc[where] * (1 + before))
    return got_key


def test_hash_paths():
    rng = np.random.default_rng(620)
    # keys that share a home slot, the LAST slot, and its probe successor slot 0: the probe sequences wrap
    voxels = TW._voxels_at_home((1023, 0), 5)
    key = np.array([key_of(*v) for v in voxels], np.int64)
    acc = np.concatenate([np.arange(1, 11)[:, None], rng.integers(0, 65536, (10, 3))], 1)
    assert (M.home(key[:5], 10) == 1023).all() and (M.home(key[5:], 10) == 0).all()
    wm = new_map(0.5, 10)
    rep = wm.merge(source(key, acc))
    slots = np.flatnonzero(wm.keys.cpu().numpy() != -1)
    assert slots.min() < 10 and slots.max() == 1023
    want, want_rep = R.merge(None, key, acc, 0.5)
    assert report_of(rep) == want_rep
    check(wm, want)
    # a destination loaded to 0.9: 930 distinct keys into 1024 slots, then the stored keys once more -- all found
    K = distinct_keys(rng, 930)
    acc = np.concatenate([rng.integers(1, 9, (930, 1)), rng.integers(0, 65536, (930, 3))], 1)
    wm = new_map(0.5, 10)
    rep = report_of(wm.merge(source(K, acc)))
    stored = _consistent(wm, K, acc, rep)
    assert len(stored) >= 0.85 * 1024 and rep["claimed"] == len(stored)
    again = np.isin(K, stored)
    rep2 = report_of(wm.merge(source(K[again], acc[again])))
    assert rep2["claimed"] == 0 and rep2["voxels_dropped"] == 0 and rep2["voxels_merged"] == len(stored)
    _consistent(wm, K[again], acc[again], dict(rep2), before=1)
    assert wm.stats()["inserted"] == 2 * rep["points_merged"] and wm.stats()["dropped_full"] == rep["points_dropped"]
    # a full destination: 4096 distinct keys into 1024 slots
    K = distinct_keys(rng, 4096, reach=60)
    acc = np.concatenate([rng.integers(1, 9, (4096, 1)), rng.integers(0, 65536, (4096, 3))], 1)
    wm = new_map(0.5, 10)
    rep = report_of(wm.merge(source(K, acc)))
    stored = _consistent(wm, K, acc, rep)
    s = wm.stats()
    assert rep["voxels_dropped"] > 0 and rep["claimed"] == len(stored) <= 1024
    assert s["inserted"] == rep["points_merged"] and s["dropped_full"] == rep["points_dropped"] > 0
    assert int(table(wm)[1][:, 0].sum()) == s["inserted"]


def test_the_window_is_a_closed_box_read_when_the_launch_runs():
    model = load_pkg("model")
    one = lambda n: np.array([[n, 3, 2, 1]], np.int64)
    c = dev(np.array([0.25, 0.25, 0.25]))
    for axis in range(3):
        at = lambda i: np.array([key_of(*[i if a == axis else 0 for a in range(3)])], np.int64)
        for i, kept in ((3, True), (4, False), (-3, True), (-4, False)):
            wm = new_map(0.5, 10)
            rep = report_of(wm.merge(source(at(i), one(2)), centre=c, radius=1.5))
            assert (rep["voxels_merged"], rep["voxels_filtered"], rep["points_filtered"]) == ((1, 0, 0) if kept else (0, 1, 2)), (axis, i)
            assert R.classify(at(i), one(2), 0.5, np.array([0.25] * 3), 1.5).tolist() == [R.ROW if kept else R.FILTERED]
            assert wm.stats()["inserted"] == (2 if kept else 0) and wm.stats()["occupied"] == int(kept)
    # min_count at n and n + 1
    for least, kept in ((5, True), (6, False)):
        wm = new_map(0.5, 10)
        rep = report_of(wm.merge(source(np.array([key_of(1, 2, 3)]), one(5)), min_count=least))
        assert (rep["voxels_merged"], rep["voxels_filtered"]) == ((1, 0) if kept else (0, 1))
    # a NaN centre keeps nothing
    rng = np.random.default_rng(630)
    K = distinct_keys(rng, 200, reach=30)
    acc = np.concatenate([rng.integers(1, 9, (200, 1)), rng.integers(0, 65536, (200, 3))], 1)
    wm = new_map(0.5, 11)
    rep = report_of(wm.merge(source(K, acc), centre=dev(np.array([0.0, np.nan, 0.0])), radius=100.0))
    assert rep["voxels_filtered"] == 200 and rep["voxels_merged"] == 0 and wm.stats() == dict.fromkeys(M.STATS, 0)
    # the centre is read when the launch RUNS: one captured merge, replayed after the centre tensor was rewritten
    centres = (np.array([4.0, -2.0, 1.0]), np.array([-6.5, 3.25, 0.0]))
    wants = [R.merge(None, K, acc, 0.5, cc, 5.0) for cc in centres]
    assert 0 < wants[0][1]["voxels_merged"] < 200 and not np.array_equal(wants[0][0]["key"], wants[1][0]["key"])
    wm = new_map(0.5, 11)
    sk, sa = source(K, acc)
    centre = dev(centres[0].copy())
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        wm.merge((sk, sa), centre=centre, radius=5.0)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with model.graph_capture(graph):
        rep = wm.merge((sk, sa), centre=centre, radius=5.0)
    for cc, (want, want_rep) in zip(centres, wants):
        wm.reset()
        centre.copy_(dev(cc))
        graph.replay()
        torch.cuda.synchronize()
        check(wm, want)
        assert report_of(rep) == want_rep                                                # (the report is zeroed inside the graph)


def test_union_of_two_maps_is_the_map_of_both_drives():
    model = load_pkg("model")
    xyz, pose, _share = M.order_case()
    X, P = dev(xyz), dev(pose)
    want = M.content(xyz, pose, 0.1)
    whole = new_map(0.1)
    whole.insert(X, P)
    check(whole, want)
    snap = TW.snapshot(whole)
    for first, second in ((slice(0, 3), slice(3, 6)), (slice(3, 6), slice(0, 3))):
        a, b = new_map(0.1), new_map(0.1, 12)                                            # (the capacities may differ)
        a.insert(X[first], P[first])
        b.insert(X[second], P[second])
        rep = report_of(a.merge(b))
        assert rep["points_merged"] == b.stats()["inserted"] and 0 < rep["claimed"] < rep["voxels_merged"]
        assert TW.same_snapshot(TW.snapshot(a), snap)
    # ... and the merge replayed from a graph
    a, b = new_map(0.1), new_map(0.1)
    a.insert(X[:3], P[:3])
    b.insert(X[3:], P[3:])
    keep = (a.keys.clone(), a.acc.clone(), a.stat_words.clone())
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        a.merge(b)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with model.graph_capture(graph):
        a.merge(b)
    for buf, was in zip((a.keys, a.acc, a.stat_words), keep):
        buf.copy_(was)
    graph.replay()
    torch.cuda.synchronize()
    assert TW.same_snapshot(TW.snapshot(a), snap)
    with pytest.raises(ValueError):
        a.merge(new_map(0.5))


def _grid_scans(n, side=24):
    """n scans (1, side, side, 3) of side^2 points each, every point in a 0.5 m voxel of its own, scan j on its own z level."""
    a, b = np.meshgrid(np.arange(-side // 2, side // 2), np.arange(-side // 2, side // 2), indexing="ij")
    return [np.stack([0.75 * a + 0.05, 0.75 * b + 0.05, 0.0 * a + 0.75 * j + 0.3], -1).reshape(1, side, side, 3).astype(np.float32) for j in range(n)]


def test_rebuild_grows_the_table():
    S = load_pkg("sensor")
    scans = _grid_scans(4)                                                               # 4 x 576 voxels: 2304 into 1024 slots
    eye = dev(TW.IDENTITY)
    # too late: a 2^10 table that dropped points keeps what it had, and no more
    lost = new_map(0.5, 10)
    for s in scans:
        lost.insert(dev(s), eye)
    before, had = lost.stats(), table(lost)
    assert before["dropped_full"] > 0
    rep = report_of(lost.rebuild(log2_capacity=14))
    assert lost.spec == S.VoxelMap(0.5, 14) and lost.keys.shape == (1 << 14,) and lost.acc.shape == (1 << 14, 4)
    assert rep["voxels_dropped"] == 0 and rep["voxels_merged"] == before["occupied"] and rep["points_merged"] == before["inserted"]
    assert lost.stats() == before and all(np.array_equal(x, y) for x, y in zip(table(lost), had))
    # in time: rebuilt to 2^14 BEFORE it overflows, then continued, the map equals the scans put into a 2^14 table
    big = new_map(0.5, 14)
    for s in scans:
        big.insert(dev(s), eye)
    grown = new_map(0.5, 10)
    grown.insert(dev(scans[0]), eye)
    assert grown.stats()["dropped_full"] == 0
    grown.rebuild(log2_capacity=14)
    assert grown.spec == S.VoxelMap(0.5, 14)
    for s in scans[1:]:
        grown.insert(dev(s), eye)
    assert TW.same_snapshot(TW.snapshot(grown), TW.snapshot(big)) and grown.stats()["occupied"] == 4 * 576
    check(grown, M.content(np.concatenate(scans), np.repeat(TW.IDENTITY, 4, 0)))
    w = grown.window_stats()
    assert w == dict(rebuilds=1, evicted_voxels=0, evicted_points=0, dropped_voxels=0, dropped_points=0)


def test_state_continues_the_drive(tmp_path):
    W = load_pkg("world_map")
    xyz, _pose, _share = M.order_case()
    rng = np.random.default_rng(640)
    rel = np.stack([np.concatenate([[1.0, 0.0, 0.01 * rng.normal(), 0.02 * rng.normal()], [0.8, 0.05 * rng.normal(), 0.0]]) for _ in range(5)])
    X, P = dev(xyz[:5]), dev(rel.astype(np.float32))
    whole = new_map(0.1)
    whole.add(X, P)
    first = new_map(0.1)
    first.add(X[:3], P[:3])
    path = str(tmp_path / "drive_state.npz")
    assert first.save_state(path) == first.stats()["occupied"]
    back = W.WorldMap.load_state(path, device=DEV)
    assert back.spec == first.spec and TW.same_snapshot(TW.snapshot(back), TW.snapshot(first))
    assert torch.equal(back.world64.view(torch.int64), first.world64.view(torch.int64))
    back.add(X[3:4], P[3:4])
    back.add(X[4:5], P[4:5])
    assert TW.same_snapshot(TW.snapshot(back), TW.snapshot(whole))
    assert torch.equal(back.world64.view(torch.int64), whole.world64.view(torch.int64))
    assert torch.equal(back.trajectory().view(torch.int64), whole.trajectory()[3:].view(torch.int64))
    # into another capacity; and a file with a malformed row is refused
    small = W.WorldMap.load_state(path, device=DEV, log2_capacity=13)
    assert small.spec.log2_capacity == 13 and TW.same_snapshot(TW.snapshot(small), TW.snapshot(first))
    state = first.state()
    state["acc"][2, 0] = 0
    np.savez(str(tmp_path / "bad.npz"), **state)
    with pytest.raises(ValueError):
        W.WorldMap.load_state(str(tmp_path / "bad.npz"), device=DEV)


def _sum_of_counts(wm):
    return int(table(wm)[1][:, 0].sum())


def test_window_untracked_is_insert_insert_rebuild():
    S, W = load_pkg("sensor"), load_pkg("world_map")
    xyz, _pose, _share = M.order_case()
    rng = np.random.default_rng(650)
    rel = np.stack([np.concatenate([[1.0, 0.0, 0.0, 0.01 * rng.normal()], [1.5, 0.1 * rng.normal(), 0.0]]) for _ in range(5)])
    X, P = dev(xyz[:5]), dev(rel)
    window = S.MapWindow(radius=30.0, every=2, min_count=2)
    wm = W.WorldMap(S.VoxelMap(0.1, 14), DEV, window=window)
    wm.add(X, P)
    split = W.WorldMap(S.VoxelMap(0.1, 14), DEV, window=window)                           # the same drive in three calls
    split.add(X[:1], P[:1])
    split.add(X[1:4], P[1:4])
    split.add(X[4:], P[4:])
    hand = new_map(0.1)
    world, reports = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device=DEV), []
    for j in range(5):
        world = W.compose(world, P[j])
        hand.insert(X[j:j + 1], world.reshape(1, 7).contiguous())
        if j % 2 == 1:
            reports.append(report_of(hand.rebuild(centre=world[4:].clone(), radius=30.0, min_count=2)))
    want = TW.snapshot(hand)
    evicted = sum(r["voxels_filtered"] for r in reports), sum(r["points_filtered"] for r in reports)
    assert evicted[0] > 0 and all(r["voxels_merged"] > 0 for r in reports)
    for m in (wm, split):
        assert TW.same_snapshot(TW.snapshot(m), want)
        assert torch.equal(m.world64.view(torch.int64), world.view(torch.int64))
        w, s = m.window_stats(), m.stats()
        assert w == dict(rebuilds=2, evicted_voxels=evicted[0], evicted_points=evicted[1], dropped_voxels=0, dropped_points=0)
        assert _sum_of_counts(m) == s["inserted"] - w["evicted_points"] - w["dropped_points"]
        assert s["occupied"] == len(table(m)[0]) and s["inserted"] == int((xyz[:5] != 0).any(-1).sum())
    # the rebuilds alternate between two buffer sets: nothing is allocated after the first
    a, b = wm.keys.data_ptr(), wm._spare[0].data_ptr()
    wm.rebuild()
    assert (wm.keys.data_ptr(), wm._spare[0].data_ptr()) == (b, a)
    wm.reset()
    assert wm.window_stats()["rebuilds"] == 0 and wm.stats()["occupied"] == 0 and wm.points()[0].shape == (0, 3)


def _fit():
    return load_pkg("sensor").MapFit(**dict(F.FIT, min_count=F.MIN_COUNT, iters=2))


def _tracked(window=None, blob=None):
    S, W = load_pkg("sensor"), load_pkg("world_map")
    scans, _rel, biased, _worlds = F.drive()
    wm = W.WorldMap(S.VoxelMap(F.VOXEL, F.LOG2), DEV, fit=_fit(), window=window)
    if blob is not None:
        wm.insert(dev(blob), dev(TW.IDENTITY))
    wm.add(dev(scans), dev(biased))
    return wm


def test_tracking_with_a_window_that_evicts_nothing_is_bit_equal():
    S = load_pkg("sensor")
    plain, windowed = _tracked(), _tracked(S.MapWindow(radius=1.0e4, every=2))
    assert torch.equal(plain.trajectory().view(torch.int64), windowed.trajectory().view(torch.int64))
    assert torch.equal(plain.fit_log().view(torch.int32), windowed.fit_log().view(torch.int32))
    assert TW.same_snapshot(TW.snapshot(plain), TW.snapshot(windowed))
    assert windowed.window_stats() == dict(rebuilds=2, evicted_voxels=0, evicted_points=0, dropped_voxels=0, dropped_points=0)
    assert plain.fit_log()[1:, 3].tolist() == [0.0] * 4                                  # (the fits ran: nothing was flagged)


def test_tracking_with_a_window_that_evicts_what_the_fit_never_uses():
    S, W = load_pkg("sensor"), load_pkg("world_map")
    scans, _rel, biased, _worlds = F.drive()
    rng = np.random.default_rng(660)
    blob = (np.array([0.0, -100.0, 0.0]) + rng.uniform(-3.0, 3.0, (1, 4, 64, 3))).astype(np.float32)     # ~100 m from the start
    blob_keys = M.content(blob, TW.IDENTITY, F.VOXEL)["key"]
    # the scene, from every sensor position, lies within `reach` of the origin on every axis; the blob does not
    reach = float(np.abs(scans).max()) + 0.8 * F.DRIVE_N + 1.0
    radius = reach + 2 * F.VOXEL
    assert radius + F.DRIVE_N + 2 * F.VOXEL < 100.0 - 3.0 - F.VOXEL
    # the unwindowed run by hand, with match=True: no cell ever associates to a blob key, on the device and in the reference
    plain = W.WorldMap(S.VoxelMap(F.VOXEL, F.LOG2), DEV, fit=_fit())
    plain.insert(dev(blob), dev(TW.IDENTITY))
    X, P = dev(scans), dev(biased)
    world = plain.world64
    for j in range(F.DRIVE_N):
        guess = W.compose(world, P[j]).reshape(1, 7).contiguous()
        res = plain.fit(X[j:j + 1], guess, match=True)
        assert not np.isin(res.match.cpu().numpy(), blob_keys).any()
        key, acc = table(plain)
        ref = F.evaluate(scans[j], res.pose[0].cpu().numpy(), {"key": key, "acc": acc, "xyz": M.centroids(key, acc, F.VOXEL)}, F.VOXEL, **F.FIT)
        assert not np.isin(ref["match"], blob_keys).any() and (j == 0 or (ref["match"] >= 0).sum() > F.MIN_COUNT)
        plain.insert(X[j:j + 1], res.pose)
        world = res.pose[0]
    whole = _tracked(blob=blob)
    assert torch.equal(whole.world64.view(torch.int64), world.view(torch.int64))
    windowed = W.WorldMap(S.VoxelMap(F.VOXEL, F.LOG2), DEV, fit=_fit(), window=S.MapWindow(radius=radius, every=2))
    windowed.insert(dev(blob), dev(TW.IDENTITY))
    windowed.add(X[:2], P[:2])
    w = windowed.window_stats()
    assert w["rebuilds"] == 1 and w["evicted_voxels"] == len(blob_keys) > 0 and w["evicted_points"] == 256
    windowed.add(X[2:], P[2:])
    assert torch.equal(windowed.trajectory().view(torch.int64), whole.trajectory().view(torch.int64))
    assert torch.equal(windowed.fit_log().view(torch.int32), whole.fit_log().view(torch.int32))
    _xyz, _count, key = windowed.points()
    assert not np.isin(key.cpu().numpy(), blob_keys).any() and np.isin(blob_keys, whole.points()[2].cpu().numpy()).all()
    w, s = windowed.window_stats(), windowed.stats()
    assert w["rebuilds"] == 2 and w["evicted_points"] == 256 and s["inserted"] == whole.stats()["inserted"]
    assert _sum_of_counts(windowed) == s["inserted"] - w["evicted_points"] - w["dropped_points"]


def test_run_sequence_with_a_window_writes_a_state_that_loads(tmp_path):
    model, ev, S, W = load_pkg("model"), load_pkg("evaluate"), load_pkg("sensor"), load_pkg("world_map")
    root = str(tmp_path / "drive")
    T_diff = write_sequence(root, "04", TW.SEQ_N, TW.SEQ_H, TW.SEQ_W)
    kw = dict(H_input=TW.SEQ_H, W_input=TW.SEQ_W, num_points=TW.SEQ_H * TW.SEQ_W, batch_size=1, lanes=0)
    net = model.PWCLONet(DEV, seed=0)
    spec, window = S.VoxelMap(0.5, 18), S.MapWindow(radius=20.0, every=2)
    out = str(tmp_path / "out")
    rows0, _ = ev.run_sequence(net, root, "04", T_diff, **kw)
    rows1, _ = ev.run_sequence(net, root, "04", T_diff, out_dir=out, world_map=spec, map_window=window, **kw)
    assert same_bits(rows0, rows1)                                                       # what the net returns does not change
    back = W.WorldMap.load_state(os.path.join(out, "04_map_state.npz"), device=DEV)
    pts, count, _key = back.points()
    saved = np.fromfile(os.path.join(out, "04_map.bin"), dtype=np.float32).reshape(-1, 4)
    assert len(saved) > 0 and same_bits(saved[:, :3], pts.cpu().numpy()) and np.array_equal(saved[:, 3], count.cpu().numpy().astype(np.float32))
    w = back.window_stats()
    assert w["rebuilds"] == TW.SEQ_N // 2 and w["evicted_voxels"] > 0
    assert _sum_of_counts(back) == back.stats()["inserted"] - w["evicted_points"] - w["dropped_points"]
    with pytest.raises(ValueError):
        ev.run_sequence(net, root, "04", T_diff, map_window=window, **kw)


def test_refusals_launch_nothing():
    L, ops = load_pkg("_lib"), load_pkg("_scan_ops")
    xyz, pose, _share = M.exact_case(1)
    wm = new_map(0.5, 10)
    wm.insert(dev(xyz), dev(pose))
    rng = np.random.default_rng(670)
    sk, sa = source(distinct_keys(rng, 32), np.concatenate([np.ones((32, 1), np.int64), rng.integers(0, 65536, (32, 3))], 1))
    centre = dev(np.zeros(3))
    report = torch.zeros(8, dtype=torch.int64, device=DEV)
    before = (wm.keys.clone(), wm.acc.clone(), wm.stat_words.clone())

    def args(**kw):
        base = dict(rows=32, src_keys=sk.data_ptr(), src_acc=sa.data_ptr(), voxel=0.5, log2_capacity=10, keys=wm.keys.data_ptr(),
                    acc=wm.acc.data_ptr(), stats=wm.stat_words.data_ptr(), centre=None, radius=0.0, min_count=1, report=report.data_ptr())
        base.update(kw)
        return L.MapMergeArgs(**base)

    L.call("elo_map_merge", args(rows=0), wm.keys)                                       # no rows is fine and does nothing
    L.call("elo_map_merge", args(rows=0, src_keys=wm.keys.data_ptr(), src_acc=wm.acc.data_ptr()), wm.keys)
    bad = [dict(src_keys=None), dict(src_acc=None), dict(keys=None), dict(acc=None), dict(stats=None), dict(report=None), dict(rows=-1),
           dict(rows=2 ** 31), dict(voxel=0.0), dict(voxel=-0.5), dict(voxel=float("inf")), dict(voxel=float("nan")),
           dict(log2_capacity=9), dict(log2_capacity=29), dict(min_count=0), dict(min_count=-4),
           dict(centre=centre.data_ptr(), radius=0.0), dict(centre=centre.data_ptr(), radius=-1.0),
           dict(centre=centre.data_ptr(), radius=float("inf")), dict(centre=centre.data_ptr(), radius=float("nan")),
           dict(src_keys=sk.data_ptr() + 4), dict(src_acc=sa.data_ptr() + 4), dict(keys=wm.keys.data_ptr() + 4),
           dict(acc=wm.acc.data_ptr() + 4), dict(stats=wm.stat_words.data_ptr() + 4), dict(report=report.data_ptr() + 4),
           dict(centre=centre.data_ptr() + 4, radius=5.0),
           dict(src_keys=wm.keys.data_ptr()), dict(src_keys=wm.acc.data_ptr() + 8 * 100), dict(src_acc=wm.acc.data_ptr()),
           dict(src_acc=wm.keys.data_ptr() + 8 * 1023), dict(rows=1024, src_keys=wm.keys.data_ptr(), src_acc=wm.acc.data_ptr())]
    for kw in bad:
        with pytest.raises(L.EloError):
            L.call("elo_map_merge", args(**kw), wm.keys)
    assert L.lib().elo_map_merge(None, None) == -1
    # the host's own: a table into itself, a float32 centre, another map's shapes
    for call, error in ((lambda: ops.map_merge(wm.keys, wm.acc, wm.stat_words, wm.keys, wm.acc, wm.spec), L.EloError),
                        (lambda: wm.merge(wm), L.EloError),
                        (lambda: ops.map_merge(wm.keys, wm.acc, wm.stat_words, sk, sa, wm.spec, centre.float(), 5.0), TypeError),
                        (lambda: ops.map_merge(wm.keys, wm.acc, wm.stat_words, sk, sa[:31], wm.spec), L.EloError),
                        (lambda: ops.map_merge(wm.keys, wm.acc, wm.stat_words, sk.cpu(), sa.cpu(), wm.spec), L.EloError),
                        (lambda: ops.map_merge(wm.keys, wm.acc, wm.stat_words, sk, sa, wm.spec, centre, None), L.EloError)):
        with pytest.raises(error):
            call()
    torch.cuda.synchronize()
    for was, now in zip(before, (wm.keys, wm.acc, wm.stat_words)):
        assert torch.equal(was, now)
    assert int(report.sum()) == 0

"""GPU: elo_scan_descriptor / elo_descriptor_search (csrc/elo_place.hip), places.PlaceIndex, world_map.WorldMap(places=) and
WorldMap.relocalise against the float64 statement of tests/place_reference.py.

The descriptor, `entry`, `shift` and `best_shift` are compared EXACTLY: tests/test_place_cpu.py vets the table of
tests/place_cases.py, so that every such decision has a gap of 1e-9 in the reference (or is a planted tie of exact values).
`dist` and `best_dist`: within DIST = 1e-12 absolute.  Derived: a term 1 - d / sqrt(a b) lies in [0, 2] and carries the roundings
of one conversion, one square root, one division and one subtraction, a few ulps of 2^-52 = 2.2e-16 each; at most 128 terms are
added in the SAME fixed order by kernel and reference, so the sum differs by at most 128 x 2 x a few ulps < 1e-13 before the one
division by `pairs`; one more digit is margin.  Infinities must be equal."""
import math

import numpy as np
import pytest
import torch

import map_fit_reference as F
import place_cases as C
import place_reference as R
from conftest import load_pkg
from test_world_map_gpu import DEV, dev, same_bits, table

pytestmark = pytest.mark.gpu
DIST = 1e-12


def ctx_of(kw):
    return load_pkg("sensor").ScanContext(**kw)


def describe(xyz, kw):
    return load_pkg("_scan_ops").scan_descriptor(dev(xyz), ctx_of(kw)).cpu().numpy()


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    inf = np.isinf(want)
    return got.shape == want.shape and np.array_equal(np.isinf(got), inf) and (np.abs(got[~inf] - want[~inf]) <= DIST).all() \
        and (got[inf] > 0).all()


def check_search(res, ref, label=""):
    with np.errstate(invalid="ignore"):                                                  # (inf - inf where both say no pair)
        err = np.abs(np.where(np.isinf(ref["best_dist"]), 0.0, res.best_dist.cpu().numpy() - ref["best_dist"]))
    print("%s: worst |best_dist - reference| = %.3g" % (label, err.max() if err.size else 0.0))
    assert res.entry.dtype == torch.int32 and res.shift.dtype == torch.int32 and res.dist.dtype == torch.float64
    assert np.array_equal(res.best_shift.cpu().numpy(), ref["best_shift"]), label
    assert close(res.best_dist.cpu().numpy(), ref["best_dist"]), label
    assert np.array_equal(res.entry.cpu().numpy(), ref["entry"]), label
    assert np.array_equal(res.shift.cpu().numpy(), ref["shift"]), label
    assert close(res.dist.cpu().numpy(), ref["dist"]), label


def same_desc(a, b):
    """Two uint16 tensors, compared as 16-bit words."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def bits(res):
    return [res.entry, res.shift, res.dist.view(torch.int64), res.best_shift, res.best_dist.view(torch.int64)]


def replayed(make):
    """`make()` run eagerly on a side stream (the warm-up a capture needs), captured, its outputs cleared, replayed -> its result."""
    model = load_pkg("model")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        make()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with model.graph_capture(graph):
        res = make()
    for v in (res if isinstance(res, list) else [res]):
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("i", range(len(C.DESCRIPTOR_SHAPES)))
def test_descriptor_matches_the_reference_exactly(i):
    xyz, kw = C.cloud(i)
    got = describe(xyz, kw)
    assert got.dtype == np.uint16 and np.array_equal(got, C.cloud_descriptor(i))
    assert (got > 0).any() or i == 5


def test_descriptor_placed_cases():
    ops = load_pkg("_scan_ops")
    x, kw, want = C.placed()
    assert np.array_equal(describe(x, kw), want) and np.array_equal(R.descriptor(x, **kw), want)
    assert not describe(np.zeros((2, 3, 64, 3), np.float32), C.context(60, 20)).any()      # an image without points
    # written into rows of a larger buffer, the rows around them untouched
    out = torch.full((4, 3, 4), 9, dtype=torch.uint16, device=DEV)
    ops.scan_descriptor(dev(x), ctx_of(kw), out=out[2:3])
    assert np.array_equal(out.cpu().numpy()[2:3], want) and (out.cpu().numpy()[[0, 1, 3]] == 9).all()
    # every point in one bin: 5 x 4 x 128 points in sector s, ring 2 of the second image; the bin holds the highest
    kw = C.context(32, 8)
    rng = np.random.default_rng(11)
    cloud = np.zeros((2, 5, 128, 3), np.float32)
    cloud[1, :, 40:44] = np.stack([rng.uniform(9.0, 9.5, (5, 4)), rng.uniform(-2.0, 2.0, (5, 4)), rng.uniform(-2.0, 3.0, (5, 4))], -1)
    got = describe(cloud, kw)
    want = R.descriptor(cloud, **kw)
    assert np.array_equal(got, want) and (got > 0).sum() == 1 and got[1, 10, 2] == int(math.floor((cloud[1, :, 40:44, 2].astype(np.float64).max() + 3.0) / 0.005)) + 1
    # every bin its own point: 8 sectors x 4 rings on an (4, 8) image, row h puts its point into ring h
    kw = C.context(8, 4, max_range=32.0)
    cloud = np.zeros((1, 4, 8, 3), np.float32)
    for h in range(4):
        for w in range(8):
            cloud[0, h, w] = (8.0 * h + 1.0, 0.5, -3.0 + 0.005 * (8 * h + w) + 0.0025)
    got = describe(cloud, kw)
    assert np.array_equal(got, R.descriptor(cloud, **kw)) and np.array_equal(got[0], (np.arange(8)[:, None] + 8 * np.arange(4)[None, :] + 1))


def test_descriptor_two_runs_and_a_graph_replay_agree():
    ops = load_pkg("_scan_ops")
    xyz, kw = C.cloud(3)
    X, spec = dev(xyz), ctx_of(kw)
    first, again = ops.scan_descriptor(X, spec), ops.scan_descriptor(X, spec)
    assert same_desc(first, again)
    res = replayed(lambda: ops.scan_descriptor(X, spec))
    assert same_desc(first, res) and np.array_equal(res.cpu().numpy(), C.cloud_descriptor(3))


@pytest.mark.parametrize("name", sorted(C.SEARCH))
def test_search_matches_the_reference(name):
    ops = load_pkg("_scan_ops")
    query, db, m, k, _tie, kw, ref = C.search_case(name)
    res = ops.descriptor_search(dev(query), dev(db), m, ctx_of(kw), k)
    assert tuple(res.entry.shape) == (len(query), k) and tuple(res.best_dist.shape) == (len(query), m)
    check_search(res, ref, name)


def test_search_planted_cases():
    ops = load_pkg("_scan_ops")
    rng = np.random.default_rng(21)
    kw = C.context(60, 20)
    spec = ctx_of(kw)
    d = C.random_descriptors(rng, 70, 60, 20)
    # duplicates at chosen indices, across a wave's and a workgroup's worth of entries: the smaller index wins, identical bits
    db = d.copy()
    db[5], db[66], db[40] = d[0], d[0], d[1]
    db[64] = d[1]
    res = ops.descriptor_search(dev(d[:2]), dev(db), 70, spec, 8)
    ref = R.search(d[:2], db, 70, 8)
    check_search(res, ref, "duplicates")
    assert res.entry.cpu().numpy()[:, :3].tolist() == [[0, 5, 66], [1, 40, 64]]
    dist = res.dist.view(torch.int64).cpu().numpy()
    assert (dist[:, 0] == dist[:, 1]).all() and (dist[:, 1] == dist[:, 2]).all()
    best = res.best_dist.view(torch.int64).cpu().numpy()
    assert best[0, 0] == best[0, 5] == best[0, 66] and best[1, 1] == best[1, 40] == best[1, 64]
    # m below the rows filled: the duplicates at 64 and 66 are beyond it and are ignored
    res = ops.descriptor_search(dev(d[:2]), dev(db), 64, spec, 3)
    check_search(res, R.search(d[:2], db, 64, 3), "m below the rows filled")
    assert res.entry.cpu().numpy()[:, :2].tolist() == [[0, 5], [1, 40]] and (res.entry.cpu().numpy() < 64).all()
    # a descriptor periodic under a shift of 30 columns: shifts s and s + 30 tie bit for bit, the smaller wins
    per = np.concatenate([d[2, :30], d[2, :30]])
    rolled = np.stack([per, np.roll(per, 1, axis=0), np.roll(per, 29, axis=0)])
    res = ops.descriptor_search(dev(per[None]), dev(rolled), 3, spec, 3)
    assert res.best_shift.cpu().numpy().tolist() == [[0, 1, 29]] and (np.abs(res.best_dist.cpu().numpy()) < DIST).all()
    check_search(res, R.search(per[None], rolled, 3, 3), "periodic")
    # the query rolled by s columns: shift s, dist 0 up to rounding
    for sectors, rings in ((60, 20), (65, 32), (128, 3)):
        kw2 = C.context(sectors, rings)
        q = C.random_descriptors(rng, 1, sectors, rings)
        rolled = np.stack([np.roll(q[0], s, axis=0) for s in (0, 1, sectors - 1)])
        res = ops.descriptor_search(dev(q), dev(rolled), 3, ctx_of(kw2), 3)
        assert res.best_shift.cpu().numpy().tolist() == [[0, 1, sectors - 1]]
        assert (np.abs(res.best_dist.cpu().numpy()) < DIST).all() and res.entry.cpu().numpy().tolist() == R.search(q, rolled, 3, 3)["entry"].tolist()
    # all-empty queries and entries: no pairs, +inf, shift 0, ranked by index
    empty = np.zeros((3, 60, 20), np.uint16)
    mixed = np.stack([empty[0], d[3], empty[0]])
    res = ops.descriptor_search(dev(np.stack([empty[0], d[3]])), dev(mixed), 3, spec, 4)
    check_search(res, R.search(np.stack([empty[0], d[3]]), mixed, 3, 4), "empty")
    assert res.entry.cpu().numpy().tolist() == [[0, 1, 2, -1], [1, 0, 2, -1]] and np.isinf(res.dist.cpu().numpy()[0]).all()
    assert res.shift.cpu().numpy().tolist() == [[0, 0, 0, -1], [0, 0, 0, -1]]
    # the largest product: level 4095 everywhere at 32 rings (4095^2 * 32 = 536 608 800 < 2^31), against itself and a half-full one
    kw3 = C.context(128, 32)
    full = np.full((1, 128, 32), C.LEVELS, np.uint16)
    other = np.stack([full[0], np.where(np.arange(32)[None, :] % 2 == 0, C.LEVELS, 0).astype(np.uint16).repeat(128, 0).reshape(128, 32),
                      C.random_descriptors(rng, 1, 128, 32)[0]])
    res = ops.descriptor_search(dev(full), dev(other), 3, ctx_of(kw3), 3)
    ref = R.search(full, other, 3, 3)
    assert res.best_dist.cpu().numpy()[0, 0] == 0.0 and abs(ref["best_dist"][0, 1] - (1.0 - 1.0 / math.sqrt(2.0))) < 1e-12
    assert close(res.best_dist.cpu().numpy(), ref["best_dist"]) and np.array_equal(res.entry.cpu().numpy(), ref["entry"])
    assert res.best_shift.cpu().numpy()[0, :2].tolist() == [0, 0]


def test_search_two_runs_and_a_graph_replay_agree():
    ops = load_pkg("_scan_ops")
    for name in ("m65_s64_r32", "m257_s60", "m0_n3_k8"):
        query, db, m, k, _tie, kw, ref = C.search_case(name)
        Q, D, spec = dev(query), dev(db), ctx_of(kw)
        first, again = bits(ops.descriptor_search(Q, D, m, spec, k)), bits(ops.descriptor_search(Q, D, m, spec, k))
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        held = []

        def make():
            held[:] = [ops.descriptor_search(Q, D, m, spec, k)]
            r = held[0]
            return [r.entry, r.shift, r.dist, r.best_shift, r.best_dist]
        replayed(make)
        assert all(torch.equal(a, b) for a, b in zip(first, bits(held[0])))
        check_search(held[0], ref, name + " replayed")


def test_refusals_launch_nothing():
    ops, L, S = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor")
    spec = S.ScanContext(4, 8)
    out = torch.full((1, 8, 4), 7, dtype=torch.uint16, device=DEV)
    with pytest.raises(L.EloError):
        ops.scan_descriptor(torch.zeros((1, 2, 7, 3), device=DEV), spec, out)                # W < sectors
    with pytest.raises(L.EloError):
        ops.scan_descriptor(torch.zeros((1, 2, 8, 3)), spec)                                 # no CPU path
    with pytest.raises(L.EloError):
        ops.descriptor_search(out, out.cpu(), 1, spec)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    # the library's own refusals: the argument blocks built by hand
    import ctypes
    a = L.ScanDescriptorArgs(1, 2, 8, 4, 8, -3.0, 0.0, 0.0, (ctypes.c_double * 33)(*spec.edge2()), out.data_ptr(), out.data_ptr())
    assert L.lib().elo_scan_descriptor(ctypes.byref(a), None) != 0                           # z_step 0
    a = L.ScanDescriptorArgs(1, 2, 8, 4, 8, -3.0, 0.1, 0.0, (ctypes.c_double * 33)(0.0, 4.0, 3.0, 5.0, 6.0), out.data_ptr(), out.data_ptr())
    assert L.lib().elo_scan_descriptor(ctypes.byref(a), None) != 0                           # edges not ascending
    b = L.DescriptorSearchArgs(1, 1, 4, 8, 9, out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr())
    assert L.lib().elo_descriptor_search(ctypes.byref(b), None) != 0                         # k = 9
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()


# ---- the index and the map ---------------------------------------------------------------------------------------------------------
def _e2e_index(capacity=8):
    P = load_pkg("places")
    e = C.e2e()
    index = P.PlaceIndex(ctx_of(C.E2E_CONTEXT), capacity, DEV)
    index.add(dev(e["keys"]), dev(e["poses"]), scan=[10 * j for j in range(6)])
    return index, e


def test_index_add_and_query_are_the_two_ops():
    ops = load_pkg("_scan_ops")
    index, e = _e2e_index()
    spec = index.spec
    assert len(index) == 6 and np.array_equal(index.desc[:6].cpu().numpy(), e["db"]) and index.scan[:6].tolist() == [0, 10, 20, 30, 40, 50]
    assert same_bits(index.pose64[:6].cpu().numpy(), e["poses"])
    both = dev(np.concatenate([e["query"], e["far"]]))
    match = index.query(both, k=4)
    by_hand = ops.descriptor_search(ops.scan_descriptor(both, spec), index.desc, 6, spec, 4)
    assert all(torch.equal(a, b) for a, b in zip(bits(match.search), bits(by_hand)))
    assert torch.equal(match.entry, by_hand.entry) and torch.equal(match.shift, by_hand.shift) and torch.equal(match.dist, by_hand.dist)
    yaw = match.yaw.cpu().numpy()
    assert yaw[0].tolist() == [R.yaw_of(int(s), spec.sectors) for s in match.shift[0].tolist()] and yaw[0, 0] == spec.yaw_of(e["shift"])
    for r in range(4):
        want = F.compose(e["poses"][int(match.entry[0, r])], C.pose_of((0.0, 0.0, 0.0), float(yaw[0, r])))
        assert np.abs(match.pose[0, r].cpu().numpy() - want).max() < 1e-14
    # skip_recent: the newest entries are left out; beyond the count nothing is searched and the rows are padding at the identity
    assert index.query(both[:1], k=1, skip_recent=3).entry.tolist() == [[int(np.argmin(e["query_search"]["best_dist"][0, :3]))]]
    none = index.query(both[:1], k=2, skip_recent=6)
    assert none.entry.tolist() == [[-1, -1]] and none.shift.tolist() == [[-1, -1]] and np.isinf(none.dist.cpu().numpy()).all()
    assert none.pose.cpu().numpy().tolist() == [[[1.0, 0, 0, 0, 0, 0, 0]] * 2] and none.yaw.tolist() == [[0.0, 0.0]]
    assert index.query(both[:1], k=1, skip_recent=60).entry.tolist() == [[-1]]
    # full: two more fit, three do not -- and nothing is added then
    with pytest.raises(IndexError):
        index.add(dev(e["keys"][:3]), dev(e["poses"][:3]))
    assert len(index) == 6 and index.add(dev(e["keys"][:2]), dev(e["poses"][:2])) == 6 and len(index) == 8
    assert index.scan[6:8].tolist() == [6, 7]
    with pytest.raises(IndexError):
        index.add(dev(e["keys"][:1]), dev(e["poses"][:1]))


def test_index_state_saved_loaded_and_queried_again(tmp_path):
    P = load_pkg("places")
    index, e = _e2e_index()
    path = str(tmp_path / "places.npz")
    assert index.save_state(path) == 6
    again = P.PlaceIndex.load_state(path, capacity=8, device=DEV)
    assert len(again) == 6 and again.spec == index.spec
    a, b = index.query(dev(e["query"]), k=4), again.query(dev(e["query"]), k=4)
    assert all(torch.equal(x, y) for x, y in zip(bits(a.search), bits(b.search))) and torch.equal(a.pose, b.pose) and torch.equal(a.yaw, b.yaw)


def _drive(places, fit=None):
    """The six keyframes and the turned query as a drive of seven scans: relative poses from the true world poses."""
    W, S = load_pkg("world_map"), load_pkg("sensor")
    e = C.e2e()
    scans = np.concatenate([e["keys"], e["query"]])
    worlds = np.concatenate([e["poses"], e["truth"][None]])
    back = lambda p: np.concatenate([[1.0, 0.0, 0.0, 0.0], -p[4:]])                        # (the keyframes' poses are translations)
    rels = np.stack([worlds[0]] + [F.compose(back(worlds[j - 1]), worlds[j]) for j in range(1, 7)])
    wm = W.WorldMap(S.VoxelMap(0.5, 16), DEV, fit=fit, places=places)
    wm.add(dev(scans[:3]), dev(rels[:3]))                                                  # batches of three, three and one
    wm.add(dev(scans[3:6]), dev(rels[3:6]))
    wm.add(dev(scans[6:]), dev(rels[6:]))
    return wm, scans


def test_world_map_logs_its_lookups_and_the_index_only_reads():
    ops, S = load_pkg("_scan_ops"), load_pkg("sensor")
    spec = ctx_of(C.E2E_CONTEXT)
    places = S.Places(spec, every=2, skip_recent=1, capacity=8)
    wm, scans = _drive(places)
    plain, _ = _drive(None)
    # the index only reads: the same table content, the same trajectory, bit for bit
    assert all(np.array_equal(a, b) for a, b in zip(table(wm), table(plain))) and wm.stats() == plain.stats()
    assert torch.equal(wm.trajectory(), plain.trajectory()) and plain.places is None
    # scans 1, 3 and 5 (every 2nd since reset) are looked up among all but the newest entry, then appended
    traj = wm.trajectory()
    db = torch.zeros((8, spec.sectors, spec.rings), dtype=torch.uint16, device=DEV)
    rows, held = [], []
    for scan in (1, 3, 5):
        desc = ops.scan_descriptor(dev(scans[scan:scan + 1]), spec)
        res = ops.descriptor_search(desc, db, max(0, len(held) - 1), spec, 1)
        entry = int(res.entry[0, 0])
        rows.append([float(scan), float(entry), float(held[entry]) if entry >= 0 else -1.0, float(res.shift[0, 0]), float(res.dist[0, 0])])
        db[len(held)] = desc[0]
        held.append(scan)
    log = wm.revisits()
    assert log.dtype == torch.float64 and tuple(log.shape) == (3, 5) and same_bits(log.cpu().numpy(), np.array(rows, np.float64))
    assert rows[0][1:] == [-1.0, -1.0, -1.0, math.inf] and rows[1][1:] == [-1.0, -1.0, -1.0, math.inf] and rows[2][1:3] == [0.0, 1.0]
    assert len(wm.places) == 3 and wm.places.scan[:3].tolist() == [1, 3, 5] and same_desc(wm.places.desc[:3], db[:3])
    assert torch.equal(wm.places.pose64[:3], traj[[1, 3, 5]])
    wm.reset()
    assert len(wm.places) == 0 and tuple(wm.revisits().shape) == (0, 5)


def test_world_map_add_with_a_lookup_due_is_enqueue_only():
    """A capture fails on any host read of a device value: an add() whose scan is looked up and appended is recorded into a graph,
    and its replay does what the eager add() of a twin map did -- content, trajectory, index and log, bit for bit."""
    model, S = load_pkg("model"), load_pkg("sensor")
    places = S.Places(ctx_of(C.E2E_CONTEXT), every=2, skip_recent=0, capacity=8)
    eager, scans = _drive(places)                                                          # seven scans; 1, 3 and 5 looked up
    W = load_pkg("world_map")
    wm = W.WorldMap(S.VoxelMap(0.5, 16), DEV, places=places)
    rel = torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.5, 0.0, 0.0]] * 6, dtype=torch.float64, device=DEV)
    rel[0, 4:] = dev(C.e2e_position(0))
    X = dev(scans)
    wm.add(X[:5], rel[:5])                                                                 # (the warm-up: every launch has run)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with model.graph_capture(graph):
        wm.add(X[5:6], rel[5:6])                                                           # scan 5: looked up among entries 0, 1, appended
    assert len(wm.places) == 3 and tuple(wm.revisits().shape) == (3, 5)
    wm._revisits[-1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    twin = W.WorldMap(S.VoxelMap(0.5, 16), DEV, places=places)
    twin.add(X[:6], rel)
    assert all(np.array_equal(a, b) for a, b in zip(table(wm), table(twin))) and torch.equal(wm.trajectory(), twin.trajectory())
    assert same_bits(wm.revisits().cpu().numpy(), twin.revisits().cpu().numpy()) and wm.revisits()[2, 1:3].tolist() in ([0.0, 1.0], [1.0, 3.0])
    assert same_desc(wm.places.desc[:3], twin.places.desc[:3]) and torch.equal(wm.places.scan[:3], twin.places.scan[:3])
    assert torch.equal(wm.places.pose64[:3], twin.places.pose64[:3]) and torch.equal(wm.world64, twin.world64)
    assert len(eager.places) == 3


def test_world_map_state_carries_the_index(tmp_path):
    W, S = load_pkg("world_map"), load_pkg("sensor")
    places = S.Places(ctx_of(C.E2E_CONTEXT), every=2, skip_recent=1, capacity=8)
    wm, scans = _drive(places)
    path = str(tmp_path / "state.npz")
    wm.save_state(path)
    back = W.WorldMap.load_state(path, DEV, places=places)
    assert len(back.places) == 3 and same_desc(back.places.desc[:3], wm.places.desc[:3]) and torch.equal(back.revisits(), wm.revisits())
    assert all(np.array_equal(a, b) for a, b in zip(table(back), table(wm)))
    assert W.WorldMap.load_state(path, DEV).places is None                                 # without places= the file's map alone
    with pytest.raises(ValueError):
        W.WorldMap.load_state(path, DEV, places=S.Places(S.ScanContext(), capacity=8))     # another ScanContext


# ---- end to end -----------------------------------------------------------------------------------------------------------------
E2E_VOXEL, E2E_ITERS = 0.5, 2
E2E_FIT = dict(gate=0.5, huber=0.1, jump_rel=0.2, min_count=30)


def test_relocalise_finds_the_place_the_heading_and_the_pose():
    W, S = load_pkg("world_map"), load_pkg("sensor")
    e = C.e2e()
    spec = ctx_of(C.E2E_CONTEXT)
    wm = W.WorldMap(S.VoxelMap(E2E_VOXEL, 16), DEV, fit=S.MapFit(iters=E2E_ITERS, **E2E_FIT), places=S.Places(spec, capacity=8))
    wm.insert(dev(e["keys"]), dev(e["poses"]))
    wm.places.add(dev(e["keys"]), dev(e["poses"]))
    # the place and the heading: keyframe 3, and the shift that stands for a heading turned by +7 sectors is sectors - 7
    match = wm.places.query(dev(e["query"]), k=4)
    assert match.entry[0].tolist() == e["query_search"]["entry"][0].tolist() and match.entry[0, 0] == C.E2E_KEY
    assert match.shift[0].tolist() == e["query_search"]["shift"][0].tolist() and match.shift[0, 0] == spec.sectors - C.E2E_TURN
    assert close(match.dist.cpu().numpy(), e["query_search"]["dist"])
    assert abs((float(match.yaw[0, 0]) - e["yaw"] + math.pi) % (2.0 * math.pi) - math.pi) < 1e-12     # the SIGN: +7 sectors
    out = wm.relocalise(dev(e["query"]), k=4)
    assert out["best"] == 0 and torch.equal(out["match"].entry, match.entry)
    guess, fitted = out["match"].pose[0, 0].cpu().numpy(), out["fits"].pose[0].cpu().numpy()
    start, end = F.pose_error(guess, e["truth"]), F.pose_error(fitted, e["truth"])
    # the reference's fit from the same guess against the reference's table: the bound of tests/test_map_fit_gpu.py's converging
    # case (test_polish_follows_the_reference_and_reports_the_pose_it_returns: `err <= errs[k - 1]`) -- after k steps the kernel
    # is no further from the truth than the reference was a step earlier
    ref_table = F.table_of(e["keys"], e["poses"], E2E_VOXEL)
    fit = {n: v for n, v in E2E_FIT.items() if n != "min_count"}
    errs = [F.pose_error(p, e["truth"]) for p in F.iterate(e["query"][0], guess, ref_table, E2E_VOXEL, E2E_ITERS, min_count=30, **fit)]
    print("guess %.4f m, fitted %.4f m; reference after 0 .. %d steps: %s" % (start, end, E2E_ITERS, ["%.4f" % v for v in errs]))
    assert abs(start - 0.1) < 1e-6 and float(out["fits"].status[0]) == 0
    assert end < start and end <= errs[E2E_ITERS - 1]
    # 100 m away nothing lies within the crop: the reference says an empty descriptor, every dist +inf -- and no candidate fits
    far = wm.relocalise(dev(e["far"]), k=4)
    assert far["match"].entry[0].tolist() == e["far_search"]["entry"][0].tolist() and np.isinf(far["match"].dist.cpu().numpy()).all()
    assert far["best"] == -1


def test_run_sequence_writes_the_revisits(tmp_path):
    import os
    import test_world_map_gpu as TW
    from kitti_tree import write_sequence
    model, ev, S = load_pkg("model"), load_pkg("evaluate"), load_pkg("sensor")
    root = str(tmp_path / "drive")
    T_diff = write_sequence(root, "04", TW.SEQ_N, TW.SEQ_H, TW.SEQ_W)
    kw = dict(H_input=TW.SEQ_H, W_input=TW.SEQ_W, num_points=TW.SEQ_H * TW.SEQ_W, batch_size=1, lanes=0)
    net = model.PWCLONet(DEV, seed=0)
    spec, places = S.VoxelMap(0.5, 18), S.Places(every=2, skip_recent=0, capacity=8)
    rows0, _ = ev.run_sequence(net, root, "04", T_diff, out_dir=str(tmp_path / "a"), world_map=spec, **kw)
    rows1, _ = ev.run_sequence(net, root, "04", T_diff, out_dir=str(tmp_path / "b"), world_map=spec, places=places, **kw)
    assert same_bits(rows0, rows1)                                                       # what the net returns does not change
    log = np.loadtxt(os.path.join(str(tmp_path / "b"), "04_revisits.txt"), ndmin=2)
    assert log.shape == (TW.SEQ_N // 2, 5) and log[:, 0].tolist() == [1.0, 3.0][:len(log)]
    assert log[0, 1:4].tolist() == [-1.0, -1.0, -1.0] and np.isinf(log[0, 4])              # the first lookup finds an empty index
    assert log[1, 1:3].tolist() == [0.0, 1.0] and 0.0 <= log[1, 4] < 1.0                   # the second: entry 0, which is scan 1
    assert not os.path.exists(os.path.join(str(tmp_path / "a"), "04_revisits.txt"))
    state = np.load(os.path.join(str(tmp_path / "b"), "04_map_state.npz"))
    assert state["place_desc"].shape == (2, 60, 20) and state["place_scan"].tolist() == [1, 3]
    with pytest.raises(ValueError):
        ev.run_sequence(net, root, "04", T_diff, places=places, **kw)

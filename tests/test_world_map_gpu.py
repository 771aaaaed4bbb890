"""GPU: the world map (elo_map_insert / elo_map_extract, world_map.WorldMap, evaluate.predict_sequence(world_map=)) against the numpy
restatement of its rule (tests/world_map_reference.py).  Every comparison is EXACT -- keys, counts, the three sums, the stats
words, the bits of the float32 centroids -- and is made on CONTENT (rows sorted by key), never on where a key sits in the table."""
import math
import os

import numpy as np
import pytest
import torch

import world_map_reference as M
from conftest import load_pkg
from kitti_tree import write_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDENTITY = np.array([[2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])         # un-normalised; R = I and p' = p exactly


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def new_map(voxel=0.5, log2_capacity=14, **kw):
    return load_pkg("world_map").WorldMap(load_pkg("sensor").VoxelMap(voxel, log2_capacity, **kw), DEV)


def table(wm):
    """The table's content, sorted by key: (key (m,), acc (m,4))."""
    keys, acc = wm.keys.cpu().numpy(), wm.acc.cpu().numpy()
    full = keys != -1
    order = np.argsort(keys[full])
    return keys[full][order], acc[full][order]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(wm, want):
    key, acc = table(wm)
    assert np.array_equal(key, want["key"])
    assert np.array_equal(acc, want["acc"])
    assert wm.stats() == want["stats"]
    xyz, count, k = wm.points()
    assert xyz.dtype == torch.float32 and count.dtype == torch.int64 and k.dtype == torch.int64
    assert np.array_equal(k.cpu().numpy(), want["key"]) and np.array_equal(count.cpu().numpy(), want["acc"][:, 0])
    assert same_bits(xyz.cpu().numpy(), want["xyz"])


def snapshot(wm):
    xyz, count, key = wm.points()
    return xyz.cpu().numpy(), count.cpu().numpy(), key.cpu().numpy(), wm.stats(), table(wm)[1]


def same_snapshot(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("voxel", M.VOXELS)
@pytest.mark.parametrize("case", range(len(M.SHAPES)))
def test_insert_matches_the_reference_exactly(case, voxel):
    xyz, pose, _share = M.exact_case(case)
    wm = new_map(voxel)
    wm.insert(dev(xyz), dev(pose))
    check(wm, M.exact_content(case, voxel))


def _in_voxels(index, rng):
    """Points inside the 0.5 m voxels `index` (n,3): float32 coordinates whose voxel survives the rounding (1 % off the faces)."""
    return ((np.asarray(index, np.float64) + rng.uniform(0.01, 0.99, (len(index), 3))) * 0.5).astype(np.float32)


def test_every_lane_in_one_voxel():
    rng = np.random.default_rng(11)
    pts = _in_voxels(np.tile([[3, -2, 1]], (256, 1)), rng)
    wm = new_map()
    wm.insert(dev(pts.reshape(1, 4, 64, 3)), dev(IDENTITY))
    key, acc = table(wm)
    assert key.tolist() == [int(M.pack([3], [-2], [1])[0])]
    g = [sum(min(int(math.floor((float(c) / 0.5 - i) * 65536.0)), 65535) for c in pts[:, a]) for a, i in enumerate((3, -2, 1))]
    assert acc.tolist() == [[256] + g]
    assert wm.stats() == {"inserted": 256, "filtered": 0, "rejected": 0, "dropped_full": 0, "occupied": 1}
    check(wm, M.content(pts.reshape(1, 4, 64, 3), IDENTITY))


def test_every_lane_in_its_own_voxel():
    a, b = np.meshgrid(np.arange(-8, 8), np.arange(-8, 8), indexing="ij")
    pts = np.stack([0.75 * a + 0.05, 0.75 * b + 0.05, 0.75 * (a + b) + 0.05], -1).reshape(1, 4, 64, 3).astype(np.float32)   # 1.5 voxels apart
    wm = new_map()
    wm.insert(dev(pts), dev(IDENTITY))
    key, acc = table(wm)
    assert len(key) == 256 and (acc[:, 0] == 1).all()
    assert wm.stats() == {"inserted": 256, "filtered": 0, "rejected": 0, "dropped_full": 0, "occupied": 256}
    check(wm, M.content(pts, IDENTITY))


def test_runs_of_equal_keys_across_lanes_and_waves():
    # cells in order carry runs of 1, 2, 63 and 64 equal keys, again and again: a wave holds 256 consecutive cells and a workgroup
    # 1024, so runs cross both (the eighth run covers cells 196 .. 259); run r lies in voxel r % 7, so equal keys also meet again
    # further on in the same wave, not only side by side.  Two scans of 8 x 160 = 1280 cells: a second, ragged workgroup each.
    rng = np.random.default_rng(12)
    n = 2 * 8 * 160
    runs = np.repeat(np.arange(n), np.tile([1, 2, 63, 64], n)[:n])[:n]
    voxels = np.stack([runs % 7 - 3, (runs % 7) * 2 - 5, np.zeros(n, np.int64) - 1], -1)
    pts = _in_voxels(voxels, rng).reshape(2, 8, 160, 3)
    pose = np.concatenate([IDENTITY, IDENTITY])
    wm = new_map()
    wm.insert(dev(pts), dev(pose))
    want = M.content(pts, pose)
    assert len(want["key"]) == 7 and want["stats"]["inserted"] == n
    check(wm, want)


def _voxels_at_home(slots, each, log2_capacity=10):
    """The first `each` voxels (ix, 7, iz) of a search over integer coordinates whose home slot -- the header's hash -- is s, for
    every s of `slots`, in that order."""
    ix, iz = np.meshgrid(np.arange(-1000, 1000), np.arange(-8, 8), indexing="ij")
    ix, iz = ix.reshape(-1), iz.reshape(-1)
    h = M.home(M.pack(ix, np.full_like(ix, 7), iz), log2_capacity)
    out = []
    for s in slots:
        hit = np.flatnonzero(h == np.uint64(s))[:each]
        out += [(int(ix[j]), 7, int(iz[j])) for j in hit]
    return out


def test_probing_wraps_around_the_table():
    # log2_capacity 10: five voxels whose home slot is the LAST slot and five whose home is slot 0, the last slot's probe successor
    voxels = _voxels_at_home((1023, 0), 5)
    assert len(voxels) == 10 and len(set(voxels)) == 10
    rng = np.random.default_rng(13)
    index = np.concatenate([np.tile([v], (j + 1, 1)) for j, v in enumerate(voxels)])      # voxel j gets j + 1 points
    pts = _in_voxels(rng.permutation(index), rng).reshape(1, 1, -1, 3)
    wm = new_map(0.5, 10)
    wm.insert(dev(pts), dev(IDENTITY))
    key, acc = table(wm)
    counts = dict(zip(key.tolist(), acc[:, 0].tolist()))
    assert counts == {int(M.pack([v[0]], [v[1]], [v[2]])[0]): j + 1 for j, v in enumerate(voxels)}
    check(wm, M.content(pts, IDENTITY))


def test_a_full_table_drops_and_says_so():
    a, b = np.meshgrid(np.arange(-32, 32), np.arange(-32, 32), indexing="ij")
    pts = np.stack([0.75 * a + 0.05, 0.75 * b + 0.05, 0.0 * a + 0.3], -1).reshape(1, 4, 1024, 3).astype(np.float32)
    want = M.content(pts, IDENTITY)
    assert len(want["key"]) == 4096
    wm = new_map(0.5, 10)
    wm.insert(dev(pts), dev(IDENTITY))
    s = wm.stats()
    key, acc = table(wm)
    assert 0 < s["occupied"] <= 1024 and s["occupied"] == len(key)
    assert s["dropped_full"] > 0 and s["inserted"] + s["dropped_full"] == 4096 and s["filtered"] == 0 and s["rejected"] == 0
    assert len(np.unique(key)) == len(key) and np.isin(key, want["key"]).all()
    assert int(acc[:, 0].sum()) == s["inserted"] and (acc[:, 0] == 1).all()              # every input voxel has one point
    where = np.searchsorted(want["key"], key)
    assert np.array_equal(acc, want["acc"][where])
    # ... and again: the stored voxels take their second point, the others are dropped again (no slot ever frees)
    wm.insert(dev(pts), dev(IDENTITY))
    s2 = wm.stats()
    key2, acc2 = table(wm)
    assert np.array_equal(key2, key) and s2["occupied"] == s["occupied"] and s2["inserted"] + s2["dropped_full"] == 8192
    assert int(acc2[:, 0].sum()) == s2["inserted"]


@pytest.mark.parametrize("gates,rejected", [((M.GATES[0], math.inf), 3), (M.GATES, 1)])
def test_every_cell_is_accounted_for_once(gates, rejected):
    # scan 2 has a zero quaternion: skipped whole, its cells count nowhere.  Scan 0 holds a NaN coordinate (its range is NaN: no
    # gate catches it, the carried point is rejected) and a 1e30 one, scan 1 a 3e6 one: beyond the index range -- rejected while
    # max_range is inf, filtered by a finite max_range.
    xyz, pose, _share = M.accounting_case()
    wm = new_map(0.5, 14, min_range=gates[0], max_range=gates[1])
    wm.insert(dev(xyz), dev(pose))
    want = M.content(xyz, pose, 0.5, *gates)
    s = wm.stats()
    live = [0, 1, 3]
    cells = int((xyz[live] != 0).any(-1).sum())
    assert s["inserted"] + s["filtered"] + s["rejected"] + s["dropped_full"] == cells and s["dropped_full"] == 0
    assert s["rejected"] == rejected and s["filtered"] > 10 and s["inserted"] > 100
    check(wm, want)
    # the gates are the source's: the same points at another pose are filtered alike
    wm2 = new_map(0.5, 14, min_range=gates[0], max_range=gates[1])
    pose2 = pose.copy()
    pose2[:, 4:] += 3.0
    wm2.insert(dev(xyz), dev(pose2))
    assert wm2.stats()["filtered"] == s["filtered"]


def test_content_does_not_depend_on_order_batching_or_replay():
    model = load_pkg("model")
    xyz, pose, _share = M.order_case()
    X, P = dev(xyz), dev(pose)
    want = M.content(xyz, pose, 0.1)
    assert want["stats"]["occupied"] < want["stats"]["inserted"]                          # scans share voxels
    forms = []
    wm = new_map(0.1)
    wm.insert(X, P)
    check(wm, want)
    forms.append(snapshot(wm))
    for order in (range(6), (4, 1, 5, 0, 3, 2)):
        wm = new_map(0.1)
        for j in order:
            wm.insert(X[j:j + 1], P[j:j + 1])
        forms.append(snapshot(wm))
    wm = new_map(0.1)
    wm.insert(X[3:], P[3:])
    wm.insert(X[:3], P[:3])
    forms.append(snapshot(wm))
    wm = new_map(0.1)                                                                    # a second run of the first form
    wm.insert(X, P)
    forms.append(snapshot(wm))
    # ... and a replay of the insert recorded into a graph (single stream)
    wm = new_map(0.1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        wm.insert(X, P)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with model.graph_capture(graph):
        wm.insert(X, P)
    wm.reset()
    graph.replay()
    forms.append(snapshot(wm))
    graph.replay()                                                                       # twice: every count and sum doubles
    torch.cuda.synchronize()
    key, acc = table(wm)
    assert np.array_equal(key, want["key"]) and np.array_equal(acc, 2 * want["acc"])
    for f in forms[1:]:
        assert same_snapshot(forms[0], f)


def _extract_direct(wm, max_out, guard=3):
    """elo_map_extract through ctypes into buffers with `guard` rows behind max_out, filled with a pattern."""
    L = load_pkg("_lib")
    key = torch.full((max_out + guard,), -77, dtype=torch.int64, device=DEV)
    count = torch.full((max_out + guard,), -78, dtype=torch.int64, device=DEV)
    xyz = torch.full((max_out + guard, 3), -79.0, dtype=torch.float32, device=DEV)
    cursor = torch.full((1,), 12345, dtype=torch.int64, device=DEV)
    a = L.MapExtractArgs(wm.spec.voxel, wm.spec.log2_capacity, max_out, wm.keys.data_ptr(), wm.acc.data_ptr(), key.data_ptr(),
                         count.data_ptr(), xyz.data_ptr(), cursor.data_ptr())
    L.call("elo_map_extract", a, wm.keys)
    return key.cpu().numpy(), count.cpu().numpy(), xyz.cpu().numpy(), int(cursor.item())


def test_extract_reports_all_and_writes_no_more_than_asked():
    xyz, pose, _share = M.exact_case(3)
    want = M.exact_content(3, 0.5)
    m = len(want["key"])
    wm = new_map(0.5)
    wm.insert(dev(xyz), dev(pose))
    for max_out in (m + 5, m, m // 3, 1, 0):
        key, count, cen, n = _extract_direct(wm, max_out)
        assert n == m                                                                    # the cursor is set by the call and counts all
        rows = min(m, max_out)
        assert (key[rows:] == -77).all() and (count[rows:] == -78).all() and (cen[rows:] == -79.0).all()
        assert len(np.unique(key[:rows])) == rows
        where = np.searchsorted(want["key"], key[:rows])
        assert np.array_equal(want["key"][where], key[:rows]) and np.array_equal(want["acc"][where, 0], count[:rows])
        assert same_bits(cen[:rows], want["xyz"][where])
    ops = load_pkg("_scan_ops")
    key, count, cen, n = ops.map_extract(wm.keys, wm.acc, wm.spec, 10)
    assert int(n.item()) == m and key.shape == (10,) and count.shape == (10,) and cen.shape == (10, 3)


def test_refusals_launch_nothing():
    L = load_pkg("_lib")
    xyz, pose, _share = M.exact_case(1)
    wm = new_map(0.5, 10)
    wm.insert(dev(xyz), dev(pose))
    X, P = dev(xyz), dev(pose)
    before = (wm.keys.clone(), wm.acc.clone(), wm.stat_words.clone())
    B, H, W = M.SHAPES[1]

    def args(**kw):
        base = dict(batch=B, H=H, W=W, voxel=0.5, min_range=0.0, max_range=math.inf, log2_capacity=10, xyz=X.data_ptr(),
                    pose=P.data_ptr(), keys=wm.keys.data_ptr(), acc=wm.acc.data_ptr(), stats=wm.stat_words.data_ptr())
        base.update(kw)
        return L.MapInsertArgs(**base)

    L.call("elo_map_insert", args(batch=0), wm.keys)                                     # an empty batch is fine and does nothing
    bad = [dict(xyz=None), dict(pose=None), dict(keys=None), dict(acc=None), dict(stats=None), dict(H=0), dict(W=0), dict(H=-1),
           dict(batch=2 ** 15, H=2 ** 8, W=2 ** 8), dict(voxel=0.0), dict(voxel=-0.5), dict(voxel=math.inf), dict(voxel=math.nan),
           dict(min_range=-1.0), dict(min_range=math.nan), dict(min_range=5.0, max_range=5.0), dict(min_range=5.0, max_range=2.0),
           dict(max_range=math.nan), dict(log2_capacity=9), dict(log2_capacity=29), dict(keys=wm.keys.data_ptr() + 4),
           dict(acc=wm.acc.data_ptr() + 4), dict(pose=P.data_ptr() + 4)]
    for kw in bad:
        with pytest.raises(L.EloError):
            L.call("elo_map_insert", args(**kw), wm.keys)
    assert L.lib().elo_map_insert(None, None) == -1
    torch.cuda.synchronize()
    for was, now in zip(before, (wm.keys, wm.acc, wm.stat_words)):
        assert torch.equal(was, now)
    # the host's own refusals: types, shapes, devices
    ops = load_pkg("_scan_ops")
    for call in (lambda: ops.map_insert(wm.keys, wm.acc, wm.stat_words, X, P.float(), wm.spec),
                 lambda: ops.map_insert(wm.keys, wm.acc, wm.stat_words, X.double(), P, wm.spec),
                 lambda: ops.map_insert(wm.keys, wm.acc, wm.stat_words, X, P, "spec")):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: ops.map_insert(wm.keys, wm.acc, wm.stat_words, X, P[:0], wm.spec),
                 lambda: ops.map_insert(wm.keys[:-1], wm.acc, wm.stat_words, X, P, wm.spec),
                 lambda: ops.map_insert(wm.keys, wm.acc, wm.stat_words, X[..., :2], P, wm.spec),
                 lambda: ops.map_extract(wm.keys, wm.acc, wm.spec, -1)):
        with pytest.raises(L.EloError):
            call()
    for was, now in zip(before, (wm.keys, wm.acc, wm.stat_words)):
        assert torch.equal(was, now)


def test_add_composes_and_save_round_trips(tmp_path):
    world_map = load_pkg("world_map")
    xyz, _pose, _share = M.order_case()
    rng = np.random.default_rng(14)
    rel = np.stack([np.concatenate([[1.0, 0.0, 0.01 * rng.normal(), 0.02 * rng.normal()], [0.8, 0.05 * rng.normal(), 0.0]]) for _ in range(4)])
    rel32 = rel.astype(np.float32)                                                       # what a net hands over
    world, rows = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float64, device=DEV), []
    for j in range(4):
        world = world_map.compose(world, dev(rel32[j]))
        rows.append(world)
    rows = torch.stack(rows).contiguous()
    xyz, _share = M.vetted(xyz[:4], rows.cpu().numpy())                                  # (vetted at the poses it is inserted at)
    wm = new_map(0.1)
    wm.add(dev(xyz), dev(rel32))
    assert same_bits(wm.world64.cpu().numpy(), world.cpu().numpy())
    by_hand = new_map(0.1)
    by_hand.insert(dev(xyz), rows)
    assert same_snapshot(snapshot(wm), snapshot(by_hand))
    check(wm, M.content(xyz, rows.cpu().numpy(), 0.1))
    # two adds of two continue the drive as one add of four; reset() starts over
    two = new_map(0.1)
    two.add(dev(xyz[:2]), dev(rel32[:2]))
    two.add(dev(xyz[2:4]), dev(rel32[2:4]))
    assert same_snapshot(snapshot(wm), snapshot(two))
    two.reset()
    assert two.stats()["occupied"] == 0 and two.points()[0].shape == (0, 3) and two.world64.tolist() == [1.0, 0, 0, 0, 0, 0, 0]
    # save: x y z count float32 rows, read back the way kitti.load_pair reads a scan
    path = str(tmp_path / "map.bin")
    m = wm.save(path)
    back = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
    pts, count, _key = wm.points()
    assert m == len(back) == len(count) > 0
    assert same_bits(back[:, :3], pts.cpu().numpy()) and np.array_equal(back[:, 3], count.cpu().numpy().astype(np.float32))


# ---- predict_sequence(world_map=): the smallest shape tests/test_evaluate_gpu.py uses ---------------------------------------------
SEQ_H, SEQ_W, SEQ_N = 64, 900, 5


@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("world_map_drive"))
    T_diff = write_sequence(root, "04", SEQ_N, SEQ_H, SEQ_W)
    return root, T_diff


def _map_by_hand(net, root, T_diff, q, t):
    """The map built from the returned poses and the input stage's frame-1 images, one sample at a time."""
    kitti, pwclo = load_pkg("kitti"), load_pkg("pwclo_model")
    wm = new_map(0.5, 18)
    n_pts = SEQ_H * SEQ_W
    eye = torch.eye(4, dtype=torch.float32, device=DEV).repeat(1, 1, 1)
    for i in range(SEQ_N):
        pos2, pos1, _n2, _n1, _T = kitti.load_pair(root, "04", i, T_diff, n_pts)
        cloud = np.zeros((1, 2 * n_pts, 3), np.float32)
        cloud[0, :n_pts], cloud[0, n_pts:] = pos2, pos1
        with torch.no_grad():
            _pts, both = pwclo.input_stage(dev(cloud), eye, np.ones(1, np.int64), SEQ_H, SEQ_W, sensor=net.sensor, beam_elev=net.beam_elev)
        wm.add(both[:1], np.concatenate([q[i], t[i]])[None])
    return wm


@pytest.mark.parametrize("lanes,batch,whose", [(0, 2, "net"), (2, 1, "net"), (0, 2, "fit"), (0, 1, "tracker"), (2, 1, "fit")])
def test_predict_sequence_fills_the_map_at_the_poses_it_returns(drive, tmp_path, lanes, batch, whose):
    model, ev, sensor = load_pkg("model"), load_pkg("evaluate"), load_pkg("sensor")
    root, T_diff = drive
    kw = dict(H_input=SEQ_H, W_input=SEQ_W, num_points=SEQ_H * SEQ_W, batch_size=batch, lanes=lanes)
    if whose != "net":                                               # the pose returned is then the fit's, or the tracker's
        kw["fit"] = sensor.PoseFit(iters=1)
    if whose == "tracker":
        kw["model"] = sensor.LocalModel(scans=2)
    net = model.PWCLONet(DEV, seed=0)
    q0, t0 = ev.predict_sequence(net, root, "04", T_diff, **kw)[:2]
    wm = new_map(0.5, 18)
    q1, t1 = ev.predict_sequence(net, root, "04", T_diff, world_map=wm, **kw)[:2]
    assert same_bits(q0, q1) and same_bits(t0, t1)
    s = wm.stats()
    assert s["inserted"] > SEQ_N * SEQ_H * SEQ_W // 4 and s["dropped_full"] == 0 and 0 < s["occupied"] < s["inserted"]
    assert same_snapshot(snapshot(wm), snapshot(_map_by_hand(net, root, T_diff, q1, t1)))
    with pytest.raises(TypeError):
        ev.predict_sequence(net, root, "04", T_diff, world_map="map", **kw)
    if lanes == 0 and whose == "net":                                # run_sequence builds the map from the value and writes it
        out = str(tmp_path / "out")
        ev.run_sequence(net, root, "04", T_diff, out_dir=out, world_map=wm.spec, **kw)
        back = np.fromfile(os.path.join(out, "04_map.bin"), dtype=np.float32).reshape(-1, 4)
        pts, count, _key = wm.points()
        assert same_bits(back[:, :3], pts.cpu().numpy()) and np.array_equal(back[:, 3], count.cpu().numpy().astype(np.float32))
        assert os.path.exists(os.path.join(out, "04_pred.txt"))

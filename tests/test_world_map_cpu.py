"""CPU: the world map's value (sensor.VoxelMap), the pose composition (world_map.compose) against evaluate.pose_rows, the numpy
reference of the insert rule (tests/world_map_reference.py) against hand-worked cases, and the share of points the case generators
remove."""
import math

import numpy as np
import pytest
import torch

import world_map_reference as M
from conftest import load_pkg


def test_voxel_map_is_a_validated_frozen_value():
    sensor = load_pkg("sensor")
    V = sensor.VoxelMap
    v = V()
    assert (v.voxel, v.log2_capacity, v.min_range, v.max_range) == (0.5, 22, 0.0, math.inf) and v.capacity == 1 << 22
    assert v == V(0.5, 22, 0.0, math.inf) and hash(v) == hash(V(voxel=0.5)) and v != V(voxel=0.25)
    assert len({V(), V(0.5), V(0.1), V(0.1, 12)}) == 3
    with pytest.raises(AttributeError):
        v.voxel = 1.0
    for spec in (V(), V(0.1, 10, 1.5, 80.0), V(2, 28, 0, 1e30)):
        assert eval(repr(spec), {"VoxelMap": V, "inf": math.inf}) == spec
    for bad in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=math.inf), dict(voxel=math.nan), dict(log2_capacity=9),
                dict(log2_capacity=29), dict(log2_capacity=12.0), dict(log2_capacity=True), dict(min_range=-0.1),
                dict(min_range=math.nan), dict(min_range=math.inf), dict(min_range=5.0, max_range=5.0), dict(min_range=5.0, max_range=1.0),
                dict(max_range=math.nan)):
        with pytest.raises(ValueError):
            V(**bad)
    assert V(log2_capacity=np.int64(10)).log2_capacity == 10 and V(log2_capacity=28).capacity == 1 << 28


def test_compose_is_the_running_product_of_pose_rows():
    wm, ev = load_pkg("world_map"), load_pkg("evaluate")
    rng = np.random.default_rng(5)
    q = rng.normal(size=(50, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-2.0, 2.0, (50, 3))
    rows = ev.pose_rows(q, t, np.eye(4))
    world = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], dtype=torch.float64)
    dist = load_pkg("distributed")
    for j in range(50):
        world = wm.compose(world, np.concatenate([q[j] * (0.5 + j), t[j]]))          # the scale of a quaternion does not matter
        assert world.dtype == torch.float64 and world.shape == (7,)
        got = np.concatenate([dist.quat2mat(world[:4].numpy()), world[4:].numpy()[:, None]], 1).reshape(12)
        assert np.abs(got - rows[j]).max() < 1e-12
        assert abs(float(world[:4].norm()) - 1.0) < 1e-14


def test_reference_floor_clamp_and_key_packing_by_hand():
    # -0.05 m in 0.5 m voxels: u = -0.1, floor -> index -1 (truncation would say 0), offset floor(0.9 * 65536) = 58982
    i, g, ok = M.axis_index(np.float32([-0.05, 0.05, 0.0, -0.5, 0.5]), 0.5)
    assert i.tolist() == [-1.0, 0.0, 0.0, -1.0, 1.0] and ok.all()
    assert g.tolist() == [58982, 6553, 0, 0, 0]
    # a tiny negative coordinate: u - floor(u) rounds to 1.0, the offset is clamped to 65535
    i, g, ok = M.axis_index(np.float32([-1e-20]), 0.5)
    assert i.tolist() == [-1.0] and g.tolist() == [65535] and ok.all()
    # the index range [-2^20, 2^20), checked in double
    i, g, ok = M.axis_index(np.float32([-524288.0, 524287.75, 524288.0, -524288.25, 1e30]), 0.5)
    assert ok.tolist() == [True, True, False, False, False] and i[:2].tolist() == [-1048576.0, 1048575.0]
    # voxel is a float32: 0.1f is not 0.1
    i, g, ok = M.axis_index(np.float32([0.3]), 0.1)
    assert i.tolist() == [math.floor(float(np.float32(0.3)) / float(np.float32(0.1)))]
    key = M.pack([0, -1, 123, 1048575], [0, -1, -456, -1048576], [0, -1, 789, 5])
    assert [hex(int(k)) for k in key] == ["0x4000020000100000", "0x3ffffdffffefffff", "0x4001edffc7100315", "0x7ffffc0000100005"]
    assert all(int(k) >> 63 == 0 for k in key)
    assert [v.tolist() for v in M.unpack(key)] == [[0, -1, 123, 1048575], [0, -1, -456, -1048576], [0, -1, 789, 5]]


def test_reference_hash_of_three_keys_written_out():
    # worked with python integers: h ^= h >> 30; h *= 0xbf58476d1ce4e5b9; h ^= h >> 27; h *= 0x94d049bb133111eb; h ^= h >> 31 (mod 2^64)
    keys = np.array([0x4000020000100000, 0x3ffffdffffefffff, 0x4001edffc7100315], np.uint64)
    assert [hex(int(h)) for h in M.mix(keys)] == ["0xc626f54750173f7d", "0xb860c17a01f763c6", "0x6a75b7dfff75a1bf"]
    assert M.home(keys, 10).tolist() == [893, 966, 447] and M.home(keys, 22).tolist() == [1523581, 3630022, 3514815]
    # the first output of the splitmix64 generator seeded with 0 (its published test vector): the finaliser of the golden gamma
    assert hex(int(M.mix(np.uint64(0x9e3779b97f4a7c15))[0])) == "0xe220a8397b1dcdaf"

    def by_hand(h):
        mask = (1 << 64) - 1
        h ^= h >> 30
        h = h * 0xbf58476d1ce4e5b9 & mask
        h ^= h >> 27
        h = h * 0x94d049bb133111eb & mask
        return h ^ h >> 31
    rng = np.random.default_rng(1)
    more = rng.integers(0, 1 << 63, 100, dtype=np.uint64)
    assert [int(h) for h in M.mix(more)] == [by_hand(int(k)) for k in more]


def test_reference_content_of_a_hand_made_scan():
    # identity pose (an un-normalised quaternion), voxel 0.5: three points in voxel (0,0,0), one in (-1,0,2), one empty cell
    xyz = np.zeros((1, 1, 6, 3), np.float32)
    xyz[0, 0, :5] = [(0.25, 0.25, 0.25), (0.125, 0.0, 0.375), (0.375, 0.25, 0.0), (-0.25, 0.125, 1.0), (0.0, 0.0, 0.0)]
    xyz[0, 0, 5] = (40.0, 0.0, 0.0)                                                 # beyond max_range
    pose = np.array([[2.0, 0, 0, 0, 0, 0, 0]])
    c = M.content(xyz, pose, 0.5, 0.0, 30.0)
    assert c["stats"] == {"inserted": 4, "filtered": 1, "rejected": 0, "dropped_full": 0, "occupied": 2}
    k0, k1 = int(M.pack([0], [0], [0])[0]), int(M.pack([-1], [0], [2])[0])
    assert c["key"].tolist() == sorted([k0, k1])
    rows = dict(zip(c["key"].tolist(), c["acc"].tolist()))
    assert rows[k0] == [3, 32768 + 16384 + 49152, 32768 + 0 + 32768, 32768 + 49152 + 0]
    assert rows[k1] == [1, 32768, 16384, 0]
    cent = dict(zip(c["key"].tolist(), c["xyz"].tolist()))
    half = 0.5 / 65536.0 * 0.5                                                      # the centre of an offset bin
    assert np.allclose(cent[k0], [0.25 + half, 1.0 / 6 + half, 5.0 / 24 + half], atol=1e-7)
    assert np.allclose(cent[k1], [-0.25 + half, 0.125 + half, 1.0 + half], atol=1e-7)
    # a zero quaternion: the scan is skipped whole and counts nothing
    c = M.content(xyz, np.zeros((1, 7)), 0.5)
    assert c["stats"] == {"inserted": 0, "filtered": 0, "rejected": 0, "dropped_full": 0, "occupied": 0} and len(c["key"]) == 0
    # two inserts merge as one
    both = M.merged([M.content(xyz, pose, 0.5), M.content(xyz, pose, 0.5)], 0.5)
    one = M.content(np.concatenate([xyz, xyz]), np.concatenate([pose, pose]), 0.5)
    assert np.array_equal(both["key"], one["key"]) and np.array_equal(both["acc"], one["acc"]) and both["stats"] == one["stats"]
    assert np.array_equal(both["xyz"].view(np.uint32), one["xyz"].view(np.uint32))


def test_ambiguity_is_a_rounding_midpoint():
    mid = (np.float64(np.float32(1.0)) + np.float64(np.nextafter(np.float32(1.0), np.float32(2.0)))) / 2
    p = np.array([[mid, 0.0, 0.0], [1.0, 2.0, 3.0], [mid + 1e-9, 5.0, 5.0], [np.nextafter(mid, 2.0), 0.0, 0.0]])
    assert M.ambiguous(p).tolist() == [True, False, False, True]


def test_generators_remove_at_most_a_thousandth_of_their_points():
    shares = M.all_shares()
    assert len(shares) == len(M.SHAPES) + 2
    assert all(0.0 <= s <= M.REMOVED_CAP for s in shares), shares
    for i in range(len(M.SHAPES)):                               # ... and what is left is worth inserting
        for voxel in M.VOXELS:
            c = M.exact_content(i, voxel)
            B, H, W = M.SHAPES[i]
            assert c["stats"]["inserted"] > 0.6 * B * H * W and c["stats"]["rejected"] == 0
            assert c["stats"]["occupied"] < c["stats"]["inserted"]              # cells share voxels
            idx = np.stack(M.unpack(c["key"]))
            assert (idx < 0).any() and (idx > 0).any()                          # negative and positive coordinates

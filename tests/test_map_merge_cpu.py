"""CPU: the numpy restatement of elo_map_merge (tests/map_merge_reference.py) against hand-worked rows, and everything about the
merge that needs no GPU: sensor.MapWindow, the refusals of _scan_ops.map_merge, the state file, the ABI and the argument block."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import map_merge_reference as R
import world_map_reference as M
from conftest import load_pkg

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def key_of(ix, iy, iz):
    return int(M.pack([ix], [iy], [iz])[0])


def test_reference_rows_by_hand():
    # voxel 0.5: index 3 -> centre 1.75, index -2 -> centre -0.75
    assert R.box_centre(np.array([key_of(3, -2, 0)]), 0.5).tolist() == [[1.75, -0.75, 0.25]]
    key = np.array([key_of(3, 0, 0), -1, key_of(-2, 5, 1), key_of(3, 0, 0)], np.int64)
    acc = np.array([[2, 10, 20, 30], [9, 9, 9, 9], [1, 65535, 0, 7], [3, 1, 2, 3]], np.int64)
    assert R.classify(key, acc, 0.5).tolist() == [R.ROW, R.SKIP, R.ROW, R.ROW]
    out, report = R.merge(None, key, acc, 0.5)
    order = np.argsort([key_of(3, 0, 0), key_of(-2, 5, 1)])
    assert out["key"].tolist() == [[key_of(3, 0, 0), key_of(-2, 5, 1)][j] for j in order]
    assert out["acc"].tolist() == [[[5, 11, 22, 33], [1, 65535, 0, 7]][j] for j in order]          # the duplicate key: one add per row
    assert report == dict(voxels_merged=3, voxels_filtered=0, voxels_rejected=0, voxels_dropped=0, points_merged=6, points_filtered=0,
                          points_dropped=0, claimed=2)
    assert out["stats"] == dict(inserted=6, filtered=0, rejected=0, dropped_full=0, occupied=2)
    # ... into a table that holds one of the keys: found, not claimed; the destination's other totals stay
    dest = {"key": np.array([key_of(3, 0, 0)], np.int64), "acc": np.array([[4, 4, 4, 4]], np.int64),
            "stats": dict(inserted=4, filtered=7, rejected=1, dropped_full=0, occupied=1)}
    out, report = R.merge(dest, key, acc, 0.5)
    assert report["claimed"] == 1 and report["voxels_merged"] == 3
    assert out["stats"] == dict(inserted=10, filtered=7, rejected=1, dropped_full=0, occupied=2)
    assert dict(zip(out["key"].tolist(), out["acc"].tolist()))[key_of(3, 0, 0)] == [9, 15, 26, 37]
    centroid = M.centroids(out["key"], out["acc"], 0.5)
    assert centroid.dtype == np.float32 and np.array_equal(centroid, out["xyz"])


def test_reference_window_is_a_closed_box():
    # voxel 0.5, index 3: centre 1.75; window centre 0.25, radius 1.5: d = 1.5 exactly -> kept; index 4 (centre 2.25): filtered
    c = np.array([0.25, 0.25, 0.25])
    one = np.array([[1, 0, 0, 0]], np.int64)
    for axis in range(3):
        at = lambda i: np.array([key_of(*[i if a == axis else 0 for a in range(3)])], np.int64)
        assert R.classify(at(3), one, 0.5, c, 1.5).tolist() == [R.ROW]
        assert R.classify(at(4), one, 0.5, c, 1.5).tolist() == [R.FILTERED]
        assert R.classify(at(-3), one, 0.5, c, 1.5).tolist() == [R.ROW]                 # centre -1.25: d = 1.5 exactly, kept
        assert R.classify(at(-4), one, 0.5, c, 1.5).tolist() == [R.FILTERED]            # centre -1.75
    # a box, not a sphere: the corner at 1.5 on every axis is kept
    assert R.classify(np.array([key_of(3, 3, -3)]), one, 0.5, c, 1.5).tolist() == [R.ROW]
    assert R.classify(np.array([key_of(0, 0, 0)]), one, 0.5, np.array([math.nan, 0.25, 0.25]), 1.5).tolist() == [R.FILTERED]
    out, report = R.merge(None, np.array([key_of(3, 0, 0), key_of(4, 0, 0)]), np.array([[2, 0, 0, 0], [5, 0, 0, 0]]), 0.5, c, 1.5)
    assert out["key"].tolist() == [key_of(3, 0, 0)] and report["voxels_filtered"] == 1 and report["points_filtered"] == 5
    assert out["stats"]["inserted"] == 2                                                 # filtered rows do not touch the stats


def test_reference_min_count_and_malformed_rows():
    k = np.array([key_of(1, 2, 3)], np.int64)
    row = np.array([[5, 1, 2, 3]], np.int64)
    assert R.classify(k, row, 0.5, min_count=5).tolist() == [R.ROW]
    assert R.classify(k, row, 0.5, min_count=6).tolist() == [R.FILTERED]
    top = np.array([key_of(1, 2, 3) | -(1 << 63)], np.int64)                              # the top bit set, not all ones
    assert top[0] != -1 and R.classify(top, row, 0.5).tolist() == [R.REJECTED]
    bad = [[0, 0, 0, 0], [1 << 40, 0, 0, 0], [2, 2 * 65535 + 1, 0, 0], [2, 0, 2 * 65535 + 1, 0], [2, 0, 0, 2 * 65535 + 1], [-3, 0, 0, 0], [2, -1, 0, 0]]
    for r in bad:
        assert R.classify(k, np.array([r], np.int64), 0.5).tolist() == [R.REJECTED], r
    assert R.classify(k, np.array([[(1 << 40) - 1, 0, 0, 65535 * ((1 << 40) - 1)]], np.int64), 0.5).tolist() == [R.ROW]
    # malformed comes before min_count and the window: it is `rejected`, not `filtered`
    assert R.classify(k, np.array([[0, 0, 0, 0]], np.int64), 0.5, np.array([900.0, 0, 0]), 1.0, min_count=9).tolist() == [R.REJECTED]
    out, report = R.merge(None, np.concatenate([k, k, top]), np.array([[5, 1, 2, 3], [0, 0, 0, 0], [5, 1, 2, 3]], np.int64), 0.5)
    assert report["voxels_rejected"] == 2 and report["voxels_merged"] == 1 and out["stats"]["inserted"] == 5


def test_reference_union_is_the_map_of_the_union_of_the_points():
    xyz, pose, _share = M.order_case()
    for voxel in M.VOXELS:
        a, b = M.content(xyz[:3], pose[:3], voxel), M.content(xyz[3:], pose[3:], voxel)
        want = M.content(xyz, pose, voxel)
        for first, second in ((a, b), (b, a)):
            out, report = R.merge(first, *R.rows_of(second), voxel)
            assert np.array_equal(out["key"], want["key"]) and np.array_equal(out["acc"], want["acc"])
            assert out["xyz"].tobytes() == want["xyz"].tobytes() and out["stats"] == want["stats"]
            assert report["points_merged"] == second["stats"]["inserted"] and report["claimed"] == len(want["key"]) - len(first["key"])
            assert 0 < report["claimed"] < report["voxels_merged"]                       # some keys found, some claimed


def test_map_window_is_a_validated_frozen_value():
    S = load_pkg("sensor")
    w = S.MapWindow(80.0)
    assert (w.radius, w.every, w.min_count) == (80.0, 10, 1)
    assert repr(S.MapWindow(30, every=2, min_count=3)) == "MapWindow(radius=30.0, every=2, min_count=3)"
    assert w == S.MapWindow(80, 10, 1) and hash(w) == hash(S.MapWindow(80, 10, 1)) and w != S.MapWindow(80.0, 5)
    assert len({w, S.MapWindow(80.0), S.MapWindow(81.0)}) == 2
    with pytest.raises(AttributeError):
        w.radius = 1.0
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=math.inf), dict(radius=math.nan), dict(radius=True),
                dict(radius=5.0, every=0), dict(radius=5.0, every=2.0), dict(radius=5.0, every=True), dict(radius=5.0, min_count=0),
                dict(radius=5.0, min_count=1.5)):
        with pytest.raises(ValueError):
            S.MapWindow(**bad)
    W = load_pkg("world_map")
    with pytest.raises(TypeError):
        W.WorldMap(S.VoxelMap(0.5, 10), "cpu", window=80.0)
    assert W.WorldMap(S.VoxelMap(0.5, 10), "cpu", window=w).window is w


def test_host_refusals_come_before_the_library(monkeypatch):
    ops, L, S = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor")

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "lib", no_library)
    spec = S.VoxelMap(0.5, 10)
    C = spec.capacity
    keys, acc, stats = torch.full((C,), -1, dtype=torch.int64), torch.zeros((C, 4), dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    sk, sa = torch.full((16,), -1, dtype=torch.int64), torch.zeros((16, 4), dtype=torch.int64)
    centre = torch.zeros(3, dtype=torch.float64)
    world = torch.zeros(7, dtype=torch.float64)
    call = lambda *a, **kw: ops.map_merge(*a, **kw)
    type_errors = [lambda: call(keys, acc, stats, sk, sa, "spec"), lambda: call(keys, acc, stats, sk.int(), sa, spec),
                   lambda: call(keys, acc, stats, sk, sa.double(), spec), lambda: call(keys, acc, stats, sk.numpy(), sa, spec),
                   lambda: call(keys.int(), acc, stats, sk, sa, spec), lambda: call(keys, acc, stats, sk, sa, spec, centre.float(), 5.0),
                   lambda: call(keys, acc, stats, sk, sa, spec, [0.0, 0.0, 0.0], 5.0)]
    for bad in type_errors:
        with pytest.raises(TypeError):
            bad()
    elo_errors = [lambda: call(keys[:-1], acc, stats, sk, sa, spec), lambda: call(keys, acc, stats[:7], sk, sa, spec),
                  lambda: call(keys, acc, stats, sk, sa[:15], spec), lambda: call(keys, acc, stats, sk.reshape(4, 4), sa, spec),
                  lambda: call(keys, acc, stats, sk, sa.t().contiguous().t(), spec),          # not contiguous
                  lambda: call(keys, acc, stats, sk[::2], sa[:8], spec),
                  lambda: call(keys, acc, stats, keys, acc, spec),                            # a table into itself
                  lambda: call(keys, acc, stats, keys[8:24], sa, spec), lambda: call(keys, acc, stats, sk, acc[:16], spec),
                  lambda: call(keys, acc, stats, sk, sa, spec, min_count=0), lambda: call(keys, acc, stats, sk, sa, spec, min_count=1.0),
                  lambda: call(keys, acc, stats, sk, sa, spec, min_count=True),
                  lambda: call(keys, acc, stats, sk, sa, spec, radius=5.0),                   # a radius about nothing
                  lambda: call(keys, acc, stats, sk, sa, spec, centre), lambda: call(keys, acc, stats, sk, sa, spec, centre, 0.0),
                  lambda: call(keys, acc, stats, sk, sa, spec, centre, -2.0), lambda: call(keys, acc, stats, sk, sa, spec, centre, math.inf),
                  lambda: call(keys, acc, stats, sk, sa, spec, centre, math.nan), lambda: call(keys, acc, stats, sk, sa, spec, world[3:], 5.0),
                  lambda: call(keys, acc, stats, sk, sa, spec, world[::2][:3], 5.0)]
    for j, bad in enumerate(elo_errors):
        with pytest.raises(L.EloError):
            bad()
    # what is well formed gets as far as the device check: there is no CPU path
    monkeypatch.undo()
    for ok in (lambda: call(keys, acc, stats, sk, sa, spec), lambda: call(keys, acc, stats, sk, sa, spec, world[4:], 5.0, min_count=3)):
        with pytest.raises(L.EloError, match="GPU"):
            ok()
    assert int((keys != -1).sum()) == 0 and int(acc.abs().sum()) == 0 and int(stats.sum()) == 0


def test_state_round_trips_through_a_pure_numpy_read(tmp_path):
    S, W = load_pkg("sensor"), load_pkg("world_map")
    wm = W.WorldMap(S.VoxelMap(0.25, 10, min_range=1.0, max_range=80.0), "cpu")            # the buffers only: nothing is launched
    rng = np.random.default_rng(5)
    slots = rng.permutation(1024)[:40]
    keys = np.array([key_of(*rng.integers(-50, 50, 3)) for _ in range(40)], np.int64)
    assert len(np.unique(keys)) == 40
    acc = np.concatenate([rng.integers(1, 9, (40, 1)), rng.integers(0, 65536, (40, 3))], 1).astype(np.int64)
    wm.keys[torch.from_numpy(slots)] = torch.from_numpy(keys)
    wm.acc[torch.from_numpy(slots)] = torch.from_numpy(acc)
    wm.stat_words[:5] = torch.tensor([int(acc[:, 0].sum()), 3, 2, 1, 40])
    wm.world64.copy_(torch.tensor([0.5, 0.5, 0.5, 0.5, 1.25, -2.5, 0.125], dtype=torch.float64))
    state = wm.state()
    order = np.argsort(keys)
    assert state["key"].dtype == np.int64 and state["acc"].dtype == np.int64 and state["acc"].shape == (40, 4)
    assert np.array_equal(state["key"], keys[order]) and np.array_equal(state["acc"], acc[order])
    assert {n: state[n] for n in W.WorldMap.STATS} == wm.stats() == dict(inserted=int(acc[:, 0].sum()), filtered=3, rejected=2, dropped_full=1, occupied=40)
    assert (state["voxel"], state["min_range"], state["max_range"], state["log2_capacity"]) == (0.25, 1.0, 80.0, 10)
    path = str(tmp_path / "state.npz")
    assert wm.save_state(path) == 40
    with np.load(path, allow_pickle=False) as f:                                         # data only: nothing to unpickle
        back = {n: f[n] for n in f.files}
    assert set(back) == set(state)
    for n, v in state.items():
        assert np.array_equal(back[n], np.asarray(v)) and back[n].dtype == np.asarray(v).dtype, n
    assert back["world64"].tolist() == [0.5, 0.5, 0.5, 0.5, 1.25, -2.5, 0.125]
    assert R.classify(back["key"], back["acc"], float(back["voxel"])).tolist() == [R.ROW] * 40   # what load_state will merge
    with pytest.raises(ValueError):
        W.WorldMap(S.VoxelMap(0.25, 10), "cpu").merge(W.WorldMap(S.VoxelMap(0.5, 10), "cpu"))    # another voxel
    with pytest.raises(TypeError):
        W.WorldMap(S.VoxelMap(0.25, 10), "cpu").merge(7)


def _declared_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            out += [re.sub(r"^.*[\s*]", "", field.strip()) for field in decl.split(",")]
    return out


def test_the_argument_block_is_declared_and_mirrored(tmp_path):
    L = load_pkg("_lib")
    with open(os.path.join(ROOT, "include", "elo.h")) as f:
        header = f.read()
    fields = ["rows", "src_keys", "src_acc", "voxel", "log2_capacity", "keys", "acc", "stats", "centre", "radius", "min_count", "report"]
    struct, mirror = "elo_map_merge_args", L.MapMergeArgs
    assert re.search(r"^int elo_map_merge\(const %s \*a, elo_stream_t stream\);" % struct, header, re.M)
    assert mirror.__name__ == struct
    assert [n for n, _ in mirror._fields_] == _declared_fields(header, struct) == fields
    assert ("elo_map_merge", ctypes.c_int, [ctypes.POINTER(mirror), ctypes.c_void_p]) in L.SYMBOLS
    assert L.ABI_VERSION == 26                                                          # additive: no existing struct moved
    assert len(L.MAP_REPORT) == 8
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "elo.h"', 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (struct, struct)]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (n, struct, n) for n in fields]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    sizes = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert ctypes.sizeof(mirror) == int(sizes[struct]) == 88
    for n in fields:
        assert getattr(mirror, n).offset == int(sizes[n]), n

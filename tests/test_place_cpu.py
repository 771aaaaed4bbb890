"""CPU: the numpy restatement of the place-recognition rule (tests/place_reference.py) against hand-worked cases, and everything
about it that needs no GPU: sensor.ScanContext and sensor.Places, the refusals of _scan_ops.scan_descriptor and _scan_ops.descriptor_search,
the argument blocks against a C compiler, the index's state file, and the gap condition of the case table the GPU file compares
exactly (tests/place_cases.py)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import place_cases as C
import place_reference as R
from conftest import load_pkg

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_reference_descriptor_by_hand():
    x, ctx, want = C.placed()
    assert R.sector_of(7, 3).tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert R.edge2(4, 32.0).tolist() == [0.0, 64.0, 256.0, 576.0, 1024.0]
    got = R.descriptor(x, **ctx)
    assert got.dtype == np.uint16 and got.shape == (1, 3, 4) and np.array_equal(got, want)
    # every placed point on its own: the edge, the two range limits, the level boundary, the clamps
    one = lambda p, w=0: R.descriptor(np.array(p, np.float32).reshape(1, 1, 1, 3).repeat(7, 2) * (np.arange(7) == w)[None, None, :, None], **ctx)[0]
    assert one((8.0, 0.0, -2.5)).tolist()[0] == [0, 2, 0, 0]                              # r2 == edge2[1]: the ring above; level 2 exactly
    assert one((7.999999, 0.0, -2.5)).tolist()[0] == [2, 0, 0, 0]
    assert one((0.0, 32.0, 5.0)).tolist()[0] == [0, 0, 0, 0]                              # r2 == edge2[rings]: out
    assert one((0.0, 31.99999, 5.0)).tolist()[0] == [0, 0, 0, 17]
    assert one((1.9999999, 0.0, 5.0)).tolist()[0] == [0, 0, 0, 0] and one((2.0, 0.0, 5.0)).tolist()[0] == [17, 0, 0, 0]
    assert one((3.0, 0.0, -3.0)).tolist()[0] == [1, 0, 0, 0] and one((3.0, 0.0, -3.0000002)).tolist()[0] == [1, 0, 0, 0]
    assert one((3.0, 0.0, -1e30)).tolist()[0] == [1, 0, 0, 0] and one((3.0, 0.0, 1e30)).tolist()[0] == [C.LEVELS, 0, 0, 0]
    assert one((3.0, 0.0, 2043.9999)).tolist()[0] == [C.LEVELS - 1, 0, 0, 0]
    assert one((3.0, 0.0, 1.0), w=6).tolist() == [[0] * 4, [0] * 4, [9, 0, 0, 0]]            # the column decides the sector
    assert not R.descriptor(np.zeros((2, 3, 7, 3), np.float32), **ctx).any()               # an image without points
    # a W that sectors does not divide: 67 columns in 8 sectors, runs of 9 and 8
    assert np.bincount(R.sector_of(67, 8)).tolist() == [9, 8, 9, 8, 8, 9, 8, 8]
    assert [int(np.argmax(R.sector_of(67, 8) == s)) for s in range(8)] == [0, 9, 17, 26, 34, 42, 51, 59]


def test_reference_distance_by_hand():
    # two sectors, two rings.  Q = [[3, 4], [0, 0]]: column 1 is empty and is skipped wherever it lands
    Q = np.array([[3, 4], [0, 0]], np.uint16)
    D = np.array([[4, 3], [3, 4]], np.uint16)
    # shift 0: Q0 . D0 = 24, a = b = 25 -> 1 - 24/25; shift 1: Q0 . D1 = 25 -> 1 - 25/25 = 0
    prof = R.shift_profile(Q, D)
    assert prof.tolist() == [1.0 - 24.0 / 25.0, 0.0] and R.best_of(prof) == (1, 0.0)
    # three sectors, one pair skipped on the entry's side: D's column 2 is empty
    Q = np.array([[1, 0], [0, 2], [2, 2]], np.uint16)
    D = np.array([[0, 1], [1, 1], [0, 0]], np.uint16)
    r2 = math.sqrt(2.0)
    want0 = ((1.0 - 0.0 / math.sqrt(1.0)) + (1.0 - 2.0 / math.sqrt(8.0))) / 2.0           # (Q0,D0) (Q1,D1); (Q2,D2) skipped
    want1 = ((1.0 - 1.0 / math.sqrt(2.0)) + (1.0 - 2.0 / math.sqrt(8.0))) / 2.0           # (Q0,D1); (Q1,D2) skipped; (Q2,D0)
    want2 = ((1.0 - 2.0 / math.sqrt(4.0)) + (1.0 - 4.0 / math.sqrt(16.0))) / 2.0          # (Q0,D2) skipped; (Q1,D0) (Q2,D1)
    assert R.shift_profile(Q, D).tolist() == [want0, want1, want2] and want2 == 0.0 and r2 > 1
    # the terms are added one after the other from 0.0, in ascending j
    rng = np.random.default_rng(1)
    Q, D = C.random_descriptors(rng, 1, 16, 5)[0], C.random_descriptors(rng, 1, 16, 5)[0]
    T, ok = R.terms(Q, D)
    for s in (0, 5, 15):
        total, n = 0.0, 0
        for j in range(16):
            c = (j + s) % 16
            if ok[j, c]:
                a, b, d = int((Q[j].astype(int) ** 2).sum()), int((D[c].astype(int) ** 2).sum()), int((Q[j].astype(int) * D[c].astype(int)).sum())
                total, n = total + (1.0 - float(d) / math.sqrt(float(a * b))), n + 1
        assert R.shift_profile(Q, D)[s] == total / n
    # no pair at all: +inf, and the smallest shift is the best one
    empty = np.zeros((3, 2), np.uint16)
    assert R.shift_profile(Q[:3, :2], empty).tolist() == [math.inf] * 3 and R.best_of(R.shift_profile(empty, empty)) == (0, math.inf)
    # the largest product fits: 4095^2 * 32 < 2^31, and identical columns give exactly 0
    full = np.full((2, 32), C.LEVELS, np.uint16)
    assert C.LEVELS ** 2 * 32 < 2 ** 31 and R.shift_profile(full, full).tolist() == [0.0, 0.0]


def test_reference_ties_and_padding():
    rng = np.random.default_rng(2)
    d = C.random_descriptors(rng, 4, 6, 3)
    db = np.stack([d[1], d[0], d[2], d[0], d[3]])                                          # entries 1 and 3 are the query itself
    ref = R.search(d[:1], db, 5, 8)
    assert ref["entry"][0, :2].tolist() == [1, 3] and ref["dist"][0, 0] == ref["dist"][0, 1] < 1e-12     # the smaller index wins
    assert ref["shift"][0, :2].tolist() == [0, 0]
    assert ref["entry"][0, 5:].tolist() == [-1] * 3 and ref["shift"][0, 5:].tolist() == [-1] * 3 and np.isinf(ref["dist"][0, 5:]).all()
    assert R.search(d[:1], db, 3, 1)["entry"].tolist() == [[1]]                              # m below the rows held: the rest is ignored
    assert R.search(d[:1], db, 1, 1)["entry"].tolist() != [[1]]
    pad = R.search(d[:2], db, 0, 2)
    assert pad["entry"].tolist() == [[-1, -1]] * 2 and np.isinf(pad["dist"]).all() and pad["best_dist"].shape == (2, 0)
    # a descriptor periodic under a shift of 3 columns: shifts 0 and 3 tie, the smaller wins; rolled by one: shifts 1 and 4
    half = C.random_descriptors(rng, 1, 3, 3)[0]
    per = np.concatenate([half, half])
    prof = R.shift_profile(per, per)
    assert prof[0] == prof[3] and R.best_of(prof)[0] == 0
    assert R.best_of(R.shift_profile(per, np.roll(per, 1, axis=0)))[0] == 1                 # D[c] = per[c - 1]: column j goes with j + 1
    for s in (0, 1, 5):
        got = R.best_of(R.shift_profile(d[0], np.roll(d[0], s, axis=0)))
        assert got[0] == s and got[1] < 1e-12
    assert R.yaw_of(0, 60) == 0.0 and R.yaw_of(59, 60) == 2.0 * math.pi / 60 and R.yaw_of(1, 60) == -2.0 * math.pi / 60
    assert R.yaw_of(30, 60) == -math.pi and R.yaw_of(31, 60) == 29 * (2.0 * math.pi / 60)


def test_the_case_table_is_decided_by_gaps():
    """Every discrete result the GPU file compares exactly -- a best shift, a rank -- is decided in the float64 reference by at
    least GAP = 1e-9, four orders above the 1e-12 bound on a dist, for the WHOLE table and for the end-to-end case; the cases
    marked `tie` hold exact values (0.0 or +inf) only."""
    for name in C.SEARCH:
        _q, _db, m, k, tie, _ctx, ref = C.search_case(name)
        if tie:
            finite = ref["profile"][np.isfinite(ref["profile"])]
            assert (finite == 0.0).all(), name
            continue
        over_shifts, over_entries = C.smallest_gaps(ref, m, k)
        print("%s: gaps %.3g over shifts, %.3g over entries" % (name, over_shifts, over_entries))
        assert over_shifts >= C.GAP and over_entries >= C.GAP, name
    e = C.e2e()
    for which in ("query_search",):
        over_shifts, over_entries = C.smallest_gaps(e[which], 6, 4)
        assert over_shifts >= C.GAP and over_entries >= C.GAP
    assert e["query_search"]["entry"][0, 0] == C.E2E_KEY and e["query_search"]["shift"][0, 0] == e["shift"] == 25
    assert np.isinf(e["far_search"]["dist"]).all() and not R.descriptor(e["far"], **C.E2E_CONTEXT).any()
    for i in range(len(C.DESCRIPTOR_SHAPES)):
        (n, _H, _W), (sectors, rings) = C.DESCRIPTOR_SHAPES[i]
        assert C.cloud_descriptor(i).shape == (n, sectors, rings)


def test_scan_context_and_places_are_validated_frozen_values():
    S = load_pkg("sensor")
    c = S.ScanContext()
    assert (c.rings, c.sectors, c.max_range, c.min_range, c.z_min, c.z_step) == (20, 60, S.KITTI_HDL64.crop_xy, 0.0, -3.0, 0.005)
    assert repr(c) == "ScanContext(rings=20, sectors=60, max_range=35.0, min_range=0.0, z_min=-3.0, z_step=0.005)"
    assert c == S.ScanContext(20, 60, 35) and hash(c) == hash(S.ScanContext(20, 60, 35.0)) and c != S.ScanContext(21)
    assert len({c, S.ScanContext(), S.ScanContext(sectors=64)}) == 2 and S.ScanContext.LEVELS == C.LEVELS
    with pytest.raises(AttributeError):
        c.rings = 3
    for bad in (dict(rings=0), dict(rings=33), dict(rings=2.0), dict(rings=True), dict(sectors=0), dict(sectors=129), dict(sectors="8"),
                dict(max_range=0.0), dict(max_range=math.inf), dict(max_range=math.nan), dict(min_range=-1.0), dict(min_range=35.0),
                dict(min_range=math.nan), dict(z_min=math.inf), dict(z_min=math.nan), dict(z_step=0.0), dict(z_step=-1.0),
                dict(z_step=math.inf), dict(z_step=True)):
        with pytest.raises(ValueError):
            S.ScanContext(**bad)
    assert S.ScanContext(32, 128).rings == 32 and S.ScanContext(1, 1).sectors == 1
    for rings, far in ((20, 35.0), (7, 80.5), (32, 0.3)):
        assert np.array_equal(np.array(S.ScanContext(rings, 8, far).edge2()), R.edge2(rings, far))
    for sectors in (1, 7, 60, 128):
        for s in range(sectors):
            assert S.ScanContext(3, sectors).yaw_of(s) == R.yaw_of(s, sectors)
    p = S.Places()
    assert (p.context, p.every, p.skip_recent, p.capacity) == (c, 5, 50, 4096)
    assert p == S.Places(c, 5, 50, 4096) and hash(p) == hash(S.Places()) and p != S.Places(every=4)
    assert repr(S.Places(every=2)).startswith("Places(context=ScanContext(") and repr(S.Places(every=2)).endswith("every=2, skip_recent=50, capacity=4096)")
    with pytest.raises(AttributeError):
        p.every = 1
    for bad in (dict(context=60), dict(every=0), dict(every=1.0), dict(every=True), dict(skip_recent=-1), dict(skip_recent=0.5),
                dict(capacity=0), dict(capacity=2 ** 31)):
        with pytest.raises(ValueError):
            S.Places(**bad)
    W = load_pkg("world_map")
    with pytest.raises(TypeError):
        W.WorldMap(S.VoxelMap(0.5, 10), "cpu", places=c)
    wm = W.WorldMap(S.VoxelMap(0.5, 10), "cpu", places=S.Places(S.ScanContext(4, 8), capacity=16))
    assert len(wm.places) == 0 and wm.places.desc.shape == (16, 8, 4) and wm.revisits().shape == (0, 5)
    with pytest.raises(ValueError):
        W.WorldMap(S.VoxelMap(0.5, 10), "cpu").relocalise(torch.zeros(1, 4, 8, 3))
    # an add() whose due scans the index has no room for is refused before anything is enqueued: the map is as it was
    wm = W.WorldMap(S.VoxelMap(0.5, 10), "cpu", places=S.Places(S.ScanContext(4, 8), every=2, capacity=3))
    wm.places._count, wm._scans = 2, 3                                                     # two entries held; scans 3 .. 6 come next
    pose = torch.tensor([[1.0, 0, 0, 0, 0.5, 0, 0]] * 4, dtype=torch.float64)
    with pytest.raises(IndexError):
        wm.add(torch.zeros((4, 3, 8, 3)), pose)                                              # scans 3 and 5 are due: one too many
    assert wm._scans == 3 and len(wm.places) == 2 and wm.trajectory().shape == (0, 7) and wm.world64.tolist() == [1.0, 0, 0, 0, 0, 0, 0]
    assert int((wm.keys != -1).sum()) == 0 and wm.revisits().shape == (0, 5)


def test_host_refusals_come_before_the_library(monkeypatch):
    ops, L, S = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor")

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "lib", no_library)
    spec = S.ScanContext(4, 8)
    xyz = torch.zeros((2, 3, 16, 3))
    out = torch.zeros((2, 8, 4), dtype=torch.uint16)
    q, db = torch.zeros((2, 8, 4), dtype=torch.uint16), torch.zeros((5, 8, 4), dtype=torch.uint16)
    D, F = ops.scan_descriptor, ops.descriptor_search
    type_errors = [lambda: D(xyz, "spec"), lambda: D(xyz.double(), spec), lambda: D(xyz.numpy(), spec), lambda: D(xyz, spec, out.int()),
                   lambda: D(xyz, spec, out.numpy()), lambda: F(q, db, 5, S.VoxelMap()), lambda: F(q.short(), db, 5, spec),
                   lambda: F(q, db.int(), 5, spec), lambda: F(q.numpy(), db, 5, spec)]
    for bad in type_errors:
        with pytest.raises(TypeError):
            bad()
    elo_errors = [lambda: D(xyz[..., :2], spec), lambda: D(xyz[0], spec), lambda: D(xyz[:, :, :7].contiguous(), spec),      # W < sectors
                  lambda: D(xyz[:, :, ::2], spec), lambda: D(xyz.permute(0, 2, 1, 3), spec),                                # layout
                  lambda: D(xyz, spec, out[:1]), lambda: D(xyz, spec, out.reshape(2, 4, 8)), lambda: D(xyz, spec, out.reshape(2, 32)),
                  lambda: D(xyz, spec, torch.zeros((2, 8, 8), dtype=torch.uint16)[:, :, :4]),
                  lambda: D(torch.zeros((2, 0, 16, 3)), spec),
                  lambda: F(q, db, -1, spec), lambda: F(q, db, 6, spec), lambda: F(q, db, 2.0, spec), lambda: F(q, db, True, spec),
                  lambda: F(q, db, 5, spec, k=0), lambda: F(q, db, 5, spec, k=9), lambda: F(q, db, 5, spec, k=1.0),
                  lambda: F(q.reshape(2, 4, 8), db, 5, spec), lambda: F(q, db.reshape(5, 32), 5, spec), lambda: F(q[0], db, 5, spec),
                  lambda: F(q, torch.zeros((5, 8, 8), dtype=torch.uint16)[:, :, :4], 5, spec), lambda: F(q, db, 5, S.ScanContext(4, 9))]
    for j, bad in enumerate(elo_errors):
        with pytest.raises(L.EloError):
            bad()
    # what is well formed gets as far as the device check: there is no CPU path
    monkeypatch.undo()
    for ok in (lambda: D(xyz, spec), lambda: D(xyz, spec, out), lambda: F(q, db, 5, spec, k=8), lambda: F(q, db, 0, spec)):
        with pytest.raises(L.EloError, match="GPU"):
            ok()
    P = load_pkg("places")
    with pytest.raises(TypeError):
        P.PlaceIndex(S.VoxelMap(), 4, "cpu")
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError):
            P.PlaceIndex(spec, bad, "cpu")
    index = P.PlaceIndex(spec, 2, "cpu")
    with pytest.raises(IndexError):
        index.add(torch.zeros((3, 3, 16, 3)), torch.zeros((3, 7), dtype=torch.float64))      # full: refused before any launch
    with pytest.raises(ValueError):
        index.add(xyz, torch.zeros((3, 7), dtype=torch.float64))
    assert len(index) == 0


def _declared_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            out += [re.sub(r"\[.*\]$", "", re.sub(r"^.*[\s*]", "", re.sub(r"\[.*\]$", "", field.strip()))) for field in decl.split(",")]
    return out


def test_the_argument_blocks_are_declared_and_mirrored(tmp_path):
    L = load_pkg("_lib")
    with open(os.path.join(ROOT, "include", "elo.h")) as f:
        header = f.read()
    blocks = {"elo_scan_descriptor_args": (L.ScanDescriptorArgs, "elo_scan_descriptor",
                                           ["batch", "H", "W", "rings", "sectors", "z_min", "z_step", "min_range2", "edge2", "xyz", "desc"], 328),
              "elo_descriptor_search_args": (L.DescriptorSearchArgs, "elo_descriptor_search",
                                             ["n", "m", "rings", "sectors", "k", "query", "db", "entry", "shift", "dist", "best_shift", "best_dist"], 80)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "elo.h"', 'int main(void) {',
             'printf("levels %d\\nrings %d\\nsectors %d\\nk %d\\n", ELO_PLACE_LEVELS, ELO_PLACE_MAX_RINGS, ELO_PLACE_MAX_SECTORS, ELO_PLACE_MAX_K);']
    for struct, (mirror, entry, fields, _size) in blocks.items():
        assert re.search(r"^int %s\(const %s \*a, elo_stream_t stream\);" % (entry, struct), header, re.M)
        assert mirror.__name__ == struct
        assert [n for n, _ in mirror._fields_] == _declared_fields(header, struct) == fields
        assert (entry, ctypes.c_int, [ctypes.POINTER(mirror), ctypes.c_void_p]) in L.SYMBOLS
        lines += ['printf("%s %%zu\\n", sizeof(%s));' % (struct, struct)]
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (struct, n, struct, n) for n in fields]
    assert L.ABI_VERSION == 26                                                          # additive: no existing struct moved
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    sizes = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert (int(sizes["levels"]), int(sizes["rings"]), int(sizes["sectors"]), int(sizes["k"])) == \
        (L.PLACE_LEVELS, L.PLACE_MAX_RINGS, L.PLACE_MAX_SECTORS, L.PLACE_MAX_K) == (4095, 32, 128, 8)
    for struct, (mirror, _entry, fields, size) in blocks.items():
        assert ctypes.sizeof(mirror) == int(sizes[struct]) == size
        for n in fields:
            assert getattr(mirror, n).offset == int(sizes["%s.%s" % (struct, n)]), n
    assert L.ScanDescriptorArgs.edge2.size == 33 * ctypes.sizeof(ctypes.c_double)


def test_index_state_round_trips_through_a_pure_numpy_read(tmp_path):
    S, P, W = load_pkg("sensor"), load_pkg("places"), load_pkg("world_map")
    spec = S.ScanContext(4, 8, 30.0, 1.0, -2.0, 0.01)
    index = P.PlaceIndex(spec, 16, "cpu")                                                  # the buffers only: nothing is launched
    rng = np.random.default_rng(3)
    desc = C.random_descriptors(rng, 5, 8, 4)
    pose = np.concatenate([np.tile([1.0, 0.0, 0.0, 0.0], (5, 1)), rng.normal(size=(5, 3))], 1)
    index.desc[:5] = torch.from_numpy(desc)
    index.pose64[:5] = torch.from_numpy(pose)
    index.scan[:5] = torch.tensor([4, 9, 14, 19, 24])
    index._count = 5
    state = index.state()
    assert state["place_desc"].dtype == np.uint16 and np.array_equal(state["place_desc"], desc)
    assert np.array_equal(state["place_pose64"], pose) and state["place_scan"].tolist() == [4, 9, 14, 19, 24]
    path = str(tmp_path / "places.npz")
    assert index.save_state(path) == 5
    with np.load(path, allow_pickle=False) as f:                                         # data only: nothing to unpickle
        back = {n: f[n] for n in f.files}
    assert set(back) == set(state)
    for n, v in state.items():
        assert np.array_equal(back[n], np.asarray(v)) and back[n].dtype == np.asarray(v).dtype, n
    again = P.PlaceIndex.load_state(path, device="cpu")
    assert len(again) == 5 and again.spec == spec and again.capacity == 4096
    assert torch.equal(again.desc[:5], index.desc[:5]) and torch.equal(again.pose64[:5], index.pose64[:5]) and torch.equal(again.scan[:5], index.scan[:5])
    malformed = [dict(place_desc=desc.astype(np.int16)), dict(place_desc=desc[:, :, :3]), dict(place_desc=desc.reshape(5, 32)),
                 dict(place_desc=np.where(desc == desc.max(), 4096, desc).astype(np.uint16)), dict(place_pose64=pose.astype(np.float32)),
                 dict(place_pose64=pose[:4]), dict(place_scan=np.arange(5, dtype=np.int32)), dict(place_scan=np.arange(4)),
                 dict(place_pose64=np.where(pose == pose[2, 5], np.nan, pose)), dict(place_rings=5), dict(place_sectors=0)]
    for j, change in enumerate(malformed):
        bad = str(tmp_path / ("bad%d.npz" % j))
        np.savez(bad, **dict(back, **change))
        with pytest.raises(ValueError):
            P.PlaceIndex.load_state(bad, device="cpu")
    np.savez(str(tmp_path / "short.npz"), **{n: v for n, v in back.items() if n != "place_scan"})
    with pytest.raises(ValueError):
        P.PlaceIndex.load_state(str(tmp_path / "short.npz"), device="cpu")
    with pytest.raises(ValueError):
        P.PlaceIndex.load_state(path, capacity=4, device="cpu")                            # more entries than the index holds
    # a map without Places keeps exactly the keys it had; with Places the index's arrays ride along under their own names
    plain = W.WorldMap(S.VoxelMap(0.5, 10), "cpu").state()
    assert not any(n.startswith("place_") for n in plain)
    wm = W.WorldMap(S.VoxelMap(0.5, 10), "cpu", places=S.Places(spec, capacity=16))
    wm.places = index
    with_places = wm.state()
    assert set(with_places) == set(plain) | set(state) | {"place_revisits"} and with_places["place_revisits"].shape == (0, 5)

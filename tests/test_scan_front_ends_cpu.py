"""CPU: what each of the ten scan-level front ends hands to the library -- the entry's name and every field of its argument block --
against values written out here.  The device check, the library and the launch are stubbed (CPU tensors pass, the three
*_scratch_words answer 64, the launch records its entry and block), so this pins the marshalling alone: sizes, the floats of the
value classes, and every pointer against the data_ptr() of the tensor that must be there, inputs and returned outputs."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from conftest import load_pkg

B, H, W, K = 2, 4, 8, 3
WORDS = 64
f32 = lambda v: ctypes.c_float(v).value
D2R = math.pi / 180
AZ = f32((360.0 / W) * D2R)                                   # the default sensor: +2.0 / -24.8 degrees
VRES = f32((2.0 * D2R - -24.8 * D2R) / (H - 1))
VOFF = f32(24.8 * D2R / ((2.0 * D2R - -24.8 * D2R) / (H - 1)))
BEAMS_DEG = (3.0, 1.0, -2.0, -6.0)


@pytest.fixture
def front(monkeypatch):
    """(the front ends' module, sensor, the list the stubbed launch appends (entry, block) to)."""
    ops, L, S = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor")
    calls = []
    words = lambda b, h, w: WORDS
    stub = types.SimpleNamespace(elo_pose_fit_scratch_words=words, elo_model_render_scratch_words=words, elo_map_fit_scratch_words=words)
    monkeypatch.setattr(L, "require_gpu", lambda *tensors: None)
    monkeypatch.setattr(L, "lib", lambda: stub)
    monkeypatch.setattr(L, "call", lambda entry, args, like: calls.append((entry, args)))
    return ops, S, calls


def fields(block):
    return {name: (list(v) if isinstance(v, ctypes.Array) else v) for name, v in ((n, getattr(block, n)) for n, _t in block._fields_)}


def the_call(calls, entry):
    assert [e for e, _a in calls] == [entry]
    got = fields(calls[0][1])
    calls.clear()
    return got


def table(spec):
    C = spec.capacity
    return torch.full((C,), -1, dtype=torch.int64), torch.zeros((C, 4), dtype=torch.int64), torch.zeros(8, dtype=torch.int64)


def test_pose_fit(front):
    ops, S, calls = front
    x1, x2, pose = torch.zeros((B, H, W, 3)), torch.zeros((B, H, W, 3)), torch.zeros((B, 7))
    fit = S.PoseFit(iters=2, gate=0.75, huber=0.2, jump_rel=0.05, min_count=7, damping=1e-3)
    res = ops.pose_fit(x1, x2, pose, fit)
    assert type(res) is ops.PoseFitResult and res.keep is None
    assert (res.pose.dtype, tuple(res.pose.shape)) == (torch.float32, (B, 7)) and tuple(res.info.shape) == (B, 6, 6)
    assert tuple(res.grad.shape) == (B, 6) and tuple(res.stats.shape) == (B, 4)
    assert (res.scratch.dtype, tuple(res.scratch.shape)) == (torch.int32, (WORDS,))
    assert all(t.dtype == torch.float32 for t in (res.info, res.grad, res.stats))
    want = dict(batch=B, H=H, W=W, az_res=AZ, vert_res=VRES, vert_off=VOFF, xyz1=x1.data_ptr(), xyz2=x2.data_ptr(), pose_in=pose.data_ptr(),
                beam_elev=None, iters=2, gate=f32(0.75), huber=f32(0.2), jump_rel=f32(0.05), min_count=7, damping=f32(1e-3),
                pose_out=res.pose.data_ptr(), info=res.info.data_ptr(), grad=res.grad.data_ptr(), stats=res.stats.data_ptr(),
                scratch=res.scratch.data_ptr())
    assert the_call(calls, "elo_pose_fit") == want
    # a sensor with a beam table: the table the launch reads lives as long as the result
    res = ops.pose_fit(x1, x2, pose, fit, sensor=S.Sensor(beam_elevations_deg=BEAMS_DEG))
    assert res.keep.dtype == torch.float32 and res.keep.tolist() == [f32(e * D2R) for e in BEAMS_DEG]
    got = the_call(calls, "elo_pose_fit")
    assert got["beam_elev"] == res.keep.data_ptr()
    assert (got["vert_res"], got["vert_off"]) == (f32((3.0 * D2R - -6.0 * D2R) / 3), f32(6.0 * D2R / ((3.0 * D2R - -6.0 * D2R) / 3)))
    assert (got["pose_out"], got["scratch"], got["xyz2"]) == (res.pose.data_ptr(), res.scratch.data_ptr(), x2.data_ptr())


def test_model_render(front):
    ops, S, calls = front
    src, pose = torch.zeros((B, K, H, W, 3)), torch.zeros((B, K, 7))
    xyz, idx = ops.model_render(src, pose)
    assert (xyz.dtype, tuple(xyz.shape), idx.dtype, tuple(idx.shape)) == (torch.float32, (B, H, W, 3), torch.int32, (B, H, W))
    got = the_call(calls, "elo_model_render")
    assert got.pop("scratch")                                 # (the call's own: not handed back)
    assert got == dict(batch=B, K=K, H=H, W=W, az_res=AZ, vert_res=VRES, vert_off=VOFF, src=src.data_ptr(), pose=pose.data_ptr(),
                       beam_elev=None, out_xyz=xyz.data_ptr(), out_src=idx.data_ptr())
    # an image of ONE row, where the row formula has no resolution: (vert_res, vert_off) = (1, 0)
    src1 = torch.zeros((B, K, 1, W, 3))
    xyz, idx = ops.model_render(src1, pose)
    got = the_call(calls, "elo_model_render")
    assert got.pop("scratch")
    assert got == dict(batch=B, K=K, H=1, W=W, az_res=AZ, vert_res=1.0, vert_off=0.0, src=src1.data_ptr(), pose=pose.data_ptr(),
                       beam_elev=None, out_xyz=xyz.data_ptr(), out_src=idx.data_ptr())
    table_rad = torch.tensor([e * D2R for e in BEAMS_DEG], dtype=torch.float64)
    ops.model_render(src, pose, beam_elev=table_rad)
    assert the_call(calls, "elo_model_render")["beam_elev"] not in (None, table_rad.data_ptr())    # (a float32 copy on the device)


def test_model_begin_and_advance(front):
    ops, _S, calls = front
    ring, state, scan = torch.zeros((K, H, W, 3)), torch.zeros(2, dtype=torch.int32), torch.zeros((H, W, 3))
    p64, p32, T = torch.zeros((K, 7), dtype=torch.float64), torch.zeros((K, 7)), torch.zeros((1, 7))
    assert ops.model_begin(ring, state, scan) is None
    assert the_call(calls, "elo_model_begin") == dict(K=K, H=H, W=W, ring=ring.data_ptr(), state=state.data_ptr(), first=scan.data_ptr())
    assert ops.model_advance(ring, p64, p32, state, scan, T) is None
    assert the_call(calls, "elo_model_advance") == dict(K=K, H=H, W=W, ring=ring.data_ptr(), poses64=p64.data_ptr(), poses32=p32.data_ptr(),
                                                        state=state.data_ptr(), scan=scan.data_ptr(), T=T.data_ptr())


def test_map_insert_and_extract(front):
    ops, S, calls = front
    spec = S.VoxelMap(0.5, 10)
    keys, acc, stats = table(spec)
    xyz, pose = torch.zeros((B, H, W, 3)), torch.zeros((B, 7), dtype=torch.float64)
    assert ops.map_insert(keys, acc, stats, xyz, pose, spec) is None
    assert the_call(calls, "elo_map_insert") == dict(batch=B, H=H, W=W, voxel=0.5, min_range=0.0, max_range=math.inf, log2_capacity=10,
                                                     xyz=xyz.data_ptr(), pose=pose.data_ptr(), keys=keys.data_ptr(), acc=acc.data_ptr(),
                                                     stats=stats.data_ptr())
    far = S.VoxelMap(0.25, 10, min_range=1.5, max_range=80.0)
    ops.map_insert(keys, acc, stats, xyz, pose, far)
    got = the_call(calls, "elo_map_insert")
    assert (got["voxel"], got["min_range"], got["max_range"]) == (0.25, 1.5, 80.0)
    for max_out in (5, np.int64(5), 0):
        key, count, out, n = ops.map_extract(keys, acc, spec, max_out)
        rows = int(max_out)
        assert (key.dtype, tuple(key.shape), count.dtype, tuple(count.shape)) == (torch.int64, (rows,), torch.int64, (rows,))
        assert (out.dtype, tuple(out.shape), n.dtype, tuple(n.shape)) == (torch.float32, (rows, 3), torch.int64, ())
        got = the_call(calls, "elo_map_extract")
        if rows:
            assert (got["out_key"], got["out_count"], got["out_xyz"]) == (key.data_ptr(), count.data_ptr(), out.data_ptr())
        else:                                                 # (room for one row all the same: the call still counts)
            assert got["out_key"] and got["out_count"] and got["out_xyz"]
        assert {k: got[k] for k in ("voxel", "log2_capacity", "max_out", "keys", "acc", "cursor")} == dict(
            voxel=0.5, log2_capacity=10, max_out=rows, keys=keys.data_ptr(), acc=acc.data_ptr(), cursor=n.data_ptr())


def test_map_merge(front):
    ops, S, calls = front
    spec = S.VoxelMap(0.5, 10)
    keys, acc, stats = table(spec)
    sk, sa = torch.full((16,), -1, dtype=torch.int64), torch.zeros((16, 4), dtype=torch.int64)
    report = ops.map_merge(keys, acc, stats, sk, sa, spec)
    assert (report.dtype, tuple(report.shape)) == (torch.int64, (8,)) and not report.any()
    assert the_call(calls, "elo_map_merge") == dict(rows=16, src_keys=sk.data_ptr(), src_acc=sa.data_ptr(), voxel=0.5, log2_capacity=10,
                                                    keys=keys.data_ptr(), acc=acc.data_ptr(), stats=stats.data_ptr(), centre=None,
                                                    radius=0.0, min_count=1, report=report.data_ptr())
    world = torch.zeros(7, dtype=torch.float64)
    report = ops.map_merge(keys, acc, stats, sk, sa, spec, world[4:], 40, min_count=np.int64(3))
    got = the_call(calls, "elo_map_merge")
    assert (got["centre"], got["radius"], got["min_count"], got["report"]) == (world.data_ptr() + 32, 40.0, 3, report.data_ptr())
    # no source rows: an empty tensor has no address, the report's stands in and nothing is read
    report = ops.map_merge(keys, acc, stats, sk[:0], sa[:0], spec)
    got = the_call(calls, "elo_map_merge")
    assert (got["rows"], got["src_keys"], got["src_acc"]) == (0, report.data_ptr(), report.data_ptr())


def test_map_fit(front):
    ops, S, calls = front
    spec = S.VoxelMap(0.5, 10)
    keys, acc, _stats = table(spec)
    xyz, pose = torch.zeros((B, H, W, 3)), torch.zeros((B, 7), dtype=torch.float64)
    fit = S.MapFit(iters=1, huber=0.2, jump_rel=0.05, min_count=7, damping=1e-3, min_points=2)
    for match in (False, True):
        res = ops.map_fit(keys, acc, xyz, pose, spec, fit, match=match)
        assert type(res) is ops.MapFitResult and res.keep is None
        assert (res.pose.dtype, tuple(res.pose.shape)) == (torch.float64, (B, 7)) and tuple(res.info.shape) == (B, 6, 6)
        assert tuple(res.grad.shape) == (B, 6) and tuple(res.stats.shape) == (B, 4)
        assert all(t.dtype == torch.float32 for t in (res.info, res.grad, res.stats))
        assert (res.scratch.dtype, tuple(res.scratch.shape)) == (torch.int32, (WORDS,))
        if match:
            assert (res.match.dtype, tuple(res.match.shape)) == (torch.int64, (B, H, W))
        else:
            assert res.match is None
        want = dict(batch=B, H=H, W=W, voxel=0.5, log2_capacity=10, keys=keys.data_ptr(), acc=acc.data_ptr(), xyz=xyz.data_ptr(),
                    pose_in=pose.data_ptr(), iters=1, gate=0.5, huber=f32(0.2), jump_rel=f32(0.05), min_count=7, damping=f32(1e-3),
                    min_points=2, pose_out=res.pose.data_ptr(), info=res.info.data_ptr(), grad=res.grad.data_ptr(),
                    stats=res.stats.data_ptr(), match=res.match.data_ptr() if match else None, scratch=res.scratch.data_ptr())
        assert the_call(calls, "elo_map_fit") == want
    ops.map_fit(keys, acc, xyz, pose, spec, S.MapFit(gate=0.25))
    assert the_call(calls, "elo_map_fit")["gate"] == 0.25
    # the rows WorldMap.add concatenates
    res.stats.copy_(torch.arange(4 * B, dtype=torch.float32).reshape(B, 4))              # (no launch wrote them: whatever was there, NaN too)
    both = ops.MapFitResult(torch.cat([res.pose, res.pose]), *(torch.cat([getattr(res, n)] * 2) for n in ("info", "grad", "stats")))
    assert both.scratch is None and both.match is None and both.keep is None and tuple(both.count.shape) == (2 * B,)
    assert all(torch.equal(getattr(both, n), both.stats[:, j]) for j, n in enumerate(("count", "cost", "rms", "status")))


def test_scan_descriptor(front):
    ops, S, calls = front
    spec = S.ScanContext(rings=4, sectors=8)
    xyz = torch.zeros((B, H, W, 3))
    edge2 = [0.0, 76.5625, 306.25, 689.0625, 1225.0] + [0.0] * 28                      # (35 j / 4)^2, then the unused rings
    for out in (None, torch.zeros((B, 8, 4), dtype=torch.uint16)):
        desc = ops.scan_descriptor(xyz, spec, out=out)
        assert (desc.dtype, tuple(desc.shape)) == (torch.uint16, (B, 8, 4)) and (out is None or desc is out)
        assert the_call(calls, "elo_scan_descriptor") == dict(batch=B, H=H, W=W, rings=4, sectors=8, z_min=-3.0, z_step=0.005,
                                                              min_range2=0.0, edge2=edge2, xyz=xyz.data_ptr(), desc=desc.data_ptr())
    near = S.ScanContext(4, 8, 20.0, 2.0, -1.5, 0.01)
    ops.scan_descriptor(xyz, near)
    got = the_call(calls, "elo_scan_descriptor")
    assert (got["z_min"], got["z_step"], got["min_range2"], got["edge2"][:5]) == (-1.5, 0.01, 4.0, [0.0, 25.0, 100.0, 225.0, 400.0])
    assert tuple(ops.scan_descriptor(xyz[:0], spec).shape) == (0, 8, 4) and not calls   # no image: nothing is launched


def test_descriptor_search(front):
    ops, S, calls = front
    spec = S.ScanContext(rings=4, sectors=8)
    query, db = torch.zeros((B, 8, 4), dtype=torch.uint16), torch.zeros((16, 8, 4), dtype=torch.uint16)
    m, k = 5, 2
    res = ops.descriptor_search(query, db, m, spec, k)
    assert type(res) is ops.PlaceSearchResult
    assert [(t.dtype, tuple(t.shape)) for t in (res.entry, res.shift, res.dist, res.best_shift, res.best_dist)] == [
        (torch.int32, (B, k)), (torch.int32, (B, k)), (torch.float64, (B, k)), (torch.int32, (B, m)), (torch.float64, (B, m))]
    assert the_call(calls, "elo_descriptor_search") == dict(
        n=B, m=m, rings=4, sectors=8, k=k, query=query.data_ptr(), db=db.data_ptr(), entry=res.entry.data_ptr(), shift=res.shift.data_ptr(),
        dist=res.dist.data_ptr(), best_shift=res.best_shift.data_ptr(), best_dist=res.best_dist.data_ptr())
    # nothing to search: the queries stand in for the database, and there is no profile to write
    res = ops.descriptor_search(query, db, 0, spec)
    assert tuple(res.entry.shape) == (B, 1) and tuple(res.best_dist.shape) == (B, 0)
    assert the_call(calls, "elo_descriptor_search") == dict(
        n=B, m=0, rings=4, sectors=8, k=1, query=query.data_ptr(), db=query.data_ptr(), entry=res.entry.data_ptr(),
        shift=res.shift.data_ptr(), dist=res.dist.data_ptr(), best_shift=None, best_dist=None)
    assert tuple(ops.descriptor_search(query[:0], db, m, spec, k).entry.shape) == (0, k) and not calls

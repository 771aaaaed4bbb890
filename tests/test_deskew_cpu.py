"""CPU: the de-skewing input stage where no GPU is needed -- `Sweep` as a value, the C ABI of elo_input_stage_deskew (declared in
include/elo.h, mirrored in _lib.py, additive to ABI 26), the refusals the host makes before it touches a device, and the float64
restatement the GPU tests lean on (tests/deskew_reference.py) agreeing with itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import deskew_reference as R
from conftest import ROOT, load_pkg


def test_sweep_validates_and_is_a_frozen_value():
    S = load_pkg("sensor")
    d = S.Sweep()
    assert (d.phase, d.phase_ref) == ("azimuth", 1.0) and load_pkg().Sweep is S.Sweep
    c = S.Sweep(3, 0.5)
    assert (c.phase, c.phase_ref) == (3, 0.5) and type(S.Sweep(np.int64(5)).phase) is int
    assert c == S.Sweep(phase=3, phase_ref=0.5) and hash(c) == hash(S.Sweep(3, 0.5)) and c != d and c != S.Sweep(3, 1.0) and c != S.Sweep(4, 0.5)
    assert len({d, S.Sweep("azimuth"), c, S.Sweep(3, 0.5), S.Sweep(3, 0)}) == 3
    for bad in (dict(phase="time"), dict(phase=2), dict(phase=0), dict(phase=-1), dict(phase=3.0), dict(phase=True), dict(phase=None),
                dict(phase_ref=float("nan")), dict(phase_ref=float("inf")), dict(phase=3, phase_ref=-float("inf"))):
        with pytest.raises(ValueError):
            S.Sweep(**bad)
    with pytest.raises(AttributeError):
        d.phase_ref = 0.0
    with pytest.raises(AttributeError):
        del d.phase
    assert S.Sweep(3, -0.25).phase_ref == -0.25                    # any finite instant, inside the sweep or not
    assert "azimuth" in repr(d) and "0.5" in repr(c)
    # Sensor is what it was
    assert S.Sensor.__slots__ == ("fov_up_deg", "fov_down_deg", "crop_xy", "beam_elevations_deg")


def test_input_stage_deskew_is_declared_and_mirrored():
    L = load_pkg("_lib")
    with open(os.path.join(ROOT, "include", "elo.h")) as f:
        header = f.read()
    assert re.search(r"int\s+elo_input_stage_deskew\s*\(\s*const\s+elo_input_stage_deskew_args\s*\*\s*a\s*,\s*elo_stream_t\s+stream\s*\)\s*;", header)
    body = re.search(r"typedef struct elo_input_stage_deskew_args \{(.*?)\} elo_input_stage_deskew_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:                                                  # "int batch, npoints" declares two fields
            declared += [re.sub(r"^.*[\s*]", "", name.strip()) for name in decl.split(",")]
    mirror = L.InputStageDeskewArgs
    mirrors = [v for v in vars(L).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__name__.startswith("elo_")]
    assert mirror in mirrors and mirror.__name__ == "elo_input_stage_deskew_args"       # tests/test_abi_layout_cpu.py checks its layout
    plain = [name for name, _ in L.InputStageArgs._fields_]
    want = plain + ["beam_elev", "motion", "motion2", "invert", "phase_mode", "phase_channel", "phase_ref"]
    assert [name for name, _ in mirror._fields_] == declared == want
    assert dict(mirror._fields_)["phase_ref"] is ctypes.c_float and dict(mirror._fields_)["motion2"] is ctypes.c_void_p
    assert ("elo_input_stage_deskew", ctypes.c_int, [ctypes.POINTER(mirror), ctypes.c_void_p]) in L.SYMBOLS
    assert L.ABI_VERSION == 26                                    # additive: no existing struct moved
    for name, value in (("ELO_PHASE_CHANNEL", L.PHASE_CHANNEL), ("ELO_PHASE_AZIMUTH", L.PHASE_AZIMUTH), ("ELO_DESKEW_MAX_BATCH", L.DESKEW_MAX_BATCH)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value
    # the staging of 2 * batch images x 7 floats stays inside a workgroup's 64 KB beside the beam kernel's midpoints
    assert 2 * L.DESKEW_MAX_BATCH * 7 * 4 + 4 * L.MAX_BEAMS <= 64 * 1024
    # the two structs it extends are what they were
    assert plain == ["batch", "npoints", "point_stride", "H", "W", "az_res", "vert_res", "vert_off", "crop_xy", "cloud", "T_trans",
                     "aug_frame", "points", "out_xyz", "scratch"]
    assert [name for name, _ in L.InputStageBeamsArgs._fields_][-1] == "beam_elev" and len(L.InputStageBeamsArgs._fields_) == 14


def test_the_host_refuses_before_it_needs_a_gpu():
    ops, S, L, evaluate = load_pkg("_ops"), load_pkg("sensor"), load_pkg("_lib"), load_pkg("evaluate")
    cloud = torch.zeros((2, 20, 4))                               # a CPU tensor: a valid call would end at "runs on an AMD GPU only"
    motion = torch.tensor([[1.0, 0, 0, 0, 0, 0, 0]] * 2)
    with pytest.raises(L.EloError, match="without a motion"):
        ops.input_stage(cloud, None, None, 8, 32, sweep=S.Sweep(3))
    with pytest.raises(L.EloError, match="without a sweep"):
        ops.input_stage(cloud, None, None, 8, 32, motion=motion)
    with pytest.raises(L.EloError, match="without a sweep"):
        ops.input_stage(cloud, None, None, 8, 32, motion2=motion)
    with pytest.raises(L.EloError, match="without a sweep"):
        ops.input_stage(cloud, None, None, 8, 32, motion_is_pose=True)
    with pytest.raises(L.EloError, match="channel 4, the cloud has 4"):
        ops.input_stage(cloud, None, None, 8, 32, sweep=S.Sweep(4), motion=motion)
    with pytest.raises(L.EloError, match="channel 3, the cloud has 3"):
        ops.input_stage(cloud[..., :3], None, None, 8, 32, sweep=S.Sweep(3), motion=motion)
    with pytest.raises(L.EloError, match="at most %d" % L.DESKEW_MAX_BATCH):
        ops.input_stage(torch.zeros((L.DESKEW_MAX_BATCH + 1, 2, 3)), None, None, 8, 32, sweep=S.Sweep(), motion=motion)
    with pytest.raises(TypeError):
        ops.input_stage(cloud, None, None, 8, 32, sweep="azimuth", motion=motion)
    with pytest.raises(L.EloError, match="AMD GPU only"):         # nothing left to refuse: it is the device that is missing
        ops.input_stage(cloud, None, None, 8, 32, sweep=S.Sweep(3), motion=motion)

    class Net:                                                    # predict_sequence looks at the net's sensor first, then refuses
        sensor, device = S.KITTI_HDL64, "cpu"
    with pytest.raises(NotImplementedError):
        evaluate.predict_sequence(Net(), "/nonexistent", "00", None, frames=[0, 1], lanes=2, sweep=S.Sweep())


def test_the_float64_restatement_agrees_with_itself():
    rng = np.random.default_rng(0)
    consts = load_pkg("_ops").projection_constants(8, 32)
    target = R.target_cloud(rng, 2, 500, 8, 32, consts)[0]
    s = rng.uniform(0, 1, len(target))
    row = R.motion_row(rng, q0_negative=True, scale=1.7)
    assert row[0] < 0
    for ref in (0.0, 0.5, 1.0):
        raw = R.skew(target, s, row, ref)
        assert np.abs(R.deskew(raw, s, row, ref) - target).max() < 1e-12 and np.abs(raw - target).max() > 0.3
    # phase 1 carried to phase 0 is the rigid transform itself
    q = row[:4].astype(np.float64) / np.linalg.norm(row[:4].astype(np.float64))
    Rm, tv = R.rotation(q), row[4:].astype(np.float64)
    ones = np.ones(len(target))
    assert np.abs(R.deskew(target, ones, row, 0.0) - (target @ Rm.T + tv)).max() < 1e-12
    back = R.inverse_row(row)
    assert np.abs(R.deskew(R.deskew(target, ones, row, 0.0), ones, back, 0.0) - target).max() < 1e-12
    assert np.abs(R.deskew(target, s, row, 0.5, invert=True) - R.deskew(target, s, back, 0.5)).max() < 1e-12
    # zero points are left alone; equal phases are a no-op
    padded = target.copy()
    padded[::7] = 0.0
    assert (R.deskew(padded, s, row, 0.0)[::7] == 0).all()
    assert np.array_equal(R.deskew(target, 0.25 * ones, row, 0.25), target)
    # the projection: the nearest of a cell wins, exact duplicates are summed, a zero point blanks its cell
    az_res, vres, voff = consts
    closest = target[np.argsort(np.linalg.norm(target, axis=-1))[:3]]           # winners of their cells, whichever those are
    pts = np.concatenate([target, closest, np.zeros((1, 3))])
    img, count = R.project(pts, 8, 32, az_res, R.formula_rows(8, vres, voff))
    assert count.max() == 2 and count.reshape(-1)[R.zero_cell(8, 32, az_res)] == 0 and (img[count == 0] == 0).all()
    for twice in img[count == 2]:
        assert min(np.abs(twice / 2 - p).max() for p in closest) < 1e-12
    nearest = np.linalg.norm(img[count == 1], axis=-1)
    assert 0 < len(nearest) <= 8 * 32 and nearest.min() >= 3.0 and np.isin(np.round((nearest - 3.0) / 0.0025, 6) % 1, (0.0, 1.0)).all()

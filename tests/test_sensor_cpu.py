"""CPU: the sensor as a value (efficientlo-net_amd/sensor.py) -- validation, the default sensor's projection constants being
today's three floats, the scene generators being unchanged by an explicit default sensor -- and the C ABI of
elo_input_stage_beams (declared in include/elo.h, mirrored in _lib.py)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg


def test_sensor_validates_and_is_a_frozen_value():
    S = load_pkg("sensor")
    d = S.Sensor()
    assert (d.fov_up_deg, d.fov_down_deg, d.crop_xy, d.beam_elevations_deg) == (2.0, -24.8, 35.0, None)
    assert S.KITTI_HDL64 == d and hash(S.KITTI_HDL64) == hash(d) and load_pkg().KITTI_HDL64 is S.KITTI_HDL64
    assert load_pkg().Sensor is S.Sensor
    for bad in (dict(fov_up_deg=-3.0, fov_down_deg=2.0), dict(fov_up_deg=1.0, fov_down_deg=1.0),      # fov_up > fov_down
                dict(crop_xy=0.0), dict(crop_xy=-5.0), dict(crop_xy=float("nan")),                   # crop_xy > 0
                dict(beam_elevations_deg=[1.0, float("nan"), -1.0]), dict(beam_elevations_deg=[1.0, float("inf"), -1.0]),   # finite
                dict(beam_elevations_deg=[-2.0, -1.0, 0.0]), dict(beam_elevations_deg=[2.0, 1.0, 1.0, 0.0])):  # strictly descending
        with pytest.raises(ValueError):
            S.Sensor(**bad)
    with pytest.raises(AttributeError):
        d.crop_xy = 40.0
    with pytest.raises(AttributeError):
        del d.crop_xy
    # a table without an explicit field of view spans it; an explicit one wins
    table = [1.5, -0.5, -2.5, -4.5, -9.5, -14, -19, -23.5]
    s = S.Sensor(beam_elevations_deg=table)
    assert (s.fov_up_deg, s.fov_down_deg) == (1.5, -23.5) and s.beam_elevations_deg == tuple(float(e) for e in table)
    e = S.Sensor(fov_up_deg=2, fov_down_deg=-24, beam_elevations_deg=table)
    assert (e.fov_up_deg, e.fov_down_deg) == (2.0, -24.0) and e != s
    assert len({s, S.Sensor(beam_elevations_deg=tuple(table)), e, d}) == 3          # hashable, equal by value
    assert s.beam_elevations_rad() == tuple(x * (math.pi / 180) for x in table) and d.beam_elevations_rad() is None
    with pytest.raises(TypeError):
        S.resolve("HDL-64")


@pytest.mark.parametrize("H,W", [(64, 1800), (16, 225), (128, 2048)])
def test_default_projection_constants_are_todays_floats(H, W):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    d2r = math.pi / 180                                           # model_util.py:189-200, the arithmetic the project has had
    az = (360.0 / W) * d2r
    down, up = -24.8 * d2r, 2.0 * d2r
    vres = (up - down) / (H - 1)
    today = (az, vres, -down / vres)
    assert ops.projection_constants(H, W) == ops.projection_constants(H, W, None) == ops.projection_constants(H, W, S.KITTI_HDL64) == today
    assert all(type(x) is float for x in ops.projection_constants(H, W, S.KITTI_HDL64))
    other = ops.projection_constants(H, W, S.Sensor(10.67, -30.67))
    assert other[0] == az and other[1] != vres and other[2] != today[2]
    # a beam table alone moves the field of view the uniform formula uses
    assert ops.projection_constants(H, W, S.Sensor(beam_elevations_deg=[3.0, -25.0])) == ops.projection_constants(H, W, S.Sensor(3.0, -25.0))


def test_input_stage_beams_is_declared_and_mirrored(tmp_path):
    L = load_pkg("_lib")
    with open(os.path.join(ROOT, "include", "elo.h")) as f:
        header = f.read()
    assert re.search(r"int\s+elo_input_stage_beams\s*\(\s*const\s+elo_input_stage_beams_args\s*\*\s*a\s*,\s*elo_stream_t\s+stream\s*\)\s*;", header)
    body = re.search(r"typedef struct elo_input_stage_beams_args \{(.*?)\} elo_input_stage_beams_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:                                                  # "int batch, npoints" declares two fields
            declared += [re.sub(r"^.*[\s*]", "", name.strip()) for name in decl.split(",")]
    mirror = L.InputStageBeamsArgs
    assert issubclass(mirror, ctypes.Structure) and mirror.__name__ == "elo_input_stage_beams_args"
    want = ["batch", "npoints", "point_stride", "H", "W", "az_res", "crop_xy", "cloud", "T_trans", "aug_frame", "points", "out_xyz",
            "scratch", "beam_elev"]
    assert [name for name, _ in mirror._fields_] == declared == want
    # the fields of elo_input_stage_args without vert_res / vert_off, plus the table
    assert want[:-1] == [name for name, _ in L.InputStageArgs._fields_ if name not in ("vert_res", "vert_off")]
    assert ("elo_input_stage_beams", ctypes.c_int, [ctypes.POINTER(mirror), ctypes.c_void_p]) in L.SYMBOLS
    assert L.ABI_VERSION == 26                                    # additive: no existing struct moved
    assert int(re.search(r"#define\s+ELO_MAX_BEAMS\s+(\d+)", header).group(1)) == L.MAX_BEAMS == 256
    # size and offsets from a C program compiled against the header (as tests/test_abi_layout_cpu.py does for every mirror)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "elo.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(elo_input_stage_beams_args));']
    lines += ['printf("%s %%zu\\n", offsetof(elo_input_stage_beams_args, %s));' % (n, n) for n in want]
    src, exe = tmp_path / "beams.c", tmp_path / "beams"
    src.write_text("\n".join(lines + ['return 0; }']))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert ctypes.sizeof(mirror) == int(got["size"])
    for name in want:
        assert getattr(mirror, name).offset == int(got[name]), name


def test_default_scenes_do_not_change_with_the_default_sensor():
    synth, S = load_pkg("synth"), load_pkg("sensor")
    for kw in (dict(H=64, W=225, seed=3), dict(H=16, W=113, seed=8, profile="kitti"), dict(H=8, W=57, seed=1, yaw=0.01, shift=(0.8, 0, 0))):
        assert np.array_equal(synth.range_image(**kw), synth.range_image(sensor=S.KITTI_HDL64, **kw))
    for kw in (dict(B=2, H=16, W=113, seed=5), dict(B=2, H=16, W=113, seed=5, profile="kitti")):
        for a, b in zip(synth.frame_pair(**kw), synth.frame_pair(sensor=S.KITTI_HDL64, **kw)):
            assert np.array_equal(a, b)
    # another sensor is another scene: its rows look along its beams, its crop bites where it says
    table = (1.5, -0.5, -2.5, -4.5, -9.5, -14.0, -19.0, -23.5)
    img = synth.range_image(H=8, W=57, seed=1, hole_rate=0.0, noise=0.0, sensor=S.Sensor(beam_elevations_deg=table))
    el = np.rad2deg(np.arcsin(img[..., 2] / np.linalg.norm(img, axis=-1)))
    assert np.allclose(el, np.asarray(table)[:, None], atol=1e-4)
    near = synth.range_image(H=8, W=57, seed=1, hole_rate=0.0, sensor=S.Sensor(crop_xy=10.0))
    assert np.hypot(near[..., 0], near[..., 1]).max() <= 10.0 < np.hypot(img[..., 0], img[..., 1]).max()
    with pytest.raises(ValueError):
        synth.range_image(H=16, W=57, sensor=S.Sensor(beam_elevations_deg=table))

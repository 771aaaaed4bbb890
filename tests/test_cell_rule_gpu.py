"""GPU: the three ways of giving a beam table -- through `sensor=`, as a host list, as the device tensor of beam_table() -- are ONE
call for _ops.input_stage (without and with a Sweep), _scan_ops.pose_fit (iters 0 and 2) and _scan_ops.model_render: bit-equal outputs.  A
device tensor is the memory the launch reads (no hidden copy), a malformed one is refused before anything is launched, and a host
table is refused inside an open capture, which then closes cleanly (tests/cell_rule_capture.py).  B = 2, N = 256 points, 8 x 32 images, K = 2 scans, a
non-uniform 8-beam table: every branch of _ops.cell_rule, in a few seconds."""
import os
import subprocess
import sys

import pytest
import torch

import deskew_reference as D
from cell_rule_capture import DEV, H, OPS, RAD8, build_calls, same as _same
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
OTHER8 = [e * D.D2R for e in (2.0, 0.5, -1.0, -4.0, -8.0, -13.0, -18.5, -24.0)]       # another valid table for the same rows


@pytest.fixture(scope="module")
def calls():
    return build_calls()


@pytest.mark.parametrize("op", OPS)
def test_three_ways_of_giving_the_table_are_one_call(calls, op):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    sensor = S.Sensor(beam_elevations_deg=D.TABLE8)
    table = ops.beam_table(sensor, H, DEV)
    want = calls[op](sensor=sensor)
    assert _same(calls[op](sensor=sensor, beam_elev=RAD8), want)                        # a host list (the sensor's field of view with it)
    assert _same(calls[op](sensor=sensor, beam_elev=table), want)                       # the device tensor its owner keeps
    assert all(torch.isfinite(x).all() for x in want if x.is_floating_point())
    if op.startswith("pose_fit"):
        assert (want[3][:, 0] >= 20).all()                                               # terms were found: the rows matched
    else:
        assert float(want[-1 if op.startswith("input") else 0].abs().max()) > 0
    assert not _same(calls[op](sensor=S.Sensor(sensor.fov_up_deg, sensor.fov_down_deg)), want)      # the formula is another rule


@pytest.mark.parametrize("op", OPS)
def test_a_device_table_is_the_memory_the_launch_reads(calls, op):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    sensor = S.Sensor(beam_elevations_deg=D.TABLE8)
    table = ops.beam_table(RAD8, H, DEV)
    first = [x.clone() for x in calls[op](sensor=sensor, beam_elev=table)]
    want = calls[op](sensor=sensor, beam_elev=OTHER8)
    table.copy_(ops.beam_table(OTHER8, H, DEV))                                         # in place: the same pointer, other rows
    again = calls[op](sensor=sensor, beam_elev=table)
    assert _same(again, want) and not _same(again, first)


def test_a_malformed_device_table_is_refused_before_any_launch(calls, monkeypatch):
    """The ops allocate their outputs themselves, so there is no buffer of theirs to pre-fill: the way to the library is watched
    instead -- a refusal that came after a launch (or after the library was asked anything) would show in `touched`."""
    ops, L, S = load_pkg("_ops"), load_pkg("_lib"), load_pkg("sensor")
    sensor = S.Sensor(beam_elevations_deg=D.TABLE8)
    good = ops.beam_table(RAD8, H, DEV)
    want = {op: [x.clone() for x in calls[op](beam_elev=good)] for op in OPS}
    touched = []
    with monkeypatch.context() as m:
        for name in ("call", "call2", "lib"):
            m.setattr(L, name, lambda *a, _name=name, **kw: touched.append(_name))
        strided = torch.zeros(2 * H, device=DEV)
        strided[::2] = good
        for bad in (good.double(), torch.cat([good, good[-1:] - 0.1]), good[:H - 1].contiguous(), strided[::2]):
            for op in OPS:
                for how in (dict(beam_elev=bad), dict(sensor=sensor, beam_elev=bad)):
                    with pytest.raises(L.EloError, match="a device beam table is a contiguous float32 tensor of H = 8 entries on the"):
                        calls[op](**how)
    assert touched == []
    for op in OPS:                                                                      # and the same calls, mended, run
        assert _same(calls[op](beam_elev=good), want[op])


def test_a_host_table_is_refused_inside_a_capture_which_then_closes():
    """tests/cell_rule_capture.py in a child process: its capture and warm-up take streams from the process-wide pool and bind
    hardware queues, which in this process would move the lanes of every later test of the suite."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cell_rule_capture.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "host tables in a capture: ok" in out.stdout

"""CPU: the one resolution of the cell rule (_ops.cell_rule for a call, _ops.bind_sensor for an owner) as far as it goes without a
GPU -- which table it takes, what it refuses, the constants it hands on -- and the values both trackers refuse alike."""
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg

TABLE8 = (1.5, -0.5, -2.5, -4.5, -9.5, -14.0, -19.0, -23.5)
RAD8 = [e * (math.pi / 180) for e in TABLE8]
H, W = 8, 32


def test_a_host_table_resolves_to_beam_tables_tensor():
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    want = ops.beam_table(RAD8, H, "cpu")
    for given in (RAD8, np.asarray(RAD8), torch.tensor(RAD8, dtype=torch.float64)):
        rule = ops.cell_rule(H, W, "cpu", beam_elev=given)
        assert rule.beam_elev.dtype == torch.float32 and rule.beam_elev.device.type == "cpu" and torch.equal(rule.beam_elev, want)
        assert rule.sensor is S.KITTI_HDL64 and tuple(rule[:3]) == S.projection_constants(H, W)
    sensor, table = ops.bind_sensor(None, "cpu", RAD8, H)
    assert sensor is S.KITTI_HDL64 and torch.equal(table, want)


def test_a_sensors_table_is_taken_where_none_is_given():
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    sensor = S.Sensor(beam_elevations_deg=TABLE8)
    want = ops.beam_table(sensor, H, "cpu")
    assert torch.equal(want, torch.tensor(RAD8, dtype=torch.float64).float())
    rule = ops.cell_rule(H, W, "cpu", sensor=sensor)
    assert torch.equal(rule.beam_elev, want) and rule.sensor is sensor
    assert (rule.az_res, rule.vert_res, rule.vert_off) == S.projection_constants(H, W, sensor)
    other = [e - 0.001 for e in RAD8]                                                   # an explicit table goes before the sensor's
    assert torch.equal(ops.cell_rule(H, W, "cpu", sensor=sensor, beam_elev=other).beam_elev, ops.beam_table(other, H, "cpu"))
    bound, table = ops.bind_sensor(sensor, torch.device("cpu"))                         # an owner: H is the table's length
    assert bound is sensor and torch.equal(table, want)


@pytest.mark.parametrize("sensor", (None, dict(fov_up_deg=10.67, fov_down_deg=-30.67, crop_xy=50.0)))
def test_no_table_anywhere_is_the_formula_alone(sensor):
    ops, S = load_pkg("_ops"), load_pkg("sensor")
    sensor = None if sensor is None else S.Sensor(**sensor)
    for h, w in ((H, W), (64, 1800), (3, 1)):
        rule = ops.cell_rule(h, w, "cpu", sensor=sensor)
        assert rule.beam_elev is None and rule.sensor is S.resolve(sensor)
        assert (rule.az_res, rule.vert_res, rule.vert_off) == S.projection_constants(h, w, sensor)
    assert ops.bind_sensor(sensor, "cpu") == (S.resolve(sensor), None)
    one = ops.cell_rule(1, W, "cpu", sensor=sensor, one_row=(1.0, 0.0))                 # (model_render's image of one row)
    assert tuple(one[:4]) == (S.projection_constants(2, W, sensor)[0], 1.0, 0.0, None)


def test_bad_tables_and_sensors_are_refused():
    ops, L, S = load_pkg("_ops"), load_pkg("_lib"), load_pkg("sensor")
    nan = list(RAD8)
    nan[3] = float("nan")
    equal = list(RAD8)
    equal[4] = equal[3]
    for bad in (RAD8[:7], RAD8 + [-0.5], [RAD8], RAD8[::-1], equal, nan):               # length, shape, order, ties, NaN
        with pytest.raises(L.EloError):
            ops.cell_rule(H, W, "cpu", beam_elev=bad)
        with pytest.raises(L.EloError):
            ops.bind_sensor(None, "cpu", bad, H)
    with pytest.raises(L.EloError):                                                     # 8 beams, 16 rows
        ops.cell_rule(16, W, "cpu", sensor=S.Sensor(beam_elevations_deg=TABLE8))
    with pytest.raises(L.EloError, match="at most 256 beams"):
        ops.cell_rule(300, W, "cpu", beam_elev=np.linspace(0.1, -0.4, 300), max_beams=L.MAX_BEAMS)
    assert ops.cell_rule(300, W, "cpu", beam_elev=np.linspace(0.1, -0.4, 300)).beam_elev.numel() == 300     # (left to the library)
    for call in (lambda: ops.cell_rule(H, W, "cpu", sensor="hdl64"), lambda: ops.bind_sensor("hdl64", "cpu")):
        with pytest.raises(TypeError):
            call()


@pytest.mark.parametrize("tracker", ("ModelTracker", "DeviceTracker"))
def test_both_trackers_refuse_the_same_values(tracker):
    """Up to where a GPU is needed: the values and the table, before any tensor of the tracker's state is made."""
    S, L = load_pkg("sensor"), load_pkg("_lib")
    make = getattr(load_pkg("local_model"), tracker)
    model, fit = S.LocalModel(resident=tracker == "DeviceTracker"), S.PoseFit(iters=1)
    for bad in (4, None, fit, dict(scans=4)):
        with pytest.raises(TypeError, match="LocalModel"):
            make(H, W, bad, fit, device="cpu")
    for bad in (1, None, model, dict(iters=1)):
        with pytest.raises(TypeError, match="PoseFit"):
            make(H, W, model, bad, device="cpu")
    with pytest.raises(TypeError, match="LocalModel"):                                  # the model is looked at first
        make(2, 0, None, None, sensor="hdl64", device="cpu")
    for h, w in ((2, W), (0, W), (H, 0), (H, -1)):
        with pytest.raises(ValueError, match="H >= 3 and W >= 1"):
            make(h, w, model, fit, device="cpu")
    with pytest.raises(TypeError, match="Sensor"):
        make(H, W, model, fit, sensor="hdl64", device="cpu")
    with pytest.raises(L.EloError, match="descending"):
        make(H, W, model, fit, beam_elev=RAD8[::-1], device="cpu")
    with pytest.raises(L.EloError, match="one elevation per image row"):
        make(16, W, model, fit, sensor=S.Sensor(beam_elevations_deg=TABLE8), device="cpu")

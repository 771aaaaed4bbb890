"""CPU: model.Lane, the holder of one captured forward -- its declared fields, the decision which recording a replay takes
(capture(check_every=N)), the pose ring's window on the host, and what a capture() that raises leaves behind.  Stub graphs and a
stub ring: neither a GPU nor the library is touched."""
import types

import pytest
import torch

from conftest import load_pkg

model = load_pkg("model")
Lane = model.Lane


def _recorded(check_every=0, fit=False):
    """A lane whose recordings are names: what take() / fit_result() hand out says which one was taken."""
    lane = Lane(graph="graph", out="out", check_every=check_every, fit="fit" if fit else None)
    if check_every:
        lane.graph_checked, lane.out_checked, lane.fit_checked = "graph_checked", "out_checked", "fit_checked" if fit else None
    return lane


def _ringed(slots=4):
    """A lane on a stub ring whose rows name their slot: row s is [[s]]."""
    return Lane(pose=types.SimpleNamespace(slots=slots, rows=torch.arange(slots, dtype=torch.float32).reshape(slots, 1, 1)))


def _slots(rows):
    return [int(v) for v in rows.reshape(-1)]


def test_a_fresh_lane_has_every_optional_field_off():
    lane = Lane()
    for name in ("stream", "order", "pair", "inputs", "pose", "graph", "out", "keep",
                 "cloud", "motion", "fit", "graph_checked", "out_checked", "fit_checked", "range_counter", "native"):
        assert getattr(lane, name) is None, name
    for name in ("check_every", "total", "replays", "base", "tainted"):
        value = getattr(lane, name)
        assert value == 0 and type(value) is int, name
    assert lane.last_checked is False and lane.motion_is_pose is False
    assert sorted(Lane.__slots__) == sorted(set(Lane.__slots__)) and not hasattr(lane, "__dict__")


def test_an_undeclared_field_is_an_error_not_new_state():
    lane = Lane()
    with pytest.raises(AttributeError):
        lane.totl = 1
    with pytest.raises(AttributeError):
        Lane(totl=1)
    assert not hasattr(Lane, "__getitem__") and not hasattr(Lane, "__contains__")      # a holder of attributes, not half a dict
    lane.stream = "another"                   # (tools/lane_queues.py moves a lane to a stream of its choice)
    assert lane.stream == "another"


@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("check_every", [0, 1, 2, 3])
def test_every_nth_replay_takes_the_checked_recording(check_every, fit):
    lane = _recorded(check_every, fit)
    assert lane.fit_result() == ("fit" if fit else None)          # before any replay: the plain recording's
    for total in range(1, 8):
        checked = bool(check_every) and total % check_every == 0
        assert lane.take() == (("graph_checked", "out_checked") if checked else ("graph", "out"))
        assert (lane.total, lane.replays) == (total, total)
        assert lane.last_checked is checked
        assert lane.fit_result() == (None if not fit else "fit_checked" if checked else "fit")


def test_a_checked_replay_of_a_lane_without_a_checked_fit_offers_the_plain_one():
    lane = _recorded(check_every=1)
    lane.fit = "fit"
    lane.take()
    assert lane.last_checked and lane.fit_result() == "fit"


def test_the_ring_window_follows_mark_and_wraps_oldest_first():
    lane = _ringed(4)
    lane.graph = lane.out = "plain"
    for _ in range(3):
        lane.take()
    assert _slots(lane.poses()) == [0, 1, 2] and _slots(lane.last_pose()) == [2]
    lane.mark()
    assert (lane.base, lane.replays, lane.total) == (3, 0, 3) and _slots(lane.poses()) == []
    for want in (3, 0, 1):
        lane.take()
        assert _slots(lane.last_pose()) == [want]
    assert _slots(lane.poses()) == [3, 0, 1]
    assert lane.poses().shape == (3, 1, 1)
    lane.take()
    assert _slots(lane.poses()) == [3, 0, 1, 2]                   # a full ring is still whole
    lane.reset()
    assert (lane.base, lane.replays) == (0, 0) and _slots(lane.poses()) == []
    lane.take()
    assert _slots(lane.poses()) == [0] and _slots(lane.last_pose()) == [0]


def test_more_replays_than_slots_without_a_mark_raise():
    lane = _ringed(4)
    lane.graph = lane.out = "plain"
    for _ in range(5):
        lane.take()
    with pytest.raises(RuntimeError, match=r"5 replays since reset_poses\(\) on a ring of 4 slots: rows were overwritten"):
        lane.poses()


def test_a_lane_without_a_ring_has_one_pose_block():
    block = torch.zeros((1, 7))
    lane = Lane(pose=block, graph="graph", out="out")
    lane.take()
    lane.take()
    assert lane.last_pose() is block


def test_the_net_delegates_its_window_methods_to_the_lane():
    net = model.PWCLONet.__new__(model.PWCLONet)                 # (no variables, no device: only the lane list)
    net._lanes = [Lane(), _ringed(4)]
    lane = net._lanes[1]
    lane.graph = lane.out = "plain"
    for _ in range(3):
        lane.take()
    assert _slots(net.lane_poses(1)) == [0, 1, 2] and _slots(net.lane_pose(1)) == [2]
    net.mark_poses(1)
    lane.take()
    assert _slots(net.lane_poses(1)) == [3] and net._lanes[0].base == 0
    with pytest.raises(RuntimeError, match="captured without a sweep: it has no motion buffer"):
        net.lane_motion(0)
    with pytest.raises(RuntimeError, match="captured without a pose fit"):
        net.lane_fit(0)


def test_a_capture_that_raises_leaves_no_captured_graph():
    net = model.PWCLONet.__new__(model.PWCLONet)
    net.device = torch.device("cpu")
    net._lanes = [Lane()]                                         # as if an earlier capture() had succeeded
    with pytest.raises(TypeError, match="fit is a PoseFit or None"):
        net.capture(1, 64, 900, fit="not a PoseFit")
    assert net._lanes == []
    for call in (net.replay, lambda: net.submit(0), lambda: net.lane_input(0)):
        with pytest.raises(RuntimeError, match=r"no captured graph: call capture\(\) first"):
            call()

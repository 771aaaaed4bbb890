"""Frame-to-model pose fit: every scan is fitted against the last few scans, rendered into ONE range image, instead of against the
last scan alone (sensor.LocalModel; elo_model_render + elo_pose_fit, include/elo.h).

A frame-2 cell gives the pair fit a term only where the cell and its four neighbours hold a point; on sparse scans most do not.
Several scans carried into one frame fill each other's holes: the model has the normals the single scan lacks.

    tracker = ModelTracker(H, W, LocalModel(scans=4), PoseFit(iters=2))
    for xyz1, xyz2, pose7 in pairs:            # consecutive pairs of one drive
        res = tracker.step(xyz1, xyz2, pose7)  # an _scan_ops.PoseFitResult; res.pose: frame 1 -> frame 2, fitted against the model

DIRECTION.  A pair is (frame 1, frame 2) = (scan n, scan n-1) -- kitti.load_pair hands over the current scan first, and the net's
pose carries frame 1 into frame 2, the running product of evaluate.pose_rows.  So pair n's frame 2 is the scan that was pair
n-1's frame 1: the tracker keeps its model in the frame of the newest scan it holds, which is the next pair's frame 2.  Where the
sequence jumps (the next pair's frame 2 is NOT the last frame 1), reset().

DeviceTracker is the same tracker with its state machine on the device (elo_model_begin / elo_model_advance): a step is a fixed launch
sequence without a host decision, recorded once into a hipGraph and replayed per scan.

    tracker = DeviceTracker(H, W, LocalModel(scans=4, resident=True), PoseFit(iters=2)).capture()
    for xyz1, xyz2, pose7 in pairs:
        res = tracker.step(xyz1, xyz2, pose7)  # three copies + one replay; res is overwritten by the next step
"""
import torch

from . import _ops, _scan_ops
from . import sensor as _sensor
from ._check import is_a
from .pose7 import rebase


class _Tracker:
    """What both trackers are built from: the values, checked before any tensor is made, and the cell rule -- the sensor and its
    beam table on the tracker's device (_ops.bind_sensor: uploaded once, owned here for every launch and graph that reads it)."""

    def __init__(self, H, W, model, fit, sensor=None, beam_elev=None, device="cuda:0"):
        self.model, self.fit = is_a("model", model, _sensor.LocalModel), is_a("fit", fit, _sensor.PoseFit)
        self.H, self.W = int(H), int(W)
        if self.H < 3 or self.W < 1:
            raise ValueError("a pose fit needs H >= 3 and W >= 1 (got %d x %d)" % (self.H, self.W))
        self.device = torch.device(device)
        self.sensor, self.beam_elev = _ops.bind_sensor(sensor, self.device, beam_elev, self.H)

    def _pair(self, xyz1, xyz2):
        want = (1, self.H, self.W, 3)
        if tuple(xyz1.shape) != want or tuple(xyz2.shape) != want:
            raise ValueError("xyz1 / xyz2 are %s range images (got %s, %s)" % (want, tuple(xyz1.shape), tuple(xyz2.shape)))


class ModelTracker(_Tracker):
    """ModelTracker(H, W, model, fit, sensor=None, beam_elev=None, device="cuda:0"): the local model of ONE drive.
    model: sensor.LocalModel; fit: sensor.PoseFit; sensor / beam_elev: the cell rule, as _scan_ops.pose_fit takes them (a sensor with a
    beam table is uploaded once, here).
    State, all on the device: `ring` (scans,H,W,3) float32, zeroed -- slot i % scans holds the i-th scan that entered since
    reset(), an unused slot is all empty cells and gives the render nothing --; `poses64` (scans,7) float64 [q | t], scan of the
    slot -> the model's frame (the frame of the newest scan held), with the float32 copy `poses32` (1,scans,7) the render reads.
    step() enqueues launches and device-side float64 torch operators only: the host never waits for the device."""

    def __init__(self, H, W, model, fit, sensor=None, beam_elev=None, device="cuda:0"):
        super().__init__(H, W, model, fit, sensor, beam_elev, device)
        K = model.scans
        self.ring = torch.zeros((K, self.H, self.W, 3), dtype=torch.float32, device=self.device)
        self._identity = torch.zeros((K, 7), dtype=torch.float64, device=self.device)
        self._identity[:, 0] = 1.0
        self.poses64 = self._identity.clone()
        self.poses32 = torch.empty((1, K, 7), dtype=torch.float32, device=self.device)
        self.entered = 0                        # scans put in since reset()

    def reset(self):
        """Forget every scan: the next step() starts a model from its frame 2."""
        self.ring.zero_()
        self.poses64.copy_(self._identity)
        self.entered = 0

    def _enter(self, xyz):
        """`xyz` (1,H,W,3) defines the model's frame from now on: it enters at the identity, over the oldest scan when all slots are taken."""
        slot = self.entered % self.model.scans
        self.ring[slot].copy_(xyz[0])
        self.poses64[slot].copy_(self._identity[0])
        self.entered += 1

    def render(self):
        """The model as it stands -> (xyz (1,H,W,3), src_idx (1,H,W)) of _scan_ops.model_render."""
        self.poses32.copy_(self.poses64.reshape(1, -1, 7))
        return _scan_ops.model_render(self.ring.unsqueeze(0), self.poses32, sensor=self.sensor, beam_elev=self.beam_elev)

    def step(self, xyz1, xyz2, pose7):
        """One pair: xyz1 / xyz2 (1,H,W,3) float32 range images on the tracker's device, pose7 (1,7) [q | t] from frame 1 to frame 2
        -> the _scan_ops.PoseFitResult of xyz1 against the MODEL at pose7.  Then the model moves into frame 1 by the pose the fit
        returned (a flagged image's is pose7, by the kernel's own guarantee) and xyz1 enters it."""
        self._pair(xyz1, xyz2)
        if self.entered == 0:
            self._enter(xyz2)
        model, _src = self.render()
        res = _scan_ops.pose_fit(xyz1, model, pose7, self.fit, sensor=self.sensor, beam_elev=self.beam_elev)
        self.poses64.copy_(rebase(self.poses64, res.pose[0]))
        self._enter(xyz1)
        return res


class DeviceTracker(_Tracker):
    """DeviceTracker(H, W, model, fit, sensor=None, beam_elev=None, device="cuda:0"): ModelTracker with the state machine on the
    device -- the same arguments, the same checks, the same model of the last `model.scans` scans.
    State, four device tensors: `ring` (scans,H,W,3) float32; `poses64` (scans,7) float64 [q | t], scan of the slot -> the model's
    frame; `poses32` (scans,7) float32, poses64 rounded once, kept current by the update launch (the render reads it as it stands);
    `state` int32[2] = {next: the slot the next scan enters, held: scans in the ring}.  After reset() the ring is zero, the poses are
    identities and state is {0, 0}.  Which slot a scan enters, whether the first frame 2 enters and the re-basing are decided by the
    launches from `state` when they run (include/elo.h, elo_model_begin / elo_model_advance): the host branches on nothing."""

    def __init__(self, H, W, model, fit, sensor=None, beam_elev=None, device="cuda:0"):
        super().__init__(H, W, model, fit, sensor, beam_elev, device)
        K = model.scans
        self.ring = torch.empty((K, self.H, self.W, 3), dtype=torch.float32, device=self.device)
        self.poses64 = torch.empty((K, 7), dtype=torch.float64, device=self.device)
        self.poses32 = torch.empty((K, 7), dtype=torch.float32, device=self.device)
        self.state = torch.empty((2,), dtype=torch.int32, device=self.device)
        self._graph = self._inputs = self._result = None
        self.reset()

    def launches(self):
        """Launches of one step: begin 1, render 3, fit 2 (iters + 1), advance 2."""
        return 6 + 2 * (self.fit.iters + 1)

    def reset(self):
        """Forget every scan: the next step starts a model from its frame 2.  Device-side fills on the current stream."""
        self.ring.zero_()
        for poses in (self.poses64, self.poses32):
            poses.zero_()
            poses[:, 0].fill_(1.0)
        self.state.zero_()

    def enqueue(self, xyz1, xyz2, pose7):
        """One pair, as ModelTracker.step takes it -- xyz1 / xyz2 (1,H,W,3) float32 on the tracker's device, pose7 (1,7) -- enqueued on
        the current stream: begin (frame 2 enters an empty model), render, the fit of xyz1 against the rendered image at pose7, advance
        (the model moves into frame 1 by the pose the fit returned, xyz1 enters).  6 + 2 (iters + 1) launches, no host branch on
        device state, no synchronisation -> the _scan_ops.PoseFitResult."""
        self._pair(xyz1, xyz2)
        _scan_ops.model_begin(self.ring, self.state, xyz2[0])
        model, _src = _scan_ops.model_render(self.ring.unsqueeze(0), self.poses32.unsqueeze(0), sensor=self.sensor, beam_elev=self.beam_elev)
        res = _scan_ops.pose_fit(xyz1, model, pose7, self.fit, sensor=self.sensor, beam_elev=self.beam_elev)
        _scan_ops.model_advance(self.ring, self.poses64, self.poses32, self.state, xyz1[0], res.pose)
        return res

    def capture(self, warmup=2):
        """Record one enqueue() into a hipGraph over static inputs (inputs()) and a static result: `warmup` eager steps on a side
        stream first (allocations, code objects), then reset() -- the state after capture() is the reset state, whatever it was
        before.  Returns self."""
        from .model import graph_capture
        dev = self.device
        self._graph = None
        inputs = (torch.zeros((1, self.H, self.W, 3), dtype=torch.float32, device=dev),
                  torch.zeros((1, self.H, self.W, 3), dtype=torch.float32, device=dev),
                  torch.zeros((1, 7), dtype=torch.float32, device=dev))
        inputs[2][:, 0].fill_(1.0)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.enqueue(*inputs)
            self.reset()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with graph_capture(graph):
            result = self.enqueue(*inputs)
        self._graph, self._inputs, self._result = graph, inputs, result
        return self

    def inputs(self):
        """The static (xyz1, xyz2, pose7) the recorded step reads: a producer on the device may write them in place."""
        if self._graph is None:
            raise RuntimeError("no recorded step: call capture() first")
        return self._inputs

    def step(self, xyz1, xyz2, pose7):
        """One pair.  Captured: three copies into the static inputs and ONE replay -> the static PoseFitResult, which the NEXT
        step() overwrites (copy what is to be kept; valid once the stream has been synchronised or waited on).  Not captured:
        enqueue()."""
        if self._graph is None:
            return self.enqueue(xyz1, xyz2, pose7)
        for dst, src in zip(self._inputs, (xyz1, xyz2, pose7)):
            dst.copy_(src, non_blocking=True)
        self._graph.replay()
        return self._result

    def held(self):
        """Scans in the ring, read from the device (synchronises): for tests and tools."""
        return int(self.state[1].item())

    def next_slot(self):
        """The slot the next scan enters, read from the device (synchronises): for tests and tools."""
        return int(self.state[0].item())

"""Place recognition: an index of scan descriptors next to the world poses they were taken at, searched on the device
(sensor.ScanContext; elo_scan_descriptor / elo_descriptor_search, include/elo.h).

    index = PlaceIndex(ScanContext())          # 60 sectors x 20 rings of integer height levels per scan
    index.add(xyz, pose64)                     # one entry per range image, at its world pose [q | t] float64
    match = index.query(xyz, k=4)              # the k nearest entries over every entry and every column shift
    match.entry, match.shift, match.dist       # (n,k): which keyframe, turned by how many sectors, how far (0 = the same place)
    match.pose                                 # (n,k,7): the guess of a fit -- the keyframe's world pose turned by match.yaw

A descriptor does not depend on the vehicle's heading up to a shift of its columns, and the search tries every shift: what comes
back is a PLACE and a HEADING, not a translation -- `pose` carries the keyframe's own position.  Nothing is thresholded: the
caller reads `dist`.  Everything is enqueued on the current stream; the count of entries is the host's.
"""
import math

import numpy as np
import torch

from . import _scan_ops
from ._check import integer, is_a
from ._check_torch import image_batch, pose_rows
from .pose7 import qmul
from .sensor import ScanContext


class PlaceMatch:
    """What PlaceIndex.query found for n scans: `entry` (n,k) int32, `shift` (n,k) int32, `dist` (n,k) float64 as
    _scan_ops.PlaceSearchResult's (padding: -1, -1, +inf), `yaw` (n,k) float64 -- the query's heading relative to the entry's about the
    scan's z axis, ScanContext.yaw_of(shift), 0 for padding -- and `pose` (n,k,7) float64 [q | t]: the entry's world pose composed
    with that rotation, the identity for padding.  `search`: the _scan_ops.PlaceSearchResult itself (the per-entry profile)."""
    __slots__ = ("entry", "shift", "dist", "yaw", "pose", "search")

    def __init__(self, entry, shift, dist, yaw, pose, search):
        self.entry, self.shift, self.dist, self.yaw, self.pose, self.search = entry, shift, dist, yaw, pose, search


class PlaceIndex:
    """PlaceIndex(spec, capacity=4096, device="cuda:0"): `desc` (capacity, sectors, rings) uint16, `pose64` (capacity,7) float64
    [q | t] scan -> world and `scan` (capacity,) int64 (the caller's number of the scan), all on the device; the count of entries
    is the host's (len())."""

    def __init__(self, spec, capacity=4096, device="cuda:0"):
        self.spec = is_a("spec", spec, ScanContext)
        self.capacity = integer("capacity", capacity, ValueError, 1, 2 ** 31 - 1)
        self.device = torch.device(device)
        self.desc = torch.zeros((self.capacity, spec.sectors, spec.rings), dtype=torch.uint16, device=self.device)
        self.pose64 = torch.zeros((self.capacity, 7), dtype=torch.float64, device=self.device)
        self.scan = torch.zeros((self.capacity,), dtype=torch.int64, device=self.device)
        self._count = 0

    def __len__(self):
        return self._count

    def reset(self):
        """Forget every entry (a host count: the buffers are overwritten as entries come)."""
        self._count = 0

    def add(self, xyz, pose64, scan=None):
        """Append one entry per image: xyz (n,H,W,3) float32 range images, pose64 (n,7) float64 [q | t] their world poses, scan the
        caller's numbers of the scans (n python integers or an int64 tensor; None: the entries' own indices).  One descriptor
        launch into the index's own rows, a device copy of the poses and device-side fills (or a device copy) of the numbers.
        With pose64 -- and scan, where it is a tensor -- ON THE DEVICE the host never waits; a HOST pose64 or scan tensor costs a
        host-to-device copy, which waits for the stream (python integers do not: they are written by fills).  Raises IndexError
        where the index has no room for all n; nothing is added then.  Returns the index of the first entry added."""
        n, first = image_batch("xyz", xyz), self._count
        pose64 = torch.as_tensor(pose64)
        pose_rows("pose64", pose64, (n, 7), "image", ValueError)
        if scan is None:
            scan = range(first, first + n)
        if isinstance(scan, torch.Tensor):
            if scan.dtype != torch.int64:
                raise ValueError("a scan tensor is int64 (got %s)" % (scan.dtype,))
            scan = scan.reshape(-1)
        else:
            scan = [integer("scan", v, ValueError) for v in scan]       # (one integer per image)
        if len(scan) != n:
            raise ValueError("scan is one number per image (got %d for %d images)" % (len(scan), n))
        if first + n > self.capacity:
            raise IndexError("the index is full: %d entries held, %d more asked for, capacity %d" % (first, n, self.capacity))
        if n == 0:
            return first
        _scan_ops.scan_descriptor(xyz, self.spec, out=self.desc[first:first + n])
        self.pose64[first:first + n].copy_(pose64.to(device=self.device, dtype=torch.float64))
        if isinstance(scan, torch.Tensor):
            self.scan[first:first + n].copy_(scan.to(self.device))
        elif scan == list(range(scan[0], scan[0] + n)):
            torch.arange(scan[0], scan[0] + n, dtype=torch.int64, device=self.device, out=self.scan[first:first + n])
        else:
            for j, v in enumerate(scan):
                self.scan[first + j].fill_(v)
        self._count = first + n
        return first

    def query(self, xyz, k=1, skip_recent=0):
        """The k nearest entries of every image xyz (n,H,W,3) float32 among the entries [0, max(0, len - skip_recent)) ->
        PlaceMatch.  A descriptor launch, the search's two, and device-side float64 operators for the poses; the host never waits."""
        m = max(0, self._count - integer("skip_recent", skip_recent, ValueError, 0))
        res = _scan_ops.descriptor_search(_scan_ops.scan_descriptor(xyz, self.spec), self.desc, m, self.spec, k)
        return self._match(res)

    def _match(self, res):
        S = self.spec.sectors
        found = res.entry >= 0
        shift = torch.where(2 * res.shift > S, res.shift - S, res.shift).to(torch.float64)
        yaw = torch.where(found & (res.shift > 0), -shift * (2.0 * math.pi / S), torch.zeros_like(shift))
        rows = self.pose64[res.entry.clamp(min=0).to(torch.int64)]                      # (n,k,7)
        q = rows[..., :4] / rows[..., :4].norm(dim=-1, keepdim=True)
        half = 0.5 * yaw
        turn = torch.stack([torch.cos(half), torch.zeros_like(half), torch.zeros_like(half), torch.sin(half)], -1)
        q = qmul(q, turn)                                                                # q_entry (x) q_z(yaw), elementwise over (n,k)
        q = q / q.norm(dim=-1, keepdim=True)
        pose = torch.cat([q, rows[..., 4:]], -1)
        # (formed by device operators: assigning a python scalar into a device tensor copies it from the host)
        identity = (torch.arange(7, device=pose.device) == 0).to(torch.float64)
        pose = torch.where(found.unsqueeze(-1), pose, identity)
        return PlaceMatch(res.entry, res.shift, res.dist, yaw, pose, res)

    NAMES = ("place_desc", "place_pose64", "place_scan")

    def state(self):
        """The entries as numpy arrays and python numbers (synchronises): `place_desc` (m, sectors, rings) uint16, `place_pose64`
        (m,7) float64, `place_scan` (m,) int64, and the ScanContext's six fields as `place_rings`, `place_sectors`,
        `place_max_range`, `place_min_range`, `place_z_min`, `place_z_step`."""
        m, s = self._count, self.spec
        return {"place_desc": self.desc[:m].cpu().numpy(), "place_pose64": self.pose64[:m].cpu().numpy(),
                "place_scan": self.scan[:m].cpu().numpy(), "place_rings": s.rings, "place_sectors": s.sectors,
                "place_max_range": s.max_range, "place_min_range": s.min_range, "place_z_min": s.z_min, "place_z_step": s.z_step}

    def save_state(self, path):
        """Write state() with numpy.savez: arrays and numbers only.  Returns the number of entries."""
        np.savez(path, **self.state())
        return self._count

    @classmethod
    def from_state(cls, state, capacity=None, device="cuda:0"):
        """The index of a state() mapping (a file is not trusted: arrays of the wrong shape or dtype, levels above 4095, poses
        that are not finite -> ValueError).  capacity: None is max(4096, the entries held)."""
        try:
            spec = ScanContext(int(state["place_rings"]), int(state["place_sectors"]), float(state["place_max_range"]),
                               float(state["place_min_range"]), float(state["place_z_min"]), float(state["place_z_step"]))
            desc, pose, scan = (np.asarray(state[name]) for name in cls.NAMES)
        except KeyError as e:
            raise ValueError("the state holds no %s" % (e,)) from None
        if desc.dtype != np.uint16 or desc.ndim != 3 or desc.shape[1:] != (spec.sectors, spec.rings):
            raise ValueError("place_desc is (m, %d, %d) uint16 (got %s %s)" % (spec.sectors, spec.rings, desc.shape, desc.dtype))
        m = desc.shape[0]
        if pose.dtype != np.float64 or pose.shape != (m, 7) or scan.dtype != np.int64 or scan.shape != (m,):
            raise ValueError("place_pose64 is (%d, 7) float64 and place_scan (%d,) int64 (got %s %s, %s %s)"
                             % (m, m, pose.shape, pose.dtype, scan.shape, scan.dtype))
        if m and int(desc.max()) > ScanContext.LEVELS:
            raise ValueError("place_desc holds a level above %d" % ScanContext.LEVELS)
        if not np.isfinite(pose).all():
            raise ValueError("place_pose64 holds a value that is not finite")
        capacity = max(4096, m) if capacity is None else capacity
        if m > capacity:
            raise ValueError("the state holds %d entries, the index %d" % (m, capacity))
        index = cls(spec, capacity, device)
        if m:
            index.desc[:m].copy_(torch.from_numpy(np.ascontiguousarray(desc)))
            index.pose64[:m].copy_(torch.from_numpy(np.ascontiguousarray(pose)))
            index.scan[:m].copy_(torch.from_numpy(np.ascontiguousarray(scan)))
        index._count = m
        return index

    @classmethod
    def load_state(cls, path, capacity=None, device="cuda:0"):
        """The index of a save_state() file."""
        with np.load(path, allow_pickle=False) as f:
            state = {name: f[name] for name in f.files}
        return cls.from_state(state, capacity, device)

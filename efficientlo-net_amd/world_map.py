"""The world map of a trajectory: every scan's range image carried by its world pose into a hash table of voxels on the device
(sensor.VoxelMap; elo_map_insert / elo_map_extract, include/elo.h) -- a point cloud of the place in the frame of the first scan.

    wmap = WorldMap(VoxelMap(voxel=0.2))
    for xyz1, pose7 in samples:                # xyz1 (1,H,W,3): the sample's frame 1; pose7 (1,7): frame 1 -> frame 2
        wmap.add(xyz1, pose7)                  # composes the pose onto the running world pose, inserts the scan there
    xyz, count, key = wmap.points()            # sorted by key: canonical
    wmap.save("04_map.bin")                    # x y z count float32 rows, readable as a KITTI scan

    wmap = WorldMap(VoxelMap(voxel=0.5), fit=MapFit(iters=2))      # TRACKING: every scan's composed pose is first fitted against
    wmap.add(xyz1, pose7)                      # the map as it stands (elo_map_fit), and the scan goes in at the fitted pose
    res = wmap.fit(xyz, pose64)                # the raw fit of scans against this map: localising in a map built earlier

DIRECTION.  A sample's pose carries frame 1 = scan n into frame 2 = scan n-1 (kitti.load_pair; local_model), so the running
product W_n = T_0 o T_1 o ... o T_n carries scan n into the frame sample 0's pose leads to: what evaluate.pose_rows forms, with Tr
the identity.  Scan n is inserted at W_n.

The voxel sums are integers: the map's content does not depend on the order the points arrive in, and two runs agree bit for bit.
Where keys sit in the table is NOT determined; points() sorts by key, and that is what makes its result canonical.
"""
import numpy as np
import torch

from . import _ops
from .local_model import _qmul
from .sensor import MapFit, VoxelMap


def compose(world64, pose7):
    """W o T: world64 (7) [q | t] (scan n-1 -> world) and pose7 (7) [q | t] (scan n -> scan n-1) -> (7) float64 (scan n -> world):
    q = q_W (x) q_T, renormalised (both are normalised where they are used); t = R(q_W) t_T + t_W.  A pure function in float64, on
    whatever device world64 lives (array-likes are taken to the CPU): no host synchronisation."""
    Wp = torch.as_tensor(world64)
    Wp = Wp.to(torch.float64).reshape(7)
    T = torch.as_tensor(pose7).to(device=Wp.device, dtype=torch.float64).reshape(7)
    qw = Wp[:4] / Wp[:4].norm()
    q = _qmul(qw, (T[:4] / T[:4].norm()).reshape(1, 4))[0]
    q = q / q.norm()
    # R(q) v = v + 2 w (u x v) + 2 u x (u x v), q = (w, u)
    v, u = T[4:], qw[1:]
    c = torch.linalg.cross(u, v)
    t = v + 2.0 * qw[0] * c + 2.0 * torch.linalg.cross(u, c) + Wp[4:]
    return torch.cat([q, t])


class WorldMap:
    """WorldMap(spec, device="cuda:0", fit=None): one voxel map and the running world pose of the drive that fills it.
    spec: sensor.VoxelMap.  State, all on the device: `keys` (C,) int64 -- the table's unsigned 64-bit words; an empty slot, all ones,
    reads -1 --, `acc` (C,4) int64 {count, sx, sy, sz}, `stat_words` (8,) int64, and `world64` (7) float64 [q | t], the pose of the
    last scan added -> world (the identity after reset()).  insert() and add() enqueue launches and device-side float64 operators
    only: the host never waits for the device.
    fit: a sensor.MapFit -- add() then holds the running pose to the map: each scan's composed pose is the guess of a fit against
    the map as it stands, the scan is inserted at the fitted pose and `world64` becomes that pose.  A flagged scan (the first one,
    against an empty map; a starved one) goes in at its guess.  `last_fit`: the _ops.MapFitResult rows of the last add()."""

    STATS = ("inserted", "filtered", "rejected", "dropped_full", "occupied")

    def __init__(self, spec, device="cuda:0", fit=None):
        if not isinstance(spec, VoxelMap):
            raise TypeError("spec is a VoxelMap (got %r)" % (type(spec).__name__,))
        if fit is not None:
            if not isinstance(fit, MapFit):
                raise TypeError("fit is a MapFit or None (got %r)" % (type(fit).__name__,))
            fit.gate_for(spec)                               # a gate beyond the voxel is refused here, not at the first scan
        self.spec, self.device, self.tracking = spec, torch.device(device), fit
        self.last_fit, self._rows, self._log = None, [], []
        C = spec.capacity
        self.keys = torch.empty((C,), dtype=torch.int64, device=self.device)
        self.acc = torch.empty((C, 4), dtype=torch.int64, device=self.device)
        self.stat_words = torch.empty((8,), dtype=torch.int64, device=self.device)
        self.world64 = torch.empty((7,), dtype=torch.float64, device=self.device)
        self.reset()

    def reset(self):
        """Forget every point and the world pose.  Device-side fills on the current stream."""
        self.keys.fill_(-1)
        self.acc.zero_()
        self.stat_words.zero_()
        self.world64.zero_()
        self.world64[0].fill_(1.0)
        self.last_fit, self._rows, self._log = None, [], []

    def insert(self, xyz, pose64):
        """The raw insert: range images xyz (n,H,W,3) float32 at the poses pose64 (n,7) float64 [q | t], scan -> world.  The running
        world pose is neither read nor moved."""
        _ops.map_insert(self.keys, self.acc, self.stat_words, xyz, pose64, self.spec)

    def fit(self, xyz, pose64, match=False, fit=None):
        """The raw fit against this map: range images xyz (n,H,W,3) float32 at the guesses pose64 (n,7) float64 [q | t], scan ->
        world -> the _ops.MapFitResult (pose: the fitted world poses, float64).  `fit`: a sensor.MapFit (None: the one this map
        was built with).  The map and the running world pose are only read."""
        fit = self.tracking if fit is None else fit
        if fit is None:
            raise ValueError("this map was built without a MapFit: pass fit=MapFit(...)")
        return _ops.map_fit(self.keys, self.acc, xyz, pose64, self.spec, fit, match=match)

    def trajectory(self):
        """(n,7) float64 on the device: the world pose every scan added since reset() was inserted at, in order."""
        if not self._rows:
            return torch.empty((0, 7), dtype=torch.float64, device=self.device)
        return torch.cat(self._rows)

    def fit_log(self):
        """(n,4) float32 on the device: [count, cost, rms, status] of the fit of every scan added since reset() (tracking maps)."""
        if not self._log:
            return torch.empty((0, 4), dtype=torch.float32, device=self.device)
        return torch.cat(self._log)

    def add(self, xyz, pose7):
        """n consecutive samples: xyz (n,H,W,3) float32 range images (each sample's frame 1) and pose7 (n,7) their relative poses
        [q | t], frame 1 -> frame 2, any float dtype.  The poses are composed in order onto `world64` and scan j is inserted at the
        world pose AFTER its own pose; one insert launch for all n.  With a MapFit the scans are taken one at a time: compose, fit
        against the map as it stands, insert at the fitted pose.  Everything is enqueued; the host never waits."""
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 4:
            raise ValueError("xyz is an (n,H,W,3) tensor of range images")
        pose7 = torch.as_tensor(pose7).to(device=self.device, dtype=torch.float64)
        n = xyz.shape[0]
        if tuple(pose7.shape) != (n, 7):
            raise ValueError("pose7 is one [q | t] row per image: (%d, 7) (got %s)" % (n, tuple(pose7.shape)))
        if n == 0:
            return
        rows, world = [], self.world64
        if self.tracking is None:
            for j in range(n):
                world = compose(world, pose7[j])
                rows.append(world)
            rows = torch.stack(rows).contiguous()
            self.insert(xyz, rows)
        else:
            fits = []
            for j in range(n):
                guess = compose(world, pose7[j]).reshape(1, 7).contiguous()
                res = self.fit(xyz[j:j + 1], guess)
                self.insert(xyz[j:j + 1], res.pose)
                world = res.pose[0]
                fits.append(res)
                rows.append(res.pose)
                self._log.append(res.stats)
            rows = torch.cat(rows)
            self.last_fit = fits[0] if n == 1 else _ops.MapFitResult(rows, *(torch.cat([getattr(f, name) for f in fits])
                                                                            for name in ("info", "grad", "stats")))
        self._rows.append(rows)
        self.world64.copy_(world)

    def stats(self):
        """{inserted, filtered, rejected, dropped_full, occupied} as python ints (synchronises)."""
        return dict(zip(self.STATS, (int(v) for v in self.stat_words[:5].cpu())))

    def points(self):
        """(xyz (m,3) float32 centroids, count (m) int64, key (m) int64), one row per occupied voxel, SORTED BY KEY (torch.sort, on the
        device): the table's own order is arbitrary, this one is canonical.  Synchronises (m is read)."""
        m = int(self.stat_words[4].item())                   # `occupied`: the rows to make room for
        key, count, xyz, n = _ops.map_extract(self.keys, self.acc, self.spec, m)
        if int(n.item()) != m:
            raise RuntimeError("the map holds %d voxels, its counter says %d: buffers nobody reset?" % (int(n.item()), m))
        key, order = torch.sort(key)
        return xyz[order], count[order], key

    def save(self, path):
        """Write the map as (m,4) float32 rows `x y z count`, sorted by key: the layout of a KITTI velodyne .bin, so whatever reads a
        scan (kitti.load_pair's reader: np.fromfile(..., float32).reshape(-1, 4)) reads it back.  Returns m."""
        xyz, count, _key = self.points()
        rows = torch.cat([xyz, count.to(torch.float32).unsqueeze(1)], 1).cpu().numpy().astype(np.float32)
        rows.tofile(path)
        return len(rows)

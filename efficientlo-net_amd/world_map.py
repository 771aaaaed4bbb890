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

    wmap = WorldMap(VoxelMap(voxel=0.5), fit=MapFit(iters=2), window=MapWindow(radius=80.0, every=10))     # a LOCAL map: after
    wmap.add(xyz1, pose7)                      # every 10th scan the table is rebuilt into a second one (elo_map_merge) and what
    wmap.window_stats()                        # lies beyond 80 m of that scan, per axis, stays behind
    wmap.rebuild(log2_capacity=24)             # GROWTH: the content moves into a larger table
    wmap.merge(other)                          # the UNION: integer sums, so exactly the map of both drives' points
    wmap.save_state("04_map_state.npz")        # keys and integer sums, the world pose, the totals: WorldMap.load_state(path)
                                               # continues the drive as if the process had never ended

    wmap = WorldMap(VoxelMap(voxel=0.5), fit=MapFit(iters=2), places=Places())      # PLACES: every 5th scan's descriptor is looked
    wmap.add(xyz1, pose7)                      # up among the earlier ones (elo_descriptor_search), then kept with its world pose
    wmap.revisits()                            # (r,5) [scan, entry, entry_scan, shift, dist]: the caller reads dist
    out = wmap.relocalise(xyz, k=4)            # a scan with NO pose guess: the k nearest places, each fitted against the map

DIRECTION.  A sample's pose carries frame 1 = scan n into frame 2 = scan n-1 (kitti.load_pair; local_model), so the running
product W_n = T_0 o T_1 o ... o T_n carries scan n into the frame sample 0's pose leads to: what evaluate.pose_rows forms, with Tr
the identity.  Scan n is inserted at W_n.

The voxel sums are integers: the map's content does not depend on the order the points arrive in, and two runs agree bit for bit.
Where keys sit in the table is NOT determined; points() sorts by key, and that is what makes its result canonical.
"""
import numpy as np
import torch

from . import _scan_ops
from ._check import is_a
from ._check_torch import image_batch, pose_rows
from .places import PlaceIndex
from .pose7 import compose
from .sensor import MapFit, MapWindow, Places, VoxelMap


class WorldMap:
    """WorldMap(spec, device="cuda:0", fit=None, window=None, places=None): one voxel map and the running world pose of the drive that fills it.
    spec: sensor.VoxelMap.  State, all on the device: `keys` (C,) int64 -- the table's unsigned 64-bit words; an empty slot, all ones,
    reads -1 --, `acc` (C,4) int64 {count, sx, sy, sz}, `stat_words` (8,) int64, and `world64` (7) float64 [q | t], the pose of the
    last scan added -> world (the identity after reset()).  insert() and add() enqueue launches and device-side float64 operators
    only: the host never waits for the device.
    fit: a sensor.MapFit -- add() then holds the running pose to the map: each scan's composed pose is the guess of a fit against
    the map as it stands, the scan is inserted at the fitted pose and `world64` becomes that pose.  A flagged scan (the first one,
    against an empty map; a starved one) goes in at its guess.  `last_fit`: the _scan_ops.MapFitResult rows of the last add().
    window: a sensor.MapWindow -- after every `every`-th scan added since reset() (a HOST count: no device value is read) the map
    is rebuilt about the translation of that scan's world pose: rebuild().  `keys`, `acc` -- and `spec`, where a rebuild changed
    the capacity -- are REBOUND by a rebuild: take them from the map after it, do not hold on to them.
    places: a sensor.Places -- the map keeps a places.PlaceIndex (`places`): every `every`-th scan added since reset() (a HOST
    count) is FIRST looked up in it, k = 1, the newest `skip_recent` entries left out, and THEN appended at the world pose it was
    inserted at.  The lookups are revisits(); nothing is thresholded.  The index only reads the scans: the map's content and the
    trajectory are those of the same drive without it."""

    STATS = ("inserted", "filtered", "rejected", "dropped_full", "occupied")

    def __init__(self, spec, device="cuda:0", fit=None, window=None, places=None):
        self.spec, self.device = is_a("spec", spec, VoxelMap), torch.device(device)
        if is_a("fit", fit, MapFit, or_none=True) is not None:
            fit.gate_for(spec)                               # a gate beyond the voxel is refused here, not at the first scan
        self.tracking, self.window = fit, is_a("window", window, MapWindow, or_none=True)
        self.place_spec = is_a("places", places, Places, or_none=True)
        self.places = PlaceIndex(places.context, places.capacity, self.device) if places is not None else None
        self._revisits = []
        self.last_fit, self._rows, self._log = None, [], []
        C = spec.capacity
        self.keys = torch.empty((C,), dtype=torch.int64, device=self.device)
        self.acc = torch.empty((C, 4), dtype=torch.int64, device=self.device)
        self.stat_words = torch.empty((8,), dtype=torch.int64, device=self.device)
        self.world64 = torch.empty((7,), dtype=torch.float64, device=self.device)
        self.window_words = torch.empty((8,), dtype=torch.int64, device=self.device)     # the reports of every rebuild, summed
        self._fresh_stats = torch.empty((8,), dtype=torch.int64, device=self.device)     # a rebuilt table's own stats
        self._spare = None                                   # the other (keys, acc) of this capacity: rebuilds alternate
        self.reset()

    def reset(self):
        """Forget every point and the world pose.  Device-side fills on the current stream."""
        self.keys.fill_(-1)
        self.acc.zero_()
        self.stat_words.zero_()
        self.world64.zero_()
        self.world64[0].fill_(1.0)
        self.window_words.zero_()
        self.last_fit, self._rows, self._log, self._revisits = None, [], [], []
        if self.places is not None:
            self.places.reset()
        self._scans = self._rebuilds = 0                     # scans added / rebuilds made since reset(): the host's counts

    def insert(self, xyz, pose64):
        """The raw insert: range images xyz (n,H,W,3) float32 at the poses pose64 (n,7) float64 [q | t], scan -> world.  The running
        world pose is neither read nor moved."""
        _scan_ops.map_insert(self.keys, self.acc, self.stat_words, xyz, pose64, self.spec)

    def fit(self, xyz, pose64, match=False, fit=None):
        """The raw fit against this map: range images xyz (n,H,W,3) float32 at the guesses pose64 (n,7) float64 [q | t], scan ->
        world -> the _scan_ops.MapFitResult (pose: the fitted world poses, float64).  `fit`: a sensor.MapFit (None: the one this map
        was built with).  The map and the running world pose are only read."""
        fit = self.tracking if fit is None else fit
        if fit is None:
            raise ValueError("this map was built without a MapFit: pass fit=MapFit(...)")
        return _scan_ops.map_fit(self.keys, self.acc, xyz, pose64, self.spec, fit, match=match)

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
        against the map as it stands, insert at the fitted pose.  Everything is enqueued; the host never waits.  With Places the
        scans due for a lookup are looked up and appended after that, by launches and device-side operators alone; where the index
        has no room for all of them IndexError is raised BEFORE anything is enqueued and the map is as it was."""
        n = image_batch("xyz", xyz)
        pose7 = torch.as_tensor(pose7).to(device=self.device, dtype=torch.float64)
        pose_rows("pose7", pose7, (n, 7), "image", ValueError)
        if n == 0:
            return
        visits = [j for j in range(n) if (self._scans + j + 1) % self.place_spec.every == 0] if self.places is not None else []
        if visits and len(self.places) + len(visits) > self.places.capacity:
            raise IndexError("the place index is full: %d entries held, %d of these scans are due, capacity %d; nothing was added"
                             % (len(self.places), len(visits), self.places.capacity))
        rows, world = [], self.world64
        every = self.window.every if self.window is not None else 0
        if self.tracking is None:
            for j in range(n):
                world = compose(world, pose7[j])
                rows.append(world)
            rows = torch.stack(rows).contiguous()
            # the one insert launch, split after every scan a rebuild is due at: the content is that of the scans taken one at a time
            cuts = [j + 1 for j in range(n) if every and (self._scans + j + 1) % every == 0]
            ends = cuts if cuts and cuts[-1] == n else cuts + [n]
            for a, b in zip([0] + ends, ends):
                self.insert(xyz[a:b], rows[a:b])
                if b in cuts:
                    self._rebuild_about(rows[b - 1, 4:])
        else:
            fits = []
            for j in range(n):
                guess = compose(world, pose7[j]).reshape(1, 7).contiguous()
                res = self.fit(xyz[j:j + 1], guess)
                self.insert(xyz[j:j + 1], res.pose)
                if every and (self._scans + j + 1) % every == 0:
                    self._rebuild_about(res.pose[0, 4:])
                world = res.pose[0]
                fits.append(res)
                rows.append(res.pose)
                self._log.append(res.stats)
            rows = torch.cat(rows)
            self.last_fit = fits[0] if n == 1 else _scan_ops.MapFitResult(rows, *(torch.cat([getattr(f, name) for f in fits])
                                                                            for name in ("info", "grad", "stats")))
        self._rows.append(rows)
        self.world64.copy_(world)
        for j in visits:
            self._visit(xyz[j:j + 1], rows[j:j + 1], self._scans + j)
        self._scans += n

    def _visit(self, xyz, pose64, scan):
        """Look scan number `scan` (xyz (1,H,W,3), inserted at pose64 (1,7)) up in the index, log the row, append the scan.  Every
        value stays a (1,) device tensor and the entry's scan number comes by a device-side gather (index_select): a 0-dim tensor
        used as an index would be read on the host."""
        match = self.places.query(xyz, k=1, skip_recent=self.place_spec.skip_recent)
        entry, shift, dist = match.entry[0], match.shift[0], match.dist[0]                  # (1,) each
        held = self.places.scan.index_select(0, entry.clamp(min=0).to(torch.int64))
        entry_scan = torch.where(entry >= 0, held, torch.full_like(held, -1))
        row = torch.cat([torch.full_like(dist, float(scan)), entry.to(torch.float64), entry_scan.to(torch.float64),
                         shift.to(torch.float64), dist])
        self._revisits.append(row.reshape(1, 5))
        self.places.add(xyz, pose64, scan=[scan])

    def revisits(self):
        """(r,5) float64 on the device: [scan, entry, entry_scan, shift, dist] of every lookup since reset() -- the number of the
        scan looked up (0-based, counted since reset()), the nearest entry of the index, the number of THAT entry's scan, its best
        column shift and its distance; -1, -1, -1, +inf where the index had nothing to search yet.  Nothing is thresholded: whether
        a row is a revisit is the caller's reading of `dist`."""
        if not self._revisits:
            return torch.empty((0, 5), dtype=torch.float64, device=self.device)
        return torch.cat(self._revisits)

    def relocalise(self, xyz, k=4, fit=None):
        """One scan xyz (1,H,W,3) float32 with NO pose guess: the k nearest places of the index (PlaceIndex.query), a fit against
        the map at each of their guesses -- the keyframe's world pose turned by the matched heading -- and the choice among them
        -> {"match": the places.PlaceMatch, "fits": the _scan_ops.MapFitResult of the k guesses (rows in rank order; padding rows are
        fitted at the identity and count as flagged), "best": a python int}.  best: the candidate that is not flagged (status 0)
        with the most terms, ties going to the better rank; -1 where every candidate is flagged.  SYNCHRONISES to choose (the k
        status words and counts are read).  `fit`: a sensor.MapFit (None: the one this map was built with).
        THE LIMIT.  A descriptor gives a place and a heading, not a translation: the guess stands at the keyframe's own position,
        and the fit's basin is its gate, at most one voxel.  A scan taken further from its keyframe than about a voxel comes back
        flagged or unmoved; it needs a coarser map first, which is not built here."""
        if self.places is None:
            raise ValueError("this map was built without Places: pass places=Places(...)")
        if image_batch("xyz", xyz) != 1:
            raise ValueError("xyz is one (1,H,W,3) range image (got %s)" % (tuple(xyz.shape),))
        match = self.places.query(xyz, k=k)
        kk = match.entry.shape[1]
        fits = self.fit(xyz.expand(kk, -1, -1, -1).contiguous(), match.pose[0].contiguous(), fit=fit)
        # the one read: per candidate [found, status, count]
        rows = torch.stack([(match.entry[0] >= 0).to(torch.float32), fits.stats[:, 3], fits.stats[:, 0]], 1).cpu().tolist()
        best, most = -1, -1.0
        for r, (found, status, count) in enumerate(rows):
            if found and status == 0.0 and count > most:
                best, most = r, count
        return {"match": match, "fits": fits, "best": best}

    def merge(self, other, centre=None, radius=None, min_count=1):
        """Add the voxels of `other` -- a WorldMap of the same voxel (ValueError otherwise; its capacity may differ), or a (key, acc)
        pair of int64 tensors: (m,) keys and (m,4) {count, sx, sy, sz} rows, those of state() for one -- into this map: the UNION.
        The sums are integers, so the result is exactly the map of both maps' points.  centre (3 float64 on the device, read when
        the launch runs), radius, min_count: the filter of _scan_ops.map_merge.  `inserted` grows by the points merged, `dropped_full` by
        those that found no slot, and a WorldMap's own `filtered`, `rejected` and `dropped_full` totals are added to this map's:
        the totals of both drives.  Returns the report, (8,) int64 on the device (_lib.MAP_REPORT); `other` is only read."""
        if isinstance(other, WorldMap):
            if other.spec.voxel != self.spec.voxel:
                raise ValueError("the maps' voxels differ (%r, %r): their keys do not mean the same places" % (self.spec.voxel, other.spec.voxel))
            key, acc = other.keys, other.acc
        else:
            try:
                key, acc = other
            except (TypeError, ValueError):
                raise TypeError("other is a WorldMap or a (key, acc) pair of int64 tensors (got %r)" % (type(other).__name__,)) from None
        report = _scan_ops.map_merge(self.keys, self.acc, self.stat_words, key, acc, self.spec, centre, radius, min_count)
        if isinstance(other, WorldMap):
            self.stat_words[1:4] += other.stat_words[1:4].to(self.device)
        return report

    def rebuild(self, log2_capacity=None, centre=None, radius=None, min_count=1):
        """The map moved into a FRESH table of the same or a new capacity (log2_capacity; `spec` is then replaced by the VoxelMap of
        that capacity), filled on the device, under the filter of _scan_ops.map_merge: GROWTH (a larger table, no filter) and EVICTION
        (a window about `centre`, a least count) are both this.  `keys` and `acc` are rebound; the two buffer sets of one capacity are
        kept and alternate, so a windowed drive allocates nothing after its first rebuild.  `inserted`, `filtered`, `rejected` and
        `dropped_full` stay the drive's running totals, `occupied` becomes the new table's; what the rebuild left behind is summed
        into window_stats().  Enqueued on the current stream; the host never waits.  Returns the report."""
        spec = self.spec
        if log2_capacity is not None and log2_capacity != spec.log2_capacity:
            spec = VoxelMap(spec.voxel, log2_capacity, spec.min_range, spec.max_range)
        if self._spare is not None and self._spare[0].shape[0] == spec.capacity:
            keys, acc = self._spare
        else:
            keys = torch.empty((spec.capacity,), dtype=torch.int64, device=self.device)
            acc = torch.empty((spec.capacity, 4), dtype=torch.int64, device=self.device)
        keys.fill_(-1)
        acc.zero_()
        self._fresh_stats.zero_()
        report = _scan_ops.map_merge(keys, acc, self._fresh_stats, self.keys, self.acc, spec, centre, radius, min_count)
        self.stat_words[4].copy_(self._fresh_stats[4])
        self.window_words += report
        self._spare = (self.keys, self.acc) if spec.capacity == self.spec.capacity else None
        self.keys, self.acc, self.spec = keys, acc, spec
        self._rebuilds += 1
        return report

    def _rebuild_about(self, centre):
        return self.rebuild(centre=centre, radius=self.window.radius, min_count=self.window.min_count)

    def stats(self):
        """{inserted, filtered, rejected, dropped_full, occupied} as python ints (synchronises).  The first four are running totals
        of the drive; `occupied` is the table's present occupancy (a rebuild may lower it)."""
        return dict(zip(self.STATS, (int(v) for v in self.stat_words[:5].cpu())))

    def window_stats(self):
        """{rebuilds, evicted_voxels, evicted_points, dropped_voxels, dropped_points} as python ints (synchronises): the rebuilds
        since reset() and what they left behind -- filtered by the window or the least count (evicted), or without a slot in the
        new table (dropped).  The counts in the table sum to inserted - evicted_points - dropped_points."""
        w = [int(v) for v in self.window_words.cpu()]
        return {"rebuilds": self._rebuilds, "evicted_voxels": w[1], "evicted_points": w[5], "dropped_voxels": w[3], "dropped_points": w[6]}

    def state(self):
        """Everything a later process needs to go on with this map, as numpy arrays and python numbers (synchronises): `key` (m,)
        int64 SORTED and `acc` (m,4) int64 {count, sx, sy, sz} -- the integers themselves, not centroids --, `world64` (7,), the five
        stats() by name, `voxel`, `min_range`, `max_range`, `log2_capacity`, and the window's counts: `scans`, `rebuilds`,
        `window_words` (8,)."""
        full = self.keys != -1
        key, order = torch.sort(self.keys[full])
        out = {"key": key.cpu().numpy(), "acc": self.acc[full][order].cpu().numpy(), "world64": self.world64.cpu().numpy()}
        out.update(self.stats())
        out.update(voxel=self.spec.voxel, min_range=self.spec.min_range, max_range=self.spec.max_range,
                   log2_capacity=self.spec.log2_capacity, scans=self._scans, rebuilds=self._rebuilds,
                   window_words=self.window_words.cpu().numpy())
        if self.places is not None:                          # (without Places the keys are exactly the ones above)
            out.update(self.places.state())
            out["place_revisits"] = self.revisits().cpu().numpy()
        return out

    def save_state(self, path):
        """Write state() with numpy.savez: arrays and numbers only, nothing a reader has to execute.  Returns the number of voxels.
        (`path` as numpy.savez takes it: a name without .npz gets it appended.)"""
        state = self.state()
        np.savez(path, **state)
        return len(state["key"])

    @classmethod
    def load_state(cls, path, device="cuda:0", log2_capacity=None, fit=None, window=None, places=None):
        """The map of a save_state() file, in a table of the saved capacity or of `log2_capacity`: the rows are merged in
        (elo_map_merge: a file is not trusted, malformed rows are refused -- ValueError), `world64`, the totals and the window's
        counts are restored, and further add() calls continue the drive as if the process had never ended.  Synchronises.
        places: a sensor.Places -- the index and the revisit log the file carries are restored too (ValueError where it carries
        none, where its descriptors are of another ScanContext, or where they are malformed: PlaceIndex.from_state)."""
        with np.load(path, allow_pickle=False) as f:
            state = {name: f[name] for name in f.files}
        log2 = int(state["log2_capacity"]) if log2_capacity is None else log2_capacity
        wm = cls(VoxelMap(float(state["voxel"]), log2, float(state["min_range"]), float(state["max_range"])), device, fit=fit, window=window)
        if is_a("places", places, Places, or_none=True) is not None:
            index = PlaceIndex.from_state(state, places.capacity, wm.device)     # (the one index this map gets: none was built above)
            if index.spec != places.context:
                raise ValueError("%s holds descriptors of %r, not of %r" % (path, index.spec, places.context))
            wm.place_spec, wm.places = places, index
            log = np.asarray(state.get("place_revisits", np.zeros((0, 5))))
            if log.dtype != np.float64 or log.ndim != 2 or log.shape[1] != 5:
                raise ValueError("place_revisits is (r, 5) float64 (got %s %s)" % (log.shape, log.dtype))
            wm._revisits = [torch.from_numpy(np.ascontiguousarray(log)).to(wm.device)] if len(log) else []
        key = torch.from_numpy(np.ascontiguousarray(state["key"], dtype=np.int64)).to(wm.device)
        acc = torch.from_numpy(np.ascontiguousarray(state["acc"], dtype=np.int64)).to(wm.device)
        report = _scan_ops.map_merge(wm.keys, wm.acc, wm._fresh_stats.zero_(), key, acc, wm.spec)
        words = [int(state[name]) for name in cls.STATS[:4]]
        wm.stat_words[:4].copy_(torch.tensor(words, dtype=torch.int64))
        wm.stat_words[4].copy_(wm._fresh_stats[4])
        wm.window_words.copy_(torch.from_numpy(np.ascontiguousarray(state["window_words"], dtype=np.int64)))
        wm.world64.copy_(torch.from_numpy(np.ascontiguousarray(state["world64"], dtype=np.float64)))
        wm._scans, wm._rebuilds = int(state["scans"]), int(state["rebuilds"])
        r = [int(v) for v in report.cpu()]
        if r[2]:
            raise ValueError("%s holds %d malformed rows (a key with its top bit set, a count of 0 or beyond 2^40, a sum beyond "
                             "65535 * count)" % (path, r[2]))
        wm.window_words[3] += r[3]                           # rows a smaller table had no slot for: not in it, and counted so
        wm.window_words[6] += r[6]
        return wm

    def points(self):
        """(xyz (m,3) float32 centroids, count (m) int64, key (m) int64), one row per occupied voxel, SORTED BY KEY (torch.sort, on the
        device): the table's own order is arbitrary, this one is canonical.  Synchronises (m is read)."""
        m = int(self.stat_words[4].item())                   # `occupied`: the rows to make room for
        key, count, xyz, n = _scan_ops.map_extract(self.keys, self.acc, self.spec, m)
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

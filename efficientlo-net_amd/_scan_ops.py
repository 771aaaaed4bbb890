"""The host side of the kernels that work on whole scans and maps, as opposed to the net's operators (_ops.py): the pose fit on a
pair's range images, the model render and the device tracker's state launches, the voxel map's insert / extract / merge / fit, the
scan descriptor and its search (include/elo.h).  Each front end refuses on the host what can be refused without a GPU or the
library (_check.py, _check_torch.py), fills the entry's argument block and enqueues it on the current stream: no host
synchronisation, capturable, and no CPU fallback -- CPU tensors raise."""
import ctypes

import numpy as np

import torch

from . import _check_torch as chk
from . import _lib as L
from . import sensor as _sensor
from ._check import integer, is_a, real
from ._ops import _ptr, cell_rule


def _scratch_words(entry, B, H, W):
    """The int32 words of scratch `entry` asks for at these sizes (its *_scratch_words query)."""
    words = getattr(L.lib(), entry + "_scratch_words")(B, H, W)
    if words < 0:
        raise L.EloError("%s refuses a (%d,%d,%d) batch of images" % (entry, B, H, W))
    return words


class PoseFitResult:
    """What elo_pose_fit wrote for a batch: pose (B,7) [q | t] -- the input pose, or the polished one --, info (B,6,6) = the
    normal matrix A at that pose (rotation first, then translation; left perturbation), grad (B,6) = b, and views of the (B,4)
    stats block: count (terms, an exact integer in float32), cost = sum w r^2, rms = sqrt(cost / sum w), status (0: fine; bits
    _lib.FIT_FEW / FIT_SINGULAR: a step was refused and the pose is the input's; FIT_FEW_FINAL: the reported evaluation has fewer
    than min_count terms).  The tensors are the launch's own outputs: valid once its stream has been synchronised or waited on."""
    __slots__ = ("pose", "info", "grad", "stats", "scratch", "keep")

    def __init__(self, pose, info, grad, stats, scratch=None, keep=None):
        self.pose, self.info, self.grad, self.stats, self.scratch = pose, info, grad, stats, scratch
        self.keep = keep                  # the beam table the launches read when they run: it lives as long as the result

    count = property(lambda self: self.stats[:, 0])
    cost = property(lambda self: self.stats[:, 1])
    rms = property(lambda self: self.stats[:, 2])
    status = property(lambda self: self.stats[:, 3])

    def covariance(self):
        """sigma^2 A^-1 with sigma^2 = cost / (count - 6), per image, (B,6,6) float64 on the host -- for reporting.  NaN rows
        where count <= 6 or A is singular."""
        A = self.info.detach().cpu().numpy().astype(np.float64)
        st = self.stats.detach().cpu().numpy().astype(np.float64)
        out = np.full(A.shape, np.nan)
        for b in range(A.shape[0]):
            if st[b, 0] > 6:
                try:
                    out[b] = st[b, 1] / (st[b, 0] - 6) * np.linalg.inv(A[b])
                except np.linalg.LinAlgError:
                    pass
        return out


class MapFitResult(PoseFitResult):
    """What elo_map_fit wrote for a batch: PoseFitResult's fields, with `pose` (B,7) FLOAT64 [q | t], scan -> world, `info` / `grad`
    for the perturbation about the sensor's position (rotation first, then translation), and `match` (B,H,W) int64 -- the key of
    the voxel each cell's term went to at `pose`, -1 where it gave none -- or None."""
    __slots__ = ("match",)

    def __init__(self, pose, info, grad, stats, scratch=None, match=None):
        PoseFitResult.__init__(self, pose, info, grad, stats, scratch)
        self.match = match


def _fit_result(cls, B, dev, pose_dtype, words, match=None, keep=None):
    """The outputs of a fit of B images as a `cls` (PoseFitResult, MapFitResult), allocated on `dev`.  words: the scratch the entry
    asked for; match: the (B,H,W) of the association to write too (MapFitResult's); keep: the table to keep alive (PoseFitResult's)."""
    outputs = (torch.empty((B, 7), dtype=pose_dtype, device=dev), torch.empty((B, 6, 6), dtype=torch.float32, device=dev),
               torch.empty((B, 6), dtype=torch.float32, device=dev), torch.empty((B, 4), dtype=torch.float32, device=dev),
               torch.empty((max(words, 1),), dtype=torch.int32, device=dev))
    if match is not None:
        return cls(*outputs, match=torch.empty(match, dtype=torch.int64, device=dev))
    return cls(*outputs) if keep is None else cls(*outputs, keep=keep)


def _check_pose_fit(xyz1, xyz2, pose7, fit):
    """What the host can refuse about a pose fit without a GPU or the library: the value, shapes, dtypes, layout, devices (the
    beam table: cell_rule) -> B, H, W."""
    is_a("fit", fit, _sensor.PoseFit)
    chk.tensors((("xyz1", xyz1, torch.float32), ("xyz2", xyz2, torch.float32), ("pose7", pose7, torch.float32)))
    B, H, W = chk.range_images("xyz1", xyz1, "BHW", min_h=3)   # (a normal needs three rows)
    if xyz2.shape != xyz1.shape:
        raise L.EloError("xyz2 holds range images of xyz1's shape %s (got %s)" % (tuple(xyz1.shape), tuple(xyz2.shape)))
    chk.pose_rows("pose7", pose7, (B, 7), "image")
    chk.one_device("xyz1, xyz2 and pose7", xyz1, xyz2, pose7)
    return B, H, W


def pose_fit(xyz1, xyz2, pose7, fit, sensor=None, beam_elev=None):
    """elo_pose_fit: the point-to-plane fit of the poses `pose7` (B,7) [q | t] (frame 1 -> frame 2) on the range images xyz1 / xyz2
    (B,H,W,3) -> PoseFitResult.  `fit`: a sensor.PoseFit.  `sensor` (None: the reference's HDL-64E) gives the field of view of the
    cell rule; a sensor with a beam table -- or an explicit `beam_elev`, as input_stage takes it -- matches by the beam-table rows
    the input stage of such a sensor wrote the images with.  Inputs are float32, contiguous and used in place: pose7 is read when
    the launches RUN (a graph that records this call fits what the row holds at every replay).  Bad shapes, dtypes or layouts
    are refused here, before anything is launched."""
    B, H, W = _check_pose_fit(xyz1, xyz2, pose7, fit)
    dev = xyz1.device
    rule = cell_rule(H, W, dev, sensor, beam_elev, "images'", L.MAX_BEAMS)
    L.require_gpu(xyz1, xyz2, pose7)
    res = _fit_result(PoseFitResult, B, dev, torch.float32, _scratch_words("elo_pose_fit", B, H, W), keep=rule.beam_elev)
    a = L.PoseFitArgs(B, H, W, rule.az_res, rule.vert_res, rule.vert_off, xyz1.data_ptr(), xyz2.data_ptr(), pose7.data_ptr(),
                      _ptr(rule.beam_elev), fit.iters, fit.gate, fit.huber, fit.jump_rel, fit.min_count, fit.damping, res.pose.data_ptr(),
                      res.info.data_ptr(), res.grad.data_ptr(), res.stats.data_ptr(), res.scratch.data_ptr())
    L.call("elo_pose_fit", a, xyz1)
    return res


def _check_scans(K):
    if K < 1 or K > L.MODEL_MAX_SCANS:
        raise L.EloError("a model holds 1 .. %d scans (K = %d)" % (L.MODEL_MAX_SCANS, K))


def _check_model_render(src, pose):
    """What the host can refuse about a model render without a GPU or the library: shapes, dtypes, layout, devices (the beam
    table: cell_rule) -> B, K, H, W."""
    chk.tensors((("src", src, torch.float32), ("pose", pose, torch.float32)))
    B, K, H, W = chk.range_images("src", src, "BKHW", below=("KHW", "BHW"))    # (K range images per batch element)
    _check_scans(K)
    chk.pose_rows("pose", pose, (B, K, 7), "source")
    chk.one_device("src and pose", src, pose)
    return B, K, H, W


def model_render(src, pose, sensor=None, beam_elev=None):
    """elo_model_render: the K range images src (B,K,H,W,3), each carried by its row of pose (B,K,7) [q | t] (source k -> the
    model's frame), rendered into one range image by nearest range -> (xyz (B,H,W,3) float32, src_idx (B,H,W) int32: (k*H + h)*W + w
    of the point each cell holds, -1 where it is empty).  `sensor` / `beam_elev`: the cell rule, as pose_fit takes them.  Inputs
    are float32, contiguous and used in place: both are read when the launches RUN (a graph that records this call renders what
    they hold at every replay).  Bad shapes, dtypes or layouts are refused here, before anything is launched."""
    B, K, H, W = _check_model_render(src, pose)
    dev = src.device
    rule = cell_rule(H, W, dev, sensor, beam_elev, "images'", L.MAX_BEAMS, one_row=(1.0, 0.0))
    L.require_gpu(src, pose)
    words = _scratch_words("elo_model_render", B, H, W)
    xyz = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    scratch = torch.empty((max(words, 2),), dtype=torch.int32, device=dev)
    a = L.ModelRenderArgs(B, K, H, W, rule.az_res, rule.vert_res, rule.vert_off, src.data_ptr(), pose.data_ptr(), _ptr(rule.beam_elev),
                          xyz.data_ptr(), idx.data_ptr(), scratch.data_ptr())
    L.call("elo_model_render", a, src)
    return xyz, idx


def _check_model_state(ring, state, image, name, poses64=None, poses32=None, pose=None):
    """What the host can refuse about a tracker-state launch without a GPU or the library: types, dtypes, layout, shapes, devices
    -> K, H, W."""
    given = [("ring", ring, torch.float32), ("state", state, torch.int32), (name, image, torch.float32)]
    if poses64 is not None or poses32 is not None or pose is not None:
        given += [("poses64", poses64, torch.float64), ("poses32", poses32, torch.float32), ("T", pose, torch.float32)]
    chk.tensors(given)
    K, H, W = chk.range_images("ring", ring, "KHW", min_h=3, below=("KHW",))   # (the K scans a model holds; a pose fit needs three rows)
    _check_scans(K)
    if state.shape != (2,):
        raise L.EloError("state is the two int32 words {next, held} (got %s)" % (tuple(state.shape),))
    if image.shape != (H, W, 3):
        raise L.EloError("%s is one (%d,%d,3) range image, as the ring's slots are (got %s)" % (name, H, W, tuple(image.shape)))
    if len(given) > 3:
        chk.pose_rows("poses64", poses64, (K, 7), "slot")
        chk.pose_rows("poses32", poses32, (K, 7), "slot")
        if pose.shape not in ((7,), (1, 7)):
            raise L.EloError("T is one [q0 q1 q2 q3 | t0 t1 t2] row (got %s)" % (tuple(pose.shape),))
    chk.one_device("the tracker's state and its images", *(t for _name, t, _dtype in given))
    return K, H, W


def model_begin(ring, state, first):
    """elo_model_begin: where the tracker state `state` (int32[2] = {next, held}) says the model is empty, the image `first` (H,W,3)
    -- the pair's frame 2 -- enters slot 0 of `ring` (K,H,W,3); otherwise nothing is written.  One launch that takes its decision
    from device memory when it RUNS: no host synchronisation, capturable.  Bad types, shapes or layouts are refused here, before
    anything is launched."""
    K, H, W = _check_model_state(ring, state, first, "first")
    L.require_gpu(ring, state, first)
    L.call("elo_model_begin", L.ModelBeginArgs(K, H, W, ring.data_ptr(), state.data_ptr(), first.data_ptr()), ring)


def model_advance(ring, poses64, poses32, state, scan, T):
    """elo_model_advance: the image `scan` (H,W,3) enters the slot of `ring` (K,H,W,3) the state names; every row of `poses64` (K,7)
    double is re-based by T^-1 (`T`: (7) or (1,7) float32 [q | t], the fit's pose of `scan` against the model), the entered row becomes
    the identity, `poses32` (K,7) becomes poses64 rounded to float32 and `state` moves on.  Two launches that take their decisions
    from device memory when they RUN: no host synchronisation, capturable.  Refusals as model_begin."""
    K, H, W = _check_model_state(ring, state, scan, "scan", poses64, poses32, T)
    L.require_gpu(ring, state, scan, poses64, poses32, T)
    a = L.ModelAdvanceArgs(K, H, W, ring.data_ptr(), poses64.data_ptr(), poses32.data_ptr(), state.data_ptr(), scan.data_ptr(),
                           T.data_ptr())
    L.call("elo_model_advance", a, ring)


def _check_map(keys, acc, spec, stats=None):
    """What the host can refuse about a world map's buffers without a GPU or the library: the value, dtypes, layout, shapes, devices.
    The table's words are unsigned 64-bit on the device; torch holds them as int64 (counts and sums stay far below 2^63, and an empty
    key, all ones, reads -1)."""
    is_a("spec", spec, _sensor.VoxelMap)
    given = [("keys", keys, torch.int64), ("acc", acc, torch.int64)] + ([("stats", stats, torch.int64)] if stats is not None else [])
    chk.tensors(given)
    C = spec.capacity
    if keys.shape != (C,) or acc.shape != (C, 4):
        raise L.EloError("a map of log2_capacity %d has keys (%d,) and acc (%d, 4) (got %s, %s)"
                         % (spec.log2_capacity, C, C, tuple(keys.shape), tuple(acc.shape)))
    if stats is not None and stats.shape != (8,):
        raise L.EloError("stats is eight 64-bit words (got %s)" % (tuple(stats.shape),))
    chk.one_device("a map's buffers", *(t for _name, t, _dtype in given))


def _check_scans_at(keys, xyz, pose64, min_h=1):
    """The range images xyz (B,H,W,3) float32 of at least min_h rows, each at its row of pose64 (B,7) float64, where the map's
    `keys` live -> B, H, W."""
    chk.tensors((("xyz", xyz, torch.float32), ("pose64", pose64, torch.float64)))
    B, H, W = chk.range_images("xyz", xyz, "BHW", min_h, below=("BHW",))        # (one range image per scan)
    chk.pose_rows("pose64", pose64, (B, 7), "scan")
    chk.one_device("the map, the images and the poses", keys, xyz, pose64)
    return B, H, W


def map_insert(keys, acc, stats, xyz, pose64, spec):
    """elo_map_insert: the range images xyz (B,H,W,3) float32, each carried by its row of pose64 (B,7) float64 [q | t] (scan ->
    world), summed into the voxel map (keys (C,), acc (C,4), stats (8,), all int64, C = spec.capacity; spec: sensor.VoxelMap).  One
    launch on the current stream, no host synchronisation, capturable; inputs are contiguous and used in place.  Bad types, shapes or
    layouts are refused here, before anything is launched."""
    _check_map(keys, acc, spec, stats)
    B, H, W = _check_scans_at(keys, xyz, pose64)
    L.require_gpu(keys, acc, stats, xyz, pose64)
    a = L.MapInsertArgs(B, H, W, spec.voxel, spec.min_range, spec.max_range, spec.log2_capacity, xyz.data_ptr(), pose64.data_ptr(),
                        keys.data_ptr(), acc.data_ptr(), stats.data_ptr())
    L.call("elo_map_insert", a, keys)


def map_extract(keys, acc, spec, max_out):
    """elo_map_extract: the occupied slots of the map as rows in ARBITRARY order -> (key (max_out,) int64, count (max_out,) int64, xyz
    (max_out,3) float32 centroids, n: a 0-dim int64 device tensor, the number of occupied slots -- it may exceed max_out; only the
    first min(n, max_out) rows are written).  Two launches on the current stream, no host synchronisation, capturable."""
    _check_map(keys, acc, spec)
    max_out = integer("max_out", max_out, L.EloError, 0)
    L.require_gpu(keys, acc)
    dev = keys.device
    rows = max(max_out, 1)                                    # (an empty tensor has no address: with max_out = 0 the call still counts)
    key = torch.empty((rows,), dtype=torch.int64, device=dev)
    count = torch.empty((rows,), dtype=torch.int64, device=dev)
    xyz = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    n = torch.empty((), dtype=torch.int64, device=dev)
    a = L.MapExtractArgs(spec.voxel, spec.log2_capacity, max_out, keys.data_ptr(), acc.data_ptr(), key.data_ptr(), count.data_ptr(),
                         xyz.data_ptr(), n.data_ptr())
    L.call("elo_map_extract", a, keys)
    return key[:max_out], count[:max_out], xyz[:max_out], n


def _ranges_meet(a, b):
    """Two tensors' memory ranges share a byte (an empty tensor shares none)."""
    na, nb = a.numel() * a.element_size(), b.numel() * b.element_size()
    return na > 0 and nb > 0 and a.data_ptr() < b.data_ptr() + nb and b.data_ptr() < a.data_ptr() + na


def _check_map_merge(keys, acc, stats, src_keys, src_acc, spec, centre, radius, min_count):
    """What the host can refuse about a merge without a GPU or the library -> (radius as a float, min_count as an int)."""
    _check_map(keys, acc, spec, stats)
    chk.tensors((("src_keys", src_keys, torch.int64), ("src_acc", src_acc, torch.int64)))
    if src_keys.dim() != 1 or src_acc.shape != (src_keys.shape[0], 4):
        raise L.EloError("source rows are src_keys (rows,) and src_acc (rows, 4) (got %s, %s)" % (tuple(src_keys.shape), tuple(src_acc.shape)))
    if src_keys.shape[0] >= 2 ** 31:
        raise L.EloError("the source is at most 2^31 - 1 rows (got %d)" % src_keys.shape[0])
    chk.one_device("the map and the source rows", keys, src_keys, src_acc)
    if any(_ranges_meet(s, d) for s in (src_keys, src_acc) for d in (keys, acc)):
        raise L.EloError("the source rows overlap the destination table: a table is not merged into itself")
    min_count = integer("min_count", min_count, L.EloError, 1, 2 ** 63 - 1)
    if centre is None:
        if radius is not None:
            raise L.EloError("a radius needs the centre it is about")
        return 0.0, min_count
    chk.tensors((("centre", centre, torch.float64),))
    if centre.numel() != 3:
        raise L.EloError("centre is 3 doubles x y z (got %s)" % (tuple(centre.shape),))
    chk.one_device("the map and the centre", keys, centre)
    return real("radius", radius, L.EloError, positive=True, takes="numbers"), min_count     # (with a centre, a radius: None is refused)


def map_merge(keys, acc, stats, src_keys, src_acc, spec, centre=None, radius=None, min_count=1):
    """elo_map_merge: the source rows src_keys (rows,), src_acc (rows,4) int64 -- another table's buffers, or the rows of a saved
    state; a key of -1 is an empty slot -- filtered and added into the voxel map (keys, acc, stats, spec as map_insert's) -> report,
    an (8,) int64 device tensor of L.MAP_REPORT.  centre: a contiguous float64 device tensor of 3 elements (a view such as
    world64[4:] qualifies), read when the launch RUNS, with radius (m): rows whose voxel centre lies outside the box are filtered;
    min_count: rows with fewer points are filtered.  One launch on the current stream, no host synchronisation, capturable.  Bad
    types, shapes, layouts, devices and overlap are refused here, before the library is touched."""
    radius, min_count = _check_map_merge(keys, acc, stats, src_keys, src_acc, spec, centre, radius, min_count)
    L.require_gpu(keys, acc, stats, src_keys, src_acc, centre)
    report = torch.zeros((8,), dtype=torch.int64, device=keys.device)
    rows = src_keys.shape[0]
    none = report.data_ptr()                                  # (an empty tensor has no address: rows = 0 reads nothing)
    a = L.MapMergeArgs(rows, src_keys.data_ptr() if rows else none, src_acc.data_ptr() if rows else none, spec.voxel,
                       spec.log2_capacity, keys.data_ptr(), acc.data_ptr(), stats.data_ptr(), _ptr(centre), radius, min_count,
                       report.data_ptr())
    L.call("elo_map_merge", a, keys)
    return report


def map_fit(keys, acc, xyz, pose64, spec, fit, match=False):
    """elo_map_fit: the range images xyz (B,H,W,3) float32, each at its row of pose64 (B,7) float64 [q | t] (scan -> world), fitted
    against the voxel map (keys (C,), acc (C,4) int64, spec: sensor.VoxelMap; only read) -> MapFitResult.  `fit`: a sensor.MapFit
    (gate None: the map's voxel).  match=True: the per-cell association is written too.  2 (iters + 1) launches on the current
    stream, no host synchronisation, capturable; inputs are contiguous and used in place, and pose64 is read when the launches RUN.
    Bad types, shapes or layouts are refused here, before anything is launched."""
    _check_map(keys, acc, spec)
    gate = is_a("fit", fit, _sensor.MapFit).gate_for(spec)
    B, H, W = _check_scans_at(keys, xyz, pose64, min_h=3)    # (a normal needs three rows)
    L.require_gpu(keys, acc, xyz, pose64)
    res = _fit_result(MapFitResult, B, xyz.device, torch.float64, _scratch_words("elo_map_fit", B, H, W), (B, H, W) if match else None)
    a = L.MapFitArgs(B, H, W, spec.voxel, spec.log2_capacity, keys.data_ptr(), acc.data_ptr(), xyz.data_ptr(), pose64.data_ptr(),
                     fit.iters, gate, fit.huber, fit.jump_rel, fit.min_count, fit.damping, fit.min_points, res.pose.data_ptr(),
                     res.info.data_ptr(), res.grad.data_ptr(), res.stats.data_ptr(), _ptr(res.match), res.scratch.data_ptr())
    L.call("elo_map_fit", a, keys)
    return res


def _check_context(spec):
    is_a("spec", spec, _sensor.ScanContext)


def _check_count(n):
    if n > 65535:
        raise L.EloError("a call takes at most 65535 scans (got n = %d)" % n)
    return n


def _check_descriptors(name, t, spec):
    chk.tensors(((name, t, torch.uint16),))
    if t.dim() != 3 or t.shape[1:] != (spec.sectors, spec.rings):
        raise L.EloError("%s is (rows, %d, %d): sectors by rings, sector-major (got %s)" % (name, spec.sectors, spec.rings, tuple(t.shape)))


def scan_descriptor(xyz, spec, out=None):
    """elo_scan_descriptor: the range images xyz (n,H,W,3) float32, W >= spec.sectors -> their descriptors (n, sectors, rings)
    uint16 (spec: sensor.ScanContext), written into `out` where one is given.  One launch on the current stream, no host
    synchronisation, capturable; inputs are contiguous and used in place.  Bad types, shapes, layouts or devices are refused here,
    before the library is touched."""
    _check_context(spec)
    chk.tensors((("xyz", xyz, torch.float32),))
    n, H, W = chk.range_images("xyz", xyz, "nHW", min_w=spec.sectors, below=("nHW",))      # (a sector needs a column)
    _check_count(n)
    if out is not None:
        _check_descriptors("out", out, spec)
        if out.shape[0] != n:
            raise L.EloError("out holds one descriptor per image: (%d, %d, %d) (got %s)" % (n, spec.sectors, spec.rings, tuple(out.shape)))
        chk.one_device("the images and the descriptors", xyz, out)
    L.require_gpu(xyz, out)
    if out is None:
        out = torch.empty((n, spec.sectors, spec.rings), dtype=torch.uint16, device=xyz.device)
    if n == 0:
        return out
    edge2 = (ctypes.c_double * (L.PLACE_MAX_RINGS + 1))(*spec.edge2())
    a = L.ScanDescriptorArgs(n, H, W, spec.rings, spec.sectors, spec.z_min, spec.z_step, spec.min_range * spec.min_range, edge2,
                             xyz.data_ptr(), out.data_ptr())
    L.call("elo_scan_descriptor", a, xyz)
    return out


class PlaceSearchResult:
    """What elo_descriptor_search wrote for n queries: `entry` (n,k) int32, `shift` (n,k) int32, `dist` (n,k) float64 -- the k
    nearest entries by (dist, entry), padded with -1, -1, +inf beyond the entries searched -- and the profile they are taken
    from, `best_shift` (n,m) int32 and `best_dist` (n,m) float64: every entry's best shift and its distance."""
    __slots__ = ("entry", "shift", "dist", "best_shift", "best_dist")

    def __init__(self, entry, shift, dist, best_shift, best_dist):
        self.entry, self.shift, self.dist, self.best_shift, self.best_dist = entry, shift, dist, best_shift, best_dist


def descriptor_search(query, db, m, spec, k=1):
    """elo_descriptor_search: the descriptors query (n, sectors, rings) against the entries [0, m) of db (cap, sectors, rings), both
    uint16 (spec: sensor.ScanContext), over every entry and every column shift -> PlaceSearchResult.  m: a python integer in 0 ..
    cap (the caller counts its entries on the host); k: 1 .. 8.  Two launches on the current stream (one where m == 0), no host
    synchronisation, capturable.  Bad types, shapes, layouts, devices, m or k are refused here, before the library is touched."""
    _check_context(spec)
    _check_descriptors("query", query, spec)
    _check_descriptors("db", db, spec)
    chk.one_device("the queries and the database", query, db)
    m = integer("m", m, L.EloError, 0, min(db.shape[0], 2 ** 31 - 1))         # (at most the rows db holds)
    k = integer("k", k, L.EloError, 1, L.PLACE_MAX_K)
    n = _check_count(query.shape[0])
    L.require_gpu(query, db)
    dev = query.device
    res = PlaceSearchResult(torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.int32, device=dev),
                            torch.empty((n, k), dtype=torch.float64, device=dev), torch.empty((n, m), dtype=torch.int32, device=dev),
                            torch.empty((n, m), dtype=torch.float64, device=dev))
    if n == 0:
        return res
    a = L.DescriptorSearchArgs(n, m, spec.rings, spec.sectors, k, query.data_ptr(), db.data_ptr() if m else query.data_ptr(),
                               res.entry.data_ptr(), res.shift.data_ptr(), res.dist.data_ptr(), res.best_shift.data_ptr() if m else None,
                               res.best_dist.data_ptr() if m else None)
    L.call("elo_descriptor_search", a, query)
    return res

"""The LiDAR's geometry as a value: vertical field of view, horizontal crop and -- optionally -- the calibrated elevation of
every beam.  `Sensor()` is the HDL-64E of the reference (model_util.py:189-200: -24.8 / +2.0 degrees, 35 m crop,
model_util.py:380); everything that projects takes `sensor=None` = that one.

The uniform row formula  row = H - int(beta / vert_res + vert_off)  at the sensor's field of view is the rule of every projection
(the level grids reuse the field of view with nLines = the level's H) except the raw-scan input stage of a
sensor WITH a beam table: there a point goes to the row of the beam nearest in elevation (elo_input_stage_beams, include/elo.h),
so every laser has its own row whatever the spacing of the blocks it is built from.

`Sweep` is the other half of a real spinning sensor: its scans are not one instant.  It says where the acquisition phase of a point
is found and which instant the input stage carries the points to, given the sensor's motion during the sweep
(elo_input_stage_deskew).  It is a value of its own: `Sensor` does not change.

`PoseFit` asks for the geometric fit of a relative pose on the pair's own range images (elo_pose_fit): residual, information
matrix and, with iters > 0, Gauss-Newton steps on them.  `LocalModel` asks for that fit against the last few scans rendered into
one range image (elo_model_render; local_model.ModelTracker) instead of against the pair's other scan.

`VoxelMap` asks for the map the poses are for: every scan carried by its world pose into a hash table of voxels on the device
(elo_map_insert; world_map.WorldMap).  `MapFit` asks for a scan's world pose to be fitted against that map before the scan goes
in (elo_map_fit; WorldMap(fit=)).  `MapWindow` asks for that map to follow the vehicle: what lies beyond a radius is dropped at a
rebuild every few scans (elo_map_merge; WorldMap(window=)).  `ScanContext` is the descriptor of a scan for place recognition and
`Places` asks the map to keep an index of them and to look every few scans up in it (elo_scan_descriptor / elo_descriptor_search;
places.PlaceIndex; WorldMap(places=)).
"""
import math

from ._check import integer, is_a, real


class _Frozen:
    """A value: its fields (the subclass's __slots__) are set once by _freeze and never again; equal where the class and every
    field are equal, hashable alike."""
    __slots__ = ()

    def _freeze(self, *values):
        for name, value in zip(self.__slots__, values):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("%s is immutable" % type(self).__name__)

    def __delattr__(self, name):
        raise AttributeError("%s is immutable" % type(self).__name__)

    def _key(self):
        return tuple(getattr(self, name) for name in self.__slots__)

    def __eq__(self, other):
        return type(other) is type(self) and self._key() == other._key()

    def __hash__(self):
        return hash((type(self).__name__, self._key()))


class Sensor(_Frozen):
    """Sensor(fov_up_deg=2.0, fov_down_deg=-24.8, crop_xy=35.0, beam_elevations_deg=None): frozen and hashable.
    beam_elevations_deg: the elevation of every beam in degrees, row 0 (the highest) first, strictly descending; with a table
    and no explicit field of view, fov_up / fov_down are its first / last entry."""
    __slots__ = ("fov_up_deg", "fov_down_deg", "crop_xy", "beam_elevations_deg")

    def __init__(self, fov_up_deg=None, fov_down_deg=None, crop_xy=35.0, beam_elevations_deg=None):
        table = None
        if beam_elevations_deg is not None:
            table = tuple(float(e) for e in beam_elevations_deg)
            if len(table) < 2:
                raise ValueError("a beam table has at least two beams")
            if not all(math.isfinite(e) for e in table):
                raise ValueError("beam elevations must be finite")
            if not all(a > b for a, b in zip(table, table[1:])):
                raise ValueError("beam elevations must be strictly descending (row 0 is the highest beam)")
        up = real("fov_up_deg", fov_up_deg, ValueError) if fov_up_deg is not None else (table[0] if table else 2.0)
        down = real("fov_down_deg", fov_down_deg, ValueError) if fov_down_deg is not None else (table[-1] if table else -24.8)
        if not up > down:
            raise ValueError("fov_up_deg must lie above fov_down_deg (got %r, %r)" % (up, down))
        crop = real("crop_xy", crop_xy, ValueError, finite=False, positive=True)
        self._freeze(up, down, crop, table)

    def __repr__(self):
        table = "" if self.beam_elevations_deg is None else ", beam_elevations_deg=<%d beams>" % len(self.beam_elevations_deg)
        return "Sensor(fov_up_deg=%r, fov_down_deg=%r, crop_xy=%r%s)" % (self.fov_up_deg, self.fov_down_deg, self.crop_xy, table)

    def beam_elevations_rad(self):
        """The table in radians (python doubles), or None."""
        if self.beam_elevations_deg is None:
            return None
        return tuple(e * (math.pi / 180) for e in self.beam_elevations_deg)

    def row_elevations_deg(self, H):
        """The elevation a generator gives row h of an H-row image: the table (which must have H beams), else H beams spread
        evenly from fov_up to fov_down."""
        if self.beam_elevations_deg is not None:
            if len(self.beam_elevations_deg) != H:
                raise ValueError("the sensor has %d beams, the image %d rows" % (len(self.beam_elevations_deg), H))
            return self.beam_elevations_deg
        return tuple(self.fov_up_deg - h * (self.fov_up_deg - self.fov_down_deg) / max(H - 1, 1) for h in range(H))


KITTI_HDL64 = Sensor()


class Sweep(_Frozen):
    """Sweep(phase="azimuth", phase_ref=1.0): how a scan that is NOT motion-compensated tells WHEN each of its points was
    acquired, and the instant the input stage carries them all to (elo_input_stage_deskew, include/elo.h).  Frozen and hashable.
    phase: "azimuth" -- the fraction of the turn, (pi - atan2(y, x)) / 2 pi, of a sensor that starts its sweep at azimuth pi --
    or an int >= 3: the channel of the cloud that holds the phase of every point (0 = start of the sweep, 1 = its end).
    phase_ref: the phase every point is carried to (finite; 1.0: the end of the sweep, where the scan's pose is usually stamped)."""
    __slots__ = ("phase", "phase_ref")

    def __init__(self, phase="azimuth", phase_ref=1.0):
        if isinstance(phase, str):
            if phase != "azimuth":
                raise ValueError("phase is \"azimuth\" or the channel of the cloud that holds it (got %r)" % (phase,))
        else:
            phase = integer("phase", phase, ValueError, 3)    # (channels 0 .. 2 of a cloud are x, y, z)
        ref = real("phase_ref", phase_ref, ValueError)
        self._freeze(phase, ref)

    def __repr__(self):
        return "Sweep(phase=%r, phase_ref=%r)" % (self.phase, self.phase_ref)


class PoseFit(_Frozen):
    """PoseFit(iters=0, gate=1.0, huber=0.1, jump_rel=0.1, min_count=50, damping=0.0): the point-to-plane fit of a pose on the two
    range images of its pair (elo_pose_fit, include/elo.h).  Frozen and hashable.
    iters: Gauss-Newton steps on the pose (0: only measure it); gate (m): a frame-1 point further than this from the point of the
    frame-2 cell it falls in gives no term; huber (m): residuals beyond it are weighted huber / |r|; jump_rel: a normal is taken
    only where the four neighbours' ranges lie within jump_rel * r of the cell's range r; min_count: an image with fewer terms is
    flagged and its pose left alone; damping: Levenberg factor on the diagonal of the normal matrix."""
    __slots__ = ("iters", "gate", "huber", "jump_rel", "min_count", "damping")

    def __init__(self, iters=0, gate=1.0, huber=0.1, jump_rel=0.1, min_count=50, damping=0.0):
        iters = integer("iters", iters, ValueError, 0, 64)
        min_count = integer("min_count", min_count, ValueError, 0, 2 ** 31 - 1)
        gate = real("gate", gate, ValueError, positive=True)
        huber = real("huber", huber, ValueError, positive=True)
        jump_rel = real("jump_rel", jump_rel, ValueError, non_negative=True)
        damping = real("damping", damping, ValueError, non_negative=True)
        self._freeze(iters, gate, huber, jump_rel, min_count, damping)

    def __repr__(self):
        return "PoseFit(iters=%r, gate=%r, huber=%r, jump_rel=%r, min_count=%r, damping=%r)" % self._key()


class LocalModel(_Frozen):
    """LocalModel(scans=4, resident=False): fit every scan against the last `scans` scans, rendered into one range image by nearest
    range (elo_model_render, include/elo.h), instead of against the last scan alone.  Frozen and hashable.
    scans: how many scans the model holds, an integer in 1 .. 16 (1: the pair fit, through the same path).
    resident: the tracker's state machine lives on the device (local_model.DeviceTracker: elo_model_begin / elo_model_advance) and a
    step is one hipGraph replay; False: local_model.ModelTracker, whose cursor is the host's."""
    __slots__ = ("scans", "resident")

    def __init__(self, scans=4, resident=False):
        scans = integer("scans", scans, ValueError, 1, 16)
        if not isinstance(resident, bool):
            raise ValueError("resident is True or False (got %r)" % (resident,))
        self._freeze(scans, resident)

    def __repr__(self):
        if self.resident:
            return "LocalModel(scans=%r, resident=True)" % (self.scans,)
        return "LocalModel(scans=%r)" % (self.scans,)


class VoxelMap(_Frozen):
    """VoxelMap(voxel=0.5, log2_capacity=22, min_range=0.0, max_range=inf): the world map of a trajectory -- every scan carried by
    its world pose into a hash table of voxels, each holding the count and the centroid of its points (elo_map_insert, include/elo.h;
    world_map.WorldMap).  Frozen and hashable.
    voxel (m): the edge of a voxel, finite and > 0; log2_capacity: the table has 1 << log2_capacity slots, an integer in 10 .. 28 (it
    does not grow by itself: points that find no slot are counted as dropped; WorldMap.rebuild moves a map into a larger one);
    min_range / max_range (m): a point whose range in its own scan lies outside [min_range, max_range] is left out, 0 <= min_range <
    max_range, max_range may be inf."""
    __slots__ = ("voxel", "log2_capacity", "min_range", "max_range")

    def __init__(self, voxel=0.5, log2_capacity=22, min_range=0.0, max_range=math.inf):
        log2_capacity = integer("log2_capacity", log2_capacity, ValueError, 10, 28)
        voxel = real("voxel", voxel, ValueError, positive=True)
        min_range = real("min_range", min_range, ValueError, non_negative=True)
        max_range = real("max_range", max_range, ValueError, finite=False)
        if not (max_range > min_range):
            raise ValueError("max_range must lie above min_range (got %r, %r)" % (max_range, min_range))
        self._freeze(voxel, log2_capacity, min_range, max_range)

    def __repr__(self):
        far = "inf" if math.isinf(self.max_range) else repr(self.max_range)
        return "VoxelMap(voxel=%r, log2_capacity=%r, min_range=%r, max_range=%s)" % (self.voxel, self.log2_capacity, self.min_range, far)

    @property
    def capacity(self):
        return 1 << self.log2_capacity


class MapFit(_Frozen):
    """MapFit(iters=0, gate=None, huber=0.1, jump_rel=0.1, min_count=50, damping=0.0, min_points=1): the point-to-plane fit of a
    scan's world pose against the voxel map (elo_map_fit, include/elo.h; world_map.WorldMap(fit=)).  Frozen and hashable.
    iters, huber, jump_rel, min_count, damping: as PoseFit's.  gate (m): a carried point further than this from the nearest voxel
    centroid gives no term; it may not exceed the map's voxel (the search looks at the 27 voxels about the point), and None means
    the map's voxel.  min_points: a voxel holding fewer points is no target, an integer >= 1."""
    __slots__ = ("iters", "gate", "huber", "jump_rel", "min_count", "damping", "min_points")

    def __init__(self, iters=0, gate=None, huber=0.1, jump_rel=0.1, min_count=50, damping=0.0, min_points=1):
        base = PoseFit(iters, 1.0 if gate is None else gate, huber, jump_rel, min_count, damping)
        min_points = integer("min_points", min_points, ValueError, 1, 2 ** 31 - 1)
        self._freeze(base.iters, None if gate is None else base.gate, base.huber, base.jump_rel, base.min_count, base.damping, min_points)

    def __repr__(self):
        return "MapFit(iters=%r, gate=%r, huber=%r, jump_rel=%r, min_count=%r, damping=%r, min_points=%r)" % self._key()

    def gate_for(self, spec):
        """The gate against the map `spec` (a VoxelMap): this value's, or the map's voxel; a gate beyond the voxel is an error."""
        gate = spec.voxel if self.gate is None else self.gate
        if gate > spec.voxel:
            raise ValueError("the gate (%r) may not exceed the map's voxel (%r)" % (gate, spec.voxel))
        return gate


class MapWindow(_Frozen):
    """MapWindow(radius, every=10, min_count=1): the world map as a LOCAL map that follows the vehicle -- after every `every`-th scan
    the table is rebuilt into a second one (elo_map_merge, include/elo.h; world_map.WorldMap(window=)) and only the voxels whose
    centre lies within `radius` of that scan's position on all three axes (a box), and that hold at least `min_count` points, are
    carried over.  Frozen and hashable.
    radius (m): finite and > 0; every: an integer >= 1; min_count: an integer >= 1."""
    __slots__ = ("radius", "every", "min_count")

    def __init__(self, radius, every=10, min_count=1):
        every = integer("every", every, ValueError, 1, 2 ** 63 - 1)
        min_count = integer("min_count", min_count, ValueError, 1, 2 ** 63 - 1)
        radius = real("radius", radius, ValueError, positive=True, takes="no_bool")
        self._freeze(radius, every, min_count)

    def __repr__(self):
        return "MapWindow(radius=%r, every=%r, min_count=%r)" % self._key()


class ScanContext(_Frozen):
    """ScanContext(rings=20, sectors=60, max_range=KITTI_HDL64.crop_xy, min_range=0.0, z_min=-3.0, z_step=0.005): the descriptor of
    a scan for place recognition -- `sectors` azimuth sectors by `rings` range rings, each bin holding the height of its highest
    point as an integer level 1 .. 4095 (0: no point) (elo_scan_descriptor, include/elo.h; places.PlaceIndex).  Frozen and hashable.
    rings: an integer in 1 .. 32; sectors: an integer in 1 .. 128; 0 <= min_range < max_range (m, in the xy plane), both finite;
    z_min (m): the height of level 1, finite; z_step (m): the height of a level, finite and > 0."""
    __slots__ = ("rings", "sectors", "max_range", "min_range", "z_min", "z_step")
    LEVELS = 4095

    def __init__(self, rings=20, sectors=60, max_range=KITTI_HDL64.crop_xy, min_range=0.0, z_min=-3.0, z_step=0.005):
        rings = integer("rings", rings, ValueError, 1, 32)
        sectors = integer("sectors", sectors, ValueError, 1, 128)
        max_range = real("max_range", max_range, ValueError, takes="no_bool")
        min_range = real("min_range", min_range, ValueError, non_negative=True, takes="no_bool")
        if not max_range > min_range:
            raise ValueError("max_range must lie above min_range (got %r, %r)" % (max_range, min_range))
        z_min = real("z_min", z_min, ValueError, takes="no_bool")
        z_step = real("z_step", z_step, ValueError, positive=True, takes="no_bool")
        self._freeze(rings, sectors, max_range, min_range, z_min, z_step)

    def __repr__(self):
        return "ScanContext(rings=%r, sectors=%r, max_range=%r, min_range=%r, z_min=%r, z_step=%r)" % self._key()

    def edge2(self):
        """The squared ring edges the kernel compares against, python doubles: edge2[j] = e_j * e_j, e_j = max_range * j / rings, for
        j = 0 .. rings (include/elo.h: formed on the host, in double)."""
        out = []
        for j in range(self.rings + 1):
            e = self.max_range * j / self.rings
            out.append(e * e)
        return tuple(out)

    def yaw_of(self, shift):
        """The rotation about the scan's z axis a column shift stands for, in radians in [-pi, pi): the query's heading relative to
        the entry's.  A shift is shift * 2 pi / sectors of a turn, and its SIGN is negative: the columns of a range image run
        against the azimuth (column w looks along pi - (w + 0.5) 2 pi / W), so a vehicle turned by +yaw sees the place in columns
        moved UP by yaw, and the search pairs its column j with the entry's column j + shift = j - yaw sectors / 2 pi."""
        shift = shift % self.sectors
        if 2 * shift > self.sectors:
            shift -= self.sectors
        return -shift * (2.0 * math.pi / self.sectors) if shift else 0.0


class Places(_Frozen):
    """Places(context=ScanContext(), every=5, skip_recent=50, capacity=4096): the world map keeps an index of scan descriptors next
    to their world poses and looks every `every`-th scan up in it before adding it (world_map.WorldMap(places=);
    places.PlaceIndex).  Frozen and hashable.
    context: a ScanContext; every: an integer >= 1; skip_recent: the newest entries a lookup leaves out (the scans just driven
    through are no revisit), an integer >= 0; capacity: the entries the index holds, an integer >= 1."""
    __slots__ = ("context", "every", "skip_recent", "capacity")

    def __init__(self, context=None, every=5, skip_recent=50, capacity=4096):
        context = ScanContext() if context is None else is_a("context", context, ScanContext, ValueError)
        every = integer("every", every, ValueError, 1, 2 ** 31 - 1)
        skip_recent = integer("skip_recent", skip_recent, ValueError, 0, 2 ** 31 - 1)
        capacity = integer("capacity", capacity, ValueError, 1, 2 ** 31 - 1)
        self._freeze(context, every, skip_recent, capacity)

    def __repr__(self):
        return "Places(context=%r, every=%r, skip_recent=%r, capacity=%r)" % self._key()


def resolve(sensor):
    """sensor=None is the reference's sensor."""
    return KITTI_HDL64 if sensor is None else is_a("sensor", sensor, Sensor)


def projection_constants(H_input, W_input, sensor=None):
    """model_util.py:189-200 at the sensor's field of view: python doubles (cast to float32 by the ctypes struct).  The
    arithmetic and its order are the reference's, so the default sensor gives the reference's three floats exactly."""
    s = resolve(sensor)
    d2r = math.pi / 180
    az = (360.0 / W_input) * d2r
    down, up = s.fov_down_deg * d2r, s.fov_up_deg * d2r
    vres = (up - down) / (H_input - 1)
    return az, vres, -down / vres

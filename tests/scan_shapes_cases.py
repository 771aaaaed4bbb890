"""TEST INFRASTRUCTURE of the scan-shape tests: the cases of tests/test_scan_shapes_gpu.py for the kernels that work on whole scans --
the solve launch of the two point-to-plane fits (fit_solve_kernel, csrc/elo_fit_device.h), elo_pose_fit on images that are no multiple
of its 512-cell tile, and the beam-table row rule (RowsByBeams, csrc/elo_project_device.h) at every length class of its padded table.
tests/test_scan_shapes_cpu.py vets every case with the float64 statements alone.  No GPU is touched here.

Part A, the solve step.  A call with iters = 0 reports info = fl32(A), grad = fl32(b) and count at the start pose; the first solve of
an iters = 1 call at the same pose works on the very same double sums (the evaluation is deterministic).  The step is restated in
float64 from the reported sums (pose_fit_reference.step / map_fit_reference.step) and compared with pose_out.  The tolerance is the
first-order perturbation bound of M d = -b, M = A + damping diag(A), under a relative change u = 2^-24 of every entry of A and b:

    dd = ||M^-1||_2 (u ||b|| + (1 + damping) u ||A||_F ||d||)                                      >= ||delta d||

    quaternion components     dd + u                    (half the rotation error, and the float32 rounding of a component <= 1)
    translation, pose fit     dd (1 + |t|) + 2u max(1, |t|)     t <- R(dq) t + v: the rotation error has the lever |t|; the float32 row
    translation, map fit      dd                        t <- t + v turns nothing, so no lever arises, and the row is double

(the map fit's bound is the pose fit's without the lever term: the sensor sits hundreds of metres from the world's origin, and
dd (1 + |t|) there would let a step with the damping of 1e-3 dropped pass).  |t| is the translation the step starts from."""
import functools
import math

import numpy as np

import deskew_reference as D
import local_model_reference as LM
import map_fit_reference as F
import pose_fit_reference as R

U = 2.0 ** -24
PERTURB = np.array((0.01, -0.008, 0.035, 0.3, 0.05, 0.02))        # about 2 degrees and 0.3 m
DAMPINGS = (0.0, 1e-3, 1.0)
OUTSIDE = 5.0                                                    # a wrong step lands at least this many tolerances away


def table_deg(H):
    """H unevenly spread beams, +2 .. -24.8 degrees (pose_fit_reference.BEAMS_DEG's shape at any length)."""
    return tuple(float(v) for v in 2.0 - 26.8 * (np.arange(H) / (H - 1.0)) ** 1.3)


# ---- A. the solve step -------------------------------------------------------------------------------------------------------------
def solve(A, b, damping, how="diag"):
    """d of M d = -b.  how: "diag" M = A + damping diag(A) (the rule); "eye" M = A + damping I; "none" M = A."""
    A = np.asarray(A, np.float64)
    M = A + {"diag": damping * np.diag(np.diag(A)), "eye": damping * np.eye(6), "none": 0.0 * A}[how]
    return -np.linalg.solve(M, np.asarray(b, np.float64))


def advance(pose7, d, about_sensor, order="left", turn="exact"):
    """The pose the update d = (omega, v) carries pose7 to.  The rule: q <- dq (x) q; t <- t + v about the sensor (the map fit),
    t <- R(dq) t + v about the origin (the pose fit).  order "right": q (x) dq; turn "first": t + omega x t in place of R(dq) t."""
    p = np.asarray(pose7, np.float64)
    q, t = p[:4] / np.linalg.norm(p[:4]), p[4:]
    w, v = np.asarray(d[:3], np.float64), np.asarray(d[3:], np.float64)
    th = np.linalg.norm(w)
    dq = np.concatenate([[math.cos(th / 2)], (math.sin(th / 2) / th if th > 1e-8 else 0.5) * w])
    nq = R.qmul(dq, q) if order == "left" else R.qmul(q, dq)
    if about_sensor:
        nt = t + v
    else:
        nt = (R.rotation(dq) @ t if turn == "exact" else t + np.cross(w, t)) + v
    return np.concatenate([nq / np.linalg.norm(nq), nt])


def reference_step(kind, pose7, A, b, count, damping, min_count):
    """The references' own step ("pose": pose_fit_reference.step, "map": map_fit_reference.step) from reported sums, or None."""
    ev = {"A": np.asarray(A, np.float64), "b": np.asarray(b, np.float64), "count": int(count)}
    return (F.step if kind == "map" else R.step)(pose7, ev, damping, min_count)


# name -> (fits it can be stated for, dampings it differs at, the wrong step).  kind: "pose", "turned" (pose fits) or "map"
MUTANTS = {
    "t about the sensor": (("pose", "turned"), DAMPINGS, lambda kind, p, A, b, g: advance(p, solve(A, b, g), True)),
    "t about the origin": (("map",), DAMPINGS, lambda kind, p, A, b, g: advance(p, solve(A, b, g), False)),
    "q (x) dq": (("pose", "turned", "map"), DAMPINGS, lambda kind, p, A, b, g: advance(p, solve(A, b, g), kind == "map", order="right")),
    "t + omega x t": (("pose", "turned"), DAMPINGS, lambda kind, p, A, b, g: advance(p, solve(A, b, g), False, turn="first")),
    "damping * I": (("pose", "turned", "map"), DAMPINGS[1:], lambda kind, p, A, b, g: advance(p, solve(A, b, g, "eye"), kind == "map")),
    "damping dropped": (("pose", "turned", "map"), DAMPINGS[1:], lambda kind, p, A, b, g: advance(p, solve(A, b, g, "none"), kind == "map")),
}
# What the plain pose-fit start cannot show.  The pair's true rotation is a yaw of 0.01 rad, and a full step lands next to it whatever
# the start: omega is then almost the negative of the start's own rotation vector, the two quaternions commute to within one
# tolerance, and dq (x) q cannot be told from q (x) dq.  (At damping 1 the step stops short unevenly and the order shows.)  The
# "turned" case is there for this: the same terms from a start whose rotation is 0.6 rad off the step's axis.
EXCUSED = {("pose", "q (x) dq", 0.0), ("pose", "q (x) dq", 1e-3)}


def step_bound(A, b, damping):
    """dd of the module's docstring."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    M = A + damping * np.diag(np.diag(A))
    d = -np.linalg.solve(M, b)
    return np.linalg.norm(np.linalg.inv(M), 2) * (U * np.linalg.norm(b) + (1.0 + damping) * U * np.linalg.norm(A) * np.linalg.norm(d))


def step_tolerances(kind, pose7, A, b, damping):
    """(tolerance of a quaternion component, of a translation component) of a step from pose7."""
    dd = step_bound(A, b, damping)
    t = float(np.linalg.norm(np.asarray(pose7, np.float64)[4:]))
    return dd + U, dd if kind == "map" else dd * (1.0 + t) + 2.0 * U * max(1.0, t)


def step_shares(kind, got, want, pose7, A, b, damping):
    """(worst quaternion error, worst translation error) of the pose `got` against `want`, each as a share of its tolerance."""
    tol_q, tol_t = step_tolerances(kind, pose7, A, b, damping)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got[:4] - want[:4]).max() / tol_q), float(np.abs(got[4:] - want[4:]).max() / tol_t)


TURN = (0.6, (0.3, -0.5, 0.8))                                    # radians about this axis


@functools.lru_cache(maxsize=None)
def pose_solve_case(turned=False):
    """(x1 (1,16,128,3), x2, start (1,7) float32, consts): image 0 of the 16 x 128 scene, started PERTURB off the ego-motion.
    turned: frame 1's points are given in a sensor frame turned by TURN -- a fit takes frame 1 as a list of points, whichever cells
    hold them -- and the start is composed with the turn's inverse: the same carried points, so the same terms to rounding, from a
    start whose rotation is large and shares no axis with the step."""
    f1, f2 = R.scene(2, 16, 128)
    start = R.retract(R.GUESS, PERTURB)
    x1 = f1[:1].copy()
    if turned:
        axis = np.asarray(TURN[1]) / np.linalg.norm(TURN[1])
        Q = np.concatenate([[math.cos(TURN[0] / 2)], math.sin(TURN[0] / 2) * axis])
        x1 = (x1.astype(np.float64) @ R.rotation(Q).T).astype(np.float32)
        start = np.concatenate([R.qmul(start[:4], Q * (1, -1, -1, -1)), start[4:]])
    return x1, f2[:1].copy(), start.astype(np.float32)[None], R.constants(16, 128)


@functools.lru_cache(maxsize=None)
def map_solve_case():
    """(scan (1,16,128,3), start (1,7) float64, table): image 0 of map_fit_reference.case(0), started PERTURB off its guess.  (The map
    is case(0)'s: tests/test_map_fit_gpu.py fills it.)"""
    _f2, _poses, table, scans, guess, _d = F.case(0)
    return scans[:1].copy(), F.retract(guess[0], PERTURB)[None], table


@functools.lru_cache(maxsize=None)
def zero_step_case():
    """(x (1,8,64,3), pose (1,7)): frame 2 of the 8 x 64 scene against itself at twice the identity -- every residual is exactly 0."""
    _f1, f2 = R.scene(1, 8, 64)
    return f2.copy(), np.array([[2.0, 0, 0, 0, 0, 0, 0]], np.float32)


WALL_X, WALL_SLIDE = 10.0, 0.05


def wall_image(H=8, W=64, within_deg=45.0):
    """(H,W,3) float32: the wall x = 10 exactly, one point per cell whose middle azimuth lies within 45 degrees of forward, each seen
    along the middle of its cell (pose_fit_reference.scene's placement)."""
    step = 26.8 / (H - 1)
    el = np.deg2rad(2.0 + 1.5 * step - np.arange(H) * step)[:, None] * np.ones((1, W))
    az = (math.pi - (np.arange(W) + 0.5) * (2 * math.pi / W))[None, :] * np.ones((H, 1))
    img = np.stack([np.full((H, W), WALL_X), WALL_X * np.tan(az), WALL_X * np.tan(el) / np.cos(az)], -1)
    img[np.abs(az) >= np.deg2rad(within_deg)] = 0.0
    return img.astype(np.float32)


@functools.lru_cache(maxsize=None)
def wall_case():
    """(x1 (2,8,64,3), x2, poses (2,7) float32, consts): image 0 is the wall against itself, slid 5 cm along x -- every normal is
    (-1, 0, 0) exactly, so the first row of A is 0 exactly --, image 1 the healthy 8 x 64 scene at its start pose."""
    f1, f2 = R.scene(1, 8, 64)
    wall = wall_image()
    poses = np.stack([np.array([1.0, 0, 0, 0, WALL_SLIDE, 0, 0], np.float32), R.start_poses(1)[0]])
    return np.stack([wall, f1[0]]), np.stack([wall, f2[0]]), poses, R.constants(8, 64)


@functools.lru_cache(maxsize=None)
def dead_rows_case():
    """(x1 (3,8,64,3) filtered, x2, good poses (3,7) float32, dead poses, consts, [share dropped]): three images of the 8 x 64 scene;
    image 2's good pose is the identity rotation with its start translation.  Dead: image 0's translation holds a NaN, image 2's
    quaternion is zero -- the identity, by pose_row_or_identity.  The filter ran at the good poses."""
    f1, f2 = R.scene(3, 8, 64)
    c = R.constants(8, 64)
    good = R.start_poses(3)
    good[2, :4] = (1.0, 0.0, 0.0, 0.0)
    x1, dropped = np.array(f1, copy=True), []
    for b in range(3):
        x1[b], share = R.filtered(f1[b], f2[b], good[b], c, **R.FIT)
        dropped.append(float(share))
    dead = good.copy()
    dead[0, 5] = np.nan
    dead[2, :4] = 0.0
    return x1, f2, good, dead, c, dropped


# ---- B. ragged and narrow images ---------------------------------------------------------------------------------------------------
RAGGED = ((1, 5, 100), (1, 3, 171), (2, 9, 120), (1, 12, 200), (1, 17, 250))
RAGGED_COUNTS = ((59,), (111,), (183, 202), (697,), (1828,))
RAGGED_STEPS = (2, 4)                                             # the cases that also take one step through part A's check
MIN_COUNT = 20                                                    # below the smallest count of parts B and C
FIT_TILE, FIT_SOLVE_LANES = 512, 8                                # csrc/elo_posefit.hip, csrc/elo_fit_device.h


@functools.lru_cache(maxsize=None)
def ragged_case(i):
    """pose_fit_reference.filtered_case at RAGGED[i], once."""
    B, H, W = RAGGED[i]
    return R.filtered_case(B, H, W, False)


def narrow_case(W, H=8):
    """(x (1,H,W,3) float32, pose (1,7) float32, consts): a FULL image of one or two columns, its points mid-cell at 10 + h metres,
    against itself at the identity.  The wrapped neighbours of a column coincide (W = 2) or are the cell itself (W = 1)."""
    step = 26.8 / (H - 1)
    el = np.deg2rad(2.0 + 1.5 * step - np.arange(H) * step)[:, None] * np.ones((1, W))
    az = (math.pi - (np.arange(W) + 0.5) * (2 * math.pi / W))[None, :] * np.ones((H, 1))
    r = 10.0 + np.arange(H)[:, None] * np.ones((1, W))
    x = D.xyz(el, az, r).astype(np.float32)[None]
    return x, np.array([[1.0, 0, 0, 0, 0, 0, 0]], np.float32), R.constants(H, W)


# ---- C. beam tables of every length class -------------------------------------------------------------------------------------------
BEAM_H = (2, 3, 5, 6, 9, 17, 40, 129, 255, 256)                   # 2 * half - 1 table entries: 1, 3, 7, 7, 15, 31, 63, 255, 255, 255
BEAM_W, BEAM_N = 32, 3000
BEAM_FIT = ((2, 9, 120), (1, 17, 64), (1, 40, 40), (1, 255, 16), (1, 256, 16))
BEAM_FIT_COUNTS = ((122, 144), (451,), (892,), (2000,), (2014,))
SIGNS = np.array([[sx, sy, sz] for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (0.0, -0.0)], np.float32)


def padded_entries(H):
    """How many of the 2 * half - 1 entries of RowsByBeams' table are padding (-inf) at H beams."""
    half = 1
    while 2 * half < H:
        half *= 2
    return 2 * half - 1 - (H - 1)


@functools.lru_cache(maxsize=None)
def beam_cloud(H, W=BEAM_W, N=BEAM_N):
    """(target (1,2N,3) float64, zero (1,2N) bool, beam (1,2N) int64 -- the row each live point belongs in --, copies (n,2): point
    [i,1] is an exact duplicate of what point [i,0] was): per frame, one point at every beam, 60 above the top beam and 60 below the
    bottom one (they clip to rows 0 and H-1), the rest at random beams -- each within 0.2 of the smaller neighbouring gap of its
    beam, 0.3 .. 0.7 into its column, at a range of its own on a 5 mm grid from 3 m (nobody reaches the 35 m crop) --, then N / 20
    exact duplicates (of every second of the N / 10 nearest points: about half of them win their cells) and, over 5 % of the random ones, zero padding."""
    rng = np.random.default_rng(7000 + H)
    table = np.asarray(table_deg(H))
    gap = np.abs(np.diff(table))
    small = np.minimum(np.concatenate([[np.inf], gap]), np.concatenate([gap, [np.inf]]))
    out = 60
    fixed = H + 2 * out
    beam = np.zeros((2, N), np.int64)
    el = np.zeros((2, N))
    for f in range(2):
        beam[f] = np.concatenate([np.arange(H), np.zeros(out, np.int64), np.full(out, H - 1), rng.integers(0, H, N - fixed)])
        el[f] = table[beam[f]] + rng.uniform(-0.2, 0.2, N) * small[beam[f]]
        el[f, H:H + out] = table[0] + rng.uniform(0.5, 3.0, out)
        el[f, H + out:fixed] = table[-1] - rng.uniform(0.5, 3.0, out)
    az = np.pi - (rng.integers(0, W, (2, N)) + rng.uniform(0.3, 0.7, (2, N))) * (2 * np.pi / W)
    r = 3.0 + 0.005 * rng.permutation(2 * N).reshape(2, N)
    target = D.xyz(np.deg2rad(el), az, r).astype(np.float32).astype(np.float64)
    zero, copies = np.zeros((2, N), bool), []
    for f in range(2):
        src, dst = np.argsort(r[f])[:N // 10:2], fixed + rng.permutation(N - fixed)[:N // 20]   # every second of the nearest: winners
        target[f, dst], beam[f, dst] = target[f, src], beam[f, src]
        copies.append(np.stack([src, dst], -1) + f * N)
        pad = fixed + np.flatnonzero(rng.random(N - fixed) < 0.05)
        zero[f, pad] = True
    return target.reshape(1, 2 * N, 3), zero.reshape(1, 2 * N), beam.reshape(1, 2 * N), np.concatenate(copies)


def plain_cloud(H):
    """(1,2N,3) float32: beam_cloud(H) as a motion-compensated scan, its padding signed zeros (all eight kinds in each frame)."""
    target, zero, _beam, _copies = beam_cloud(H)
    cloud = target.astype(np.float32)
    n = int(zero.sum())
    cloud[zero] = SIGNS[np.arange(n) % 8]
    return cloud


DESKEW_PHASE_REF = 0.5


@functools.lru_cache(maxsize=None)
def skewed_cloud(H):
    """(raw (1,2N,4) float32 with the phase in channel 3, motion (1,7) float32): the raw scan whose correction to DESKEW_PHASE_REF by
    `motion` is beam_cloud(H) -- duplicates share their phase, the padding is signed zeros."""
    target, zero, _beam, copies = beam_cloud(H)
    rng = np.random.default_rng(9000 + H)
    motion = D.motion_row(rng)[None]
    N2 = target.shape[1]
    phase = rng.uniform(0.0, 1.0, N2).astype(np.float32)
    phase[copies[:, 1]] = phase[copies[:, 0]]                                           # (as beam_cloud copied the points)
    raw = np.zeros((1, N2, 4), np.float32)
    raw[0, :, :3] = D.skew(target[0], phase.astype(np.float64), motion[0], DESKEW_PHASE_REF)
    raw[0, :, 3] = phase
    n = int(zero.sum())
    raw[0, zero[0], :3] = SIGNS[np.arange(n) % 8]
    return raw, motion


def project(points, H, W=BEAM_W):
    """deskew_reference.project of one image's points under the nearest-beam rule of table_deg(H) -> (image (H,W,3) float64, how many
    points each cell sums (H,W))."""
    rad = np.asarray(table_deg(H)) * (math.pi / 180)
    return D.project(np.asarray(points, np.float64), H, W, R.constants(H, W)[0], D.nearest_beam(rad.astype(np.float32).astype(np.float64)))


@functools.lru_cache(maxsize=None)
def beam_fit_case(i):
    """pose_fit_reference.filtered_case at BEAM_FIT[i] with table_deg(H), once."""
    B, H, W = BEAM_FIT[i]
    return R.filtered_case(B, H, W, False, table_deg(H))


# the model render: (B, K, H, W, beams of the table or 0, what the case is for)
RENDERS = ((1, 3, 40, 64, 40, "a 40-beam table: 63 entries, 24 of them padding"),
           (1, 3, 17, 67, 0, "H W = 1139 is no multiple of 4: the loads go one float at a time, the last strip is cut short"))


@functools.lru_cache(maxsize=None)
def rendered(i):
    """(src, pose, consts, beam table in radians or None, [the reference's render per batch element]) of RENDERS[i]."""
    B, K, H, W, beams, _why = RENDERS[i]
    src, pose, consts, beam = LM.render_inputs(B, K, H, W, table_deg(beams) if beams else None, len(LM.CASES) + i)
    return src, pose, consts, beam, [LM.render(src[b], pose[b], consts, beam) for b in range(B)]

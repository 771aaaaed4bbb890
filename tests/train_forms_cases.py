"""TEST INFRASTRUCTURE: ONE table of cases for every launch form of the training-layer row kernels (csrc/elo_train.hip):
elo_dense_weight_grad picks one of 42 compiled kernels by the widths and the operands' alignment (include/elo.h:
elo_dense_weight_grad_form), and the batch-norm kernels (elo_bn_stats / elo_bn_apply / elo_bn_backward) change their trip structure with
the rows per group against rpb = 1024 / C, the rows of one block iteration (elo_bn_parts).  Each case names what it is built to reach.
tests/test_train_forms_cpu.py asks the library whether it does (no GPU: the queries read the argument block only);
tests/test_train_forms_gpu.py runs the cases against float64 at the bounds of tests/train_forms_bounds.py.

The launcher's choices are restated here in Python (wgrad_plan, wgrad_slices, bn_parts): the CPU test holds every restatement against
the library for every case, and the bounds and the float32 restatements of tests/train_forms_bounds.py take their counts from them.

The inputs of a case are made here too (numpy, seeded by the case), so that the CPU test (restatements, mutants) and the GPU test
see the same numbers."""
import collections

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- weight gradient
# x_off / g_off: bytes past a 16-byte boundary of x / g (0 or 4).   kernel: a name of _lib.WGRAD_FORMS ('ci4co4/xvgs': x loaded as
# vectors, g one channel per tile).   grid: (gy, gz, waves) the block grid and the waves per workgroup.   why: what the case is for.
Wgrad = collections.namedtuple("Wgrad", "rows cin cout x_off g_off kernel grid why")

WGRAD_ROWS = (1, 3, 5, 33, 65, 129, 257, 4096)      # a lone partial group; trips shorter than U; a ragged second half of the double-buffered
#                                                     loop; two and three slices; 4096: 33 slices of 32 groups over 1024 groups, the last empty
CIN_OF = {1: (1, 16), 2: (17, 32), 3: (33,), 4: (49, 64)}        # CI: (scalar member, vector member); CI = 3 is never a vector
COUT_OF = {1: (1, 16), 2: (17, 32), 4: (49, 64)}


def wgrad_slices(rows, cin, cout):
    """elo_weight_grad_slices restated."""
    groups = (rows + 3) // 4
    s = min(groups // 32 + 1, 2048, (32 << 20) // (cin * cout * 4))
    return max(s, 1)


def wgrad_plan(rows, cin, cout, x_off=0, g_off=0):
    """The launcher's choice restated: dict(CI, CO, xv, gv, gy, gz, waves, slices, per_slice) -- per_slice: row groups of 4 per slice."""
    cit, cot = (cin + 15) // 16, (cout + 15) // 16
    CO = 4 if cot >= 4 else 2 if cot >= 2 else 1
    CI = 1
    for c in (2, 3, 4):
        padded = (cit + c - 1) // c * c
        if padded <= (cit + CI - 1) // CI * CI or padded * 4 <= cit * 5:
            CI = c
    gy, gz = (cit + CI - 1) // CI, (cot + CO - 1) // CO
    slices = wgrad_slices(rows, cin, cout)
    groups = (rows + 3) // 4
    return dict(CI=CI, CO=CO, xv=int(CI != 3 and cin % (16 * CI) == 0 and x_off % 16 == 0), gv=int(cout % (16 * CO) == 0 and g_off % 16 == 0),
                gy=gy, gz=gz, waves=min(gy * gz, 4), slices=slices, per_slice=(groups + slices - 1) // slices)


def _wg(rows, cin, cout, why, x_off=0, g_off=0):
    p = wgrad_plan(rows, cin, cout, x_off, g_off)
    kernel = "ci%dco%d/x%sg%s" % (p["CI"], p["CO"], "sv"[p["xv"]], "sv"[p["gv"]])
    return Wgrad(rows, cin, cout, x_off, g_off, kernel, (p["gy"], p["gz"], p["waves"]), why)


# (the expected kernel of the 42 smallest shapes is WRITTEN OUT, not computed by wgrad_plan: the table says which form a shape is for)
WGRAD_SMALL = [Wgrad(rows, cin, cout, 0, 0, "ci%dco%d/x%sg%s" % (ci, co, "sv"[xi], "sv"[gi]), (1, 1, 1), "smallest")
               for ci in (1, 2, 3, 4) for xi, cin in enumerate(CIN_OF[ci]) for co in (1, 2, 4) for gi, cout in enumerate(COUT_OF[co])
               for rows in WGRAD_ROWS]
WGRAD_MORE = (
    # the alignment demotion: (64, 64) with x, and separately g, a contiguous view 4 bytes into its storage
    [_wg(rows, 64, 64, "x 4 bytes off", x_off=4) for rows in (5, 257, 4096)] + [_wg(rows, 64, 64, "g 4 bytes off", g_off=4) for rows in (5, 257, 4096)]
    # CI = 3 on several blocks: 138 = 9 tiles (3 blocks of 3), 80 = 5 tiles (2 blocks of 3, one tile of padding) x 2 column blocks
    + [_wg(rows, 138, 64, "CI = 3, 3 blocks") for rows in (5, 257, 4096)] + [_wg(rows, 80, 128, "CI = 3, 2 x 2 blocks") for rows in (5, 257, 4096)]
    # 20 blocks: five workgroups of four waves in y
    + [_wg(rows, 272, 256, "20 blocks, 5 workgroups in y") for rows in (5, 257, 4096)]
    # 5 blocks on 4-wave workgroups: the second workgroup's three idle waves return at once; x as vectors
    + [_wg(rows, 320, 64, "5 blocks, idle waves") for rows in (5, 257, 4096)]
    # the caps of the slice count: 32 MB of partial blocks (128 slices, three of them empty); 2048 slices
    + [_wg(16391, 256, 256, "32 MB cap"), _wg(262149, 1, 1, "2048-slice cap")])
WGRAD = WGRAD_SMALL + WGRAD_MORE


def wgrad_id(c):
    off = "+x4" if c.x_off else "+g4" if c.g_off else ""
    return "%s@%dx%dw%d-%dx%d%s-r%d" % ((c.kernel,) + c.grid + (c.cin, c.cout, off, c.rows))


def wgrad_inputs(c):
    """x (rows, cin), g (rows, cout): float32."""
    rng = np.random.default_rng([c.rows, c.cin, c.cout])
    return rng.normal(0.3, 1.0, (c.rows, c.cin)).astype(np.float32), rng.normal(0.0, 1.0, (c.rows, c.cout)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- batch norm
# M: rows per group.   running: the moving averages are updated.   edge: the name of M against rpb = 1024 / C (BN_EDGES).
Bn = collections.namedtuple("Bn", "C M groups relu running edge")

BN_WIDTHS = (4, 8, 16, 32, 64, 128, 256)
BN_MAX_PARTS = 512                                   # ELO_BN_MAX_PARTS
BN_EDGES = collections.OrderedDict([                 # rows per group as a function of rpb
    ("one", lambda r: 1), ("two", lambda r: 2),                                  # one row: the variance is 0, the moving variance takes it as it is
    ("below", lambda r: r - 1), ("iter", lambda r: r), ("over", lambda r: r + 1),           # around one block iteration
    ("trip-", lambda r: 8 * r - 1), ("trip+", lambda r: 8 * r + 1),                          # around one unrolled trip (8 iterations; backward: 2 of 4)
    ("ragged", lambda r: 24 * r + 5),                                            # 4 blocks, the last with a ragged trip
    ("cap", lambda r: 512 * 8 * r + 24 * r + 1)])                                # beyond 512 parts: 9 iterations per block, blocks that own no row


def bn_parts(M, C):
    """elo_bn_parts restated."""
    rpb = 1024 // C
    iters = (M + rpb - 1) // rpb
    return max(1, min(BN_MAX_PARTS, (iters + 7) // 8))


def bn_per(M, C):
    """Block iterations of `rpb` rows in one thread's chain: ceil(ceil(M / rpb) / parts)."""
    rpb = 1024 // C
    parts = bn_parts(M, C)
    return ((M + rpb - 1) // rpb + parts - 1) // parts


def _bn_cases():
    out = []
    for C in BN_WIDTHS:
        r = 1024 // C
        out += [Bn(C, rows(r), 1, 1, 1, edge) for edge, rows in BN_EDGES.items()]        # (rpb >= 4: the nine row counts differ)
        out += [Bn(C, 24 * r + 5, 2, 1, 1, "ragged"), Bn(C, 24 * r + 5, 3, 0, 1, "ragged"), Bn(C, r + 1, 64, 1, 0, "over"),
                Bn(C, 8 * r + 1, 1, 0, 0, "trip+"), Bn(C, 1, 2, 1, 1, "one"), Bn(C, r - 1, 3, 1, 0, "below")]
    return out


BN = _bn_cases()
# beyond the 8192-block cap of the two elementwise kernels (one block per 1024 float4): data made on the device by the GPU test
BN_BIG = Bn(256, 131075, 1, 1, 0, "blocks")
BN_EPS, BN_MOMENTUM = np.float32(1e-3), np.float32(0.3)


def bn_id(c):
    return "C%d-%s%d-g%d%s%s" % (c.C, c.edge, c.M, c.groups, "-relu" if c.relu else "", "-avg" if c.running else "")


TIE_MEAN, TIE_INVSTD, TIE_Z = np.float32(0.5), np.float32(2.0), np.float32(0.5)     # (0.5 - 0.5) * 2 * (+-1) + (+-0) = +-0 exactly


def bn_inputs(c):
    """The tensors of a case, float32: z, dy (groups * M, C); mean, invstd (groups, C); gamma, beta, rm, rv (C); tie (groups * M, C) bool.
    mean, invstd, gamma and beta are INPUTS of elo_bn_apply / elo_bn_backward (the kernels are called directly), so exact ties of the
    recomputed ReLU decision can be placed: channels 0 and 1 have mean 0.5, invstd 2, beta 0 and gamma +1 / -1, their z are multiples of
    1/8, and z = 0.5 (`tie`) gives a pre-activation of exactly +0 / -0.  Everywhere else z is moved until the pre-activation is at least
    4 rounding bounds (train_forms_bounds.apply_bound) away from zero: the fp32 decision then IS the float64 one, and nothing has to be
    excluded when results are compared."""
    import train_forms_bounds as bounds
    rng = np.random.default_rng([c.C, c.M, c.groups])
    rows, C, G = c.M * c.groups, c.C, c.groups
    f = np.float32
    z = rng.normal(0.3, 1.5, (rows, C)).astype(f)
    dy = rng.normal(0.0, 1.0, (rows, C)).astype(f)
    mean, invstd = rng.normal(0.3, 0.2, (G, C)).astype(f), rng.uniform(0.4, 1.2, (G, C)).astype(f)
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.3, -1.0, 1.0)).astype(f)
    beta = rng.normal(0.0, 0.3, C).astype(f)
    rm, rv = rng.normal(0.0, 0.5, C).astype(f), rng.uniform(0.5, 2.0, C).astype(f)
    mean[:, :2], invstd[:, :2], gamma[0], gamma[1] = TIE_MEAN, TIE_INVSTD, 1.0, -1.0
    beta[0], beta[1] = 0.0, -0.0                                     # ((-0) + (+0) would be +0)
    z[:, :2] = np.clip(np.round(rng.normal(0.5, 1.0, (rows, 2)) * 8) / 8, -3, 4)
    tie = np.zeros((rows, C), bool)
    tie[:, :2] = rng.random((rows, 2)) < 0.25
    tie[::c.M, :2] = True                                            # (every group has one: its first row)
    z[tie] = TIE_Z
    tie[:, :2] = z[:, :2] == TIE_Z                                   # (a multiple of 1/8 that happened to be 0.5 is a tie as well)
    for _ in range(4):
        pre, bound = bounds.preactivation(z, mean, invstd, gamma, beta, G)
        near = (np.abs(pre) <= 4 * bound) & ~tie
        if not near.any():
            break
        z[near] += f(1.0)                                            # (moves the pre-activation by invstd * |gamma| >= 0.2)
    return dict(z=z, dy=dy, mean=mean, invstd=invstd, gamma=gamma, beta=beta, rm=rm, rv=rv, tie=tie)

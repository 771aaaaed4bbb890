"""TEST INFRASTRUCTURE: ONE table of cases for every forward form of the per-operator feature kernels (csrc/elo_features.hip):
which kernel elo_cv_encode1 / elo_cv_encode2 / elo_masked_softmax_pool launch is a ladder over row count, channel count, K, storage
type and pointer alignment (include/elo.h: the elo_*_form queries).  Each case names the form it is built to reach.
tests/test_forward_forms_cpu.py asks the library whether it does (no GPU: the queries read the argument block only) and that every
form has a case; tests/test_forward_forms_gpu.py runs the cases against float64 and asks again with the real pointers.

Shapes are the smallest that reach a form and still have a tail: the row count is no multiple of the form's workgroup span
(32 / 64 / 128 rows; 60, 55, 115 ... for the column-owner form), K does not divide it (a workgroup begins mid-centre), and with B = 2
one workgroup straddles the batch boundary.  The encode kernels' workgroup size goes by rows = B * N * K: 32 below 65536, 64 from
there, 128 above 524288 -- the big cases keep C tiny so that their outputs stay in the tens of megabytes."""
import collections

# op: "encode1" | "encode2" | "pool".   dtype: "f32" | "f16" (storage of the feature tensors).
# encode1: N centres anywhere, neighbours on the H x W grid.   encode2: the H x W grid's pixels are the centres (N = H * W).
# C / Cc: channels (Cc: encode2's cost width).   wide: (width, first) -- the pool's values are channels first..first+C of a
# `width`-channel tensor -- or None.   offset: bytes past a 16-byte boundary of the feature tensors (encode1: feat1 and feat2,
# encode2: feat1 and cost, pool: values).   tuning: (field, value) pairs of the library tuning for the call.   form: the expected answer of the query.
Case = collections.namedtuple("Case", "op dtype B N H W K C Cc wide offset tuning form")
Refusal = collections.namedtuple("Refusal", "why case")

GRID = (8, 29)                                         # encode1's neighbour grid: small, so that the hot cells are really hot


def _e1(dtype, form, B, N, K, C, offset=0):
    return Case("encode1", dtype, B, N, GRID[0], GRID[1], K, C, None, None, offset, None, form)


def _e2(dtype, form, B, H, W, K, C, Cc, offset=0):
    return Case("encode2", dtype, B, H * W, H, W, K, C, Cc, None, offset, None, form)


def _pool(dtype, form, K, C, wide=None, offset=0, tuning=None):
    return Case("pool", dtype, 2, 301, None, None, K, C, None, wide, offset, tuning, form)          # B * N = 602: not a multiple of 4


SMALL, MID = (1, 228, 6), (2, 701, 6)                  # (B, N, K): 1368 rows (a batch-1 l2 level: 228 x 6); 8412 rows (>= 8192: staged)
MID7 = (2, 601, 7)                                     # 8414 rows: for the column-owner spans that 6 divides (60 rows at C = 16)
ROWS_64K, ROWS_512K = (2, 5462, 6), (2, 43691, 6)      # 65544 rows (>= 65536); 524292 rows (> 524288)

ENCODE1 = [
    # staged<128 / 64>: >= 8192 rows, 16-byte aligned, C % 4 == 0 (fp16: % 8); the tile within 40 KB
    _e1("f32", "staged128", *MID, 16), _e1("f32", "staged128", *MID, 32), _e1("f32", "staged64", *MID, 36),
    _e1("f32", "staged64", *MID, 64), _e1("f32", "staged64", *MID, 72),
    _e1("f16", "staged128", *MID, 16), _e1("f16", "staged128", *MID, 72), _e1("f16", "staged64", *MID, 80),
    _e1("f16", "staged64", *MID, 128), _e1("f16", "staged64", *MID, 152),
    # col<64>: row lengths that tile the 256 threads -- below 8192 rows, 8 bytes off, C no multiple of a 16-byte chunk, a tile too large
    _e1("f32", "col64", 1, 228, 7, 16), _e1("f32", "col64", 2, 115, 6, 18), _e1("f32", "col64", *MID7, 16, 8),
    _e1("f32", "col64", *MID, 18), _e1("f32", "col64", *MID7, 76), _e1("f32", "col64", 1, 228, 7, 122),
    _e1("f16", "col64", 1, 228, 7, 16), _e1("f16", "col64", *MID7, 16, 8), _e1("f16", "col64", *MID, 20), _e1("f16", "col64", *MID7, 16, 4),
    # col<128>: above 512 Ki rows (C = 6: 23 rows of 11 slots per pass, a 115-row span)
    _e1("f32", "col128", *ROWS_512K, 6), _e1("f16", "col128", *ROWS_512K, 6),
    # vec<32 / 64 / 128>: everything else with an even C
    _e1("f32", "vec32", *SMALL, 64), _e1("f32", "vec32", 2, 115, 6, 64), _e1("f32", "vec32", *SMALL, 2), _e1("f32", "vec32", *SMALL, 24),
    _e1("f32", "vec32", *MID, 64, 8), _e1("f32", "vec32", *SMALL, 6),
    _e1("f16", "vec32", *SMALL, 64), _e1("f16", "vec32", 2, 115, 6, 64), _e1("f16", "vec32", *MID, 64, 4), _e1("f16", "vec32", *MID, 160),
    _e1("f32", "vec64", *ROWS_64K, 2), _e1("f32", "vec64", *ROWS_64K, 24, 8), _e1("f16", "vec64", *ROWS_64K, 2),
    _e1("f32", "vec128", *ROWS_512K, 2), _e1("f16", "vec128", *ROWS_512K, 2),
    # scalar (fp32 only): odd C, or 4 bytes off
    _e1("f32", "scalar", *SMALL, 3), _e1("f32", "scalar", 2, 115, 6, 17), _e1("f32", "scalar", *SMALL, 16, 4), _e1("f32", "scalar", *MID, 64, 12),
]

ENCODE2 = [
    _e2("f32", "vec32", 2, 4, 57, 6, 4, 4), _e2("f32", "vec32", 2, 4, 57, 5, 64, 32), _e2("f32", "vec32", 1, 8, 113, 6, 16, 64),
    _e2("f32", "vec64", 2, 8, 683, 6, 4, 8), _e2("f32", "vec128", 2, 16, 2731, 6, 4, 4),
    _e2("f16", "vec32", 2, 4, 57, 6, 8, 8), _e2("f16", "vec32", 2, 4, 57, 5, 64, 16), _e2("f16", "vec64", 2, 8, 683, 6, 8, 16),
    _e2("f16", "vec128", 2, 16, 2731, 6, 8, 8),
    # scalar (fp32 only): C or Cc no multiple of 4, or off 16-byte alignment
    _e2("f32", "scalar", 2, 4, 57, 6, 6, 6), _e2("f32", "scalar", 2, 4, 57, 6, 4, 6), _e2("f32", "scalar", 2, 4, 57, 6, 4, 4, 4),
    _e2("f32", "scalar", 2, 4, 57, 6, 64, 32, 8),
]

_WAVE_OF_K = {1: "wave1", 3: "wave1", 4: "wave1", 5: "wave2", 8: "wave2", 9: "wave4", 16: "wave4", 17: "wave8", 32: "wave8"}
_NO_WAVE = (("pool_wave", 0),)
_vec = lambda K: "vec6" if K % 6 == 0 else "vec4"


def _with_slice(cases):
    """every case, and the same with the values a channel slice (32 channels in) of a tensor 32 channels wider"""
    return [c for case in cases for c in (case, case._replace(wide=(case.C + 32, 32)))]


POOL = _with_slice(
    # wave<J>: fp32, C = 64, K <= 32 (J = 1, 2, 4, 8 rows per lane group; K = 1 and 3 leave whole lane groups without a neighbour)
    [_pool("f32", form, K, 64) for K, form in _WAVE_OF_K.items()] +
    # vec<U> in fp32: the wave form switched off, another C, or K > 32
    [_pool("f32", _vec(K), K, 64, tuning=_NO_WAVE) for K in (4, 5, 6, 7, 12, 32)] +
    [_pool("f32", _vec(K), K, C) for K, C in ((6, 4), (5, 16), (6, 128), (5, 1024))] +
    [_pool("f32", _vec(K), K, 64) for K in (33, 36)] +
    [_pool("f16", _vec(K), K, C) for K in (4, 5, 6, 32) for C in (16, 64)])
POOL += [
    # scalar (fp32 only): C % 4 != 0, 256 % (C / 4) != 0, values 4 bytes off, a values stride that is no multiple of 4
    _pool("f32", "scalar", 6, 6), _pool("f32", "scalar", 5, 12), _pool("f32", "scalar", 8, 24), _pool("f32", "scalar", 6, 64, offset=4),
    _pool("f32", "scalar", 32, 64, wide=(98, 17)), _pool("f32", "scalar", 4, 64, wide=(98, 0)),
    _pool("f32", "scalar", 6, 64, offset=8),             # (fp32's 16-byte vectors need 16-byte alignment ...)
    _pool("f16", "vec6", 6, 64, offset=8),               # (... fp16's 8-byte vectors 8)
]

CASES = ENCODE1 + ENCODE2 + POOL

# what fp16 storage cannot take (it has no scalar form): the entry points answer ELO_ERR_ARG and launch nothing
REFUSALS = [
    Refusal("fp16 with an odd C", _e1("f16", None, *SMALL, 15)),
    Refusal("fp16 2 bytes off", _e1("f16", None, *SMALL, 16, 2)),
    Refusal("fp16 cv_encode2 with C % 8 != 0", _e2("f16", None, 2, 4, 57, 6, 12, 8)),
    Refusal("fp16 cv_encode2 with Cc % 8 != 0", _e2("f16", None, 2, 4, 57, 6, 8, 12)),
    Refusal("fp16 cv_encode2 2 bytes off", _e2("f16", None, 2, 4, 57, 6, 8, 8, 2)),
    Refusal("fp16 pool with C % 4 != 0", _pool("f16", None, 6, 6)),
    Refusal("fp16 pool 4 bytes off", _pool("f16", None, 6, 64, offset=4)),
]

# the ladder's row thresholds, asked with fake pointers only (rows = B * N * K with K = 1): (rows, C, offset, form)
ENCODE1_THRESHOLDS = [(8191, 16, 0, "col64"), (8192, 16, 0, "staged128"), (65535, 64, 8, "vec32"), (65536, 64, 8, "vec64"),
                      (524288, 64, 8, "vec64"), (524289, 64, 8, "vec128"), (524288, 6, 0, "vec64"), (524289, 6, 0, "col128")]


def rows(case):
    return case.B * case.N * (case.K if case.op != "pool" else 1)


def case_id(case):
    s = "%s-%s-%s-B%d-N%d-K%d-C%d" % (case.op, case.dtype, case.form, case.B, case.N, case.K, case.C)
    if case.Cc is not None:
        s += "-Cc%d" % case.Cc
    if case.wide:
        s += "-values_wide%d[%d:%d]" % (case.wide[0], case.wide[1], case.wide[1] + case.C)
    if case.offset:
        s += "-%d_bytes_off" % case.offset
    if case.tuning:
        s += "-" + "-".join("%s=%d" % kv for kv in case.tuning)
    return s


def span(case):
    """rows per workgroup of an encode case's form (csrc/elo_features.hip: the column-owner form takes a whole number of 5-deep passes
    of 256 / (5 + C) rows)"""
    if case.form.startswith("col"):
        batch_rows = 256 // (5 + case.C) * 5
        return int(case.form[3:]) // batch_rows * batch_rows
    return 64 if case.form == "scalar" else int(case.form.lstrip("abcdefghijklmnopqrstuvwxyz"))

"""CPU: every refusal of the scan-level entry points that return before any launch on an empty block, through ctypes with _lib's
argument structs -- the status and the exact text of elo_last_error().

Each entry point starts from one admissible block with batch (rows, n) = 0 and small fabricated non-null addresses at the required
alignment: the empty-work return sits behind every check, so that block answers 0 and leaves the error text alone, and no call
here launches anything.  A case changes the fields it names; a check that stopped refusing answers 0 and fails the assertion.
Where a case changes two fields, both would be refused and the text is the earlier check's: the order of the checks is pinned too.

Not here: elo_map_extract, elo_model_begin and elo_model_advance have no empty-work return (their refusals, the `overlaps` of the
ring among them, are covered on real tensors by test_device_tracker_gpu and the world-map tests), and elo_map_merge's overlap
refusal at rows > 0 for the same reason -- its zero-length edge (rows = 0: nothing overlaps, whatever the pointers) is here."""
import ctypes
import math

import pytest

from conftest import load_pkg

L = load_pkg("_lib")
INF, NAN = math.inf, math.nan
ERR_ARG = -1
TABLE = "voxel is positive and finite, log2_capacity ELO_MAP_MIN_LOG2 .. ELO_MAP_MAX_LOG2"
SHAPE = "rings is 1 .. ELO_PLACE_MAX_RINGS, sectors 1 .. ELO_PLACE_MAX_SECTORS"
JD = "jump_rel / damping must be >= 0"
BIG = dict(batch=65535, H=256, W=256)                   # H * W fits, batch * H * W = 2^32 - 2^16 does not
WIDE = dict(H=65536, W=32768)                           # H * W = 2^31


def edges(**changed):
    e = [0.0] + [float(j * j) for j in range(1, L.PLACE_MAX_RINGS + 1)]
    for k, v in changed.items():
        e[int(k[1:])] = v
    return (ctypes.c_double * (L.PLACE_MAX_RINGS + 1))(*e)


GOOD = {
    "elo_pose_fit": (L.PoseFitArgs, dict(
        batch=0, H=8, W=16, az_res=0.1, vert_res=0.1, vert_off=0.0, xyz1=0x1000, xyz2=0x2000, pose_in=0x3000, beam_elev=None, iters=1,
        gate=1.0, huber=0.5, jump_rel=0.1, min_count=6, damping=0.0, pose_out=0x4000, info=0x5000, grad=0x6000, stats=0x7000,
        scratch=0x8000)),
    "elo_map_fit": (L.MapFitArgs, dict(
        batch=0, H=8, W=16, voxel=1.0, log2_capacity=12, keys=0x1000, acc=0x2000, xyz=0x3004, pose_in=0x4000, iters=1, gate=0.5,
        huber=0.5, jump_rel=0.1, min_count=6, damping=0.0, min_points=1, pose_out=0x5000, info=0x6004, grad=0x7004, stats=0x8004,
        match=None, scratch=0x9004)),
    "elo_model_render": (L.ModelRenderArgs, dict(
        batch=0, K=2, H=8, W=16, az_res=0.1, vert_res=0.1, vert_off=0.0, src=0x1000, pose=0x2000, beam_elev=None, out_xyz=0x1004,
        out_src=0x4000, scratch=0x5000)),                # (out_xyz four bytes into src: an empty batch aliases only at src itself)
    "elo_map_insert": (L.MapInsertArgs, dict(
        batch=0, H=8, W=16, voxel=1.0, min_range=0.0, max_range=50.0, log2_capacity=12, xyz=0x1004, pose=0x2000, keys=0x3000,
        acc=0x4000, stats=0x5000)),
    "elo_map_merge": (L.MapMergeArgs, dict(               # (the source IS the destination: no row, so nothing overlaps)
        rows=0, src_keys=0x1000, src_acc=0x2000, voxel=1.0, log2_capacity=12, keys=0x1000, acc=0x2000, stats=0x3000, centre=None,
        radius=0.0, min_count=1, report=0x4000)),
    "elo_scan_descriptor": (L.ScanDescriptorArgs, dict(
        batch=0, H=8, W=64, rings=4, sectors=16, z_min=-2.0, z_step=0.01, min_range2=0.0, edge2=edges(), xyz=0x1004, desc=0x2002)),
    "elo_descriptor_search": (L.DescriptorSearchArgs, dict(
        n=0, m=0, rings=4, sectors=16, k=1, query=0x1002, db=0x2002, entry=0x3004, shift=0x4004, dist=0x5000, best_shift=None,
        best_dist=None)),
}

# entry point -> (changed fields, the text behind "<entry point>: ")
REFUSED = {
    "elo_pose_fit": [
        (dict(H=2), "a normal needs three rows: H >= 3"), (dict(H=2, batch=-1), "a normal needs three rows: H >= 3"),
        (dict(batch=-1), "bad sizes"), (dict(W=0), "bad sizes"), (dict(batch=65536), "bad sizes"), (BIG, "bad sizes"),
        (WIDE, "bad sizes"), (dict(W=0, iters=-1), "bad sizes"),
        (dict(iters=-1), "negative iters"), (dict(iters=-1, gate=0.0), "negative iters"),
        (dict(gate=0.0), "gate must be positive and finite"), (dict(gate=-1.0), "gate must be positive and finite"),
        (dict(gate=INF), "gate must be positive and finite"), (dict(gate=NAN), "gate must be positive and finite"),
        (dict(gate=INF, huber=0.0), "gate must be positive and finite"),
        (dict(huber=0.0), "huber must be positive and finite"), (dict(huber=INF), "huber must be positive and finite"),
        (dict(huber=NAN), "huber must be positive and finite"),
        (dict(jump_rel=-0.5), JD), (dict(jump_rel=NAN), JD), (dict(damping=-0.5), JD), (dict(damping=INF), JD), (dict(damping=NAN), JD),
        (dict(beam_elev=0x9000, H=257), "more beams than ELO_MAX_BEAMS"),
        (dict(az_res=0.0), "bad projection constants"), (dict(vert_res=0.0), "bad projection constants"),
        (dict(az_res=NAN), "bad projection constants"), (dict(beam_elev=0x9000, az_res=-1.0), "bad projection constants"),
        (dict(xyz1=None), "null image or pose"), (dict(xyz2=None), "null image or pose"), (dict(pose_in=None), "null image or pose"),
        (dict(pose_in=None, pose_out=None), "null image or pose"),
        (dict(pose_out=None), "null output or scratch pointer"), (dict(info=None), "null output or scratch pointer"),
        (dict(grad=None), "null output or scratch pointer"), (dict(stats=None), "null output or scratch pointer"),
        (dict(scratch=None), "null output or scratch pointer"),
        (dict(pose_out=0x3000), "pose_out aliases pose_in"),
    ],
    "elo_map_fit": [
        (dict(H=2), "a normal needs three rows: H >= 3"),
        (dict(batch=-1), "bad sizes"), (dict(W=0), "bad sizes"), (dict(batch=65536), "bad sizes"), (BIG, "bad sizes"), (WIDE, "bad sizes"),
        (dict(W=0, voxel=0.0), "bad sizes"),
        (dict(voxel=0.0), TABLE), (dict(voxel=INF), TABLE), (dict(voxel=NAN), TABLE), (dict(log2_capacity=9), TABLE),
        (dict(log2_capacity=29), TABLE), (dict(voxel=0.0, iters=-1), TABLE),
        (dict(iters=-1), "negative iters"),
        (dict(gate=0.0), "gate must be positive and at most the voxel"), (dict(gate=1.5), "gate must be positive and at most the voxel"),
        (dict(gate=NAN), "gate must be positive and at most the voxel"),
        (dict(huber=0.0), "huber must be positive and finite"), (dict(huber=INF), "huber must be positive and finite"),
        (dict(jump_rel=-0.5), JD), (dict(damping=-0.5), JD), (dict(damping=INF), JD),
        (dict(min_points=0), "min_points is >= 1"),
        (dict(keys=None), "null table, image or pose"), (dict(acc=None), "null table, image or pose"),
        (dict(xyz=None), "null table, image or pose"), (dict(pose_in=None), "null table, image or pose"),
        (dict(pose_out=None), "null output or scratch pointer"), (dict(info=None), "null output or scratch pointer"),
        (dict(grad=None), "null output or scratch pointer"), (dict(stats=None), "null output or scratch pointer"),
        (dict(scratch=None), "null output or scratch pointer"),
        (dict(pose_out=0x4000), "pose_out aliases pose_in"),
    ] + [({f: GOOD["elo_map_fit"][1][f] + 4 if GOOD["elo_map_fit"][1][f] else 0xa004}, "keys, acc, pose_in, pose_out and match must be 8-byte aligned")
         for f in ("keys", "acc", "pose_in", "pose_out", "match")],
    "elo_model_render": [
        (dict(K=0), "K is 1 .. ELO_MODEL_MAX_SCANS"), (dict(K=17), "K is 1 .. ELO_MODEL_MAX_SCANS"),
        (dict(K=0, batch=-1), "K is 1 .. ELO_MODEL_MAX_SCANS"),
        (dict(batch=-1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"), (BIG, "bad sizes"), (WIDE, "bad sizes"),
        (dict(K=16, H=32768, W=8192), "K * H * W beyond 2^31"),
        (dict(beam_elev=0x9000, H=257), "more beams than ELO_MAX_BEAMS"),
        (dict(az_res=0.0), "bad projection constants"), (dict(vert_res=0.0), "bad projection constants"),
        (dict(src=None), "null image or pose"), (dict(pose=None), "null image or pose"),
        (dict(out_xyz=None), "null output or scratch pointer"), (dict(out_src=None), "null output or scratch pointer"),
        (dict(scratch=None), "null output or scratch pointer"), (dict(scratch=0x5004), "scratch must be 8-byte aligned"),
        (dict(out_xyz=0x1000), "out_xyz aliases src"),
    ],
    "elo_map_insert": [
        (dict(batch=-1), "bad sizes"), (dict(H=0), "bad sizes"), (dict(W=0), "bad sizes"), (dict(W=0, voxel=0.0), "bad sizes"),
        (BIG, "batch * H * W beyond 2^31"), (WIDE, "batch * H * W beyond 2^31"),
        (dict(voxel=0.0), TABLE), (dict(voxel=INF), TABLE), (dict(voxel=NAN), TABLE), (dict(log2_capacity=9), TABLE),
        (dict(log2_capacity=29), TABLE),
        (dict(min_range=-1.0), "min_range is >= 0"), (dict(min_range=NAN), "min_range is >= 0"),
        (dict(max_range=0.0), "max_range lies above min_range"), (dict(max_range=NAN), "max_range lies above min_range"),
        (dict(xyz=None), "null pointer"), (dict(pose=None), "null pointer"), (dict(keys=None), "null pointer"),
        (dict(acc=None), "null pointer"), (dict(stats=None), "null pointer"),
    ] + [({f: GOOD["elo_map_insert"][1][f] + 4}, "pose, keys, acc and stats must be 8-byte aligned") for f in ("pose", "keys", "acc", "stats")],
    "elo_map_merge": [
        (dict(rows=-1), "rows is 0 .. 2^31 - 1"), (dict(rows=1 << 31), "rows is 0 .. 2^31 - 1"), (dict(rows=-1, voxel=0.0), "rows is 0 .. 2^31 - 1"),
        (dict(voxel=0.0), TABLE), (dict(voxel=INF), TABLE), (dict(log2_capacity=9), TABLE), (dict(log2_capacity=29), TABLE),
        (dict(min_count=0), "min_count is >= 1"),
        (dict(centre=0x5000), "with a centre, radius is positive and finite"),
        (dict(centre=0x5000, radius=INF), "with a centre, radius is positive and finite"),
        (dict(centre=0x5000, radius=NAN), "with a centre, radius is positive and finite"),
        (dict(src_keys=None), "null pointer"), (dict(src_acc=None), "null pointer"), (dict(keys=None), "null pointer"),
        (dict(acc=None), "null pointer"), (dict(stats=None), "null pointer"), (dict(report=None), "null pointer"),
    ] + [({f: 0x6004, "radius": 1.0}, "src_keys, src_acc, keys, acc, stats, centre and report must be 8-byte aligned")
         for f in ("src_keys", "src_acc", "keys", "acc", "stats", "centre", "report")],
    "elo_scan_descriptor": [
        (dict(rings=0), SHAPE), (dict(rings=33), SHAPE), (dict(sectors=0), SHAPE), (dict(sectors=129), SHAPE), (dict(rings=0, batch=-1), SHAPE),
        (dict(batch=-1), "bad sizes: batch >= 0, H >= 1, W >= sectors"), (dict(H=0), "bad sizes: batch >= 0, H >= 1, W >= sectors"),
        (dict(W=15), "bad sizes: batch >= 0, H >= 1, W >= sectors"),
        (BIG, "batch * H * W beyond 2^31"), (WIDE, "batch * H * W beyond 2^31"),
        (dict(batch=65536), "batch beyond 65535"),
        (dict(z_step=0.0), "z_step is positive and finite, z_min finite"), (dict(z_step=INF), "z_step is positive and finite, z_min finite"),
        (dict(z_min=INF), "z_step is positive and finite, z_min finite"), (dict(z_min=NAN), "z_step is positive and finite, z_min finite"),
        (dict(min_range2=-1.0), "min_range2 is >= 0"), (dict(min_range2=NAN), "min_range2 is >= 0"),
        (dict(edge2=edges(e1=0.0)), "edge2[1 .. rings] is positive, finite and ascending"),
        (dict(edge2=edges(e3=4.0)), "edge2[1 .. rings] is positive, finite and ascending"),
        (dict(edge2=edges(e4=INF)), "edge2[1 .. rings] is positive, finite and ascending"),
        (dict(edge2=edges(e2=NAN)), "edge2[1 .. rings] is positive, finite and ascending"),
        (dict(edge2=edges(e2=NAN), xyz=None), "edge2[1 .. rings] is positive, finite and ascending"),
        (dict(xyz=None), "null pointer"), (dict(desc=None), "null pointer"),
    ],
    "elo_descriptor_search": [
        (dict(rings=0), SHAPE), (dict(rings=33), SHAPE), (dict(sectors=0), SHAPE), (dict(sectors=129), SHAPE),
        (dict(n=-1), "bad sizes: n is 0 .. 65535, m >= 0"), (dict(n=65536), "bad sizes: n is 0 .. 65535, m >= 0"),
        (dict(m=-1), "bad sizes: n is 0 .. 65535, m >= 0"),
        (dict(k=0), "k is 1 .. ELO_PLACE_MAX_K"), (dict(k=9), "k is 1 .. ELO_PLACE_MAX_K"),
        (dict(query=None), "null pointer"), (dict(db=None), "null pointer"), (dict(entry=None), "null pointer"),
        (dict(shift=None), "null pointer"), (dict(dist=None), "null pointer"),
        (dict(m=1), "null pointer"), (dict(m=1, best_shift=0x6004), "null pointer"), (dict(m=1, best_dist=0x7000), "null pointer"),
        (dict(dist=0x5004), "dist and best_dist must be 8-byte aligned"),
        (dict(m=1, best_shift=0x6004, best_dist=0x7004), "dist and best_dist must be 8-byte aligned"),
    ],
}

# what the empty block still takes: the far side of a bound, and each overlap check at its zero-length edge
ADMITTED = {
    "elo_pose_fit": [dict(iters=0), dict(jump_rel=INF), dict(jump_rel=0.0), dict(beam_elev=0x9000, vert_res=0.0), dict(H=3, W=1),
                     dict(beam_elev=0x9000, H=256), dict(batch=0, H=32768, W=65535)],
    "elo_map_fit": [dict(gate=1.0), dict(match=0xa000), dict(log2_capacity=10), dict(log2_capacity=28)],
    "elo_model_render": [dict(out_xyz=0x0ffc), dict(out_xyz=0x1004, K=16), dict(H=1, W=1)],
    "elo_map_insert": [dict(max_range=INF), dict(H=1, W=1)],
    "elo_map_merge": [dict(src_keys=0x2000, src_acc=0x1000), dict(centre=0x5000, radius=1.0), dict(radius=NAN)],
    "elo_scan_descriptor": [dict(W=16), dict(batch=0, rings=32, sectors=128, W=128), dict(z_min=0.0)],
    "elo_descriptor_search": [dict(m=5, best_shift=0x6004, best_dist=0x7000), dict(k=8)],
}


def run(entry, changed):
    struct, fields = GOOD[entry]
    block = struct(**dict(fields, **changed))
    return getattr(L.lib(), entry)(ctypes.byref(block), None)


def last_error():
    return L.lib().elo_last_error().decode()


def mark_error_text():
    """leave a known text in the thread's error buffer: an admitted block must not touch it"""
    assert L.lib().elo_pose_fit(None, None) == ERR_ARG
    assert last_error() == "elo_pose_fit: null argument block"
    return last_error()


@pytest.mark.parametrize("entry", sorted(GOOD))
def test_empty_block_is_admitted(entry):
    before = mark_error_text()
    assert run(entry, {}) == 0 and last_error() == before
    for changed in ADMITTED[entry]:
        assert run(entry, changed) == 0 and last_error() == before, changed


@pytest.mark.parametrize("entry", sorted(GOOD))
def test_null_block(entry):
    mark_error_text()
    assert getattr(L.lib(), entry)(None, None) == ERR_ARG
    assert last_error() == entry + ": null argument block"


@pytest.mark.parametrize("entry,case", [(e, i) for e in sorted(REFUSED) for i in range(len(REFUSED[e]))])
def test_refused(entry, case):
    changed, text = REFUSED[entry][case]
    mark_error_text()
    assert run(entry, changed) == ERR_ARG, changed
    assert last_error() == "%s: %s" % (entry, text), changed


def test_every_refusal_text_has_a_case():
    """the texts above are the entry points' own: every `who, "..."` of the three units that carry them appears in a case"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc")
    skipped = ("elo_map_extract", "elo_model_begin", "elo_model_advance")
    for unit in ("elo_posefit.hip", "elo_mapfit.hip", "elo_model.hip", "elo_map.hip", "elo_place.hip"):
        with open(os.path.join(csrc, unit)) as f:
            text = f.read()
        for body in re.split(r'\nextern "C" ', text)[1:]:
            who = re.search(r'const char \*who = "(\w+)"', body)
            if not who or who.group(1) in skipped:
                continue
            have = {t for _c, t in REFUSED[who.group(1)]} | {"null argument block"}
            for said in re.findall(r'who,\s*"((?:[^"\\]|\\.)*)"\s*\)', body):
                if said == "the source rows overlap the destination table":
                    continue                            # (rows > 0 only: see the module's docstring)
                assert said in have, (who.group(1), said)


@pytest.mark.parametrize("name,tile", [("elo_pose_fit", 512), ("elo_map_fit", 256)])
def test_parts_and_scratch_words(name, tile):
    parts, words = getattr(L.lib(), name + "_parts"), getattr(L.lib(), name + "_scratch_words")
    for H, W in ((2, 16), (8, 0), (0, 16), (-1, -1), (65536, 32768)):
        assert parts(H, W) == -1 and words(1, H, W) == -1
    for batch in (-1, 65536):
        assert words(batch, 8, 16) == -1
    assert words(65535, 256, 256) == -1                 # batch * H * W beyond 2^31
    for H, W in ((3, 1), (8, 16), (64, 1800), (37, 203)):
        want = (H * W + tile - 1) // tile
        assert parts(H, W) == want
        for batch in (0, 1, 3, 65535 if H * W <= 128 else 17):
            assert words(batch, H, W) == batch * want * 32 + batch
    assert parts(64, 1800) == {512: 225, 256: 450}[tile]
    assert words(2, 64, 1800) == {512: 14402, 256: 28802}[tile]


def test_model_render_scratch_words():
    words = L.lib().elo_model_render_scratch_words
    for batch, H, W in ((-1, 8, 16), (1, 0, 16), (1, 8, 0), (65535, 256, 256), (1, 65536, 32768)):
        assert words(batch, H, W) == -1
    assert words(0, 8, 16) == 0 and words(2, 64, 1800) == 2 * 2 * 64 * 1800 and words(70000, 1, 1) == 140000

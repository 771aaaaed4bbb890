"""A numpy restatement of elo_map_merge (include/elo.h), on top of tests/world_map_reference.py (merged, centroids, unpack, home): the
rule for one source row -- empty, malformed, min_count, the window's box -- and the destination's content, stats and the report
after a merge that drops nothing.  The window's decision is three IEEE operations in double per axis, so numpy reproduces it bit for
bit and the tests compare EXACTLY, on content sorted by key.
"""
import numpy as np

import world_map_reference as M

REPORT = ("voxels_merged", "voxels_filtered", "voxels_rejected", "voxels_dropped", "points_merged", "points_filtered",
          "points_dropped", "claimed")
SKIP, REJECTED, FILTERED, ROW = 0, 1, 2, 3
COUNT_CAP = 1 << 40


def box_centre(key, voxel):
    """(m,3) float64: c = ((double)i + 0.5) * (double)voxel per axis, i = the key's field - 2^20."""
    v = np.float64(np.float32(voxel))
    return np.stack([(i.astype(np.float64) + 0.5) * v for i in M.unpack(key)], -1)


def classify(key, acc, voxel, centre=None, radius=None, min_count=1):
    """The kind of every source row: key (m,) int64 (-1: an empty slot), acc (m,4) int64 -> (m,) of SKIP / REJECTED / FILTERED / ROW,
    the rule's steps in the header's order."""
    key = np.asarray(key, np.int64).reshape(-1)
    u = np.asarray(acc, np.int64).reshape(-1, 4).astype(np.uint64)
    n = u[:, 0]
    kind = np.full(len(key), ROW, np.int64)
    with np.errstate(over="ignore"):
        most = np.uint64(65535) * np.minimum(n, np.uint64(COUNT_CAP))                   # (no wrap: n is capped first)
    bad = (key < 0) | (n == 0) | (n >= np.uint64(COUNT_CAP)) | (u[:, 1:] > most[:, None]).any(-1)
    few = n < np.uint64(min_count)
    out = np.zeros(len(key), bool)
    if centre is not None:
        with np.errstate(invalid="ignore"):
            d = np.abs(box_centre(np.where(key < 0, 0, key), voxel) - np.asarray(centre, np.float64).reshape(1, 3))
            out = ~(d <= np.float64(np.float32(radius))).all(-1)                        # (a NaN centre keeps nothing)
    kind[out] = FILTERED
    kind[few] = FILTERED
    kind[bad] = REJECTED
    kind[key == -1] = SKIP
    return kind


def empty(voxel):
    return {"key": np.zeros(0, np.int64), "acc": np.zeros((0, 4), np.int64), "stats": dict.fromkeys(M.STATS, 0),
            "xyz": np.zeros((0, 3), np.float32)}


def merge(dest, key, acc, voxel, centre=None, radius=None, min_count=1):
    """The destination's content (world_map_reference.content's dict; None: an empty table) after the rows (key, acc) were merged
    into a table large enough to drop nothing -> (content, report dict).  Duplicate keys among the rows are added one by one."""
    dest = empty(voxel) if dest is None else dest
    key = np.asarray(key, np.int64).reshape(-1)
    acc = np.asarray(acc, np.int64).reshape(-1, 4)
    kind = classify(key, acc, voxel, centre, radius, min_count)
    row, cut = kind == ROW, kind == FILTERED
    rows = {"key": key[row], "acc": acc[row], "stats": dict.fromkeys(M.STATS, 0)}
    out = M.merged([dest, rows], voxel)
    points = int(acc[row, 0].sum())
    claimed = len(out["key"]) - len(dest["key"])
    out["stats"] = dict(dest["stats"], inserted=dest["stats"]["inserted"] + points, occupied=dest["stats"]["occupied"] + claimed)
    report = dict(zip(REPORT, (int(row.sum()), int(cut.sum()), int((kind == REJECTED).sum()), 0, points, int(acc[cut, 0].sum()), 0, claimed)))
    return out, report


def rows_of(content):
    """(key, acc) of a content dict: what a merge takes as its source."""
    return content["key"], content["acc"]

"""CPU: the data side of training from raw scans -- training.kitti_batches over a synthetic KITTI tree (every sample once
per epoch, remainder dropped, seeded, [pos2 | pos1] layout, augmentation with its exact inverse) -- and the C ABI of
elo_preprocess_gt (declared in include/elo.h, mirrored in _lib.py; tests/test_abi_layout_cpu.py checks the offsets)."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT, load_pkg
from kitti_tree import write_sequence

N, BATCH = 600, 2                                              # points kept per scan (8 x 64 images: ~490 valid), batch size


def _tree(tmp_path):
    root = str(tmp_path)
    T_diffs = {"04": write_sequence(root, "04", 4, 8, 64, seed=50), "05": write_sequence(root, "05", 3, 8, 64, seed=70)}
    return root, ["04", "05"], T_diffs


def _epoch(root, seqs, T_diffs, seed, **kw):
    training = load_pkg("training")
    return list(training.kitti_batches(root, seqs, T_diffs, BATCH, np.random.default_rng(seed), num_points=N, **kw))


def test_an_epoch_visits_every_sample_once_and_drops_the_remainder(tmp_path):
    kitti = load_pkg("kitti")
    root, seqs, T_diffs = _tree(tmp_path)
    table = [(seq, i) + tuple(kitti.load_pair(root, seq, i, T_diffs[seq], N)) for seq in seqs for i in range(len(T_diffs[seq]))]
    assert len(table) == 7
    batches = _epoch(root, seqs, T_diffs, 0)
    assert len(batches) == 7 // BATCH                             # the remainder (one sample) is dropped
    seen = []
    for cloud, T_gt, T_trans, T_trans_inv, aug in batches:
        assert cloud.shape == (BATCH, 2 * N, 3) and cloud.dtype == np.float32
        assert T_gt.shape == T_trans.shape == T_trans_inv.shape == (BATCH, 4, 4) and aug.shape == (BATCH,)
        assert aug.dtype == np.int32 and set(aug.tolist()) <= {1, 2}
        for j in range(BATCH):
            hit = [k for k, row in enumerate(table) if np.array_equal(cloud[j, :N], row[2].astype(np.float32))]
            assert len(hit) == 1                                  # the first half is pos2 (the sample's own scan) ...
            _seq, _i, _pos2, pos1, _n2, _n1, T = table[hit[0]]
            assert np.array_equal(cloud[j, N:], pos1.astype(np.float32))     # ... the second pos1 (the scan before it)
            assert np.array_equal(T_gt[j], T)
            seen.append(hit[0])
    assert len(set(seen)) == len(seen) == 6                       # no sample twice
    # over several epochs of one generator every sample turns up (the remainder is a different one each time)
    training = load_pkg("training")
    rng, union = np.random.default_rng(3), set()
    for _ in range(8):
        for cloud, *_rest in training.kitti_batches(root, seqs, T_diffs, BATCH, rng, num_points=N):
            union |= {k for j in range(BATCH) for k, row in enumerate(table) if np.array_equal(cloud[j, :N], row[2].astype(np.float32))}
    assert union == set(range(7))
    # batch size 7: one batch holding every sample index once; batch size 8: nothing
    (one,) = list(training.kitti_batches(root, seqs, T_diffs, 7, np.random.default_rng(1), num_points=N))
    assert sorted(k for j in range(7) for k, row in enumerate(table) if np.array_equal(one[0][j, :N], row[2].astype(np.float32))) == list(range(7))
    assert list(training.kitti_batches(root, seqs, T_diffs, 8, np.random.default_rng(1), num_points=N)) == []


def test_epochs_are_seeded(tmp_path):
    root, seqs, T_diffs = _tree(tmp_path)
    a, b, c = _epoch(root, seqs, T_diffs, 5), _epoch(root, seqs, T_diffs, 5), _epoch(root, seqs, T_diffs, 6)
    assert len(a) == len(b) == len(c) == 3
    for x, y in zip(a, b):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(a, c))          # another order ...
    assert all(not np.array_equal(x[2], y[2]) for x, y in zip(a, c))          # ... and other augmentations
    # a list of T_diff arrays in the order of `seqs` is the dictionary
    d = _epoch(root, seqs, [T_diffs[s] for s in seqs], 5)
    assert all(np.array_equal(u, v) for x, y in zip(a, d) for u, v in zip(x, y))


def test_augmentation_comes_with_its_inverse(tmp_path):
    root, seqs, T_diffs = _tree(tmp_path)
    eye = np.tile(np.eye(4), (BATCH, 1, 1))
    for _cloud, _T_gt, T_trans, T_trans_inv, _aug in _epoch(root, seqs, T_diffs, 2):
        assert T_trans.dtype == np.float64
        assert np.abs(T_trans_inv @ T_trans - eye).max() <= 1e-12
        assert np.abs(T_trans - eye).max() > 1e-4                 # a real draw of data_augmentation, per sample
        assert not np.array_equal(T_trans[0], T_trans[1])
    for _cloud, _T_gt, T_trans, T_trans_inv, aug in _epoch(root, seqs, T_diffs, 2, augment=False):
        assert np.array_equal(T_trans, eye) and np.array_equal(T_trans_inv, eye) and set(aug.tolist()) <= {1, 2}


def test_preprocess_gt_is_declared_and_mirrored():
    L = load_pkg("_lib")
    with open(os.path.join(ROOT, "include", "elo.h")) as f:
        header = f.read()
    assert re.search(r"int\s+elo_preprocess_gt\s*\(\s*const\s+elo_preprocess_gt_args\s*\*\s*a\s*,\s*elo_stream_t\s+stream\s*\)\s*;", header)
    body = re.search(r"typedef struct elo_preprocess_gt_args \{(.*?)\} elo_preprocess_gt_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"^.*[\s*]", "", d.strip()) for d in body.split(";") if d.strip()]
    mirror = L.PreprocessGtArgs
    assert issubclass(mirror, ctypes.Structure) and mirror.__name__ == "elo_preprocess_gt_args"
    assert [name for name, _ in mirror._fields_] == declared == ["batch", "T_gt", "T_trans", "T_trans_inv", "aug_frame", "q_gt", "t_gt"]
    assert ("elo_preprocess_gt", ctypes.c_int, [ctypes.POINTER(mirror), ctypes.c_void_p]) in L.SYMBOLS
    assert L.ABI_VERSION == 26                                    # additive: no existing struct moved

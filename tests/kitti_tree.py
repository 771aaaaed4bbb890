"""A synthetic KITTI odometry tree for the tests of the training data path: <root>/<seq>/velodyne/NNNNNN.bin + calib.txt,
written the way tests/test_evaluate_gpu.py writes its sequence, and the sequence's frame-to-previous-frame transforms."""
import os

import numpy as np

from conftest import load_pkg

TR = np.array([4.276802385584e-04, -9.999672484946e-01, -8.084491683471e-03, -1.198459927713e-02,
               -7.210626507497e-03, 8.081198471645e-03, -9.999413164504e-01, -5.403984729748e-02,
               9.999738645903e-01, 4.859485810390e-04, -7.206933692422e-03, -2.921968648686e-01])   # KITTI-style Tr


def write_sequence(root, seq, n_frames, H, W, seed=50):
    """-> T_diff (n_frames, 12).  Scan i is the valid pixels of a synthetic H x W range image moved 0.8 m forward per frame."""
    synth, kitti = load_pkg("synth"), load_pkg("kitti")
    d = os.path.join(root, seq, "velodyne")
    os.makedirs(d)
    with open(os.path.join(root, seq, "calib.txt"), "w") as f:
        f.write("P0: 1 0 0 0 0 1 0 0 0 0 1 0\nTr: " + " ".join("%.12e" % v for v in TR) + "\n")
    poses = []
    for i in range(n_frames):
        img = synth.range_image(H, W, seed=seed + i, yaw=0.01 * i, shift=(0.8 * i, 0.0, 0.0))
        pts = img.reshape(-1, 3)
        pts = pts[np.any(pts != 0, -1)]
        np.concatenate([pts, np.ones((len(pts), 1), np.float32)], 1).astype(np.float32).tofile(
            os.path.join(d, "%06d.bin" % i))
        P = np.eye(4)
        P[2, 3] = 0.8 * i                                   # camera z forward
        poses.append(P[:3].reshape(12))
    return kitti.relative_from_absolute(np.stack(poses))

"""GPU: elo_pose_fit (csrc/elo_posefit.hip) against the float64 statement of tests/pose_fit_reference.py.

The scenes are the ones tests/test_pose_fit_cpu.py vets: every frame-1 point whose discrete decisions (cell borders, gate, range
jumps, the normal's orientation) lie within 1e-3 of their own scale was removed, so kernel and reference compare the SAME terms
and `count` is equal exactly.

The bound on a sum.  The kernel forms every product of a term in double and rounds it to float32 once; the float32 additions that
follow are, in the kernel's reduction order,
    a thread over its strip      ceil(H W / parts / 256) cells, parts = elo_pose_fit_parts(H, W) workgroups per image
    a wave by DPP                log2(64) = 6 steps
    the waves of a workgroup     256 / 64 - 1 = 3 additions
and the partial rows of the workgroups are added in double.  n = strip + 6 + 3 is the longest chain of float32 additions a term
goes through; |error| <= (n + 16) 2^-24 sum |terms|  (the standard bound for n additions, plus the term's own rounding, the
rounding of the reported float32 and slack, 16 in all)."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pose_fit_reference as R
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
TRIU = np.triu_indices(6)


def _fit(**kw):
    return load_pkg("sensor").PoseFit(**dict(R.FIT, **kw))


def _chain(H, W):
    parts = load_pkg("_lib").lib().elo_pose_fit_parts(H, W)
    assert parts >= 1
    return math.ceil(H * W / parts / 256) + 6 + 3, parts


@functools.lru_cache(maxsize=None)
def _case(i):
    """(x1, x2, poses, consts, beam, [reference evaluation per image]) of scene i (len(SHAPES): the beam-table sensor), once."""
    if i < len(R.SHAPES):
        x1, x2, poses, c, beam, _dropped = R.filtered_case(*R.SHAPES[i])
    else:
        x1, x2, poses, c, beam, _dropped = R.filtered_case(2, 16, 128, False, R.BEAMS_DEG)
    want = [R.evaluate(x1[b], x2[b], poses[b], c, beam_elev=beam, **R.FIT) for b in range(len(x1))]
    return x1, x2, poses, c, beam, want


def _run(x1, x2, poses, beam=None, **kw):
    ops, S = load_pkg("_scan_ops"), load_pkg("sensor")
    sensor = None if beam is None else S.Sensor(beam_elevations_deg=R.BEAMS_DEG)
    res = ops.pose_fit(t(x1), t(x2), t(poses), _fit(**kw), sensor=sensor)
    torch.cuda.synchronize()
    return res


def _compare(res, want, H, W):
    n, _parts = _chain(H, W)
    eps = (n + 16) * 2.0 ** -24
    info, grad, stats = (x.cpu().numpy().astype(np.float64) for x in (res.info, res.grad, res.stats))
    for b, ev in enumerate(want):
        dA, db, dc = np.abs(info[b] - ev["A"]), np.abs(grad[b] - ev["b"]), abs(stats[b, 1] - ev["cost"])
        print("image %d: count %d (reference %d); worst share of the bound: A %.3g, b %.3g; cost off by %.3g, bound %.3g" % (
            b, stats[b, 0], ev["count"], (dA / np.maximum(eps * ev["absA"], 1e-300)).max(),
            (db / np.maximum(eps * ev["absb"], 1e-300)).max(), dc, eps * ev["abscost"]))
        assert stats[b, 0] == ev["count"]
        assert (dA <= eps * ev["absA"]).all() and (db <= eps * ev["absb"]).all() and dc <= eps * ev["abscost"]
        assert np.array_equal(info[b], info[b].T)
        rms = math.sqrt(ev["cost"] / ev["sw"]) if ev["sw"] > 0 else 0.0
        assert abs(stats[b, 2] - rms) <= 1e-5 * rms            # (both sums within eps of float64, the root, one float32 rounding)


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_one_evaluation_against_float64(i):
    x1, x2, poses, _c, _beam, want = _case(i)
    B, H, W, starved = R.SHAPES[i]
    _n, parts = _chain(H, W)
    assert parts > 1 or i == 2                                                        # several workgroups per image at the two larger shapes
    res = _run(x1, x2, poses)
    _compare(res, want, H, W)
    assert torch.equal(res.pose.view(torch.int32), t(poses).view(torch.int32))        # iters = 0: pose_out is pose_in, bits
    status = res.status.cpu().numpy()
    assert (status[:B - 1] == 0).all() and status[B - 1] == (4 if starved else 0)


def test_a_starved_image_is_flagged_and_leaks_no_nan():
    L = load_pkg("_lib")
    x1, x2, poses, _c, _beam, want = _case(1)
    assert want[-1]["count"] == 0
    for iters in (0, 2):
        res = _run(x1, x2, poses, iters=iters)
        for x in (res.pose, res.info, res.grad, res.stats):
            assert torch.isfinite(x).all()
        status = res.status.cpu().numpy().astype(np.int64)
        assert status[-1] == (L.FIT_FEW_FINAL if iters == 0 else L.FIT_FEW | L.FIT_FEW_FINAL) and (status[:-1] == 0).all()
        assert torch.equal(res.pose[-1].view(torch.int32), t(poses[-1]).view(torch.int32))      # left exactly as it came
        assert float(res.count[-1]) == 0 and float(res.rms[-1]) == 0 and not res.info[-1].any()
        if iters:
            assert not torch.equal(res.pose[0], t(poses[0]))                                    # the others moved
    cov = _run(x1, x2, poses).covariance()
    assert np.isnan(cov[-1]).all() and np.isfinite(cov[:-1]).all() and (np.linalg.eigvalsh(cov[0]) > 0).all()


def test_seam_columns_count_and_edge_rows_do_not():
    """Frame 1 cut down to the points that fall into columns 0 and W-1 of frame 2 -- their normals reach across the wrap -- and,
    second, to the points that fall into rows 0 and H-1, where there is no normal: nothing may be counted."""
    x1, x2, poses, c, _beam, _want = _case(0)
    B, H, W, _ = R.SHAPES[0]
    seam, edge = np.zeros_like(x1), np.zeros_like(x1)
    for b in range(B):
        _q, Rm, tr = R.split_pose(poses[b])
        src = np.flatnonzero(x1[b].any(-1).reshape(-1))
        row, col, _m = R.cells(x1[b].reshape(-1, 3)[src].astype(np.float64) @ Rm.T + tr, H, W, c)
        for keep, dst in (((col == 0) | (col == W - 1), seam), ((row == 0) | (row == H - 1), edge)):
            dst[b].reshape(-1, 3)[src[keep]] = x1[b].reshape(-1, 3)[src[keep]]
    want = [R.evaluate(seam[b], x2[b], poses[b], c, **R.FIT) for b in range(B)]
    assert all(ev["count"] >= 8 for ev in want)
    _compare(_run(seam, x2, poses), want, H, W)
    assert all(edge[b].any() for b in range(B))
    res = _run(edge, x2, poses)
    assert not res.count.any() and not res.info.any() and not res.grad.any() and not res.cost.any()


def test_beam_table_rows():
    x1, x2, poses, _c, beam, want = _case(len(R.SHAPES))
    assert all(ev["count"] >= 50 for ev in want)
    res = _run(x1, x2, poses, beam=beam)
    _compare(res, want, 16, 128)
    plain = _run(x1, x2, poses)                                   # the uniform formula puts these beams into other rows
    assert not torch.equal(plain.info, res.info)


def test_two_calls_agree_bit_for_bit():
    x1, x2, poses, _c, _beam, _want = _case(1)
    for iters in (0, 2):
        a, b = _run(x1, x2, poses, iters=iters), _run(x1, x2, poses, iters=iters)
        for u, v in zip((a.pose, a.info, a.grad, a.stats), (b.pose, b.info, b.grad, b.stats)):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_polish_reaches_the_reference_fixed_point():
    """Started 0.1 m / 0.76 degrees off the reference's own fixed point, the kernel after k steps is no further from it than the
    reference after k - 1 (tests/test_pose_fit_cpu.py checks that the reference's step k at least halves its error: the room left
    for the association flips of float32)."""
    f1, f2 = R.scene(3, 32, 256)
    starts, fixed, ref = [], [], []
    for b in range(2):
        fx, st, errs = R.polish_case(b)
        starts.append(st); fixed.append(fx); ref.append(errs)
    starts.append(starts[0])
    res = _run(f1, f2, np.stack(starts), iters=R.POLISH_K)
    got = res.pose.cpu().numpy()
    assert not res.status.any()
    for b in range(2):
        err = R.pose_error(got[b], fixed[b])
        print("image %d: kernel %.3g after %d steps; reference %s" % (b, err, R.POLISH_K, ["%.3g" % e for e in ref[b]]))
        assert err <= ref[b][R.POLISH_K - 1]
    # info / grad / stats are those of the LAST evaluation, at pose_out
    at = _run(f1, f2, got)
    assert torch.equal(at.info, res.info) and torch.equal(at.grad, res.grad) and torch.equal(at.stats, res.stats)


def test_abi_refusals_launch_nothing():
    L = load_pkg("_lib")
    lib = L.lib()
    B, H, W = 1, 8, 64
    x = torch.ones((B, H, W, 3), device=DEV)
    pose = t(np.array([[1, 0, 0, 0, 0, 0, 0]], np.float32))
    beam = torch.linspace(0.1, -0.4, 300, device=DEV)
    outs = [torch.full(s, -7.0, device=DEV) for s in ((B, 7), (B, 6, 6), (B, 6), (B, 4))]
    scratch = torch.full((lib.elo_pose_fit_scratch_words(B, H, W),), -7, dtype=torch.int32, device=DEV)
    az, vres, voff = R.constants(H, W)

    def args(**kw):
        a = L.PoseFitArgs(B, H, W, az, vres, voff, x.data_ptr(), x.data_ptr(), pose.data_ptr(), None, 0, 1.0, 0.1, 0.1, 50, 0.0,
                          *(o.data_ptr() for o in outs), scratch.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = L.stream_ptr(x)
    for bad in (dict(xyz1=None), dict(xyz2=None), dict(pose_in=None), dict(H=2), dict(gate=0.0), dict(gate=-1.0), dict(huber=0.0),
                dict(huber=float("nan")), dict(iters=-1), dict(H=300, beam_elev=beam.data_ptr()), dict(pose_out=None),
                dict(scratch=None), dict(pose_out=pose.data_ptr()), dict(damping=-1.0)):
        assert lib.elo_pose_fit(ctypes.byref(args(**bad)), stream) == -1, bad               # ELO_ERR_ARG
        assert b"elo_pose_fit" in lib.elo_last_error()
    torch.cuda.synchronize()
    assert all((o == -7.0).all() for o in outs) and (scratch == -7).all()                   # nothing ran
    assert lib.elo_pose_fit_scratch_words(B, 2, W) < 0
    assert lib.elo_pose_fit(ctypes.byref(args()), stream) == 0                              # the same block, mended, runs
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() and not (o == -7.0).all() for o in outs)


def test_through_the_net_eager_and_replayed():
    """tests/pose_fit_net_replay.py in a child process (its captures take streams from the process-wide pool and bind hardware
    queues, which in this process would move the lanes of every later test of the suite): forward(fit=) against _scan_ops.pose_fit,
    capture(fit=) + submit + lane_fit against the eager result, a plain graph replay of the entry against its eager call,
    capture(fit=None) against today's outputs, the sequence evaluation's fit file."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pose_fit_net_replay.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pose fit through the net: ok" in out.stdout

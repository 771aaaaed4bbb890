"""GPU: the tracker state on the device (csrc/elo_model_state.hip: elo_model_begin / elo_model_advance) and the tracker built on it
(local_model.DeviceTracker; evaluate.predict_sequence(model=LocalModel(resident=True))).

Every step is compared with a statement made BY HAND from the state read back before it: the ring, the state words and the fit's
result bit for bit (the launches copy, count and call the kernels the by-hand statement calls), the re-based poses within 1e-12 of
the float64 numpy re-basing (tests/local_model_reference.py: the bound the project holds its torch re-basing to), per step.  The
state transitions themselves are those of tests/device_tracker_reference.py, which tests/test_device_tracker_cpu.py vets."""
import ctypes

import numpy as np
import pytest
import torch

import device_tracker_reference as D
import local_model_reference as M
import pose_fit_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
bits = lambda x: x.contiguous().view(torch.int32)
IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
H, W = M.BOX_H, M.BOX_W


def _pkgs():
    return load_pkg("_scan_ops"), load_pkg("sensor"), load_pkg("_lib"), load_pkg("local_model")


def _fit(S, iters=2):
    return S.PoseFit(iters=iters, **R.FIT)


def _box():
    return [(t(x1[None]), t(x2[None]), t(p[None])) for x1, x2, p in M.box_pairs()]


def _same_result(a, b):
    return all(torch.equal(bits(u), bits(v)) for u, v in zip((a.pose, a.info, a.grad, a.stats), (b.pose, b.info, b.grad, b.stats)))


def _keep(res):
    """A copy of a result (a captured tracker's is overwritten by its next step)."""
    return load_pkg("_scan_ops").PoseFitResult(res.pose.clone(), res.info.clone(), res.grad.clone(), res.stats.clone())


def _snapshot(tr):
    torch.cuda.synchronize()
    return dict(ring=tr.ring.clone(), poses64=tr.poses64.clone(), poses32=tr.poses32.clone(), state=tuple(int(v) for v in tr.state.cpu()))


def _same_state(a, b):
    return (torch.equal(bits(a.ring), bits(b.ring)) and torch.equal(a.poses64.view(torch.int64), b.poses64.view(torch.int64))
            and torch.equal(bits(a.poses32), bits(b.poses32)) and torch.equal(a.state, b.state))


def _is_reset(tr):
    K = tr.model.scans
    ident = t(np.tile(IDENTITY, (K, 1)))
    return (not bits(tr.ring).any() and torch.equal(tr.poses64, ident.double()) and torch.equal(bits(tr.poses32), bits(ident))
            and tr.state.tolist() == [0, 0] and tr.held() == 0 and tr.next_slot() == 0)


def _check_step(tr, before, x1, x2, pose7, res, fit, sensor=None):
    """One step against the statement made by hand from `before`, the state read back ahead of it: (a) - (e) of the module's
    docstring order -- result, ring and state, re-based poses, the entered row, the float32 copy.  -> the by-hand fit."""
    ops = load_pkg("_scan_ops")
    K = tr.model.scans
    torch.cuda.synchronize()
    nxt, held = before["state"]
    ring = before["ring"].clone()
    if held == 0:
        ring[0] = x2[0]                                       # the first frame 2 starts the model in slot 0, at the identity
    model, _src = ops.model_render(ring.unsqueeze(0), before["poses32"].unsqueeze(0).contiguous(), sensor=sensor)
    hand = ops.pose_fit(x1, model, pose7, fit, sensor=sensor)
    torch.cuda.synchronize()
    assert _same_result(res, hand)                                                      # (a)
    slot, found = D.entry(nxt, held, K)
    ring[slot] = x1[0]
    assert torch.equal(bits(tr.ring), bits(ring))                                       # (b)
    assert tuple(tr.state.tolist()) == D.after(nxt, held, K) == ((slot + 1) % K, min(found + 1, K))
    assert (tr.next_slot(), tr.held()) == D.after(nxt, held, K)
    want = M.rebase(before["poses64"].cpu().numpy(), res.pose[0].cpu().numpy())         # by the step's own returned float32 pose
    want[slot] = IDENTITY
    got = tr.poses64.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-12                                            # (c)
    assert np.array_equal(got[slot], IDENTITY.astype(np.float64)) and not np.signbit(got[slot]).any()    # (d)
    assert torch.equal(bits(tr.poses32), bits(tr.poses64.to(torch.float32)))            # (e)
    return hand


@pytest.mark.parametrize("K", (1, 3, 4))
def test_state_against_a_by_hand_statement_every_step(K):
    """The box scene's five pairs enter six scans: every K wraps its cursor, K = 3 at a non-power of two."""
    ops, S, L, lm = _pkgs()
    fit = _fit(S)
    tr = lm.DeviceTracker(H, W, S.LocalModel(K, resident=True), fit, device=DEV)
    assert _is_reset(tr) and tr.launches() == 6 + 2 * 3
    for n, (x1, x2, pose7) in enumerate(_box()):
        before = _snapshot(tr)
        res = tr.step(x1, x2, pose7)
        _check_step(tr, before, x1, x2, pose7, res, fit)
        pair = ops.pose_fit(x1, x2, pose7, fit)
        torch.cuda.synchronize()
        cm, cp, sm, sp = (int(v) for v in (res.count[0], pair.count[0], res.status[0], pair.status[0]))
        print("K = %d step %d: state %s -> %s; terms %d against the model, %d against the pair; status %d / %d" % (
            K, n, before["state"], tuple(tr.state.tolist()), cm, cp, sm, sp))
        assert tr.held() == min(n + 2, K)
        if K == 4 and n >= 2:                                 # (tests/test_local_model_gpu.py's statement of the host tracker)
            assert cm > cp and sm == 0 and (sp & L.FIT_FEW)


def test_one_scan_is_the_pair_fit():
    ops, S, _L, lm = _pkgs()
    fit = _fit(S)
    dev_tr = lm.DeviceTracker(H, W, S.LocalModel(1, resident=True), fit, device=DEV)
    host_tr = lm.ModelTracker(H, W, S.LocalModel(1), fit, device=DEV)
    for n, (x1, x2, pose7) in enumerate(_box()):
        res, host, pair = dev_tr.step(x1, x2, pose7), host_tr.step(x1, x2, pose7), ops.pose_fit(x1, x2, pose7, fit)
        torch.cuda.synchronize()
        assert _same_result(res, pair), n
        assert _same_result(res, host), n
        assert torch.equal(dev_tr.poses64, host_tr.poses64) and torch.equal(bits(dev_tr.ring), bits(host_tr.ring))
        assert dev_tr.state.tolist() == [0, 1]


def test_a_replay_is_the_enqueue():
    _ops, S, _L, lm = _pkgs()
    fit = _fit(S)
    model = S.LocalModel(3, resident=True)
    eager, replayed = lm.DeviceTracker(H, W, model, fit, device=DEV), lm.DeviceTracker(H, W, model, fit, device=DEV)
    with pytest.raises(RuntimeError):
        replayed.inputs()
    pairs = _box()
    replayed.step(*pairs[2])                                  # a state to forget: capture() leaves the reset state
    assert replayed.capture() is replayed
    torch.cuda.synchronize()
    assert _is_reset(replayed)                                # the warm-up did not leak, nor what was there before
    assert [tuple(x.shape) for x in replayed.inputs()] == [(1, H, W, 3), (1, H, W, 3), (1, 7)]
    first = []
    for x1, x2, pose7 in pairs:
        a, b = eager.step(x1, x2, pose7), replayed.step(x1, x2, pose7)
        torch.cuda.synchronize()
        assert b is replayed._result                          # the static result
        assert _same_result(a, b) and _same_state(eager, replayed)
        first.append(_keep(b))
    replayed.capture()                                        # capturing twice gives the same
    torch.cuda.synchronize()
    assert _is_reset(replayed)
    eager.reset()
    for n, (x1, x2, pose7) in enumerate(pairs):
        a, b = eager.step(x1, x2, pose7), replayed.step(x1, x2, pose7)
        torch.cuda.synchronize()
        assert _same_result(a, b) and _same_result(b, first[n]) and _same_state(eager, replayed)
    # a producer on the device writes the static inputs in place
    replayed.reset()
    for dst, src in zip(replayed.inputs(), pairs[0]):
        dst.copy_(src)
    replayed._graph.replay()
    torch.cuda.synchronize()
    assert _same_result(replayed._result, first[0])


def _random_pairs(h, w, n, seed):
    """n consecutive pairs of random half-empty (h,w,3) images: pair k = (scan k+1, scan k)."""
    rng = np.random.default_rng(seed)
    scans = []
    for _ in range(n + 1):
        img = rng.uniform(-20.0, 20.0, (h, w, 3)).astype(np.float32)
        img[rng.random((h, w)) < 0.5] = 0.0
        scans.append(img)
    return [(scans[k + 1], scans[k], IDENTITY) for k in range(n)]


@pytest.mark.parametrize("case", ("vector", "scalar", "unaligned"))
def test_copy_paths(case):
    """vector: H W % 4 == 0 and aligned pointers, 16-byte accesses.  scalar: a 5 x 7 image, H W = 35.  unaligned: the box images as
    views one float into a larger buffer -- H W % 4 == 0, but the pointer is not 16-byte aligned.  Three steps each, K = 2: the
    cursor wraps.  Empty cells stay exact zeros."""
    _ops, S, _L, lm = _pkgs()
    fit = _fit(S)
    if case == "scalar":
        h, w, pairs = 5, 7, _random_pairs(5, 7, 3, seed=5)
    else:
        h, w, pairs = H, W, M.box_pairs()[:3]
    assert (h * w % 4 == 0) == (case != "scalar")

    def place(img):
        if case != "unaligned":
            out = t(img[None])
            assert out.data_ptr() % 16 == 0
            return out
        buf = torch.zeros(img.size + 4, device=DEV)
        view = buf[1:1 + img.size].view(1, h, w, 3)
        view.copy_(t(img[None]))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    tr = lm.DeviceTracker(h, w, S.LocalModel(2, resident=True), fit, device=DEV)
    for x1, x2, pose7 in pairs:
        before = _snapshot(tr)
        d1, d2, dp = place(x1), place(x2), t(pose7[None])
        res = tr.enqueue(d1, d2, dp)
        _check_step(tr, before, d1, d2, dp, res, fit)
        slot = D.entry(*before["state"], 2)[0]
        empty = t(~x1.any(-1))
        assert empty.any() and not empty.all()
        assert not bits(tr.ring[slot])[empty].any()           # zeros, every bit
        assert torch.equal(bits(tr.ring[slot]), bits(d1[0]))
    assert tr.state.tolist() == [0, 2]


def test_reset_mid_drive():
    _ops, S, _L, lm = _pkgs()
    fit = _fit(S)
    K = 4
    pairs = _box()
    tr, fresh = lm.DeviceTracker(H, W, S.LocalModel(K, resident=True), fit, device=DEV), \
        lm.DeviceTracker(H, W, S.LocalModel(K, resident=True), fit, device=DEV)
    for pair in pairs[:3]:
        tr.step(*pair)
    torch.cuda.synchronize()
    assert tr.held() == 4 and not _is_reset(tr)
    tr.reset()
    torch.cuda.synchronize()
    assert _is_reset(tr)
    a, b = tr.step(*pairs[3]), fresh.step(*pairs[3])
    torch.cuda.synchronize()
    assert _same_result(a, b) and _same_state(tr, fresh)
    assert torch.equal(bits(tr.ring[0]), bits(pairs[3][1][0])) and torch.equal(bits(tr.ring[1]), bits(pairs[3][0][0]))
    assert not bits(tr.ring[2:]).any() and tr.state.tolist() == [2, 2]
    tr.reset()                                                # (slots 1 .. K-1 are zero once the first frame 2 is in)
    load_pkg("_scan_ops").model_begin(tr.ring, tr.state, pairs[0][1][0])
    torch.cuda.synchronize()
    assert torch.equal(bits(tr.ring[0]), bits(pairs[0][1][0])) and not bits(tr.ring[1:]).any() and tr.state.tolist() == [0, 0]


def test_abi_refusals_launch_nothing():
    L = load_pkg("_lib")
    lib = L.lib()
    K, h, w = 2, 8, 64
    ring = torch.full((K, h, w, 3), -7.0, device=DEV)
    poses64 = torch.full((K, 7), -7.0, dtype=torch.float64, device=DEV)
    poses32 = torch.full((K, 7), -7.0, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)     # {0, 0}: a launch that ran WOULD write slot 0, the poses and the state
    image = torch.ones((h, w, 3), device=DEV)
    T = t(IDENTITY)

    def begin(**kw):
        a = L.ModelBeginArgs(K, h, w, ring.data_ptr(), state.data_ptr(), image.data_ptr())
        for k, v in kw.items():
            setattr(a, "first" if k == "scan" else k, v)
        return a

    def advance(**kw):
        a = L.ModelAdvanceArgs(K, h, w, ring.data_ptr(), poses64.data_ptr(), poses32.data_ptr(), state.data_ptr(), image.data_ptr(),
                               T.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    stream = L.stream_ptr(ring)
    shared = (dict(ring=None), dict(state=None), dict(scan=None), dict(K=0), dict(K=17), dict(H=2), dict(W=0), dict(H=-1),
              dict(H=1 << 16, W=1 << 16), dict(K=16, H=1 << 14, W=1 << 13),       # H W, K H W at or beyond 2^31: fit / render bounds
              dict(scan=ring.data_ptr()), dict(scan=ring.data_ptr() + 12 * h * w),          # the second slot: inside the ring
              dict(scan=ring.data_ptr() - 12), dict(scan=ring.data_ptr() + 12 * (K * h * w - 1)))   # one cell over either end
    for entry, args, more in ((lib.elo_model_begin, begin, ()),
                              (lib.elo_model_advance, advance, (dict(poses64=None), dict(poses32=None), dict(T=None)))):
        assert entry(None, stream) == -1
        for bad in shared + more:
            assert entry(ctypes.byref(args(**bad)), stream) == -1, bad                      # ELO_ERR_ARG
            assert entry.__name__.encode() in lib.elo_last_error()
    torch.cuda.synchronize()
    assert (ring == -7.0).all() and (poses64 == -7.0).all() and (poses32 == -7.0).all() and state.tolist() == [0, 0]    # nothing ran
    # a state outside its domain: the launches run and write nothing
    state.copy_(torch.tensor([K, 1], dtype=torch.int32))
    assert lib.elo_model_begin(ctypes.byref(begin()), stream) == 0 and lib.elo_model_advance(ctypes.byref(advance()), stream) == 0
    torch.cuda.synchronize()
    assert (ring == -7.0).all() and (poses64 == -7.0).all() and (poses32 == -7.0).all() and state.tolist() == [K, 1]
    # the same blocks, mended, run
    state.zero_()
    poses64.copy_(t(np.tile(IDENTITY, (K, 1))).double())
    assert lib.elo_model_begin(ctypes.byref(begin()), stream) == 0
    torch.cuda.synchronize()
    assert (ring[0] == 1.0).all() and (ring[1] == -7.0).all() and state.tolist() == [0, 0]
    assert lib.elo_model_advance(ctypes.byref(advance()), stream) == 0
    torch.cuda.synchronize()
    assert (ring == 1.0).all() and state.tolist() == [0, 2]
    assert torch.equal(poses64, t(np.tile(IDENTITY, (K, 1))).double()) and torch.equal(poses32, poses64.float())


# ---- through the evaluator ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """A five-scan 64 x 900 tree (tests/kitti_tree.py), one net for the sequential path and one for the lanes, and the runs made so
    far: every predict_sequence of these tests is computed once."""
    import kitti_tree
    root = str(tmp_path_factory.mktemp("tracker_tree"))
    T_diff = kitti_tree.write_sequence(root, "04", 5, 64, 900)
    model = load_pkg("model")
    nets = {False: model.PWCLONet(DEV, seed=0), True: model.PWCLONet(DEV, seed=0)}
    runs = {}

    def run(frames=None, lanes=0, scans=None):
        key = (None if frames is None else tuple(frames), lanes, scans)
        if key not in runs:
            ev, S = load_pkg("evaluate"), load_pkg("sensor")
            kw = dict(H_input=64, W_input=900, num_points=64 * 900, batch_size=2, frames=frames, lanes=lanes, fit=S.PoseFit(iters=1))
            if scans is not None:
                kw["model"] = S.LocalModel(scans, resident=True)
            runs[key] = ev.predict_sequence(nets[lanes > 0], root, "04", T_diff, **kw)
        return runs[key]

    return run


def _equal_runs(a, b, n):
    assert a[0].shape == b[0].shape == (n, 4) and a[2].shape == b[2].shape == (n, 24)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert (a[2][:, 0] >= 50).all()                           # (the fit did run: these scans are dense)


@pytest.mark.parametrize("frames", (None, [0, 1, 3, 4]))
def test_lanes_feed_the_tracker_one_scan_is_the_pair_fit(sequence, frames):
    """Across the gap in `frames` only the reset keeps the model from holding the wrong scan."""
    _equal_runs(sequence(frames, lanes=2, scans=1), sequence(frames, lanes=2), 5 if frames is None else 4)


def test_sequential_path_one_scan_is_the_pair_fit(sequence):
    _equal_runs(sequence(scans=1), sequence(), 5)
    _equal_runs(sequence(scans=1), sequence(lanes=2, scans=1), 5)


def test_lanes_and_sequential_path_agree_on_four_scans(sequence):
    """The same tracker, the same inputs, the same order."""
    _equal_runs(sequence(lanes=2, scans=4), sequence(scans=4), 5)
    assert not np.array_equal(sequence(scans=4)[2], sequence()[2])       # (a model of four scans is not the pair)

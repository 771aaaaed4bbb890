"""CPU: the tracker state on the device as far as it can be checked without one -- the LocalModel(resident=) value, the ctypes
mirror of elo_model_begin_args / elo_model_advance_args against include/elo.h, the host's refusals of _scan_ops.model_begin /
_scan_ops.model_advance (before the library is touched), DeviceTracker's and predict_sequence's argument errors, and the numpy state
machine tests/test_device_tracker_gpu.py compares the kernels with (tests/device_tracker_reference.py) against a plain list of "the
last K scans"."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import device_tracker_reference as D
from conftest import ROOT, load_pkg


def test_local_model_resident_value():
    S = load_pkg("sensor")
    m, r = S.LocalModel(), S.LocalModel(resident=True)
    assert m.resident is False and r.resident is True and r.scans == 4
    assert m != r and r == S.LocalModel(4, True) and hash(r) == hash(S.LocalModel(scans=4, resident=True))
    assert len({m, r, S.LocalModel(4), S.LocalModel(4, resident=True)}) == 2 and r != S.LocalModel(3, resident=True)
    assert repr(m) == "LocalModel(scans=4)" and repr(S.LocalModel(2, resident=False)) == "LocalModel(scans=2)"       # unchanged while False
    assert "resident=True" in repr(r) and "scans=4" in repr(r)
    for name in ("resident", "scans"):
        with pytest.raises(AttributeError):
            setattr(r, name, 1)
        with pytest.raises(AttributeError):
            delattr(r, name)
    for bad in (1, 0, None, "yes", np.bool_(True)):
        with pytest.raises(ValueError):
            S.LocalModel(4, resident=bad)
    for bad in (0, 17, True, 2.0):
        with pytest.raises(ValueError):
            S.LocalModel(bad, resident=True)


def _declared_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            out += [re.sub(r"^.*[\s*]", "", field.strip()) for field in decl.split(",")]
    return out


def test_the_argument_blocks_are_declared_and_mirrored(tmp_path):
    L = load_pkg("_lib")
    with open(os.path.join(ROOT, "include", "elo.h")) as f:
        header = f.read()
    want = {"elo_model_begin": (L.ModelBeginArgs, ["K", "H", "W", "ring", "state", "first"]),
            "elo_model_advance": (L.ModelAdvanceArgs, ["K", "H", "W", "ring", "poses64", "poses32", "state", "scan", "T"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "elo.h"', 'int main(void) {']
    for entry, (mirror, fields) in want.items():
        struct = entry + "_args"
        assert re.search(r"^int %s\(const %s \*a, elo_stream_t stream\);" % (entry, struct), header, re.M)
        assert mirror.__name__ == struct                                                # (tests/test_abi_layout_cpu.py finds it by this name)
        assert [n for n, _ in mirror._fields_] == _declared_fields(header, struct) == fields
        assert all(t is (ctypes.c_int if n in "KHW" else ctypes.c_void_p) for n, t in mirror._fields_)
        assert (entry, ctypes.c_int, [ctypes.POINTER(mirror), ctypes.c_void_p]) in L.SYMBOLS
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (struct, struct))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (struct, n, struct, n) for n in fields]
    assert L.ABI_VERSION == 26                                                          # additive: no existing struct moved
    assert int(re.search(r"#define\s+ELO_MODEL_MAX_SCANS\s+(\d+)", header).group(1)) == L.MODEL_MAX_SCANS
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    sizes = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for entry, (mirror, fields) in want.items():
        assert ctypes.sizeof(mirror) == int(sizes[entry + "_args"])
        for n in fields:
            assert getattr(mirror, n).offset == int(sizes["%s_args.%s" % (entry, n)]), (entry, n)


def test_host_refusals_come_before_the_library(monkeypatch):
    ops, L, S, lm = load_pkg("_scan_ops"), load_pkg("_lib"), load_pkg("sensor"), load_pkg("local_model")

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "lib", no_library)
    K, H, W = 3, 8, 16
    good = dict(ring=torch.zeros((K, H, W, 3)), poses64=torch.zeros((K, 7), dtype=torch.float64), poses32=torch.zeros((K, 7)),
                state=torch.zeros(2, dtype=torch.int32), scan=torch.zeros((H, W, 3)), T=torch.zeros(7))

    def begin(**kw):
        a = {**good, **kw}
        ops.model_begin(a["ring"], a["state"], a["scan"])

    def advance(**kw):
        a = {**good, **kw}
        ops.model_advance(a["ring"], a["poses64"], a["poses32"], a["state"], a["scan"], a["T"])

    for call in (begin, advance):
        for bad in (dict(ring=good["ring"].double()), dict(state=torch.zeros(2, dtype=torch.int64)), dict(scan=good["scan"].half()),
                    dict(ring=good["ring"].numpy()), dict(state=[0, 0]), dict(scan=None)):
            with pytest.raises(TypeError):
                call(**bad)
        with pytest.raises(L.EloError, match="contiguous"):
            call(ring=torch.zeros((K, W, H, 3)).transpose(1, 2))
        with pytest.raises(L.EloError, match="contiguous"):
            call(scan=torch.zeros((W, H, 3)).transpose(0, 1))
        with pytest.raises(L.EloError, match="K,H,W,3"):
            call(ring=torch.zeros((H, W, 3)))
        with pytest.raises(L.EloError, match="K,H,W,3"):
            call(ring=torch.zeros((K, H, W, 4)))
        with pytest.raises(L.EloError, match="1 .. 16 scans"):
            call(ring=torch.zeros((17, H, W, 3)), poses64=torch.zeros((17, 7), dtype=torch.float64), poses32=torch.zeros((17, 7)))
        with pytest.raises(L.EloError, match="1 .. 16 scans"):
            call(ring=torch.zeros((0, H, W, 3)))
        with pytest.raises(L.EloError, match="H >= 3"):
            call(ring=torch.zeros((K, 2, W, 3)), scan=torch.zeros((2, W, 3)))
        with pytest.raises(L.EloError, match="W >= 1"):
            call(ring=torch.zeros((K, H, 0, 3)), scan=torch.zeros((H, 0, 3)))
        with pytest.raises(L.EloError, match="next, held"):
            call(state=torch.zeros(3, dtype=torch.int32))
        with pytest.raises(L.EloError, match="range image"):
            call(scan=torch.zeros((1, H, W, 3)))
        with pytest.raises(L.EloError, match="range image"):
            call(scan=torch.zeros((H, W + 1, 3)))
        with pytest.raises(L.EloError, match="no CPU fallback"):                        # well-formed, but not on a GPU
            call()
    for bad in (dict(poses64=good["poses64"].float()), dict(poses32=good["poses32"].double()), dict(T=good["T"].double()),
                dict(T=np.zeros(7, np.float32))):
        with pytest.raises(TypeError):
            advance(**bad)
    with pytest.raises(L.EloError, match="row per slot"):
        advance(poses64=torch.zeros((K + 1, 7), dtype=torch.float64))
    with pytest.raises(L.EloError, match="row per slot"):
        advance(poses32=torch.zeros((1, K, 7)))
    with pytest.raises(L.EloError, match="contiguous"):
        advance(poses64=torch.zeros((7, K), dtype=torch.float64).t())
    with pytest.raises(L.EloError, match="row"):
        advance(T=torch.zeros((2, 7)))
    advance_ok = dict(T=torch.zeros((1, 7)))                                            # (a fit's (1,7) pose block is taken as it is)
    with pytest.raises(L.EloError, match="no CPU fallback"):
        advance(**advance_ok)
    # the tracker's values, before any tensor is made
    with pytest.raises(TypeError):
        lm.DeviceTracker(8, 16, 4, S.PoseFit(), device="cpu")
    with pytest.raises(TypeError):
        lm.DeviceTracker(8, 16, S.LocalModel(resident=True), dict(iters=1), device="cpu")
    with pytest.raises(TypeError):
        lm.DeviceTracker(8, 16, S.LocalModel(), S.PoseFit(), sensor="hdl64", device="cpu")
    with pytest.raises(ValueError):
        lm.DeviceTracker(2, 16, S.LocalModel(), S.PoseFit(), device="cpu")


def test_predict_sequence_argument_errors():
    ev, S = load_pkg("evaluate"), load_pkg("sensor")
    with pytest.raises(ValueError, match="fit"):
        ev.predict_sequence(None, "/nowhere", "00", None, model=S.LocalModel(resident=True), lanes=2)
    with pytest.raises(ValueError, match="fit"):
        ev.predict_sequence(None, "/nowhere", "00", None, model=S.LocalModel(resident=True))
    with pytest.raises(NotImplementedError):                                            # the host-driven tracker still cannot follow lanes
        ev.predict_sequence(None, "/nowhere", "00", None, fit=S.PoseFit(iters=1), model=S.LocalModel(), lanes=2)
    with pytest.raises(NotImplementedError):
        ev.predict_sequence(None, "/nowhere", "00", None, fit=S.PoseFit(iters=1), model=S.LocalModel(resident=False), lanes=1)


@pytest.mark.parametrize("K", (1, 3, 4))
@pytest.mark.parametrize("reset_at", (None, 3, 5))
def test_the_state_machine_holds_the_last_k_scans(K, reset_at):
    """Eight steps of a drive whose scans are numbered: pair n = (scan n+1, scan n).  The ring of the numpy machine holds exactly the
    last min(entered, K) scans a plain list keeps, the newest in the slot the step entered, and `state` is {entered % K, min(entered,
    K)} -- the host cursor of local_model.ModelTracker."""
    m = D.Machine(K, dtype=np.int64, empty=-1)
    entered, base = [], 0                                      # the plain model: every scan since the last reset, in order
    assert m.state == (0, 0) and (m.ring == -1).all()
    for n in range(8):
        if n == reset_at:
            m.reset()
            entered = []
            assert m.state == (0, 0) and (m.ring == -1).all() and (m.poses64 == D.IDENTITY).all()
        first, scan = base + n, base + n + 1
        before = m.state
        m.begin(first)
        if not entered:
            entered.append(first)
            assert m.ring[0] == first and m.state == before    # begin never moves the state
        assert sorted(m.ring[m.ring >= 0]) == entered[-K:]     # what the render sees: the last K scans, frame 2 the newest
        slot = m.advance(scan)
        entered.append(scan)
        assert slot == (len(entered) - 1) % K and m.ring[slot] == scan
        assert m.state == (len(entered) % K, min(len(entered), K)) == D.after(*before, K)
        assert sorted(m.ring[m.ring >= 0]) == entered[-K:]
        assert (m.poses64[slot] == D.IDENTITY).all()
    assert 0 <= m.state[0] < K and m.state[1] == K


def test_the_machine_rebases_as_the_host_tracker_does():
    """Poses of the numpy machine after three steps with real motions: each held scan's row carries it into the newest scan's
    frame -- the product of the inverse motions since it entered -- as local_model.rebase leaves them."""
    import pose_fit_reference as R
    lm = load_pkg("local_model")
    K = 3
    m = D.Machine(K, dtype=np.int64, empty=-1)
    host = torch.tensor(np.tile(D.IDENTITY, (K, 1)))
    motions = [R.retract(D.IDENTITY, np.array([0.0, 0.0, 0.01 * (n + 1), 0.8, 0.02 * n, 0.0])).astype(np.float32) for n in range(4)]
    entered = 1
    for n, T in enumerate(motions):
        m.step(n + 1, n, T)
        host = lm.rebase(host, T)
        host[entered % K] = torch.tensor(D.IDENTITY)
        entered += 1
        assert np.abs(m.poses64 - host.numpy()).max() <= 1e-12
    assert m.state == (entered % K, K)

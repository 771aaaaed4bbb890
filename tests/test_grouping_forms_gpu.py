"""GPU: every case of tests/grouping_forms_cases.py through the HIP grouping kernels, in the form it names.

For each case the library's form query is asked first (the launcher switches on the same function), then the entry point runs
and all four outputs are compared with the CPU oracle bit for bit (np.array_equal: integer indices and 0/1 masks, no
tolerance), again without the two prefix masks, and -- for the LDS-tiled entry points -- against the general kernel on the same
inputs.  The oracle itself is pinned to the reference's stored outputs on the same table in tests/test_grouping_forms_cpu.py.
Forced tuning is restored by tuning.override's `finally`.  A refused case asserts the refusal of the query AND of the entry
point, and that the stream still works afterwards.  The placed-tie clouds also go through the in-kernel grouping of
fused.cv_stage1 (wave_select_k on the buffer-resource grid) with every pixel a centre.
"""
import ctypes

import numpy as np
import pytest
import torch

import grouping_forms_cases as T
from conftest import load_pkg
from oracle import grouping as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RUN = [c["name"] for c in T.CASES if c["refuse"] is None]
REFUSED = [c["name"] for c in T.CASES if c["refuse"] is not None]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _K(case):
    return T.resolve_K(case, load_pkg("_lib").lib().elo_fused_conv_random_k_dense_fits)


def _form(case, K, want_valid):
    return load_pkg("fused_conv").grouping_form(case["op"], T.batch_of(case), case["H"], case["W"], case["N"], case["kH"], case["kW"], K,
                                                case["fc"], case["dist"], case["sh"], case["sw"], want_valid=want_valid, dense=case["dense"])


def _oracle(case, K, **kw):
    fn = G.fused_conv_random_k if case["op"] == "random" else G.fused_conv_select_k
    return fn(*T.oracle_args(case, K, **kw))


def _numpy(out):
    torch.cuda.synchronize()
    return [o.cpu().numpy() if o is not None else None for o in out]


@pytest.mark.parametrize("name", RUN)
def test_case_is_bit_exact_in_the_form_it_names(name):
    case = T.BY_NAME[name]
    elo, tuning = load_pkg(), load_pkg("tuning")
    K = _K(case)
    a = T.inputs(case)
    fn = elo.fused_conv_random_k if case["op"] == "random" else elo.fused_conv_select_k
    args = (_t(a["xyz1"]), _t(a["xyz2"]), _t(a["idx"]), _t(a["perm"]), case["H"], case["W"], a["idx"].shape[1], case["kH"], case["kW"], K,
            case["fc"], case["dist"], case["sh"], case["sw"])
    counts = "+counts" if case["op"] == "select" and case["dense"] else ""
    with tuning.override(**case["tuning"]):                      # (restores the forced fields in its `finally`)
        assert _form(case, K, True) == case["form"] + counts
        assert _form(case, K, False) == case["form"]
        got = _numpy(fn(*args, dense=case["dense"]))
        lean = _numpy(fn(*args, dense=case["dense"], want_valid=False))
    want = _oracle(case, K)
    for g, w, what in zip(got, want, ("sel", "valid", "indis", "mask")):
        assert g.dtype == w.dtype and np.array_equal(g, w), what
    assert lean[1] is None and lean[2] is None
    assert np.array_equal(lean[0], want[0]) and np.array_equal(lean[3], want[3])
    if case["dense"]:                                            # ... and the general kernel agrees on the same inputs
        for g, w in zip(_numpy(fn(*args, dense=False)), got):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_sizes_are_refused_and_leave_the_stream_clean(name):
    case = T.BY_NAME[name]
    L, tuning = load_pkg("_lib"), load_pkg("tuning")
    K = _K(case)
    H2, W2 = -(-case["H"] // case["sh"]), -(-case["W"] // case["sw"])
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)        # real addresses; a refusal comes before any launch
    p = buf.data_ptr()
    block = L.GroupArgs(1, case["H"], case["W"], H2, W2, case["N"], case["kH"], case["kW"], K, case["fc"], case["dist"], case["sh"], case["sw"],
                        p, p, p, p, p, p, p, p)
    entry = "elo_fused_conv_%s_k%s" % (case["op"], "_dense" if case["dense"] else "")
    with tuning.override(**case["tuning"]):
        assert getattr(L.lib(), entry + "_form")(ctypes.byref(block)) == case["refuse"]       # host only: asked first
        assert getattr(L.lib(), entry)(ctypes.byref(block), L.stream_ptr(buf)) == case["refuse"]
    assert L.lib().elo_last_error()
    torch.cuda.synchronize()                                      # no launch happened, nothing is pending or broken
    assert float((buf + 1).sum().item()) == 64.0 and not buf.any()


@pytest.mark.parametrize("name,storage", T.IN_KERNEL)
def test_placed_clouds_through_the_in_kernel_grouping(name, storage):
    """fused.cv_stage1 groups in-kernel (wave_select_k, queried grid read through a buffer resource): with every pixel of the
    placed clouds a centre, its neighbour indices and mask equal the oracle's select-k bit for bit."""
    case = T.BY_NAME[name]
    fused, tf_util = load_pkg("fused"), load_pkg("tf_util")
    a = T.inputs(case)
    B, H, W = a["xyz1"].shape[:3]
    N, K = H * W, case["K"]
    C = 64 if storage == "f16" else 16
    rng = np.random.default_rng(len(name))
    fa, fb = (rng.normal(0, 1, (B, H, W, C)).astype(np.float16 if storage == "f16" else np.float32) for _ in range(2))
    store = tf_util.VariableStore(DEV, seed=0)
    with tf_util.default_store(store), torch.no_grad():
        P = fused.packed_layer
        c0 = P("c0", 10 + 2 * C, 128, row_order=fused.cv0_row_order(C)) if storage == "f16" else P("c0", 10 + 2 * C, 128)
        g = fused.Grouping(_t(a["perm"]), [case["kH"], case["kW"]], case["dist"], want_indices=True)
        out = fused.cv_stage1(_t(a["xyz1"]).reshape(B, N, 3), _t(fa).reshape(B, N, C), _t(a["xyz2"]), _t(fb), None, None,
                              c0, P("c1", 128, 64), P("c2", 64, 64), P("cx", 10, 64), P("s0", 128, 128), P("s1", 128, 64), group=g, K=K)
    torch.cuda.synchronize()
    assert out.dtype == (torch.float16 if storage == "f16" else torch.float32)
    want = _oracle(case, K, all_centres=True)
    assert np.array_equal(g.idx.cpu().numpy(), want[0])
    assert np.array_equal(g.mask.cpu().numpy()[..., None], want[3])
    designed = a["idx"][0, 0, 0] * W + a["idx"][0, 0, 1]           # the designed centre is among them, with its ties
    assert np.array_equal(want[0][:, designed], _oracle(case, K)[0][:, 0])

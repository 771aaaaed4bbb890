"""GPU: the register-resident chain kernels of csrc/elo_fused.hip (cv1_rr_kernel, cv2_rr_kernel, setconv_rr_kernel, mlp2_rr_kernel,
cv1_setconv_rr_kernel) -- the kernels the library launches by default -- at the shapes they admit and the pyramid never runs: every
case of tests/chain_shapes_cases.py in fp32 and fp16 storage, with split and half products.  Per run:

  * the form query with the call's real pointers answers chain/<products>, and the launch counter of the kernel advances by exactly
    the launches made: the kernel under test is the one that ran;
  * EVERY output element is within the per-element bound tests/fused_shapes_bounds.py derives of the float64 statement of
    tests/fused_shapes_reference.py;
  * the same call under chain_forms=0 -- the tile kernel -- gives the same bits, as the comments above the kernels claim.

Each test prints the worst error it saw as a fraction of its bound (profiles/chain_shapes_errors.txt records them; the bounds never
come from there)."""
import ctypes

import numpy as np
import pytest
import torch

import chain_shapes_cases as chain
import fused_shapes_bounds as bounds
import fused_shapes_reference as R
from conftest import load_pkg
from test_fused_shapes_gpu import DEV, _standalone_random_k, check, dev_feat, packed, t

pytestmark = pytest.mark.gpu
CV1, CV2, SETCONV, MLP2 = range(4)                        # elo_debug_rr_launches' indices


def _runs(part):
    return [pytest.param(*run, id=chain.run_id(run)) for run in chain.runs(part)]


def _needs_chain_kernels():
    if load_pkg("fused").fp32_mfma():
        pytest.skip("the fp32-MFMA comparison build has no chain kernels")


def _launches(reset=True):
    counts = (ctypes.c_ulonglong * 4)()
    load_pkg("_lib").lib().elo_debug_rr_launches(counts, 1 if reset else 0)
    return list(counts)


def chain_and_tile(form, call, products, which, launches=1):
    """(the call's result on the chain kernel, on its tile twin): the form is asked with the call's own pointers, and the launch
    counters say which kernel ran"""
    tuning = load_pkg("tuning")
    want = [launches if i == which else 0 for i in range(4)]
    with tuning.override(**chain.CHAIN_TUNING):
        assert form() == "chain/" + products
        _launches()
        got = call()
        assert _launches() == want, "the chain kernel is the one under test"
    with tuning.override(**chain.TILE_TUNING):
        assert form().startswith("tile") and form().endswith("/" + products)
        twin = call()
        assert _launches() == [0, 0, 0, 0]
    torch.cuda.synchronize()
    return got, twin


def report(what, ratio):
    print("CHAIN_SHAPES %s %.3f of the bound" % (what, ratio))


def same_bits(got, twin, what):
    assert got.dtype == twin.dtype and got.shape == twin.shape and torch.equal(got, twin), \
        "%s: %d elements differ from the tile kernel's" % (what, int((got != twin).sum()))


# ---------------------------------------------------------------------------- part A: the cost volumes
def _cv_args(case, inp, storage, products):
    fused = load_pkg("fused")
    C, L = case.C, inp["layers"]
    one = lambda name, order=None: packed([L[name]], products, order)[0]
    idx, mask = t(inp["idx"]), t(inp["mask"])
    if case.stage == 1:
        layers = (one("cv0", fused.cv0_row_order(C)), one("cv1"), one("cv2"), one("cv_xyz"),
                  one("sum_cv0", list(range(64, 128)) + list(range(64))), one("sum_cv1"))                       # kernel order [x | enc]
        return (t(inp["xyz1"]), dev_feat(inp["feat1"], storage), t(inp["xyz2"]), dev_feat(inp["feat2"], storage), idx, mask) + layers
    order = list(range(64 + C, 128 + C)) + list(range(64)) + list(range(64, 64 + C))                            # [grouped | enc | feat1]
    layers = (one("xyz_enc"), one("sum_cost0", order), one("sum_cost1"))
    return (t(inp["xyz1"]), dev_feat(inp["feat1"], storage), dev_feat(inp["cost"], storage), idx, mask) + layers


def _cv_expect(case, inp, products, storage):
    want, bound, spread = (bounds.cv1_expect if case.stage == 1 else bounds.cv2_expect)(R, inp, products, storage)
    assert case.far or spread < 30.0, "the first-order softmax term needs |l - max| < 30 on the slots that carry weight (%.1f)" % spread
    return want, bound


@pytest.mark.parametrize("case,storage,products", _runs("cv"))
def test_cost_volume_chain_kernels(case, storage, products):
    _needs_chain_kernels()
    fused = load_pkg("fused")
    inp = chain.cv_inputs(case, storage)
    args = _cv_args(case, inp, storage, products)
    form, call = (fused.cv_stage1_form, fused.cv_stage1) if case.stage == 1 else (fused.cv_stage2_form, fused.cv_stage2)
    out, twin = chain_and_tile(lambda: form(*args), lambda: call(*args), products, CV1 if case.stage == 1 else CV2)
    what = "cv%d %s %s %s" % (case.stage, case.name, storage, products)
    want, bound = _cv_expect(case, inp, products, storage)
    report(what, check(out, want, bound, storage, what))
    same_bits(out, twin, what)


# ---------------------------------------------------------------------------- part B: set-conv with in-kernel random-k
def _setconv_job(case, inp, storage, products):
    fused = load_pkg("fused")
    kh, kw, dist, sh, sw = case.group
    job = dict(src_xyz=t(inp["src_xyz"]), src_feat=dev_feat(inp["src_feat"], storage), idx=None, mask=None, xyz1_grid=t(inp["xyz1_grid"]),
               layers=packed(inp["layers"], products, fused.setconv_row_order(64)), K=case.K,
               group=fused.Grouping(t(inp["order"]), [kh, kw], dist, sh, sw))        # (no indices: the chain form cannot return them)
    if "centre_hw" in inp:
        job["centre_hw"] = t(inp["centre_hw"])
    return job


def _check_setconv(case, inp, job, out, new_xyz, storage, products, what):
    """one job's output against the statement on the slots the stand-alone random-k gives for the same inputs (pinned bit-exact to
    the oracle by tests/test_grouping_gpu.py); new_xyz and the all-clear points exactly"""
    assert job["group"].idx is None and job["group"].mask is None
    centre = chain.setconv_centres(inp)
    sel, mask = _standalone_random_k(case, inp, job)
    idx, mask = sel.cpu().numpy(), mask.cpu().numpy()
    assert (idx[mask == 0] == 0).all() and 0 < mask.mean() < 1, what
    if case.centre == "hw":
        assert np.array_equal(new_xyz.cpu().numpy(), centre), what + ": new_xyz"
    else:
        assert new_xyz is None
    want, bound = bounds.setconv_expect(R, inp, centre, idx, mask, products, storage)
    ratio = check(out, want, bound, storage, what)
    clear = mask.sum(-1) == 0
    assert clear.any() and (out.float().cpu().numpy()[clear] == 0).all(), what + ": an all-clear point pools to 0"
    return ratio


@pytest.mark.parametrize("case,storage,products", _runs("setconv"))
def test_setconv_chain_kernel(case, storage, products):
    _needs_chain_kernels()
    fused = load_pkg("fused")
    inputs = [chain.setconv_inputs(case, storage, j) for j in range(2 if case.pair else 1)]
    jobs = [_setconv_job(case, inp, storage, products) for inp in inputs]
    call = (lambda: fused.setconv_pair(*jobs)) if case.pair else (lambda: [fused.setconv(**jobs[0])])
    outs, twins = chain_and_tile(lambda: fused.setconv_form(*jobs), call, products, SETCONV)
    for j, (inp, job, (out, new_xyz), (twin, twin_xyz)) in enumerate(zip(inputs, jobs, outs, twins)):
        what = "setconv %s %s %s job%d" % (case.name, storage, products, j)
        report(what, _check_setconv(case, inp, job, out, new_xyz, storage, products, what))
        same_bits(out, twin, what)
        assert new_xyz is None or torch.equal(new_xyz, twin_xyz)


# ---------------------------------------------------------------------------- part C: the two-stage MLP
def _mlp_job(case, inp, storage, products):
    fused = load_pkg("fused")
    return dict(sources=[dev_feat(s, storage) for s in inp["sources"]], layers=packed(inp["layers"], products),
                before=dev_feat(inp["before"], storage), after=dev_feat(inp["after"], storage),
                layers2=packed(inp["layers2"], products, fused.stage2_row_order(case.C, 64, 64)))


def _dirty_projection_buffers(storage):
    """ProjectionBuffers of a 2 x 3 x 5 projection of 7 points, 8 channels, filled with a pattern the clear must overwrite"""
    ops = load_pkg("_ops")
    buf = ops.ProjectionBuffers(2, 7, 3, 5, 8, DEV, torch.float16 if storage == "f16" else torch.float32)
    buf.out_xyz.fill_(3.25)
    buf.out_feat.fill_(-1.5)
    buf.scratch.copy_(torch.arange(buf.scratch.numel(), dtype=torch.int32, device=DEV) * 7 + 1)
    return buf


@pytest.mark.parametrize("case,storage,products", _runs("mlp"))
def test_two_stage_mlp_chain_kernel(case, storage, products):
    _needs_chain_kernels()
    fused = load_pkg("fused")
    inputs = [chain.mlp_inputs(case, storage, j) for j in range(2 if case.pair else 1)]
    jobs = [_mlp_job(case, inp, storage, products) for inp in inputs]
    cleared = []

    def call():
        if not case.pair:
            return [fused.mlp2(**jobs[0])]
        cleared.append(_dirty_projection_buffers(storage) if case.clear else None)
        return fused.mlp2_pair(*jobs, clear=cleared[-1])
    outs, twins = chain_and_tile(lambda: fused.mlp_form(*jobs), call, products, MLP2)
    for j, (inp, (out, out2), (twin, twin2)) in enumerate(zip(inputs, outs, twins)):
        what = "mlp2 %s %s %s job%d" % (case.name, storage, products, j)
        want, bound = bounds.mlp_expect(R, inp, products, storage)
        report(what + " out", check(out, want, bound, storage, what + " out"))
        want2, bound2 = bounds.mlp_expect(R, inp, products, storage, first_stage=out.double().cpu().numpy())
        report(what + " out2", check(out2, want2, bound2, storage, what + " out2"))
        same_bits(out, twin, what + " out")
        same_bits(out2, twin2, what + " out2")
    if case.clear:                                       # what the side job leaves equals, element for element, what the tile form leaves
        by_chain, by_tile = cleared
        assert by_chain.cleared and by_tile.cleared
        for name in ("scratch", "out_xyz", "out_feat"):
            assert torch.equal(getattr(by_chain, name), getattr(by_tile, name)), name
        assert not torch.equal(by_chain.out_xyz, torch.full_like(by_chain.out_xyz, 3.25))


# ---------------------------------------------------------------------------- part D: the heterogeneous chain launch
@pytest.mark.parametrize("case,storage,products", _runs("pair"))
def test_heterogeneous_chain_launch(case, storage, products):
    """elo_cv_stage1_setconv_chain on pre-grouped stage-1 inputs: n_cv + 2 n_sc workgroups, each body with its own sub-grid"""
    _needs_chain_kernels()
    fused, L, tuning = load_pkg("fused"), load_pkg("_lib"), load_pkg("tuning")
    cv_inp = chain.cv_inputs(case.cv, storage)
    cv_args = _cv_args(case.cv, cv_inp, storage, products)
    sc_inputs = [chain.setconv_inputs(case.sc, storage, j) for j in range(2)]
    sc_jobs = [_setconv_job(case.sc, inp, storage, products) for inp in sc_inputs]
    n_pair = ctypes.c_ulonglong(0)
    with tuning.override(**chain.CHAIN_TUNING):
        a, out, grouped, _keep = fused._cv1_args(*cv_args)
        side = [fused._setconv_args(**job) for job in sc_jobs]                       # (args, out, new_xyz, keep-alive)
        assert not grouped and a.K == case.cv.K
        assert L.lib().elo_cv_stage1_setconv_chain_form(ctypes.byref(a), ctypes.byref(side[0][0]), ctypes.byref(side[1][0])) == 1
        L.check(L.lib().elo_debug_chain_pair_launches(None, 1))
        _launches()
        L.call3("elo_cv_stage1_setconv_chain", a, side[0][0], side[1][0], out)
        L.check(L.lib().elo_debug_chain_pair_launches(ctypes.byref(n_pair), 1))
        assert n_pair.value == 1 and _launches() == [1, 0, 1, 0], "cv1_setconv_rr_kernel is the one under test"
        alone = fused.cv_stage1(*cv_args)                                            # the separate chain launches
        alone_side = fused.setconv_pair(*sc_jobs)
        L.check(L.lib().elo_debug_chain_pair_launches(ctypes.byref(n_pair), 1))
        assert n_pair.value == 0 and _launches() == [1, 0, 1, 0]
    torch.cuda.synchronize()
    what = "pair %s %s %s" % (case.name, storage, products)
    want, bound = _cv_expect(case.cv, cv_inp, products, storage)
    report(what + " cv1", check(out, want, bound, storage, what + " cv1"))
    same_bits(out, alone, what + " cv1")
    for j, (inp, job, (_a, sc_out, new_xyz, _k), (alone_out, alone_xyz)) in enumerate(zip(sc_inputs, sc_jobs, side, alone_side)):
        report(what + " job%d" % j, _check_setconv(case.sc, inp, job, sc_out, new_xyz, storage, products, what + " job%d" % j))
        same_bits(sc_out, alone_out, what + " job%d" % j)
        assert torch.equal(new_xyz, alone_xyz)

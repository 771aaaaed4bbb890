"""GPU: the tile kernels of csrc/elo_fused.hip (setconv_kernel, mlp_kernel, cv1_meta_kernel, cv2_kernel) at the shapes the ABI admits and
the pyramid never runs -- every case of tests/fused_shapes_cases.py in fp32 and fp16 storage, with split and half products (and three
cases per part on the range-checked instances), against the float64 statement of tests/fused_shapes_reference.py, EVERY element within
the per-element bound tests/fused_shapes_bounds.py derives.  Before a case runs, the library is asked with the call's real pointers
which kernel it launches (the elo_*_form queries): the tile kernel of the height the case names.

Each test prints the worst error it saw as a fraction of its bound (profiles/fused_shapes_errors.txt records them; the bounds never
come from there)."""
import numpy as np
import pytest
import torch

import fused_shapes_bounds as bounds
import fused_shapes_cases as table
import fused_shapes_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_feat(x, storage):
    return None if x is None else (t(x).half() if storage == "f16" else t(x))


def _runs(part):
    return [pytest.param(*run, id=table.run_id(run)) for run in table.runs(part)]


_PACKED = {}


def packed(layers, products, first_order=None):
    """fused.PackedDense of a chain's (W, b, relu), ONCE per (layers, products mode, row order of the first layer)"""
    fused = load_pkg("fused")
    key = (tuple(id(W) for W, _b, _r in layers), products == "half", None if first_order is None else tuple(first_order))
    hit = _PACKED.get(key)
    if hit is None:
        hit = (layers, [fused.PackedDense(t(W), t(b), relu, t(np.asarray(first_order)) if i == 0 and first_order is not None else None,
                                          products == "half") for i, (W, b, relu) in enumerate(layers)])
        _PACKED[key] = hit                                # (holds the arrays: their ids cannot be reused meanwhile)
    return hit[1]


class running:
    """the tuning a case runs under: tile kernels only, the case's tile height, the range check for a checked run"""

    def __init__(self, case, products):
        self.fields = dict(chain_forms=0, small_tile_units=table.tile_units(case.tile), range_check=1 if products == "checked" else 0)
        self.checked = products == "checked"

    def __enter__(self):
        L = load_pkg("_lib")
        self.ctx = load_pkg("tuning").override(**self.fields)
        self.ctx.__enter__()
        if self.checked:
            L.range_violations(torch.empty(1, device=DEV))          # (read and clear)
        return self

    def __exit__(self, *exc):
        try:
            if self.checked and exc[0] is None:
                assert load_pkg("_lib").range_violations(torch.empty(1, device=DEV)) == 0
        finally:
            self.ctx.__exit__(*exc)


def _skip_half_on_the_fp32_build(products):
    if products == "half" and load_pkg("fused").fp32_mfma():
        pytest.skip("the fp32-MFMA comparison build has no fp16 products")


def check(got, want, bound, storage, what):
    """every element: finite, of the storage dtype, within its bound; returns the worst error / bound"""
    assert got.dtype == (torch.float16 if storage == "f16" else torch.float32), what
    g = got.detach().double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(g).all(), what
    err = np.abs(g - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("FUSED_SHAPES %s %.3f of the bound (worst |error| %.3e)" % (what, ratio, float(err.max())))
    bad = err > bound
    assert not bad.any(), "%s: %d of %d elements beyond their bound, worst %.2f x at %s (want %.7g got %.7g)" % (
        what, int(bad.sum()), bad.size, ratio, np.unravel_index((err / np.maximum(bound, 1e-300)).argmax(), err.shape),
        want.flat[(err / np.maximum(bound, 1e-300)).argmax()], g.flat[(err / np.maximum(bound, 1e-300)).argmax()])
    return ratio


# ---------------------------------------------------------------------------- part A: row-wise MLP
@pytest.mark.parametrize("case,storage,products", _runs("mlp"))
def test_mlp_tile_kernel(case, storage, products):
    _skip_half_on_the_fp32_build(products)
    fused = load_pkg("fused")
    inputs = [table.mlp_inputs(case, storage, j) for j in range(2 if case.pair else 1)]
    jobs = []
    for inp in inputs:
        job = dict(sources=[dev_feat(s, storage) for s in inp["sources"]], layers=packed(inp["layers"], products))
        if case.stage2:
            wb, wa, _l2 = case.stage2
            job.update(before=dev_feat(inp["before"], storage), after=dev_feat(inp["after"], storage),
                       layers2=packed(inp["layers2"], products, fused.stage2_row_order(wb, case.layers[-1], wa)))
        jobs.append(job)
    with running(case, products):
        assert fused.mlp_form(*jobs) == table.expected_form(case, products)
        if case.stage2:
            outs = fused.mlp2_pair(*jobs) if case.pair else [fused.mlp2(**jobs[0])]
        else:
            outs = [(o, None) for o in (fused.mlp_pair(jobs[0]["sources"], jobs[0]["layers"], jobs[1]["sources"], jobs[1]["layers"])
                                        if case.pair else [fused.mlp(jobs[0]["sources"], jobs[0]["layers"])])]
        torch.cuda.synchronize()
    for j, (inp, (out, out2)) in enumerate(zip(inputs, outs)):
        what = "mlp %s %s %s job%d" % (case.name, storage, products, j)
        want, bound = bounds.mlp_expect(R, inp, products, storage)
        check(out, want, bound, storage, what + " out")
        if case.stage2:
            want2, bound2 = bounds.mlp_expect(R, inp, products, storage, first_stage=out.double().cpu().numpy())
            check(out2, want2, bound2, storage, what + " out2")


# ---------------------------------------------------------------------------- part B: set-conv
def _setconv_job(case, inp, storage, products):
    fused = load_pkg("fused")
    job = dict(src_xyz=t(inp["src_xyz"]), src_feat=dev_feat(inp["src_feat"], storage), idx=None, mask=None,
               layers=packed(inp["layers"], products, fused.setconv_row_order(case.C)), K=case.K)
    for name in ("xyz1_grid", "centre_hw", "centre_xyz"):
        if name in inp:
            job[name] = t(inp[name])
    if case.group:
        kh, kw, dist, sh, sw = case.group
        job["group"] = fused.Grouping(t(inp["order"]), [kh, kw], dist, sh, sw, want_indices=True)
    else:
        job["idx"], job["mask"] = t(inp["idx"]), t(inp["mask"])
    return job


def _standalone_random_k(case, inp, job):
    """the indices and mask elo_fused_conv_random_k gives for the job's centres: what the in-kernel grouping must reproduce bit for bit"""
    fused, fc = load_pkg("fused"), load_pkg("fused_conv")
    kh, kw, dist, sh, sw = case.group
    B, H, W, _ = inp["xyz1_grid"].shape
    centres = job["centre_hw"] if "centre_hw" in job else fused._all_pixels(B, H, W, DEV)
    sel, _v, _d, mask = fc.fused_conv_random_k(job["xyz1_grid"], job["src_xyz"], centres, job["group"].random_hw, H, W, centres.shape[1], kh, kw,
                                               case.K, 0, dist, sh, sw, want_valid=False, dense=False)
    return sel, mask[..., 0]


@pytest.mark.parametrize("case,storage,products", _runs("setconv"))
def test_setconv_tile_kernel(case, storage, products):
    _skip_half_on_the_fp32_build(products)
    fused = load_pkg("fused")
    inputs = [table.setconv_inputs(case, storage, j) for j in range(2 if case.pair else 1)]
    jobs = [_setconv_job(case, inp, storage, products) for inp in inputs]
    with running(case, products):
        assert fused.setconv_form(*jobs) == table.expected_form(case, products)
        outs = fused.setconv_pair(*jobs) if case.pair else [fused.setconv(**jobs[0])]
        torch.cuda.synchronize()
    for j, (inp, job, (out, new_xyz)) in enumerate(zip(inputs, jobs, outs)):
        what = "setconv %s %s %s job%d" % (case.name, storage, products, j)
        centre = table.setconv_centres(inp)
        if case.group:
            sel, mask = _standalone_random_k(case, inp, job)
            assert torch.equal(job["group"].idx, sel) and torch.equal(job["group"].mask, mask), what + ": in-kernel grouping"
            idx, mask = sel.cpu().numpy(), mask.cpu().numpy()
            assert (idx[mask == 0] == 0).all() and 0 < mask.mean() < 1, what
        else:
            idx, mask = inp["idx"], inp["mask"]
        if case.centre == "hw":
            assert np.array_equal(new_xyz.cpu().numpy(), centre), what + ": new_xyz"
        else:
            assert new_xyz is None
        want, bound = bounds.setconv_expect(R, inp, centre, idx, mask, products, storage)
        check(out, want, bound, storage, what)
        clear = mask.sum(-1) == 0
        assert not clear.any() or (out.float().cpu().numpy()[clear] == 0).all(), what + ": an all-clear point pools to 0"


# ---------------------------------------------------------------------------- part C: the cost volumes
@pytest.mark.parametrize("case,storage,products", _runs("cv"))
def test_cost_volume_tile_kernels(case, storage, products):
    _skip_half_on_the_fp32_build(products)
    fused = load_pkg("fused")
    inp = table.cv_inputs(case, storage)
    C, L = inp["C"], inp["layers"]
    one = lambda name, order=None: packed([L[name]], products, order)[0]
    idx, mask = t(inp["idx"]), t(inp["mask"])
    if case.stage == 1:
        layers = (one("cv0", fused.cv0_row_order(C)), one("cv1"), one("cv2"), one("cv_xyz"),
                  one("sum_cv0", list(range(64, 128)) + list(range(64))), one("sum_cv1"))                       # kernel order [x | enc]
        args = (t(inp["xyz1"]), dev_feat(inp["feat1"], storage), t(inp["xyz2"]), dev_feat(inp["feat2"], storage), idx, mask) + layers
        form, call, expect = fused.cv_stage1_form, fused.cv_stage1, bounds.cv1_expect
    else:
        order = list(range(64 + C, 128 + C)) + list(range(64)) + list(range(64, 64 + C))                        # [grouped | enc | feat1]
        layers = (one("xyz_enc"), one("sum_cost0", order), one("sum_cost1"))
        args = (t(inp["xyz1"]), dev_feat(inp["feat1"], storage), dev_feat(inp["cost"], storage), idx, mask) + layers
        form, call, expect = fused.cv_stage2_form, fused.cv_stage2, bounds.cv2_expect
    with running(case, products):
        assert form(*args) == table.expected_form(case, products)
        out = call(*args)
        torch.cuda.synchronize()
    want, bound, spread = expect(R, inp, products, storage)
    assert spread < 30.0, "the first-order softmax term needs |l - max| < 30 on the slots that carry weight (%.1f)" % spread
    check(out, want, bound, storage, "cv%d %s %s %s" % (case.stage, case.name, storage, products))


def test_refusals_raise_through_the_front_ends_and_launch_nothing():
    """The LDS limit through fused.mlp / fused.setconv with real tensors: ELO_ERR_LIMIT with its message, from the query and from the
    entry point alike, and the stream has seen no launch error afterwards."""
    fused, L, tuning = load_pkg("fused"), load_pkg("_lib"), load_pkg("tuning")
    rng = np.random.default_rng(0)
    srcs = [t(rng.normal(0, 1, (33, w)).astype(np.float32)) for w in (200, 200, 104)]
    layers = packed(table.make_layers(504, (16,)), "split")
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(32)):
        for fn in (lambda: fused.mlp_form(dict(sources=srcs, layers=layers)), lambda: fused.mlp(srcs, layers)):
            with pytest.raises(L.EloError, match="bytes of LDS"):
                fn()
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(16)):
        assert fused.mlp_form(dict(sources=srcs, layers=layers)) == "tile16/split"
        out = fused.mlp(srcs, layers)
    torch.cuda.synchronize()
    want, bound = bounds.mlp_expect(R, {"sources": [s.cpu().numpy() for s in srcs], "layers": table.make_layers(504, (16,))}, "split", "f32")
    check(out, want, bound, "f32", "mlp 504 columns on the 16-row tile")

"""GPU: a refinement level's set-upconv stage 2 riding on its cost-volume stage-2 launch (cv2_upconv_kernel,
elo_cv_stage2_upconv_fused; tuning upconv_ride).  The predictor launch behind it then runs its own two layers on
[out | points_f1 | cost] read back from HBM.  `out` continues in the fused two-stage tile AS STORED (store_quad), so the
one-stage predictor sees the same operands in both storage types: every output must be the bits of the plain launches.
A launch counter proves which kernel ran."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rides(reset=False):
    lib = load_pkg("_lib")
    n = ctypes.c_ulonglong(0)
    lib.check(lib.lib().elo_debug_upconv_ride_launches(ctypes.byref(n), 1 if reset else 0))
    return n.value


def _level(B, H, W, C, dt, seed):
    """The inputs and layers of one refinement level's cost-volume stage 2 + set-upconv stage 2 + predictors."""
    fused, tf_util = load_pkg("fused"), load_pkg("tf_util")
    rng = np.random.default_rng(seed)
    store = tf_util.VariableStore(DEV, seed=seed)
    N = H * W
    r = lambda *s: t(rng.normal(0, 1, s).astype(np.float32)).to(dt)
    with tf_util.default_store(store), torch.no_grad(), tf_util.variable_scope("upconv_ride"):
        P = fused.packed_layer
        order = list(range(64 + C, 128 + C)) + list(range(64)) + list(range(64, 64 + C))
        cv = [P("enc", 10, 64), P("sc0", 128 + C, 128, row_order=order), P("sc1", 128, 64)]
        up = {k: [P("u%s0" % k, 64 + C, 128), P("u%s1" % k, 128, 64)] for k in "wc"}
        pred = {k: [P("p%s0" % k, C + 64 + 64, 128, row_order=fused.stage2_row_order(C, 64, 64)), P("p%s1" % k, 128, 64)] for k in "wc"}
        for p_ in cv + up["w"] + up["c"] + pred["w"] + pred["c"]:
            p_.b.copy_(torch.from_numpy(rng.normal(0, 0.1, p_.b.shape).astype(np.float32)))
    xyz = rng.normal(0, 5, (B, H, W, 3)).astype(np.float32)
    xyz[rng.random((B, H, W)) < 0.2] = 0
    group = fused.Grouping(t(rng.permutation(15).astype(np.int32)), [3, 5], 4.0)
    return dict(xyz=t(xyz), feat1=r(B, H, W, C), cost_in=r(B, H, W, 64), pooled={k: r(B, N, 64) for k in "wc"},
                points1=r(B, N, C), cv=cv, up=up, pred=pred, group=group)


@pytest.mark.parametrize("products", ["split", "half"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,H,W,C", [(1, 4, 57, 64), (1, 8, 113, 32), (1, 16, 225, 16), (2, 4, 57, 64), (1, 3, 7, 32)])
def test_the_merged_launch_and_the_one_stage_predictors_equal_the_plain_launches(B, H, W, C, dt, products):
    """Cost-volume stage 2 + the two set-upconv stage-2 jobs as ONE launch, then the predictors alone (with the softmax_valid
    ride), against elo_cv_stage2_fused + the two-stage elo_mlp_fused2: the cost, both set-upconv outputs, both predictor outputs
    and the partial sums, bit for bit.  The level sizes of a 64 x 1800 pyramid (228, 904, 3600 points: ragged 16- and 32-row
    tiles) and a 21-point one (a single ragged tile)."""
    fused, ops = load_pkg("fused"), load_pkg("_ops")
    if products == "half" and fused.fp32_mfma():
        pytest.skip("the fp32-MFMA comparison build has no fp16-product kernels")
    with fused.products(products):
        lv = _level(B, H, W, C, dt, seed=H * W + C + B)
        N = H * W
        before = lv["points1"]
        cv_args = (lv["xyz"], lv["feat1"], lv["cost_in"], None, None, *lv["cv"])
        cost = fused.cv_stage2(*cv_args, group=lv["group"], K=4)
        xyz_bn3 = lv["xyz"].reshape(B, N, 3)
        jobs2 = [dict(sources=[lv["pooled"][k], lv["points1"]], layers=lv["up"][k], before=before, after=cost, layers2=lv["pred"][k])
                 for k in "wc"]
        sv_two = ops.SvPartials(xyz_bn3)
        (out_w, pred_w), (out_c, pred_c) = fused.mlp2_pair(jobs2[0], jobs2[1], sv=sv_two)

        _rides(reset=True)
        side = [dict(sources=[lv["pooled"][k], lv["points1"]], layers=lv["up"][k]) for k in "wc"]
        cost_r, ups = fused.cv_stage2(*cv_args, group=lv["group"], K=4, side=side)
        assert ups is not None and _rides() == 1
        assert torch.equal(cost_r, cost)
        assert torch.equal(ups[0], out_w) and torch.equal(ups[1], out_c)
        sv_one = ops.SvPartials(xyz_bn3)
        got_w, got_c = fused.mlp_pair([ups[0], before, cost_r], lv["pred"]["w"], [ups[1], before, cost_r], lv["pred"]["c"], sv=sv_one)
        assert torch.equal(got_w, pred_w) and torch.equal(got_c, pred_c)
        assert sv_one.parts == sv_two.parts > 0
        view = lambda sv: sv.scratch.reshape(3, B, -1, 64)[:, :, :sv.parts]
        assert torch.equal(view(sv_one), view(sv_two))


def test_the_form_is_refused_where_a_half_is_not_a_tile_kernel():
    """The pair of set-upconv / predictor MLPs in the chain kernel's regime (2 x 7200 rows: l0 of a batch-2 64 x 1800 forward) and
    batch 8: cv_stage2 runs the cost volume alone and hands the jobs back (None); the counter stays put."""
    fused = load_pkg("fused")
    if fused.fp32_mfma():
        pytest.skip("the fp32-MFMA comparison build has no register-resident kernels")
    for B, H, W in ((2, 16, 225), (8, 4, 57)):
        lv = _level(B, H, W, 16, torch.float32, seed=B)
        side = [dict(sources=[lv["pooled"][k], lv["points1"]], layers=lv["up"][k]) for k in "wc"]
        _rides(reset=True)
        cost, ups = fused.cv_stage2(lv["xyz"], lv["feat1"], lv["cost_in"], None, None, *lv["cv"], group=lv["group"], K=4, side=side)
        assert ups is None and _rides() == 0
        assert torch.equal(cost, fused.cv_stage2(lv["xyz"], lv["feat1"], lv["cost_in"], None, None, *lv["cv"], group=lv["group"], K=4))


def _net(feat):
    from util_params import shuffle_fn
    model, perm = load_pkg("model"), load_pkg("perm")
    return model.PWCLONet(DEV, seed=5, perm_source=perm.PermSource(fn=shuffle_fn), feature_dtype=feat)


# launches of cv2_upconv_kernel per forward: the levels where cost-volume stage 2 and the set-upconv / predictor pair are tile
# kernels and stage 1 handed the set-upconv outputs over (64 x 1800 batch 1: l2, l1, l0; batch 2: l0's pair is in the chain
# kernel's regime; 128 x 2048: l1 is neither merged nor a chain pair, l0 is in the chain regime; batch 8: never)
_RIDES = {(1, 64, 1800): 3, (2, 64, 1800): 2, (1, 128, 2048): 1, (8, 64, 1800): 0}


@pytest.mark.parametrize("feat", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,H,W,profile", [k + ("dense",) for k in _RIDES] + [(1, 64, 1800, "kitti"), (2, 64, 1800, "kitti")])
def test_a_forward_with_the_ride_equals_the_forward_without(B, H, W, profile, feat):
    """Whole forward, eager: all nine outputs bit-identical with tuning.upconv_ride on and off (the dense scene at every size,
    the sparse one at 64 x 1800)."""
    from util_params import randomise
    synth, tuning = load_pkg("synth"), load_pkg("tuning")
    kw = {} if profile == "dense" else dict(profile="kitti")
    f1, f2 = synth.frame_pair(B, H, W, seed=17, **kw)
    both = torch.from_numpy(np.concatenate([f1, f2], 0)).to(DEV)
    net = _net(feat)
    net.forward(both[:B], both[B:])
    randomise(net.store, seed=7)
    outs = {}
    for ride in (True, False):
        with tuning.override(upconv_ride=ride):
            _rides(reset=True)
            outs[ride] = [x.clone() for x in net.forward(both[:B], both[B:])]
            assert _rides() == (_RIDES[(B, H, W)] if ride else 0)
    assert len(outs[True]) == 9
    for a, b in zip(outs[True], outs[False]):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.parametrize("feat", [torch.float32, torch.float16])
@pytest.mark.parametrize("check_every", [0, 1])
def test_captured_graphs_with_the_ride_equal_the_graphs_without(check_every, feat):
    """The captured forward (and the range-checked graph, replayed every step with check_every=1: the MODE_CHECKED instances)
    with the ride on and off: the same poses bit for bit, pair after pair, and no range violation."""
    synth, tuning = load_pkg("synth"), load_pkg("tuning")
    pairs = []
    for i in range(3):
        f1, f2 = synth.frame_pair(1, 64, 1800, seed=30 + i)
        pairs.append(torch.from_numpy(np.concatenate([f1, f2], 0)).to(DEV))
    got = {}
    for ride in (True, False):
        with tuning.override(upconv_ride=ride):
            _rides(reset=True)
            net = _net(feat)
            net.capture(1, 64, 1800, lanes=1, pose_ring=8, check_every=check_every)
            assert (_rides() > 0) == ride
            net.reset_poses(0)
            for p_ in pairs:
                net.submit(0, p_)
            got[ride] = net.collect(0).clone()
    assert got[True].shape[0] == len(pairs) and torch.isfinite(got[True]).all()
    assert torch.equal(got[True], got[False])

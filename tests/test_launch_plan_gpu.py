"""GPU: the launch schedule of the fused inference forward, plan by plan (pointnet_util.level_plan / fused_level).

Three things a move of that host code can change without any numeric test noticing, pinned to literals recorded BEFORE the
schedule was gathered into level_plan / fused_level (a 64 x 1800 pair at batch 1, every plan forced with tuning.override):
  (a) the C-ABI entries a forward calls, in order (_lib.call / call2 / call3 are the only doors from Python to a launch);
  (b) the order in which a fresh VariableStore creates its variables (Xavier draws come from one generator, in that order);
  (c) the order in which a fresh PermSource(seed=...) first draws its visiting orders (the draws are numbered).
(b) and (c) are the same in every plan; (a) and what fused.recording() keeps differ plan by plan."""
import numpy as np
import pytest
import torch

from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_CHAIN_ALL = dict(merge_level_points=0, cv_prepass=1, setconv_chain_rows=0, mlp_chain_rows=0)    # (the row hooks of test_chain_ops_gpu.py)
# plan -> (tuning fields, fp16 storage, the entries stage by stage [encoder | l2 origin + coarse pose | l2 | l1 | l0] without
# their elo_ prefix, fused.recording()'s (stage, side) tags: "1+" = stage 1 called with side jobs)
PLANS = {
    # the product's own choice: l2 and l1 merged, l0 the chain pair, every set-upconv stage 2 riding
    "default": ({}, False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_setconv_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain cv_stage2_upconv_fused mlp_fused2 pose_head"), "1+ 2 1+ 2+ 1+ 2+ 1+ 2+"),
    "merged": (dict(merge_level_points=1 << 30), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_setconv_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head"), "1+ 2 1+ 2+ 1+ 2+ 1+ 2+"),
    "merged, no upconv ride": (dict(merge_level_points=1 << 30, upconv_ride=False), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_setconv_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_fused mlp_fused2 pose_head"), "1+ 2 1+ 2 1+ 2 1+ 2"),
    "merged, fp16 storage": (dict(merge_level_points=1 << 30), True, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_setconv_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_upconv_fused mlp_fused2 pose_head"), "1+ 2 1+ 2+ 1+ 2+ 1+ 2+"),
    # the chain pair asked for at every level: taken at l0, l2 and l1 (below the chain kernels' rows) fall back on two launches
    "chain pair": (dict(merge_level_points=0), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain cv_stage2_upconv_fused mlp_fused2 pose_head"), "1 2 1+ 2 1+ 2 1+ 2+"),
    "chain pair, no upconv ride": (dict(merge_level_points=0, upconv_ride=False), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain cv_stage2_fused mlp_fused2 pose_head"), "1 2 1+ 2 1+ 2 1+ 2"),
    # ... and with every row threshold at 0 the chain pair at every level (stage 2 then is a chain launch too and carries nothing)
    "chain pair, every level": (_CHAIN_ALL, False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "fused_conv_select_k cv_stage1_fused fused_conv_random_k_dense cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain fused_conv_random_k_dense cv_stage2_fused mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain fused_conv_random_k_dense cv_stage2_fused mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain fused_conv_random_k_dense cv_stage2_fused mlp_fused2 pose_head"), "1 2 1+ 2+ 1+ 2+ 1+ 2+"),
    "chain pair, every level, no upconv ride": (dict(_CHAIN_ALL, upconv_ride=False), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "fused_conv_select_k cv_stage1_fused fused_conv_random_k_dense cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain fused_conv_random_k_dense cv_stage2_fused mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain fused_conv_random_k_dense cv_stage2_fused mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain fused_conv_random_k_dense cv_stage2_fused mlp_fused2 pose_head"), "1 2 1+ 2 1+ 2 1+ 2"),
    "separate": (dict(merge_level_points=0, chain_pair=False), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head"), "1 2 1 2 1 2 1 2"),
    "separate, no upconv ride": (dict(merge_level_points=0, chain_pair=False, upconv_ride=False), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_fused cv_stage2_fused setconv_fused2 mlp_fused2 pose_head"), "1 2 1 2 1 2 1 2"),
    "no sv ride": (dict(sv_ride=False), False, (
        "setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused setconv_fused",
        "cv_stage1_setconv_fused cv_stage2_fused setconv_fused mlp_fused pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_fused mlp_fused2 pose_head_warp",
        "cv_stage1_setconv_fused cv_stage2_fused mlp_fused2 pose_head_warp",
        "fused_conv_select_k cv_stage1_setconv_chain cv_stage2_fused mlp_fused2 pose_head"), "1+ 2 1+ 2 1+ 2 1+ 2"),
}

# (b) the layers in the order a fresh store first meets them; each creates weights, biases and -- but for the pose heads' -- the four
# batch-norm variables, in that order
_CV = ("CV_0", "CV_1", "CV_2", "CV_xyz", "sum_CV_0", "sum_CV_1", "sum_xyz_encoding", "sum_cost_volume_0", "sum_cost_volume_1")
_LEVEL = (["up_sa_layer_layer_l%dw/up_1_0", "up_sa_layer_layer_l%dw/up_1_1", "up_sa_layer_layer_l%dcostvolume/up_1_0",
           "up_sa_layer_layer_l%dcostvolume/up_1_1"] + ["flow_embedding_l%d/" + name for name in _CV] +
          ["up_sa_layer_layer_l%dw/up_2_0", "up_sa_layer_layer_l%dw/up_2_1", "l%d_w_predict/conv_predictor0", "l%d_w_predict/conv_predictor1",
           "up_sa_layer_layer_l%dcostvolume/up_2_0", "up_sa_layer_layer_l%dcostvolume/up_2_1", "l%d_costvolume_predict/conv_predictor0",
           "l%d_costvolume_predict/conv_predictor1", "l%d_big", "l%d_q_det", "l%d_t_det"])
LAYERS = (["sa1/layer%d/conv%d" % (i, j) for i in range(4) for j in range(3)] + ["flow_embedding_l2_origin/" + name for name in _CV] +
          ["new_layer3/conv0", "new_layer3/conv1", "new_layer3/conv2", "l3_costvolume_predict_ww/conv_predictor0",
           "l3_costvolume_predict_ww/conv_predictor1", "l3_big", "l3_q_coarse", "l3_t_coarse"] +
          [name % level for level in (2, 1, 0) for name in _LEVEL])
_POSE_HEADS = ("_big", "_q_coarse", "_t_coarse", "_q_det", "_t_det")
VARIABLES = [layer + leaf for layer in LAYERS
             for leaf in (("/weights", "/biases") if layer.endswith(_POSE_HEADS) else
                          ("/weights", "/biases", "/bn/gamma", "/bn/beta", "/bn/moving_mean", "/bn/moving_variance"))]

# (c) (scope, tag, KT) in draw order
DRAWS = [("sa1/layer0", "random_HW", 135), ("sa1/layer1", "random_HW", 77), ("sa1/layer2", "random_HW", 45), ("sa1/layer3", "random_HW", 45),
         ("flow_embedding_l2_origin", "random_HW_q", 175), ("flow_embedding_l2_origin", "random_HW_p", 15), ("new_layer3", "random_HW", 45),
         ("up_sa_layer_layer_l2w", "random_HW", 105), ("up_sa_layer_layer_l2costvolume", "random_HW", 105),
         ("flow_embedding_l2", "random_HW_q", 75), ("flow_embedding_l2", "random_HW_p", 15),
         ("up_sa_layer_layer_l1w", "random_HW", 105), ("up_sa_layer_layer_l1costvolume", "random_HW", 105),
         ("flow_embedding_l1", "random_HW_q", 175), ("flow_embedding_l1", "random_HW_p", 15),
         ("up_sa_layer_layer_l0w", "random_HW", 105), ("up_sa_layer_layer_l0costvolume", "random_HW", 105),
         ("flow_embedding_l0", "random_HW_q", 451), ("flow_embedding_l0", "random_HW_p", 15)]


@pytest.fixture(scope="module")
def pair():
    f1, f2 = load_pkg("synth").frame_pair(1, 64, 1800, seed=17)
    return torch.from_numpy(np.ascontiguousarray(f1)).to(DEV), torch.from_numpy(np.ascontiguousarray(f2)).to(DEV)


@pytest.mark.parametrize("plan", list(PLANS))
def test_a_plan_launches_creates_and_draws_in_the_recorded_order(plan, pair, monkeypatch):
    """One eager forward of a fresh net under the plan's tuning: the entries it calls, the variables it creates, the orders it draws and the
    cost-volume calls fused.recording() keeps -- each exactly once -- are the recorded ones."""
    L, fused, model, tuning = load_pkg("_lib"), load_pkg("fused"), load_pkg("model"), load_pkg("tuning")
    if fused.fp32_mfma():
        pytest.skip("the fp32-MFMA comparison build has no register-resident kernels: other plans")
    fields, half, stages, recorded = PLANS[plan]
    entries = []
    for door in ("call", "call2", "call3"):
        monkeypatch.setattr(L, door, (lambda real: lambda entry, *args: (entries.append(entry), real(entry, *args))[1])(getattr(L, door)))
    with tuning.override(fused=True, **fields):
        net = model.PWCLONet(DEV, seed=3, feature_dtype=torch.float16 if half else torch.float32)
        with fused.recording() as calls:
            out = net.forward(*pair)
        torch.cuda.synchronize()
    assert all(torch.isfinite(x.float()).all() for x in out)
    assert entries == ["elo_" + name for stage in stages for name in stage.split()]
    assert list(net.store.tf_shapes) == VARIABLES
    assert [key[:3] for key in net.perms._bufs] == DRAWS and net.perms._draws == len(DRAWS)
    assert ["%d%s" % (c[0], "+" if c[3] else "") for c in calls] == recorded.split() and len(calls) == 8

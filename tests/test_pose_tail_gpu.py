"""GPU: the pose tail -- softmax_valid_partial_kernel, softmax_valid_merge_kernel, pose_head_kernel with its in-launch warp,
scatter_min_kernel behind it, mlp_sv_kernel -- on every case of tests/pose_tail_cases.py against the float64 statements of
tests/pose_tail_reference.py, EVERY element within the bound tests/pose_tail_bounds.py derives from the summation structure.  Before a
case runs, the library is asked with the call's real pointers which form it takes (elo_pose_head_form).  The merged vector is read
out of the head exactly (a 0/1 selection head: pose_tail_cases.selection_weights), so the softmax forms are held to their own bound;
the dense layers and the composition are bounded on random weights.  Every call is made twice: the same bits.

Each test prints the worst error it saw as a fraction of its bound (profiles/pose_tail_errors.txt records them per form; the bounds
never come from there)."""
import ctypes

import numpy as np
import pytest
import torch

import pose_tail_bounds as bounds
import pose_tail_cases as table
import pose_tail_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
ids = lambda v: v.name if hasattr(v, "name") else str(v)
BND, D = bounds.BND, np.float64
WORST = {}
WARP_UNITS = 48     # a warped coordinate passes two Hamilton products (7 roundings each), the inverse (10) and the add: 25 -> 48 units


def host(x):
    return x.detach().double().cpu().numpy()


def hold(form, case, got, want, bound):
    """every element finite and within its bound; records and prints the worst error / bound of the form"""
    got, want, bound = np.asarray(got, D), np.asarray(want, D), np.asarray(bound, D)
    assert got.shape == want.shape == bound.shape and np.isfinite(got).all() and np.isfinite(bound).all(), (form, case.name)
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if got.size else 0.0
    WORST[form] = max(WORST.get(form, 0.0), ratio)
    print("POSE_TAIL %-26s %-44s %.3f of the bound (worst |error| %.3e)" % (form, case.name, ratio, float(err.max()) if got.size else 0.0))
    assert ratio <= 1.0, "%s %s: %d of %d elements beyond their bound, worst %.2f x" % (form, case.name, int((err > bound).sum()), err.size, ratio)
    return ratio


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def stored(x):
    """a numpy array as stored -> the device tensor of its dtype (float16 arrays stay fp16 storage)"""
    return t(x)


# ---------------------------------------------------------------------------- (a) the stand-alone op, statistics included
@pytest.mark.parametrize("case", table.SV, ids=ids)
def test_softmax_valid(case):
    ops = load_pkg("_ops")
    f, w = table.logits_features(case.name, case.B, case.N, case.C)
    xyz = table.cloud(case.name, case.B, case.N, case.pattern, case.none_element)
    parts = ops.softmax_valid_parts(case.N)
    assert parts == table.sv_parts(case.N)
    runs = []
    for _ in range(2):
        stats = torch.full((case.B, 2, case.C), float("nan"), device=DEV)
        runs.append((ops._softmax_valid(t(f), t(w), t(xyz), stats), stats))
    torch.cuda.synchronize()
    assert same_bits(runs[0], runs[1])
    got, stats = host(runs[0][0])[:, 0], host(runs[0][1])
    want, wstats = R.softmax_valid(f, w, xyz)
    (pv, pe), Mx, (dv, de) = bounds.merge_seq(BND, bounds.partial_sums(BND, w, f, R.valid(xyz), parts), parts)
    some = wstats[:, 1] > 0
    assert np.array_equal(stats[:, 0], wstats[:, 0])                                  # the maximum, -inf where no point is valid
    assert (got[~some] == 0).all() and (stats[:, 1][~some] == 0).all()
    hold("partial_f32+sv_merge", case, got[some], want[some], pe[some])
    hold("partial_f32+sv_merge/den", case, stats[:, 1][some], wstats[:, 1][some], de[some])


# ---------------------------------------------------------------------------- (b) the head's own partial-sums launch
def _pose_check(form, case, got, weights, q_c, t_c, pooled, e_pooled):
    raw, _big = R.head(pooled, *weights)
    e_raw = bounds.head_bound(pooled, e_pooled, *weights)
    want = R.compose(raw, q_c, t_c)
    eb = bounds.pose_bound(R, raw, e_raw, q_c, t_c)
    for name, g, wnt, e in zip(("q", "t", "q_norm"), got, want, eb):
        hold("%s/%s" % (form, name), case, host(g), wnt, e)


@pytest.mark.parametrize("case", table.HEAD, ids=ids)
def test_pose_head_with_its_partial_sums_launch(case):
    ops = load_pkg("_ops")
    f, w = table.logits_features(case.name, case.B, case.N, case.C, case.storage)
    xyz = table.cloud(case.name, case.B, case.N, case.pattern)
    weights = table.head_weights(case.name, case.C, case.hidden)
    q_c, t_c = table.coarse_pose(case.name, case.B) if case.coarse else (None, None)
    kw = dict(q_coarse=t(q_c), t_coarse=t(t_c)) if case.coarse else {}
    df, dw, dxyz, dev_w = stored(f), stored(w), t(xyz), [t(x) for x in weights]
    assert ops.pose_head_form(df, dw, dxyz, *dev_w, **kw) == table.expected_form(case)
    parts = table.sv_parts(case.N)
    pooled, _ = R.softmax_valid(f, w, xyz)
    pv, pe = bounds.head_pool(BND, bounds.partial_sums(BND, w, f, R.valid(xyz), parts), parts, case.C)
    tag = "partial_%s+head_%s" % (case.storage, "trips16")
    # the pooled vector, read out exactly through a selection head: the softmax's own bound
    for chans in table.readout_channels(case.C, case.hidden):
        sel = [t(x) for x in table.selection_weights(case.C, case.hidden, chans)]
        a, b = (ops.pose_head(df, dw, dxyz, *sel) for _ in range(2))
        assert same_bits(a, b)
        hold(tag + ("/wide" if max(chans) >= 64 else ""), case, host(a[1])[:, :len(chans)], pooled[:, chans], pe[:, chans])
        assert (host(a[0]) == np.array([1.0, 0, 0, 0])).all()
    # dense weights: the two layers and the composition on top
    pose7 = None
    if case.pose7 == "row":
        pose7 = torch.full((case.B, 7), float("nan"), device=DEV)
    got = ops.pose_head(df, dw, dxyz, *dev_w, pose7=pose7, **kw)
    again = ops.pose_head(df, dw, dxyz, *dev_w, **kw)
    torch.cuda.synchronize()
    assert same_bits(got, again)
    _pose_check("head_%s" % ("model" if (case.C, case.hidden) == table.MODEL else "generic"), case, got, weights, q_c, t_c, pooled, pe)
    if case.pose7 == "row":
        assert torch.equal(pose7, torch.cat([got[2], got[1]], -1))
    if case.pose7 == "ring":                                     # 3 slots, 4 calls with their own t bias: the cursor wraps onto slot 0
        ring = ops.PoseRing(3, case.B, DEV)
        outs = []
        for k in range(4):
            wk = list(dev_w)
            wk[5] = dev_w[5] + float(k)
            outs.append(ops.pose_head(df, dw, dxyz, *wk, pose7=ring, **kw))
        torch.cuda.synchronize()
        assert (ring.cursor == 4).all()
        for slot, k in ((0, 3), (1, 1), (2, 2)):
            assert torch.equal(ring.rows[slot], torch.cat([outs[k][2], outs[k][1]], -1)), slot
        assert not torch.equal(outs[0][1], outs[3][1])


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("C,hidden", (table.MODEL,) + table.GENERIC, ids=lambda v: str(v))
def test_dense_layers_without_rounding(C, hidden, storage):
    """The worst-case bound of the two dense layers adds the roundings of every hidden unit with one sign (it is 100 to 1000 times
    what random weights show: profiles/pose_tail_errors.txt).  Here nothing rounds in them (pose_tail_cases.integer_head): t of the
    coarsest level is the float64 value bit for bit, and q, q_norm and the composed pose carry the composition's own units only -- a
    missing term, a wrong index or a wrong stride in either layer is an error of whole units."""
    ops = load_pkg("_ops")
    B = 3
    name = "dense_%d_%d_%s" % (C, hidden, storage)
    case = table.Head(name, B, 1, C, hidden, storage, True, "none", "all")
    f, weights = table.integer_head(name, B, C, hidden)
    w = np.zeros_like(f)
    xyz = table.cloud(name, B, 1, "all")
    dt = np.float16 if storage == "f16" else np.float32
    args = (t(f.astype(dt)), t(w.astype(dt)), t(xyz)) + tuple(t(x) for x in weights)
    raw, _big = R.head(f[:, 0], *weights)
    assert np.array_equal(raw, np.round(raw)) and np.abs(raw).max() < 2 ** 24
    q_c, t_c = table.coarse_pose(name, B)
    form = "head_%s_exact" % ("model" if (C, hidden) == table.MODEL else "generic")
    plain = ops.pose_head(*args)
    assert np.array_equal(host(plain[1]), raw[:, 4:])                                # t = t_det: exact
    for coarse, got in ((False, plain), (True, ops.pose_head(*args, q_coarse=t(q_c), t_coarse=t(t_c)))):
        qc, tc = (q_c, t_c) if coarse else (None, None)
        for part, g, wnt, e in zip(("q", "t", "q_norm"), got, R.compose(raw, qc, tc), bounds.pose_bound(R, raw, np.zeros((B, 7)), qc, tc)):
            hold("%s/%s" % (form, part), case, host(g), wnt, e)


# ---------------------------------------------------------------------------- (c) hand-made partial sums into the in-head merge
def _partials(ops, B, mx, den, acc, N=4):
    """an SvPartials whose scratch holds the (B, parts, 64) triples at the layout's pitch (3, B, ELO_SV_MAX_PARTS, 64)"""
    sv = ops.SvPartials(torch.ones((B, N, 3), device=DEV))
    parts = mx.shape[1]
    full = np.full((3, B, table.SV_MAX_PARTS, 64), np.nan, np.float32)      # (slices beyond `parts` are never read: NaN would show)
    full[0, :, :parts], full[1, :, :parts], full[2, :, :parts] = mx, den, acc
    sv.scratch.copy_(t(full.reshape(-1)))
    sv.parts = parts
    return sv


@pytest.mark.parametrize("case", table.MERGE, ids=ids)
def test_in_head_merge_of_hand_made_partial_sums(case):
    ops = load_pkg("_ops")
    mx, den, acc = table.merge_triples(case)
    sv = _partials(ops, case.B, mx, den, acc)
    dummy = torch.zeros((case.B, 4, 64), device=DEV)
    assert ops.pose_head_form(dummy, dummy, sv.xyz, *[t(x) for x in table.model_selection_weights(0)[1]], partials=sv) == table.expected_form(case)
    want = R.merge_triples(mx, den, acc)
    pv, pe = bounds.merge_head(BND, bounds.lift_triple(BND, mx, den, acc), case.parts)
    got = np.full((case.B, 64), np.nan)
    for call in range(22):                                       # all 64 channels, three per call
        chans, weights = table.model_selection_weights(call)
        out = ops.pose_head(dummy, dummy, sv.xyz, *[t(x) for x in weights], partials=sv)
        got[:, chans] = host(out[1])[:, :len(chans)]
        if call == 0:
            assert same_bits(out, ops.pose_head(dummy, dummy, sv.xyz, *[t(x) for x in weights], partials=sv))
    hold("head_merge/%s" % ("trips16" if case.parts <= 64 else "trips32"), case, got, want, pe)
    weights = table.head_weights(case.name, 64, 256)
    q_c, t_c = table.coarse_pose(case.name, case.B)
    out = ops.pose_head(dummy, dummy, sv.xyz, *[t(x) for x in weights], q_coarse=t(q_c), t_coarse=t(t_c), partials=sv)
    _pose_check("head_model", case, out, weights, q_c, t_c, want, pe)


# ---------------------------------------------------------------------------- (d) the MLP ride
@pytest.mark.parametrize("case", table.RIDE, ids=ids)
def test_mlp_ride_leaves_the_partial_sums(case):
    ops, fused, tuning, L = load_pkg("_ops"), load_pkg("fused"), load_pkg("tuning"), load_pkg("_lib")
    inp = table.ride_inputs(case)
    xyz = table.ride_cloud(case)
    layer = lambda W, b: [fused.PackedDense(t(W), t(b), False, None, False)]
    x, la = stored(inp["x"]), layer(inp["W"], inp["b"])
    with tuning.override(chain_forms=0, small_tile_units=table.tile_units(case.tile)):
        if case.pair:
            x2, lb = stored(inp["x2"]), layer(inp["W2"], inp["b2"])
            plain, plain_f = fused.mlp_pair([x], la, [x2], lb)
            sv = ops.SvPartials(t(xyz))
            logits, feature = fused.mlp_pair([x], la, [x2], lb, sv=sv)
            assert torch.equal(plain_f, feature)
            a, _o, _k = fused._mlp_args([x], la)
            b, _o2, _k2 = fused._mlp_args([x2], lb)
        else:
            feature = stored(inp["feature"])
            plain = fused.mlp([x], la)
            sv = ops.SvPartials(t(xyz), feature)
            logits = fused.mlp([x], la, sv=sv)
            a, _o, _k = fused._mlp_args([x], la)
            b = None
        a.sv_npoints = case.N
        want_parts = L.lib().elo_mlp_sv_parts(ctypes.byref(a), ctypes.byref(b) if b is not None else None)
        form = fused.mlp_form(dict(sources=[x], layers=la)) if not case.pair else None
    torch.cuda.synchronize()
    tiles = -(-case.N // case.tile)
    assert sv.parts == want_parts == tiles and torch.equal(plain, logits)      # the expected count is the library's; same layer: same bits
    assert form in (None, "tile%d/split" % case.tile)
    lg, ft = host(logits), host(feature)                          # the rows as stored: what the reduction read
    ok = R.valid(xyz)
    want, _ = R.softmax_valid(ft, lg, xyz)
    # the triples themselves: each tile's maximum exact, and their float64 merge within the reduction's bound
    scratch = host(sv.scratch).reshape(3, case.B, table.SV_MAX_PARTS, 64)[:, :, :tiles]
    tb = bounds.ride_sums(BND, lg, ft, ok, case.tile)
    assert np.array_equal(scratch[0], tb[0])
    empty = ~np.isfinite(tb[0])
    assert (scratch[1][empty] == 0).all() and (scratch[2][empty] == 0).all()
    pv, pe = bounds.merged_exactly(tb)
    hold("ride_%s/tile%d" % (case.storage, case.tile), case, R.merge_triples(*scratch), want, pe)
    # hand-over against two launches, both against float64
    hv, he = bounds.merge_head(BND, tb, tiles)
    parts2 = table.sv_parts(case.N)
    tv, te = bounds.head_pool(BND, bounds.partial_sums(BND, lg, ft, ok, parts2), parts2, 64)
    dxyz = t(xyz)
    one, two = np.zeros((case.B, 6)), np.zeros((case.B, 6))
    for k, chans in enumerate(([0, 1, 2], [61, 62, 63])):
        sel = [t(x) for x in table.selection_weights(64, 256, chans)]
        assert ops.pose_head_form(feature, logits, dxyz, *sel, partials=sv) == table.expected_form(case)
        a1 = ops.pose_head(feature, logits, dxyz, *sel, partials=sv)
        assert same_bits(a1, ops.pose_head(feature, logits, dxyz, *sel, partials=sv))
        a2 = ops.pose_head(feature, logits, dxyz, *sel)
        one[:, 3 * k:3 * k + 3], two[:, 3 * k:3 * k + 3] = host(a1[1]), host(a2[1])
    ch = [0, 1, 2, 61, 62, 63]
    hold("ride+head_merge", case, one, want[:, ch], he[:, ch])
    hold("partial_%s+head_trips16" % case.storage, case, two, want[:, ch], te[:, ch])
    assert (np.abs(one - two) <= he[:, ch] + te[:, ch]).all()
    weights = table.head_weights(case.name, 64, 256)
    q_c, t_c = table.coarse_pose(case.name, case.B)
    kw = dict(q_coarse=t(q_c), t_coarse=t(t_c))
    dev_w = [t(x) for x in weights]
    p1 = ops.pose_head(feature, logits, dxyz, *dev_w, partials=sv, **kw)
    p2 = ops.pose_head(feature, logits, dxyz, *dev_w, **kw)
    _pose_check("head_model", case, p1, weights, q_c, t_c, want, he)
    _pose_check("head_model", case, p2, weights, q_c, t_c, want, te)


# ---------------------------------------------------------------------------- (e) the warp inside the head
def _garbage(buf):
    buf.out_xyz.fill_(float("nan")); buf.scratch.fill_(-1)
    if buf.out_feat is not None:
        buf.out_feat.fill_(3.0)
    return buf


@pytest.mark.parametrize("case", table.WARP, ids=ids)
def test_warp_inside_the_head(case):
    ops = load_pkg("_ops")
    B, N, H, W, C = case.B, case.N, case.H, case.W, case.C
    dt = torch.float16 if case.storage == "f16" else torch.float32
    f, w = table.logits_features(case.name, B, 17, 64, case.storage)
    hxyz = table.cloud(case.name, B, 17, "random")
    weights = table.pose_weights(case, B)
    xyz, special = table.warp_cloud(case, R)
    feat = table.rng_of("wf|" + case.name).normal(0, 1, (B, N, C)).astype(np.float16 if case.storage == "f16" else np.float32) if C else None
    df, dw, dh, dev_w, dx, dfeat = stored(f), stored(w), t(hxyz), [t(x) for x in weights], t(xyz), (stored(feat) if C else None)
    plain = ops.pose_head(df, dw, dh, *dev_w)
    runs = []
    for _ in range(2):
        buf = _garbage(ops.ProjectionBuffers(B, N, H, W, C, DEV, dt))
        assert ops.pose_head_form(df, dw, dh, *dev_w, clear=buf, warp=(dx, dfeat)) == table.expected_form(case)
        pose = ops.pose_head(df, dw, dh, *dev_w, clear=buf, warp=(dx, dfeat))
        torch.cuda.synchronize()
        cells = buf.scratch[B * H * W + 4 * B: B * H * W + 4 * B + B * N].clone().reshape(B, N)
        runs.append((pose, buf.result, cells, buf))
    (pose, (warped, out_xyz, out_feat), cells, buf) = runs[0]
    assert same_bits(pose, plain) and same_bits(pose, runs[1][0])                      # the same q, t, q_norm bits as the plain call
    assert same_bits(runs[0][1][:2], runs[1][1][:2]) and torch.equal(cells, runs[1][2])
    # the pose: the head's raw output IS the biases; the composition on top
    raw = np.concatenate([weights[3], weights[5]])[None].repeat(B, 0).astype(D)
    e_raw = np.zeros((B, 7))                                     # (W_q = W_t = 0: every product is by 0 and b + 0 is exact)
    for name, g, wnt, e in zip(("q", "t", "q_norm"), pose, R.compose(raw), bounds.pose_bound(R, raw, e_raw, None, None)):
        hold("head_model/%s" % name, case, host(g), wnt, e)
    # the warp, on the pose the launch returned
    q, tt = host(pose[0]), host(pose[1])
    want = R.warp(xyz, q, tt)
    col, tmp, r = R.cell_coordinates(want, H, W)
    near = lambda v: np.abs(v - np.round(v)) < table.BORDER
    origin = (r > 0) & (r < table.ORIGIN_RANGE)
    excluded = ((near(col) | near(tmp)) & (r > 0)) | origin
    assert excluded.mean(-1).max() <= table.EXCLUDED_CAP
    scale = (np.abs(q).sum(-1) ** 2 / (q * q).sum(-1))[:, None, None]
    e_warp = WARP_UNITS * bounds.U * (np.abs(xyz.astype(D)).sum(-1, keepdims=True) * scale + np.abs(tt)[:, None, :]) * np.ones(3)
    gw = host(warped)
    hold("warp", case, gw[~origin], want[~origin], e_warp[~origin])
    w32 = R.warp32(xyz, pose[0].cpu().numpy(), pose[1].cpu().numpy())
    zero = ~R.valid(xyz) | origin                                 # zero points and the point on the origin: their BITS (signs of zero)
    assert np.array_equal(warped.cpu().numpy().view(np.uint32)[zero], w32.view(np.uint32)[zero])
    if "origin" in special:
        assert origin[:, special["origin"]].all() and (gw[:, special["origin"]] == 0).all()
    # the cell rule, exactly; the point on the origin by the float32 statement
    want_cell = np.where(origin, R.cells(w32.astype(D), H, W), R.cells(want, H, W))
    got_cell = cells.cpu().numpy()
    assert np.array_equal(got_cell[~excluded | origin], want_cell[~excluded | origin])
    # the winner rule: the image of the launch's own warped points under the reference cells, exactly; features to the atomic order of summed ties
    atol = 1e-3 if case.storage == "f16" else 1e-4
    for b in range(B):
        img, fimg, won = R.project(warped[b].cpu().numpy(), None if feat is None else feat[b], want_cell[b], H, W)
        keep = np.ones(H * W, bool)
        keep[np.concatenate([want_cell[b][excluded[b] & ~origin[b]], got_cell[b][excluded[b] & ~origin[b]]]).astype(int)] = False
        gimg = host(out_xyz[b]).reshape(H * W, 3)
        differ = np.flatnonzero(keep & (gimg != img.reshape(H * W, 3)).any(-1))
        assert differ.size == 0, [(int(c), gimg[c].tolist(), img.reshape(H * W, 3)[c].tolist(), np.flatnonzero(want_cell[b] == c).tolist()) for c in differ[:4]]
        if C:
            assert np.allclose(host(out_feat[b]).reshape(H * W, C)[keep], fimg.reshape(H * W, C)[keep], atol=atol, rtol=1e-3 if case.storage == "f16" else 1e-6)
        for i, j in special.get("ties", ()):
            assert won[i] and won[j] and np.array_equal(host(out_xyz[b]).reshape(H * W, 3)[want_cell[b, i]], 2.0 * gw[b, i])
    # ... and the stand-alone warp_project on the returned pose: warped points, cells and image bit for bit
    alone = ops.ProjectionBuffers(B, N, H, W, C, DEV, dt)
    sw, sxyz, sfeat = ops.warp_project(dx, dfeat, pose[0], pose[1], H, W, buffers=alone)
    handed = ops.warp_project(dx, dfeat, pose[0], pose[1], H, W, buffers=buf)          # hands the launch's own result over
    torch.cuda.synchronize()
    assert buf.result is None and same_bits((sw, sxyz), handed[:2])
    assert torch.equal(alone.scratch[B * H * W + 4 * B: B * H * W + 4 * B + B * N].reshape(B, N), cells)
    if C:
        assert torch.allclose(sfeat.float(), handed[2].float(), atol=atol)


def test_zz_worst_ratio_per_form():
    """The record behind profiles/pose_tail_errors.txt (run the file with -s): every form's worst error / bound, at most 1."""
    for form in sorted(WORST):
        print("POSE_TAIL_WORST %-30s %.3f" % (form, WORST[form]))
    assert all(v <= 1.0 for v in WORST.values())

"""The decoders' forward across operand magnitudes and with non-finite values in the map (-m gpu): the range contract of include/nsk.h
(nsk_set_matmul_mode) and DESIGN.md section 2.  The transforms of tests/operand_range.py move hidden values, weights and grid features over
34 binary orders of magnitude WITHOUT changing the function (proved on the CPU, tests/test_operand_range_cpu.py), so the unscaled fp32 / fp64
oracle results are the reference at every scale.  Non-finite expectations come from ATen on the CPU (oracle/torch_ref.py); the plain-C
oracle's ReLU drops NaNs and is not a reference here (see test_operand_range_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import operand_range as OR
import scenes
from gpu_util import cu, make_ctx
from scenes import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4
SC = OR.op_scene()
PTS = OR.op_points(SC)
RAYS = OR.op_rays(SC)
INB = np.all((PTS < SC["bound"][:, 1]) & (PTS > SC["bound"][:, 0]), axis=1)
MODES = [2, 1, 0]


@functools.lru_cache(maxsize=None)
def _ref_points(stage, o32, o64):
    """fp32 and fp64 oracle raw at PTS (unscaled scene), computed once per stage"""
    return tuple(o.eval_points(SC["bound"], SC["grids"], SC["decoders"], stage, PTS) for o in (o32, o64))


@functools.lru_cache(maxsize=None)
def _ref_render(stage, o32, o64):
    return tuple(o.render_forward(o.opts(SC["bound"]), SC["grids"], SC["decoders"], stage, RAYS["rays_o"], RAYS["rays_d"], RAYS["gt_depth"]) for o in (o32, o64))


@functools.lru_cache(maxsize=None)
def _preacts(stage, which, batch, o64):
    """fp64 oracle ReLU inputs [M, 5, 32] of decoder `which` at scale 1 over PTS inside the bound ("points") or the samples of RAYS ("rays")"""
    if batch == "points":
        return o64.point_preacts(SC["bound"], SC["grids"], SC["decoders"], stage, which, PTS)[INB]
    return o64.preacts(o64.opts(SC["bound"]), SC["grids"], SC["decoders"], stage, which, RAYS["rays_o"], RAYS["rays_d"], RAYS["gt_depth"])


def _peaks(stage, batch, o64):
    return {w: np.abs(_preacts(stage, w, batch, o64)).max(axis=(0, 2)) for w in OR.DECODERS_OF[stage]}


def _load(ctx, grids, decoders, stage):
    for k in OR.DECODERS_OF[stage]:
        ctx.grid_upload(k, grids[k])
        ctx.decoder_upload(k, decoders[k])


def _values(raw):
    """what is compared of an eval_points result: everything inside the bound, the colour outside (the occupancy there is the constant 100)"""
    return np.concatenate([raw[INB].ravel(), raw[~INB, :3].ravel()])


def _check(got, ref32, ref64, what, worst):
    """the project's allowances: rel L2 against the fp32 oracle below TOL; against the fp64 oracle at most 3 x the fp32 oracle's own error
    plus 1e-5 (test_forward_bf16_split_mode_matches_oracle)"""
    e32, e64, eo = rel_l2(got, ref32), rel_l2(got, ref64), rel_l2(ref32, ref64)
    worst[0], worst[1] = max(worst[0], e32), max(worst[1], e64)
    assert np.isfinite(got).all(), what
    assert e32 < TOL, "%s: %.2e against the fp32 oracle" % (what, e32)
    assert e64 <= 3 * eo + 1e-5, "%s: %.2e against the fp64 oracle (fp32 oracle: %.2e)" % (what, e64, eo)
    return e32, e64


# ---- 2. in-range magnitudes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stage", ["coarse", "middle", "fine", "color"])
def test_eval_points_across_magnitudes(stage, mode, oracle32, oracle64):
    """nsk_eval_points with the peak hidden value of each block near 2^-14, 2^-8, 1, 2^8, 2^14 (weights below 2^15), all blocks at once with
    alternating signs, and each level's features at those peaks: the 1e-4 contract and the fp64 allowance hold at every scale in every
    matmul mode; mode 0 (plain fp32) is bit-identical to its own unscaled run."""
    r32, r64 = _ref_points(stage, oracle32, oracle64)
    ctx = make_ctx(SC)
    ctx.set_matmul_mode(mode)
    base = ctx.eval_points(stage, cu(PTS)).cpu().numpy()
    worst = [0.0, 0.0]
    _check(_values(base), _values(r32), _values(r64), "unscaled", worst)
    assert (base[~INB, 3] == 100).all()
    per_target = {}
    for label, g, d in OR.in_range_cases(SC, stage, _peaks(stage, "points", oracle64)):
        _load(ctx, g, d, stage)
        raw = ctx.eval_points(stage, cu(PTS)).cpu().numpy()
        e32, e64 = _check(_values(raw), _values(r32), _values(r64), "%s mode %d %s" % (stage, mode, label), worst)
        per_target[label] = (e32, e64)
        if mode == 0:
            assert np.array_equal(raw, base), label
    lo = max(per_target.items(), key=lambda kv: kv[1][1])
    print("eval_points %s mode %d: worst rel L2 over %d scaled scenes: %.2e vs fp32 oracle, %.2e vs fp64 oracle (at %s); fp32 oracle vs fp64 %.2e"
          % (stage, mode, len(per_target), worst[0], worst[1], lo[0], rel_l2(_values(r32), _values(r64))))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stage", ["fine", "color"])
def test_render_forward_across_magnitudes(stage, mode, oracle32, oracle64):
    """the same scaled scenes through nsk_render_forward (48 rays x (32 + 16) samples; peaks read over the rays' samples): depth, weights,
    variance and colour per scale"""
    r32, r64 = _ref_render(stage, oracle32, oracle64)
    ctx = make_ctx(SC)
    ctx.set_matmul_mode(mode)
    ro, rd, gd = cu(RAYS["rays_o"]), cu(RAYS["rays_d"]), cu(RAYS["gt_depth"])
    names = ["depth", "weights", "var"] + (["rgb"] if stage == "color" else [])

    def run():
        rgb, depth, var, w = ctx.render_forward(stage, ro, rd, gd)
        return dict(rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy(), var=var.cpu().numpy(), weights=w.cpu().numpy())

    base = run()
    worst = {k: [0.0, 0.0] for k in names}
    cases = OR.in_range_cases(SC, stage, _peaks(stage, "rays", oracle64))
    for label, g, d in cases:
        _load(ctx, g, d, stage)
        out = run()
        for k in names:
            _check(out[k], r32[k], r64[k], "%s mode %d %s %s" % (stage, mode, label, k), worst[k])
            if mode == 0:
                assert np.array_equal(out[k], base[k]), (label, k)
    print("render_forward %s mode %d: worst rel L2 over %d scaled scenes (vs fp32 oracle, vs fp64 oracle):" % (stage, mode, len(cases)),
          {k: ("%.2e" % v[0], "%.2e" % v[1]) for k, v in worst.items()}, "fp32 oracle vs fp64:", {k: "%.2e" % rel_l2(r32[k], r64[k]) for k in names})


# ---- 3. over the edge ---------------------------------------------------------------------------------------------------------------
def _subset_ok(got, ref32, ref64, ok, what):
    """the finite outputs (rows `ok`) within the in-range allowances of the truth"""
    if not ok.any():
        return
    g, a, b = got[ok], ref32[ok], ref64[ok]
    e32, e64, eo = rel_l2(g, a), rel_l2(g, b), rel_l2(a, b)
    assert e32 < TOL and e64 <= 3 * eo + 1e-5, "%s: %d finite outputs are wrong: %.2e against the fp32 oracle, %.2e against the fp64 oracle (fp32 oracle %.2e)" % (
        what, int(ok.sum()), e32, e64, eo)


def _over_range_cases(stage, batch, o64):
    """[(label, grids, decoders, ref32, ref64 or None)]: each block of each decoder with its peak hidden value at 2^17 and 2^20 (function
    unchanged: the unscaled oracle results are the truth); features of each level at a peak of 2^17 >= 1e5; one hidden weight set to 1e5
    (a different function: its own oracle results, marked by None).  The non-vacuity assertions are made here, on the fp64 oracle's numbers."""
    cases = []
    for which in OR.DECODERS_OF[stage]:
        pre = _preacts(stage, which, batch, o64)
        for i in range(5):
            for t in (17, 20):
                a = OR.exponent_for(np.abs(pre[:, i]).max(), t)
                if t == 20:
                    big = pre[:, i] * 2.0 ** a
                    both = ((big > OR.F16_MAX).any(axis=1) & (big < -OR.F16_MAX).any(axis=1))
                    assert both.any(), "no sample with hidden values beyond fp16 of both signs in block %d of %s" % (i, which)
                cases.append(("%s block %d x 2^%d" % (which, i, a), SC["grids"], dict(SC["decoders"], **{which: OR.rebalance(SC["decoders"][which], which, i, a)}), False))
    for level in OR.DECODERS_OF[stage]:
        peak = float(np.abs(SC["grids"][level]).max())
        a = int(np.ceil(np.log2(1e5 / peak)))
        g, d = OR.scale_features(SC["grids"], SC["decoders"], level, a)
        assert np.isfinite(g[level]).all() and (g[level] > OR.F16_MAX).any() and (g[level] < -OR.F16_MAX).any() and np.abs(g[level]).max() >= 1e5
        cases.append(("%s features x 2^%d" % (level, a), g, d, False))
    for which in OR.DECODERS_OF[stage]:
        lay = OR.T.decoder_layout(which)
        P = SC["decoders"][which].copy()
        OR._view(P, lay["W"][1])[3, 5] = 1e5
        cases.append(("%s pts_linear[1].weight[3, 5] = 1e5" % which, SC["grids"], dict(SC["decoders"], **{which: P}), True))
    return cases


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stage", ["coarse", "color"])
def test_eval_points_beyond_fp16_stays_exact(stage, mode, oracle32, oracle64):
    """Hidden values, features and a weight beyond fp16's range (65504) through nsk_eval_points.  Its launches (one decoder each, as the
    one-decoder stages coarse and middle of the renderer) run on the fp32 MFMA whatever the matmul mode -- measured: the three modes give
    the same bits -- so there is no limit here short of fp32's: every point is finite and within the in-range allowances of the truth in
    every mode.  (The two-piece operands and their limit are reached through nsk_render_forward, next test.)"""
    r32, r64 = _ref_points(stage, oracle32, oracle64)
    o32, o64 = oracle32, oracle64
    ctx = make_ctx(SC)
    ctx.set_matmul_mode(mode)
    n_bad = 0
    for label, g, d, own_ref in _over_range_cases(stage, "points", oracle64):
        a32, a64 = (tuple(o.eval_points(SC["bound"], g, d, stage, PTS) for o in (o32, o64)) if own_ref else (r32, r64))
        _load(ctx, g, d, stage)
        raw = ctx.eval_points(stage, cu(PTS)).cpu().numpy()
        ok = np.isfinite(raw).all(axis=1)
        n_bad += int((~ok).sum())
        what = "%s mode %d %s" % (stage, mode, label)
        assert ok.all(), "%s: %d non-finite points" % (what, int((~ok).sum()))
        vals = lambda r: np.where(INB[:, None], r, r * np.array([1, 1, 1, 0], r.dtype))      # outside the bound: the colour only
        _subset_ok(vals(raw), vals(a32), vals(a64), ok, what)
    print("eval_points %s mode %d beyond fp16: %d non-finite point outputs in all" % (stage, mode, n_bad))


@pytest.mark.parametrize("mode", MODES)
def test_render_forward_beyond_fp16_is_never_silently_wrong(mode, oracle32, oracle64):
    """The same scenes per ray through nsk_render_forward (colour stage: the middle, fine and colour decoders on the operands of the matmul
    mode).  Mode 2: a ray is non-finite or within the in-range allowances of the truth, never a finite wrong number -- and some rays must
    come out non-finite, or the test would not have reached the limit; modes 1 and 0 have no such limit: every ray finite and within the
    allowances."""
    stage = "color"
    r32, r64 = _ref_render(stage, oracle32, oracle64)
    o32, o64 = oracle32, oracle64
    ctx = make_ctx(SC)
    ctx.set_matmul_mode(mode)
    ro, rd, gd = cu(RAYS["rays_o"]), cu(RAYS["rays_d"]), cu(RAYS["gt_depth"])
    n_bad = 0
    for label, g, d, own_ref in _over_range_cases(stage, "rays", oracle64):
        a32, a64 = (tuple(o.render_forward(o.opts(SC["bound"]), g, d, stage, RAYS["rays_o"], RAYS["rays_d"], RAYS["gt_depth"]) for o in (o32, o64)) if own_ref else (r32, r64))
        _load(ctx, g, d, stage)
        rgb, depth, var, w = ctx.render_forward(stage, ro, rd, gd)
        out = dict(rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy()[:, None], weights=w.cpu().numpy())
        ok = np.all([np.isfinite(v).all(axis=1) for v in out.values()], axis=0)
        n_bad += int((~ok).sum())
        what = "%s mode %d %s" % (stage, mode, label)
        if mode != 2:
            assert ok.all(), "%s: %d non-finite rays" % (what, int((~ok).sum()))
        for k, v in out.items():
            _subset_ok(v, a32[k].reshape(v.shape), a64[k].reshape(v.shape), ok, what + " " + k)
    print("render_forward mode %d beyond fp16: %d non-finite rays in all" % (mode, n_bad))
    assert mode != 2 or n_bad > 0


# ---- 4. non-finites already in the map -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stage", ["coarse", "color"])
def test_poisoned_voxel_reaches_exactly_the_points_that_touch_it(stage, mode):
    """One voxel row of each level in turn set to +inf, -inf, NaN 0x7fc00000 or NaN 0xffc00000 (written by bit pattern), in all 32 channels or in
    one: the outputs of nsk_eval_points that are non-finite are exactly those ATen makes non-finite (element by element), and every
    untouched point is bit-identical to the clean run."""
    ctx = make_ctx(SC)
    ctx.set_matmul_mode(mode)
    clean = ctx.eval_points(stage, cu(PTS)).cpu().numpy()
    assert np.isfinite(clean).all()
    for level in OR.DECODERS_OF[stage]:
        zyx = OR.central_voxel(SC, level)
        for name in OR.POISON_BITS:
            for channels in (None, [5]):
                g = OR.poison_voxel(SC["grids"], level, zyx, name, channels)
                want = OR.aten_eval_points(SC, stage, PTS, grids=g)
                ctx.grid_upload(level, g[level])
                raw = ctx.eval_points(stage, cu(PTS)).cpu().numpy()
                what = "%s mode %d, %s voxel %s = %s in %s" % (stage, mode, level, zyx, name, "all channels" if channels is None else "channel 5")
                touched = ~np.isfinite(want).all(axis=1)
                assert touched.sum() >= 3, what
                miss = np.isfinite(raw) != np.isfinite(want)
                assert not miss.any(), "%s: %d outputs finite here / non-finite in ATen or the reverse, e.g. point %d: %s (ATen %s)" % (
                    what, int(miss.sum()), np.argwhere(miss)[0][0], raw[np.argwhere(miss)[0][0]], want[np.argwhere(miss)[0][0]])
                assert np.array_equal(raw[~touched], clean[~touched]), what
        ctx.grid_upload(level, SC["grids"][level])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", scenes.LEVELS)
def test_poisoned_decoder_makes_every_output_non_finite(which, mode):
    """one NaN (either sign bit) in a hidden weight, or in a hidden bias, of a decoder: every output of that decoder is non-finite (ATen: the
    NaN reaches every unit of the next layer)"""
    lay = OR.T.decoder_layout(which)
    ctx = make_ctx(SC)
    ctx.set_matmul_mode(mode)
    for name in ("nan+", "nan-"):
        for key, idx in (("W", (7, 9)), ("b", (11,))):
            for layer in (1, 4):
                P = SC["decoders"][which].copy()
                OR._view(P, lay[key][layer])[idx] = OR.poison_value(name)
                want = OR.aten_eval_points(SC, which, PTS, decoders=dict(SC["decoders"], **{which: P}))
                ctx.decoder_upload(which, P)
                raw = ctx.eval_points(which, cu(PTS)).cpu().numpy()
                what = "%s mode %d %s in %s[%d]%s" % (which, mode, name, key, layer, idx)
                if which == "color":
                    assert not np.isfinite(want[:, :3]).any() and not np.isfinite(raw[:, :3]).any(), what
                else:
                    assert not np.isfinite(want[INB, 3]).any(), what
                    assert not np.isfinite(raw[INB, 3]).any(), "%s: %d of %d points came out finite" % (what, int(np.isfinite(raw[INB, 3]).sum()), int(INB.sum()))


@pytest.mark.parametrize("stage,trainable", [("fine", []), ("color", ["color"])])
def test_map_step_with_a_nan_voxel(stage, trainable):
    """One nsk_map_step (NSK_GRAD_GRIDS | NSK_GRAD_DECODERS, no ray mask) on a scene with one NaN voxel in the stage's own level.  Expected is
    what ATen autograd gives on the CPU chain (render_batch_ray, loss_map, backward): the loss is non-finite; the gradient row of every voxel
    touched by a ray with a poisoned sample is non-finite; rows of voxels touched by clean rays only are finite and agree (1e-5, the
    tolerance for regrouped sums of test_backward_chains_keep_relative_accuracy_across_decades) with a step on the clean rays alone; the
    trainable decoder's gradient is non-finite.  Which rows and which decoder entries are non-finite is read off ATen's result one by one:
    ATEN DECIDES, and it differs from the rule above in the colour stage with the NaN in the colour level: the depth stays finite, the colour
    loss |gt - c| has the derivative sgn(NaN) = 0, so the colour level's gradient and part of the decoder's stay finite (zero contributions
    of the poisoned rays), while the middle and fine levels get NaN through d rgb / d weights = the NaN colour itself."""
    rays = OR.op_rays(SC, zero_frac=0.0)
    level = "fine" if stage == "fine" else "color"
    g = OR.poison_voxel(SC["grids"], level, OR.central_voxel(SC, level), "nan+")
    gmax = float(rays["gt_depth"].max())
    use_color = stage == "color"
    want = OR.aten_map_step(SC, stage, rays, trainable, 0.2, use_color, gmax, grids=g)
    bad_ray = ~(np.isfinite(want["depth"]) & np.isfinite(want["rgb"]).all(axis=1))
    assert 2 <= bad_ray.sum() <= len(bad_ray) - 8 and not np.isfinite(want["loss"])

    def step(sel, grids):
        ctx = make_ctx(dict(SC, grids=grids), trainable=trainable)
        loss = torch.zeros(1, device="cuda")
        a = [cu(rays[k][sel]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]
        ctx.map_step(stage, a[0], a[1], a[2], a[3], gmax, 0.2, use_color, flags=3, loss=loss)
        ctx.sync()
        return float(loss), {k: ctx.grid_download(k, grad=True) for k in OR.DECODERS_OF[stage]}, {k: ctx.decoder_download(k, grad=True) for k in trainable}

    loss, gg, gd = step(np.ones(len(bad_ray), bool), g)
    _, gg_clean, _ = step(~bad_ray, g)
    # the voxels a poisoned ray touches: non-zero gradient rows of ATen's step on those rays alone in the CLEAN scene
    hit_by_bad = OR.aten_map_step(SC, stage, {k: rays[k][bad_ray] for k in ("rays_o", "rays_d", "gt_depth", "gt_color")}, [], 0.2, use_color, gmax)["g_grids"]
    assert not np.isfinite(loss)
    for k in OR.DECODERS_OF[stage]:
        fin_want, fin = OR.voxel_rows_finite(want["g_grids"][k]), OR.voxel_rows_finite(gg[k])
        assert fin_want.any()
        assert np.array_equal(fin, fin_want), "%s: %d voxel rows finite here / non-finite in ATen or the reverse" % (k, int((fin != fin_want).sum()))
        assert np.isfinite(gg_clean[k]).all()
        # (a row that is non-finite in ATen is touched by a poisoned ray even where that ray's gradient in the clean scene is exactly zero)
        clean_only = ~(hit_by_bad[k] != 0).any(axis=0) & fin_want
        assert clean_only.sum() >= 3
        e = rel_l2(gg[k][:, clean_only], gg_clean[k][:, clean_only])
        both = fin_want & ~clean_only                                  # finite in ATen although a poisoned ray passes: figure only
        e_at = rel_l2(gg[k][:, both], want["g_grids"][k][:, both]) if both.any() else 0.0
        print("map_step %s, level %s: %d non-finite voxel rows; %d rows of clean rays only differ from the clean rays' own step by %.2e; %d finite rows that a "
              "poisoned ray touches differ from ATen's by %.2e" % (stage, k, int((~fin).sum()), int(clean_only.sum()), e, int(both.sum()), e_at))
        assert e < 1e-5, (k, e)
    assert any((~OR.voxel_rows_finite(want["g_grids"][k])).any() for k in OR.DECODERS_OF[stage])
    for k in trainable:
        lay = OR.T.decoder_layout(k)
        body = slice(lay["W"][0][0], None)                           # the embedding matrix B is no parameter of the optimiser
        fin_want, fin = np.isfinite(want["g_decoders"][k][body]), np.isfinite(gd[k][body])
        print("map_step %s: decoder %s gradient: %d of %d entries non-finite (ATen: %d)" % (stage, k, int((~fin).sum()), fin.size, int((~fin_want).sum())))
        assert (~fin_want).any() and (~fin).any()
        assert np.array_equal(fin, fin_want), "%d decoder gradient entries finite here / non-finite in ATen or the reverse" % int((fin != fin_want).sum())

"""GPU tests (-m gpu): a decoder launch's results must not depend on how the host planner (csrc/nsk_split.h) divides its workgroups over
the roles.  The planner's tuning keys are pushed to their extremes, nsk_debug_last_split shows the split that was launched, and

  forward   everything a sample's arithmetic produces is bit-equal to the default split's in the same matmul mode and sample order;
  backward  the gradients are held to the oracle by the parity tests' own assertion (split_checks.assert_gradients: strict 1e-4 against the
            fp32 oracle on the rays the fragility filter keeps, its all-rays rule against the fp64 oracle) -- a lost tile of 999 moves a
            gradient by ~3e-2, a lost decoder-gradient slab by far more;
  Adam      the colour decoder after nsk_adam_step against the oracle's Adam on the GPU's own gradient (test_gpu_configs.py's 2e-5), with the
            slabs summed by the fused kernel (nothing reads the gradient first) -- 6 slabs and one per 8-tile group;
  Tracker   loss and median threshold bit-equal to the default split's, ray gradients within the Tracker test's max(5e-4, 3 x fp32-vs-fp64);
  dead-tile skip, riders: see the tests.

Every skewed case must show a split that differs from the default's (a knob that no longer reaches the planner fails here); the conditions
are stated against the observed default, so they hold on any CU count."""
import numpy as np
import pytest
import torch

import split_checks as sk
import scenes
from gpu_util import cu, make_ctx
from scenes import rel_l2
from split_checks import TOL

pytestmark = pytest.mark.gpu
LR = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]

# forward knob settings: (name, keys, stages whose launch has the role the key weighs).  The fine stage has no colour role, and its merged
# form is a single role: a key that weighs a role the launch does not have cannot move its split, and must then leave it as it was.
FWD_BASE = {"roles": {"no_occ_role": 1}, "merged": {"no_occ_role": 2}}
FWD_KNOBS = [
    ("roles", "fine+color cost 1", {"no_occ_role": 1, "fwd_fine_cost": 1, "fwd_color_cost": 1}, ("fine", "color")),
    ("roles", "fine cost 100000", {"no_occ_role": 1, "fwd_fine_cost": 100000}, ("fine", "color")),
    ("roles", "color cost 100000", {"no_occ_role": 1, "fwd_color_cost": 100000}, ("color",)),
    ("merged", "occ cost 1", {"no_occ_role": 2, "fwd_occ_cost": 1}, ("color",)),
    ("merged", "occ cost 100000", {"no_occ_role": 2, "fwd_occ_cost": 100000}, ("color",)),
]


def _forward_run(ctx, stage, tiles, t, knobs):
    sk.tune(ctx, knobs)
    ro, rd, gd, gc = t
    rgb, depth, var, w = ctx.render_forward(stage, ro, rd, gd)
    split_render = ctx.debug_last_split()
    loss = torch.zeros(1, device="cuda")
    ctx.zero_grads()
    ctx.map_step(stage, ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss)
    ctx.sync()
    split = ctx.debug_last_split()
    M = ro.shape[0] * w.shape[1]
    got = dict(rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy(), var=var.cpu().numpy(), weights=w.cpu().numpy(), loss=np.float32(float(loss)),
               occ1=ctx.debug_fetch("occ1", M), occ2=ctx.debug_fetch("occ2", M), g_raw=ctx.debug_fetch("g_raw", M),
               bits_middle=ctx.debug_relu_bits("middle", M), bits_fine=ctx.debug_relu_bits("fine", M))
    if stage == "color":
        got.update(rgb4=ctx.debug_fetch("rgb4", M), bits_color=ctx.debug_relu_bits("color", M))
    return got, split_render, split


@pytest.mark.parametrize("tiles", [999, 14, 3])
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_forward_is_bit_equal_under_every_split(mode, tiles, oracle32):
    """render_forward, then map_step(flags=3) with a loss, under seven knob settings (the three-role and the merged default, three and two
    skews of them), stages fine and colour, both sample orders: bit-equal to the three-role default of the same mode and order (the merged
    form's equality to it is test_gpu_parity's).  The merged form exists only in mode 2."""
    r = sk.batch(tiles)
    t = [cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]
    cap = (tiles + 7) // 8
    seen = []
    for stage in ("fine", "color"):
        ref = sk.forward_reference(oracle32, stage, tiles) if tiles == 999 else None
        for sort_mode in (0, 1):
            ctx = make_ctx(sk.scene(), trainable=["color"] if stage == "color" else [], **sk.opts_of(tiles))
            ctx.set_matmul_mode(mode)
            ctx.set_sort_mode(sort_mode)
            base = {name: _forward_run(ctx, stage, tiles, t, knobs) for name, knobs in FWD_BASE.items()}
            for name, (got, s_render, s_step) in base.items():
                assert s_step["tiles"] == tiles and s_render["tiles"] == tiles
                want_form = "merged" if (name == "merged" and mode == 2) else ("multi" if mode == 0 else "multi_split")
                assert s_step["form"] == want_form and s_render["form"] == want_form, (name, s_step, s_render)
                assert s_step["which"] == ((1, 3) if stage == "color" else (1,)) if want_form == "merged" else s_step["which"] == ((1, 2, 3) if stage == "color" else (1, 2))
                assert s_step["grid"] == sum(s_step["wgs"]) and all(1 <= x <= cap for x in s_step["wgs"]), s_step
            for k, v in base["merged"][0].items():
                assert np.array_equal(v, base["roles"][0][k], equal_nan=True), (stage, sort_mode, "merged default", k)
            if ref is not None:
                for k in ("depth", "var", "weights") + (("rgb",) if stage == "color" else ()):
                    assert rel_l2(base["roles"][0][k], ref[k]) < TOL, (stage, k)
            for family, name, knobs, stages in FWD_KNOBS:
                got, s_render, s_step = _forward_run(ctx, stage, tiles, t, knobs)
                print("forward mode %d %s sort %d %4d tiles  %-18s %s %s (default %s %s)" % (mode, stage, sort_mode, tiles, name, s_step["form"], s_step["wgs"],
                                                                                           base[family][2]["form"], base[family][2]["wgs"]))
                if family == "merged" and mode != 2:
                    assert s_step["form"] != "merged" and s_render["form"] != "merged"          # the debug call says it did not run
                    applies = False                       # fwd_occ_cost weighs a role that exists in mode 2 only
                else:
                    assert s_step["form"] == base[family][2]["form"]
                    applies = stage in stages
                for s, b in ((s_render, base[family][1]), (s_step, base[family][2])):
                    if applies and tiles > 3:
                        assert sk.signature(s) != sk.signature(b), "%s did not move the split: %s" % (name, s)
                    elif not applies or tiles == 3:
                        assert sk.signature(s) == sk.signature(b), (name, s, b)      # no role to weigh / one tile per role: nothing to move
                    assert all(1 <= x <= cap for x in s["wgs"]) and s["grid"] == sum(s["wgs"]), s
                seen.extend(s_step["wgs"])
                for k, v in got.items():
                    assert np.array_equal(v, base["roles"][0][k], equal_nan=True), (stage, sort_mode, name, k, s_step)
                if ref is not None:
                    for k in ("depth", "var", "weights") + (("rgb",) if stage == "color" else ()):
                        assert rel_l2(got[k], ref[k]) < TOL, (stage, name, k)
            ctx.close()
    if tiles == 999:          # the sweep reached both ends: a role on one workgroup, a role at its cap
        assert 1 in seen and cap in seen, sorted(set(seen))


BWD_GROUPS = {
    # name: (stage, trainable, flags, backward mode, [knob settings; the first is the default split])
    "color": ("color", ["color"], 3, 2, [{}, {"frozen_cost": 100000}, {"frozen_mid_pct": 10}, {"frozen_mid_pct": 1000}]),
    "color-rays": ("color", ["color"], 7, 2, [{}, {"frozen_cost_rays": 100000}, {"frozen_mid_pct": 10}, {"frozen_mid_pct": 1000}]),
    "fine-frozen": ("fine", [], 1, 2, [{}, {"frozen_mid_pct": 10}, {"frozen_mid_pct": 1000}, {"no_frozen_kernel": 1}]),
    "color-full": ("color", ["color"], 3, 0, [{}, {"frozen_cost": 100000}]),
}
BWD_FORM = {"color": "multi", "color-rays": "multi", "fine-frozen": "frozen", "color-full": "multi_full"}


@pytest.mark.parametrize("group", list(BWD_GROUPS))
def test_backward_gradients_match_the_oracle_under_every_split(group, oracle32, oracle64, tiles=999):
    """the parity tests' gradient assertion, unchanged, for the default split and every skewed one: the grids of every level the stage touches,
    the trainable decoder, the rays where asked.  At 999 tiles only: the backward's roles are capped at ceil(tiles / 8) workgroups each and share
    every CU, so at 14 tiles (cap 2) or one ray (cap 1) all of them sit at the cap whatever the costs -- the planner has nothing to move, and the
    default split at those sizes is the existing tests'."""
    stage, trainable, flags, bmode, settings = BWD_GROUPS[group]
    splits = []
    for filtered in ((False, True) if tiles > 3 else (False,)):
        R = sk.backward_reference(oracle32, oracle64, stage, tiles, filtered)
        for i, knobs in enumerate(settings):
            out, split = sk.run_backward(R, stage, tiles, trainable, flags, knobs, bmode)
            print("backward %-11s %4d tiles %-9s %-28s %-10s which %s wgs %s  worst hip-vs-f32 %.2e" % (
                group, tiles, "filtered" if filtered else "all rays", knobs or "default", split["form"], split["which"], split["wgs"], sk.worst(out)))
            want_form = "multi" if knobs.get("no_frozen_kernel") else BWD_FORM[group]
            assert split["form"] == want_form and split["tiles"] == tiles and split["scan_wgs"] == 0 and split["loss_wg"] == 0, split
            assert split["which"] == ((3, 2, 1) if stage == "color" else (2, 1)) and split["train"] == ((1, 0, 0) if stage == "color" else (0, 0)), split
            assert split["grid"] == sum(split["wgs"]), split
            if i == 0:
                default = split
            elif tiles > 3:
                assert sk.signature(split) != sk.signature(default), "%s did not move the split: %s" % (knobs, split)
            splits.append(split)
            sk.assert_gradients(out, "filtered" if filtered else "all rays")
    if group == "color" and tiles == 999:
        t_wgs = [s["wgs"][0] for s in splits]
        # few slabs and several panel iterations per workgroup in one case, one workgroup per 8-tile group in another
        assert min(t_wgs) <= 8 and max(t_wgs) == (tiles + 7) // 8, t_wgs


@pytest.mark.parametrize("knobs", [{}, {"frozen_cost": 100000}], ids=["default", "frozen_cost"])
def test_adam_sums_the_slabs_the_split_wrote(knobs, oracle32):
    """map_step + adam_step with nothing reading the gradient in between: k_adam_multi sums the trainable role's per-workgroup slabs itself.
    The colour decoder after the step = the oracle's Adam on the gradient a second context (same knobs) downloads (flush_pending sums its slabs)."""
    sc, r = sk.scene(), sk.batch(999)
    t = [cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]
    res = []
    for step_adam in (False, True):
        ctx = make_ctx(sc, trainable=["color"])
        sk.tune(ctx, knobs)
        loss = torch.zeros(1, device="cuda")
        ctx.map_step("color", *t, -1.0, 0.5, True, flags=3, loss=loss)
        split = ctx.debug_last_split(backward=True)
        if step_adam:
            ctx.adam_step(LR)
            ctx.sync()
            res.append(ctx.decoder_download("color"))
        else:
            ctx.sync()
            res.append(ctx.decoder_download("color", grad=True))
        ctx.close()
    assert split["form"] == "multi" and split["train"] == (1, 0, 0) and split["loss_wg"] == 1 and split["grid"] == sum(split["wgs"]) + 1, split
    slabs = split["wgs"][0]
    assert (slabs <= 8) if knobs else (slabs == (999 + 7) // 8), split          # few slabs / one per 8-tile group
    g, after = res
    p0 = sc["decoders"]["color"]
    expect = p0.copy()
    oracle32.adam_step(expect, g, np.zeros_like(p0), np.zeros_like(p0), LR[0], 1)
    e = rel_l2(after - p0, expect - p0)
    print("adam %-22s trainable role on %3d workgroups: colour decoder update off by %.2e" % (knobs or "default", slabs, e))
    assert np.abs(after - p0).max() > 0 and e < 2e-5, (e, split)


def test_tracker_launch_under_skewed_splits(oracle32, oracle64):
    """nsk_track_step, default flags, 200 rays, deferred-median form (k_decode_bwd_track: three frozen roles + the median workgroup last)"""
    sc = scenes.make_scene(33, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    rays = scenes.make_rays(34, 200, sc["bound"], n_frames=1, zero_frac=0.1)
    refs = []
    for o in (oracle32, oracle64):
        op = o.opts(sc["bound"])
        fw = o.render_forward(op, sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"])
        l_ref, gD, gC, gV = o.loss_track(fw["depth"], fw["rgb"], fw["var"], rays["gt_depth"], rays["gt_color"], 0.5, True, True, True)
        bw = o.render_backward(op, sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"], -1.0, gC, gD, None,
                               want_grids=False, want_decoders=False)
        refs.append((l_ref, bw["g_rays_o"], bw["g_rays_d"]))
    ro, rd, gd, gc = [cu(rays[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]
    base = None
    for knobs in ({}, {"frozen_mid_pct": 10}, {"frozen_mid_pct": 1000}):
        ctx = make_ctx(sc)
        sk.tune(ctx, knobs)
        g_ro = torch.empty_like(ro); g_rd = torch.empty_like(rd); loss = torch.zeros(1, device="cuda")
        ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, True, True, True, loss=loss, g_rays=(g_ro, g_rd))
        ctx.sync()
        split = ctx.debug_last_split(backward=True)
        got = (np.float32(float(loss)), ctx.debug_fetch("median_thr", 200 * 48)[0], g_ro.cpu().numpy(), g_rd.cpu().numpy())
        ctx.close()
        assert split["form"] == "track" and split["which"] == (3, 2, 1) and split["train"] == (0, 0, 0) and split["median_wg"] == 1, split
        assert split["grid"] == sum(split["wgs"]) + 1 and split["loss_wg"] == 1 and split["tiles"] == 600, split
        errs = []
        for a, r32, r64 in ((got[2], refs[0][1], refs[1][1]), (got[3], refs[0][2], refs[1][2])):
            e64, eo = rel_l2(a, r64), rel_l2(r32, r64)
            errs.append((e64, eo))
            assert e64 < max(5 * TOL, 3 * eo), (knobs, e64, eo)
        print("tracker %-24s wgs %s  loss %.6f thr %.6f  rays_o / rays_d hip-vs-f64 %.2e / %.2e (f32-vs-f64 %.2e / %.2e)" % (
            knobs or "default", split["wgs"], got[0], got[1], errs[0][0], errs[1][0], errs[0][1], errs[1][1]))
        assert abs(got[0] - refs[0][0]) < 1e-3 * abs(refs[0][0]) and np.isfinite(got[1]) and got[1] > 0
        if base is None:
            base = (got, split)
        else:
            assert sk.signature(split) != sk.signature(base[1]), "%s did not move the split: %s" % (knobs, split)
            assert got[0] == base[0][0] and got[1] == base[0][1], (knobs, got[:2], base[0][:2])
            assert np.array_equal(np.all(got[3] == 0, axis=1), np.all(base[0][3] == 0, axis=1))


@pytest.mark.parametrize("sort_mode", [0, 1])
@pytest.mark.parametrize("stage", ["color", "fine"])
def test_dead_tile_counts_stay_exact_when_the_counting_roles_move(stage, sort_mode):
    """an optimiser mask on every level (test_gpu_dead_skip.py's scene, tests/live_tiles.py's CPU model), two steps of the same kind so the second
    is planned on the first one's counts: after each, the counts equal the model and the publishing ticket fired (counts[3] == 1: live_wgs
    matched the counting roles' workgroups); the gradients equal those of no_dead_skip=1 to the atomic-order bound of that file (1e-5)."""
    import test_gpu_dead_skip as ds
    masks, r = ds._masks("half"), ds._rays()
    full = ds._step(stage, masks, r, tune={"no_dead_skip": 1}, sort_mode=sort_mode)
    flags = 3 if stage == "color" else 1
    default = None
    for knobs in ({}, {"dead_tile_pct": 0, "frozen_mid_pct": 10}, {"dead_tile_pct": 0, "frozen_mid_pct": 1000},
                  {"dead_tile_pct": 100, "frozen_mid_pct": 10}, {"dead_tile_pct": 100, "frozen_mid_pct": 1000}):
        ctx = ds._new_ctx(stage, masks, knobs, sort_mode)
        ro, rd, gd, gc = ds._tensors(r)
        loss = torch.zeros(1, device="cuda")
        seen = []
        for step in range(2):
            ctx.zero_grads()
            ctx.map_step(stage, ro, rd, gd, gc, -1.0, 0.5, stage == "color", flags=flags, loss=loss)
            ctx.sync()
            counts = ds._check_counts(ctx, stage, masks, r, 48, ["middle", "fine"])
            assert counts[3] == 1 and (sort_mode == 0 or 0 < counts[1] < 960), counts          # (cell-sorted: the case does skip, as in test_gpu_dead_skip.py)
            split = ctx.debug_last_split(backward=True)
            assert split["form"] == ("multi" if stage == "color" else "frozen") and split["loss_wg"] == 1, split
            seen.append(split)
        print("dead skip %s sort %d %-48s step 1 %s step 2 %s counts %s" % (stage, sort_mode, knobs or "default", seen[0]["wgs"], seen[1]["wgs"], counts[:3]))
        if default is None:
            default = seen
        else:
            assert sk.signature(seen[0]) != sk.signature(default[0]), "%s did not move the split: %s" % (knobs, seen[0])
        got = dict(loss=float(loss), g={k: ctx.grid_download(k, grad=True) for k in full["g"]},
                   dec=ctx.decoder_download("color", grad=True) if stage == "color" else None)
        ctx.close()
        ds._same_step(got, full, exact=False)


@pytest.mark.parametrize("stage", ["fine", "color"])
def test_riders_sit_behind_a_skewed_split(stage):
    """nsk_map_prepare + frozen_mid_pct=1000 + a loss: the next batch's cell-sort scan rides behind the roles and the loss workgroup is the
    launch's last (fine stage: k_decode_bwd_frozen, colour stage: k_decode_bwd_multi); three steps give what the same sequence gives with
    no_piggyback=1, under test_gpu_dist.py::test_map_prepare_gives_the_unprepared_steps' comparison."""
    sc = sk.scene()
    batches = []
    for k in range(2):
        r = scenes.make_rays(50 + k, 333, sc["bound"], n_frames=3)
        batches.append([cu(r[x]) for x in ("rays_o", "rays_d", "gt_depth", "gt_color")] + [float(r["gt_depth"].max())])
    flags = 3 if stage == "color" else 1
    out = []
    for off in (1, 0):
        ctx = make_ctx(sc, trainable=["color"] if stage == "color" else [])
        ctx.set_sort_mode(1)
        sk.tune(ctx, {"frozen_mid_pct": 1000, "no_piggyback": off})
        loss = torch.zeros(1, device="cuda")
        losses, splits = [], []
        with torch.cuda.stream(ctx.tstream):
            for i in range(3):
                ro, rd, gd, gc, gm = batches[i % 2]
                n = batches[(i + 1) % 2]
                ctx.map_prepare(stage, n[0], n[1], n[2], n[4], flags=flags)
                ctx.map_step(stage, ro, rd, gd, gc, gm, 0.2, stage == "color", flags=flags, loss=loss)
                splits.append(ctx.debug_last_split(backward=True))
                ctx.adam_step(LR)
                losses.append(float(loss))
        out.append((losses, {k: ctx.grid_download(k) for k in ("middle", "fine", "color")}, ctx.decoder_download("color"), splits))
        ctx.close()
    (l0, g0, d0, s0), (l1, g1, d1, s1) = out
    ctx = make_ctx(sc, trainable=["color"] if stage == "color" else [])          # the default split of the same step, to see that the knob moved it
    ctx.set_sort_mode(1)
    ro, rd, gd, gc, gm = batches[0]
    ctx.map_step(stage, ro, rd, gd, gc, gm, 0.2, stage == "color", flags=flags, loss=torch.zeros(1, device="cuda"))
    assert sk.signature(ctx.debug_last_split(backward=True)) != sk.signature(s1[0]), s1[0]
    ctx.close()
    for a, b in zip(s0, s1):
        print("riders %s: %s wgs %s scan %d loss %d grid %d (no_piggyback: scan %d grid %d)" % (stage, b["form"], b["wgs"], b["scan_wgs"], b["loss_wg"], b["grid"], a["scan_wgs"], a["grid"]))
        assert b["form"] == ("multi" if stage == "color" else "frozen") and a["form"] == b["form"] and a["wgs"] == b["wgs"]
        assert a["scan_wgs"] == 0 and a["loss_wg"] == 1 and a["grid"] == sum(a["wgs"]) + 1, a
        assert b["scan_wgs"] > 0 and b["loss_wg"] == 1 and b["grid"] == sum(b["wgs"]) + b["scan_wgs"] + 1, b
    assert np.allclose(l0, l1, rtol=1e-5)
    for k in g0:
        assert rel_l2(g1[k] - sc["grids"][k], g0[k] - sc["grids"][k]) < 5e-3, k
    assert rel_l2(d1, d0) < 1e-4


def test_cost_keys_outside_their_range_are_refused():
    import nice_slam_cpp_amd as pkg
    ctx = make_ctx(sk.scene())
    for key in ("frozen_cost", "frozen_cost_rays", "fwd_fine_cost", "fwd_occ_cost", "fwd_color_cost"):
        for bad in (-1, 1000001):
            with pytest.raises(pkg.NskError, match="%s out of range" % key):
                ctx.set_tuning(key, bad)
        ctx.set_tuning(key, 1000000)
        ctx.set_tuning(key, 0)
    ctx.close()

"""GPU tests (-m gpu): one iteration of every optimiser of the reference -- Mapper, Tracker, Mapper with bundle adjustment -- on the HIP path
against the reference's op sequence on ATen-CPU with autograd and torch.optim.Adam (oracle/torch_ref.py, tests/aten_chains.py): no formula of
this repository on the reference side.  All rays, nothing filtered or handed over; the tolerance is north_star's 1e-4 relative L2.

Each test's docstring holds its measured worst figures, and each test prints what it measured.  A single step from a common pose agrees
within 1.5e-6 wherever HIP and ATen take the same ReLU branches; the two steps of the 10-iteration Tracker loop that do not are explained there."""
import numpy as np
import pytest
import torch

import aten_chains as A
import scenes
from gpu_util import cu, make_ctx, stage_levels
from oracle import torch_ref as T
from scenes import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4
GROUP = {"coarse": 1, "middle": 2, "fine": 3, "color": 4}
# config/nice_slam.yaml:72-95 (decoders, coarse, middle, fine, color, camera)
STAGE_LR = {"coarse": [0.0, 0.001, 0.0, 0.0, 0.0, 0.0], "middle": [0.0, 0.0, 0.1, 0.0, 0.0, 0.0], "fine": [0.0, 0.0, 0.005, 0.005, 0.0, 0.0],
            "color": [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]}
CAM_COFUSION = dict(H=480, W=640, fx=360.0, fy=360.0, cx=320.0, cy=240.0)           # config/cofusion.yaml:24-29


def _map_case(name):
    """scene, rays, stage, trainable decoders (reference order), group rates, gt_depth_max (None: the batch's own), render and operand options"""
    from test_gpu_configs import _strict_case
    c = dict(decs=(), gmax=None, ns=32, nsurf=16, matmul=None, backward=None, sort=None, masks=False)
    if name == "K1-coarse":                      # configs[0]: the reference's bound and grid shapes, the first stage of every mapping run
        sc = scenes.make_scene(11)
        rays = scenes.make_rays(12, 200, sc["bound"], n_frames=2, **CAM_COFUSION)
        c.update(stage="coarse", ns=16, nsurf=0)
    elif name == "K2-middle":
        sc, rays, _, _ = _strict_case("K2-color")
        c.update(stage="middle")
    elif name in ("K3-fine", "K4-shard"):
        sc, rays, stage, gmax = _strict_case(name)
        c.update(stage=stage, gmax=gmax)
    else:
        sc, rays, _, _ = _strict_case("K2-color")
        c.update(stage="color", decs=("color",))
        if name == "K2-color-fine-decoder":      # mapping.fix_fine: False
            c.update(decs=("fine", "color"))
        elif name == "K2-fine-fine-decoder":
            c.update(stage="fine", decs=("fine", "color"))
        elif name == "K2-color-matmul-1":
            c.update(matmul=1)
        elif name == "K2-color-matmul-0":
            c.update(matmul=0)
        elif name == "K2-color-backward-0":
            c.update(backward=0)
        elif name == "K2-color-ragged-sorted":
            rays = scenes.make_rays(53, 333, sc["bound"], n_frames=3)
            c.update(sort=1)
        elif name == "K2-color-frustum-masks":
            c.update(masks=True)
    lr = list(STAGE_LR[c["stage"]])
    if c["decs"]:
        lr[0] = 0.005                             # (the fine stage's decoders_lr is 0 in the config; a rate > 0 tests the decoder's update)
    c.update(sc=sc, rays=rays, lr=lr)
    return c


def _aten_map(c, masks):
    """src/Mapper.cpp:254-301,330,430-446: trained levels as leaves (grid[mask] with frustum masks), group 0 = the trainable decoders in the
    reference's order (fine, then colour), render_batch_ray, loss_map, backward, torch.optim.Adam"""
    sc, rays, stage = c["sc"], c["rays"], c["stage"]
    bound, grids, decs = A.torch_scene(sc)
    leaves, asm = {}, {}
    for k in stage_levels(stage):
        if masks is None:
            leaves[k] = grids[k].requires_grad_(True)
        else:
            leaves[k], asm[k] = T.masked_leaf(grids[k], torch.tensor(masks[k]))
    for d in c["decs"]:
        decs[d].requires_grad_(True)
    groups = ([{"params": [decs[d] for d in c["decs"]], "lr": c["lr"][0]}] if c["decs"] else []) + \
             [{"params": [leaves[k]], "lr": c["lr"][GROUP[k]]} for k in leaves]
    opt = torch.optim.Adam(groups)
    used = dict(grids)
    used.update({k: a() for k, a in asm.items()})
    t = {k: torch.tensor(rays[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")}
    rgb, depth, var, _ = T.render_batch_ray(used, decs, t["rays_d"], t["rays_o"], stage, t["gt_depth"], bound, n_samples=c["ns"],
                                            n_surface=c["nsurf"], gt_depth_max=c["gmax"])
    loss = T.loss_map(depth, rgb, t["gt_depth"], t["gt_color"], 0.5, stage == "color")
    opt.zero_grad()
    loss.backward()

    def full(k, v):
        if masks is None:
            return v[0].numpy().copy()
        out = torch.zeros_like(grids[k])
        return out.masked_scatter(torch.tensor(masks[k])[None, None].expand_as(out), v).detach()[0].numpy()
    out = dict(rgb=rgb.detach().numpy(), depth=depth.detach().numpy(), var=var.detach().numpy(), loss=float(loss.detach()),
               g={k: full(k, leaves[k].grad) for k in leaves}, g_dec={d: (decs[d].grad.numpy().copy() if decs[d].grad is not None else np.zeros_like(sc["decoders"][d])) for d in c["decs"]})
    opt.step()
    out["p"] = {k: (asm[k]().detach()[0].numpy() if masks is not None else grids[k].detach()[0].numpy().copy()) for k in leaves}
    out["p_dec"] = {d: decs[d].detach().numpy().copy() for d in c["decs"]}
    return out


MAP_CASES = ["K1-coarse", "K2-middle", "K3-fine", "K4-shard", "K2-color-fine-decoder", "K2-fine-fine-decoder", "K2-color-matmul-1",
             "K2-color-matmul-0", "K2-color-backward-0", "K2-color-ragged-sorted", "K2-color-frustum-masks"]


@pytest.mark.parametrize("case", MAP_CASES)
def test_mapping_iteration_against_aten_autograd(case):
    """One mapping iteration (src/Mapper.cpp:430-446) per case against ATen autograd + torch.optim.Adam, ALL rays:
      K1-coarse      configs[0]: reference bound and grid shapes (coarse [32,5,3,8]), cofusion camera, 200 rays x 16 samples, no surface
                     samples, coarse group at lr 0.001
      K2-middle      the middle stage at lr 0.1
      K3-fine        the fine stage at K3's size (5000 rays); K4-shard: the 1250-ray shard with the 10 000-ray batch's maximum passed to both sides
      *-fine-decoder mapping.fix_fine: False, fine and colour decoders in group 0 (the fine body on the fp32 MFMA, one backward launch per
                     decoder), in the colour and in the fine stage
      matmul-1 / matmul-0 / backward-0: the other operand forms; ragged-sorted: 333 rays cell-sorted; frustum-masks: the parameter is grid[mask]
    Checks: rendering, the loss, every read level's gradient and every trainable decoder's gradient (exactly zero where ATen's is, e.g. the
    colour decoder in the fine stage), the Adam update (elements off by more than 0.1 lr counted, < 0.1 %), frozen decoders and levels the
    stage does not read bit-unchanged.
    Measured worst relative L2 (rendering | loss | gradients), Adam far counts 0 except K4-shard grid_fine 1.5e-6:
      K1-coarse 4.0e-6 | 4.7e-7 | 5.0e-7;  K2-middle 5.1e-7 | 1.1e-7 | 3.9e-7;  K3-fine 2.5e-7 | 8.4e-8 | 7.1e-7;  K4-shard 2.5e-7 | 1.0e-7 | 1.1e-6;
      K2-color-fine-decoder 4.1e-7 | 0 | 6.6e-7;  K2-fine-fine-decoder 4.1e-7 | 0 | 7.0e-7;  K2-color-matmul-1 5.3e-7 | 7.8e-8 | 3.2e-7;
      K2-color-matmul-0 4.7e-7 | 7.8e-8 | 3.1e-7;  K2-color-backward-0 4.1e-7 | 7.8e-8 | 3.1e-7;  K2-color-ragged-sorted 4.8e-7 | 1.2e-7 | 4.2e-7;
      K2-color-frustum-masks 4.1e-7 | 7.8e-8 | 3.5e-7."""
    c = _map_case(case)
    sc, rays, stage = c["sc"], c["rays"], c["stage"]
    torch.set_num_threads(16)
    masks = None
    if c["masks"]:
        rng = np.random.default_rng(5)
        masks = {k: rng.random(sc["grids"][k].shape[1:]) < 0.8 for k in stage_levels(stage)}
    ref = _aten_map(c, masks)
    ctx = make_ctx(sc, n_samples=c["ns"], n_surface=c["nsurf"], trainable=c["decs"])
    if c["matmul"] is not None:
        ctx.set_matmul_mode(c["matmul"])
    if c["backward"] is not None:
        ctx.set_backward_mode(c["backward"])
    if c["sort"] is not None:
        ctx.set_sort_mode(c["sort"])
    for k, m in (masks or {}).items():
        ctx.set_mask(k, m)
    N = rays["rays_o"].shape[0]
    out = (torch.zeros(N, 3, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"))
    loss_t = torch.zeros(1, device="cuda")
    ctx.map_step(stage, cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"]), -1.0 if c["gmax"] is None else c["gmax"],
                 0.5, stage == "color", flags=1 | (2 if c["decs"] else 0), loss=loss_t, outputs=out)
    e_r = {"rgb": rel_l2(out[0].cpu().numpy(), ref["rgb"]), "depth": rel_l2(out[1].cpu().numpy(), ref["depth"]), "var": rel_l2(out[2].cpu().numpy(), ref["var"])}
    if stage != "color":
        e_r.pop("rgb")                           # (zero on both sides)
        assert not out[0].any()
    e_l = abs(float(loss_t) - ref["loss"]) / ref["loss"]
    g = {k: ctx.grid_download(k, grad=True) for k in ref["g"]}
    e_g = {"grid_" + k: rel_l2(g[k], ref["g"][k]) for k in ref["g"]}
    for d in c["decs"]:
        gd_hip = ctx.decoder_download(d, grad=True)
        if ref["g_dec"][d].any():
            e_g[d + " decoder"] = rel_l2(gd_hip, ref["g_dec"][d])
        else:                                    # (a trainable decoder the stage does not evaluate: the colour decoder in the fine stage)
            assert not gd_hip.any(), (case, d)
    if masks is not None:
        for k in masks:
            assert not g[k][:, ~masks[k]].any(), k
    ctx.adam_step(c["lr"])
    far = {}
    for k in ref["p"]:
        got = ctx.grid_download(k)
        far["grid_" + k] = float((np.abs(got - ref["p"][k]) > 0.1 * c["lr"][GROUP[k]]).mean()) if c["lr"][GROUP[k]] > 0 else float((got != ref["p"][k]).mean())
        if masks is not None:
            assert np.array_equal(got[:, ~masks[k]], sc["grids"][k][:, ~masks[k]]), k
    for d in c["decs"]:
        far[d + " decoder"] = float((np.abs(ctx.decoder_download(d) - ref["p_dec"][d]) > 0.1 * c["lr"][0]).mean())
    print("%s against ATen autograd, all %d rays: rendering %s | loss %.1e | gradients %s | Adam far %s" % (
        case, N, {k: "%.1e" % v for k, v in e_r.items()}, e_l, {k: "%.1e" % v for k, v in e_g.items()}, far))
    for k in scenes.LEVELS:
        if k not in ref["p"]:
            assert np.array_equal(ctx.grid_download(k), sc["grids"][k]), k
        if k not in c["decs"]:
            assert np.array_equal(ctx.decoder_download(k), sc["decoders"][k]), k
    ctx.close()
    assert max(e_r.values()) < TOL, e_r
    assert e_l < 2e-5, e_l
    for k, e in e_g.items():
        assert e < TOL, (case, k, e)
    for k, f in far.items():
        assert f < 1e-3, (case, k, f)


_CACHE = {}


def _k5():
    if "sc" not in _CACHE:
        _CACHE["sc"] = A.k5_scene()
    return _CACHE["sc"]


def _frame(n):
    base = 1500 if n > 200 else 200
    if base not in _CACHE:
        _CACHE[base] = A.tracking_frame(_k5(), base)
    return A.first_rays(_CACHE[base], n)


def _gpu_track(ctx, fr, flags, iters=1, lr=A.TRACK_LR, poses=None):
    """the product form of Tracker::optimize_cam_in_batch (host/src/nsk_host.cpp): rays_from_camera -> inside_filter -> set_ray_mask(keep) ->
    track_step(NSK_GRAD_RAYS) -> pose_step (rays_backward + camera_backward + Adam, d loss / d pose out).  poses: the pose each iteration
    starts from (the Adam moments stay the HIP path's own)"""
    hd, dv, uc = flags
    pi, pj = cu(fr["pix_i"], torch.int32), cu(fr["pix_j"], torch.int32)
    gd, gc = cu(fr["gt_depth"]), cu(fr["gt_color"])
    cam, m, v = cu(fr["cam0"]), torch.zeros(7, device="cuda"), torch.zeros(7, device="cuda")
    loss, g_cam = torch.zeros(1, device="cuda"), torch.zeros(7, device="cuda")
    out = dict(hist=[])
    for it in range(iters):
        if poses is not None:
            cam.copy_(cu(poses[it]))
        ro, rd = ctx.rays_from_camera(pi, pj, fr["intr"], cam)
        keep = ctx._inside_filter_u8(ro, rd, gd)
        g_ro, g_rd = torch.empty_like(ro), torch.empty_like(rd)
        ctx.set_ray_mask(keep)
        ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, bool(uc), bool(hd), bool(dv), flags=4, loss=loss, g_rays=(g_ro, g_rd))
        ctx.set_ray_mask(None)
        ctx.pose_step(pi, pj, fr["intr"], g_ro, g_rd, cam, m, v, lr, it + 1, g_cam_out=g_cam)
        ctx.sync()
        out["hist"].append((float(loss), g_cam.cpu().numpy(), cam.cpu().numpy(), int(keep.sum())))
        if it == 0:
            out.update(keep=keep.cpu().numpy().astype(bool), loss=float(loss), grad=g_cam.cpu().numpy(), cam1=cam.cpu().numpy())
    ctx.sync()
    out["cam"] = cam.cpu().numpy()
    return out


@pytest.mark.parametrize("n", [200, 199, 1500])
@pytest.mark.parametrize("flags", [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)], ids=lambda f: "dyn%d-detach%d-color%d" % f)
def test_tracker_iteration_against_aten_autograd(flags, n):
    """Tracker::optimize_cam_in_batch (src/Tracker.cpp:41-89) on the constructed K5 frame (tests/aten_chains.py tracking_frame: the inside
    filter drops the ~5 % of rays beyond the box exit, the 10 x median mask drops the dynamic outliers) from a perturbed pose, flags
    (handle_dynamic, detach_var, use_color); N = 199 (odd: torch.median's lower middle), 1500 (the k_median_thr path); the default median
    form and the three-launch form ("no_fused_median").  ATen compacts the rays, the HIP path masks them: the keep masks, the loss, the 7 pose
    gradients (1e-4) and the pose after the Adam step must agree.
    Measured over all 24 runs: loss <= 2.6e-7, pose gradient <= 4.1e-7, pose update <= 1.4e-7; 10 / 10 / 75 rays dropped by the inside filter
    and 9 / 8 / 122 by the dynamic mask at N = 200 / 199 / 1500."""
    sc, fr = _k5(), _frame(n)
    torch.set_num_threads(16)
    ref = A.aten_track(sc, fr, *flags)
    assert (~ref["keep"]).sum() >= fr["n_beyond"] * n // len(fr["gt_depth"]) // 2 and (~ref["keep"]).any()
    if flags[0]:
        assert ref["dyn_dropped"] >= 5, ref["dyn_dropped"]
    for form in ("default", "no_fused_median"):
        ctx = make_ctx(sc)
        if form != "default":
            ctx.set_tuning("no_fused_median", 1)
        got = _gpu_track(ctx, fr, flags)
        ctx.close()
        e_l = abs(got["loss"] - ref["loss"]) / ref["loss"]
        e_g = rel_l2(got["grad"], ref["grad"])
        e_p = rel_l2(got["cam1"] - fr["cam0"], ref["cam1"] - fr["cam0"])
        print("tracker N=%d flags %s %s: %d of %d rays kept, %d dynamic dropped | loss %.1e | pose gradient %.1e | pose update %.1e" % (
            n, flags, form, ref["keep"].sum(), n, ref["dyn_dropped"], e_l, e_g, e_p))
        assert np.array_equal(got["keep"], ref["keep"])
        assert e_l < 2e-5, (form, e_l)
        assert e_g < TOL, (form, e_g)
        assert e_p < TOL, (form, e_p)


def test_tracker_ten_iterations_against_aten_autograd():
    """Tracker::run's 10 iterations (src/Tracker.cpp:92-113) at N = 200, default flags, Adam's moments carried across the steps on both sides.
    Every iteration starts the HIP path from ATen's pose of that iteration, and the pose gradient and the pose after the step must agree
    within 1e-4.  The two trajectories are not compared free-running: on this frame the reference chain itself is chaotic -- ATen started
    from a pose 1e-7 away ends 1.8e-2 (relative L2) away after 10 iterations -- so any rounding difference grows to the same size.
    Measured: pose gradient 2e-7 .. 9e-7 in eight of the ten steps; 1.2e-5 at iteration 1 and 3.3e-5 at iteration 2, each from ONE
    rounding-level ReLU flip of the fine decoder (found with nsk_debug_preact against the fp32 oracle's inputs; rss from nso_preact_bounds):
    iteration 1, kept ray 189, sample 0, layer 1, unit 27, HIP -3.18e-7 against +2.98e-7, rss 2.0e-4 (0.002 rss from zero); iteration 2,
    kept ray 100, sample 16, layer 4, unit 18, HIP +6.2e-9 against -4.77e-7, rss 2.5e-4 (0.002 rss).  Pose updates <= 4e-5."""
    sc, fr = _k5(), _frame(200)
    torch.set_num_threads(16)
    ref = A.aten_track(sc, fr, iters=10)
    starts = [fr["cam0"]] + [h[2] for h in ref["hist"][:-1]]
    ctx = make_ctx(sc)
    got = _gpu_track(ctx, fr, (1, 1, 1), iters=10, poses=starts)
    ctx.close()
    e_g = [rel_l2(b[1], a[1]) for a, b in zip(ref["hist"], got["hist"])]
    e_p = [rel_l2(b[2] - s0, a[2] - s0) for a, b, s0 in zip(ref["hist"], got["hist"], starts)]
    print("tracker, 10 iterations from ATen's poses: pose moved %.1e; pose gradients %s; updates %s" % (
        np.abs(ref["cam"] - fr["cam0"]).max(), ["%.0e" % e for e in e_g], ["%.0e" % e for e in e_p]))
    assert np.abs(ref["cam"] - fr["cam0"]).max() > 1e-2
    assert [a[3] for a in ref["hist"]] == [b[3] for b in got["hist"]]
    assert max(e_g) < TOL and max(e_p) < TOL, (e_g, e_p)


def test_bundle_adjustment_iteration_against_aten_autograd():
    """One colour-stage Mapper iteration with BA (src/Mapper.cpp:305-329,430-446) on a K5 window of three frames (300 / 450 / 250 rays, the
    oldest frame fixed, ~5 % of every frame's rays beyond the box exit), in the product's form (host/src/nsk_host.cpp, Mapper::optimize_map):
    set_ray_mask -> map_step(GRIDS | DECODERS | RAYS) -> pose_step_multi(step 0: per-frame gradients and the kept-ray count) -> adam_step and
    adam_vector on the poses.  ATen: a leaf per active pose, rays concatenated and compacted, loss_map, backward, Adam over decoders, middle,
    fine, colour and camera.  Measured: 951 of 1000 rays kept (count exact), loss 0, gradients <= 1.5e-6 (grid_color), pose gradients 5.3e-7 /
    2.7e-7, pose updates exact, Adam far counts 0."""
    sc = _k5()
    win = A.ba_window(sc)
    torch.set_num_threads(16)
    lr = STAGE_LR["color"]
    ref = A.aten_ba(sc, win, lr)
    fr = win["frames"]
    nf = len(fr)
    ctx = make_ctx(sc, trainable=["color"])
    cams = cu(np.stack([np.concatenate([f["cam0"], [0.0]]) for f in fr]))
    ro, rd = zip(*[ctx.rays_from_camera(cu(f["pix_i"], torch.int32), cu(f["pix_j"], torch.int32), win["intr"], cams[i, :7].contiguous())
                   for i, f in enumerate(fr)])
    ro, rd = torch.cat(ro).contiguous(), torch.cat(rd).contiguous()
    pi, pj = cu(np.concatenate([f["pix_i"] for f in fr]), torch.int32), cu(np.concatenate([f["pix_j"] for f in fr]), torch.int32)
    gd, gc = cu(np.concatenate([f["gt_depth"] for f in fr])), cu(np.concatenate([f["gt_color"] for f in fr]))
    keep = ctx._inside_filter_u8(ro, rd, gd)
    N = ro.shape[0]
    g_ro, g_rd = torch.empty_like(ro), torch.empty_like(rd)
    loss = torch.zeros(1, device="cuda")
    ctx.set_ray_mask(keep)
    ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=7, loss=loss, g_rays=(g_ro, g_rd))
    ctx.set_ray_mask(None)
    first = list(np.cumsum([0] + win["counts"][:-1]))
    g_cams = torch.zeros(8 * nf + 8, device="cuda")
    ctx.pose_step_multi(first, win["counts"], [int(f["active"]) for f in fr], pi, pj, win["intr"], g_ro, g_rd, cams, step=0, g_cams=g_cams, keep=keep)
    ctx.sync()
    gcam = g_cams.cpu().numpy()
    k_got = keep.cpu().numpy().astype(bool)
    e_g = {"grid_" + k: rel_l2(ctx.grid_download(k, grad=True), ref["g_grids"][k]) for k in ref["g_grids"]}
    e_g["colour decoder"] = rel_l2(ctx.decoder_download("color", grad=True), ref["g_dec"])
    e_c = [rel_l2(gcam[8 * i:8 * i + 7], ref["g_cams"][i]) for i in range(nf) if fr[i]["active"]]
    ctx.adam_step(lr)
    m, v = torch.zeros(8 * nf, device="cuda"), torch.zeros(8 * nf, device="cuda")
    ctx.adam_vector(cams.view(-1), g_cams[:8 * nf].contiguous(), m, v, A.BA_CAM_LR, 1)
    ctx.sync()
    cams_after = cams.cpu().numpy()
    far = {k: float((np.abs(ctx.grid_download(k) - ref["grids"][k]) > 0.1 * lr[GROUP[k]]).mean()) for k in ref["grids"]}
    far["colour decoder"] = float((np.abs(ctx.decoder_download("color") - ref["dec"]) > 0.1 * lr[0]).mean())
    e_p = [rel_l2(cams_after[i, :7] - fr[i]["cam0"], ref["cams"][i] - fr[i]["cam0"]) for i in range(nf) if fr[i]["active"]]
    print("BA against ATen autograd: %d of %d rays kept | loss %.1e | gradients %s | pose gradients %s | pose updates %s | Adam far %s" % (
        k_got.sum(), N, abs(float(loss) - ref["loss"]) / ref["loss"], {k: "%.1e" % e for k, e in e_g.items()}, ["%.1e" % e for e in e_c],
        ["%.1e" % e for e in e_p], far))
    ctx.close()
    assert np.array_equal(k_got, ref["keep"]) and 0 < (~k_got).sum()
    assert int(gcam[8 * nf + 1]) == k_got.sum()
    assert abs(float(loss) - ref["loss"]) < 2e-5 * ref["loss"]
    for k, e in e_g.items():
        assert e < TOL, (k, e)
    for e in e_c + e_p:
        assert e < TOL, (e_c, e_p)
    assert not gcam[:7].any() and np.array_equal(cams_after[0, :7], fr[0]["cam0"])      # the oldest frame: no gradient, no move
    for k, f in far.items():
        assert f < 1e-3, (k, f)

"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against the CPU oracle and the committed
golden vectors.  Tolerance: north_star's 1e-4 relative L2 on rendered depth / colour and on optimised grids /
poses; raw gradients are compared on rays whose ReLU inputs are not within rounding of a kink (see
oracle/nso.c nso_ray_fragility) because d ReLU jumps there and two fp32 evaluations may legitimately differ."""
import glob
import os

import numpy as np
import pytest
import torch

import local_parity as LP
import scenes
from gpu_util import cu, make_ctx, stage_levels
from scenes import rel_l2
from split_checks import assert_gradients as _assert_gradients      # (shared with tests/test_gpu_split.py)

pytestmark = pytest.mark.gpu
TOL = 1e-4
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "render_*.npz")))


def _scene(seed=3, shapes=None, grid_std=0.3, bias_std=0.1):
    return scenes.make_scene(seed, shapes or scenes.SMALL_GRID_SHAPES, grid_std=grid_std, bias_std=bias_std)


@pytest.mark.parametrize("stage", ["coarse", "middle", "fine", "color"])
@pytest.mark.parametrize("with_gt", [True, False])
def test_forward_matches_oracle(stage, with_gt, oracle32):
    sc = _scene()
    rays = scenes.make_rays(4, 100, sc["bound"], n_frames=2, zero_frac=0.1)
    gd = rays["gt_depth"] if with_gt else None
    ref = oracle32.render_forward(oracle32.opts(sc["bound"]), sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], gd)
    ctx = make_ctx(sc)
    rgb, depth, var, w = ctx.render_forward(stage, cu(rays["rays_o"]), cu(rays["rays_d"]), None if gd is None else cu(gd))
    ctx.sync()
    assert rel_l2(depth.cpu().numpy(), ref["depth"]) < TOL
    assert rel_l2(var.cpu().numpy(), ref["var"]) < TOL
    assert rel_l2(w.cpu().numpy(), ref["weights"]) < TOL
    if stage == "color":
        assert rel_l2(rgb.cpu().numpy(), ref["rgb"]) < TOL
    else:
        assert float(rgb.abs().max()) == 0.0


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[7:-4] for p in GOLDEN])
def test_forward_matches_golden(path):
    z = np.load(path, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    sc = dict(bound=g["bound"], grids={k: g["grid_" + k] for k in scenes.LEVELS}, decoders={k: g["dec_" + k] for k in scenes.LEVELS})
    ctx = make_ctx(sc, occupancy=bool(g["occupancy"]))
    gd = cu(g["gt_depth"]) if bool(g["with_gt"]) else None
    rgb, depth, var, w = ctx.render_forward(str(g["stage"]), cu(g["rays_o"]), cu(g["rays_d"]), gd)
    assert rel_l2(depth.cpu().numpy(), g["depth"]) < TOL
    assert rel_l2(w.cpu().numpy(), g["weights"]) < TOL
    assert rel_l2(var.cpu().numpy(), g["var"]) < TOL
    if str(g["stage"]) == "color":
        assert rel_l2(rgb.cpu().numpy(), g["rgb"]) < TOL


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[7:-4] for p in GOLDEN])
def test_backward_matches_golden(path):
    """the backward fields of the committed golden vectors (fp64 autograd over the reference's ATen op sequence, tests/golden/
    make_golden.py): d L / d grids, d L / d every decoder of the stage (all trainable at once: the fine decoder's trainable body and
    the one-launch-per-decoder path run here), d L / d rays -- all 24 rays, no filtering, 1e-4 relative L2"""
    z = np.load(path, allow_pickle=False)
    g = {k: z[k] for k in z.files}
    stage = str(g["stage"])
    sc = dict(bound=g["bound"], grids={k: g["grid_" + k] for k in scenes.LEVELS}, decoders={k: g["dec_" + k] for k in scenes.LEVELS})
    levels = stage_levels(stage)
    ctx = make_ctx(sc, occupancy=bool(g["occupancy"]), trainable=levels)
    gd = cu(g["gt_depth"]) if bool(g["with_gt"]) else None
    g_ro, g_rd = ctx.render_backward(stage, cu(g["rays_o"]), cu(g["rays_d"]), gd, -1.0, cu(g["g_rgb"]), cu(g["g_depth"]), cu(g["g_var"]), flags=7)
    ctx.sync()
    errs = {"rays_o": rel_l2(g_ro.cpu().numpy(), g["g_rays_o"]), "rays_d": rel_l2(g_rd.cpu().numpy(), g["g_rays_d"])}
    for k in levels:
        if "g_grid_" + k in g:
            errs["grid_" + k] = rel_l2(ctx.grid_download(k, grad=True), g["g_grid_" + k])
        if "g_dec_" + k in g:
            errs["dec_" + k] = rel_l2(ctx.decoder_download(k, grad=True), g["g_dec_" + k])
    assert len(errs) >= 4, errs
    for k, e in errs.items():
        assert e < TOL, (k, e, errs)


@pytest.mark.parametrize("stage,trainable", [("fine", []), ("color", ["color"])])
def test_backward_chains_keep_relative_accuracy_across_decades(stage, trainable):
    """The backward chains run on fp16 pieces of a per-sample power-of-two multiple of the upstream gradient (chain_scale).  Upstream
    gradients that differ by sixty decades between rays -- 2^-100 ... 2^100, far outside fp16 in both directions -- must come out with
    the accuracy of the unscaled run, ray group by ray group (the gradient is linear in the upstream gradient and the factors are powers
    of two: apart from the order of the atomic sums the results are the unscaled ones times the factor), and a batch that mixes all the
    scales must give the sum of the single-scale runs."""
    sc = _scene(51, grid_std=0.3)
    rays = scenes.make_rays(52, 48, sc["bound"], n_frames=2)
    ro, rd, gd = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"])
    N = rays["rays_o"].shape[0]
    rng = np.random.default_rng(9)
    g_rgb = rng.standard_normal((N, 3)).astype(np.float32)
    g_d = rng.standard_normal(N).astype(np.float32)
    levels = stage_levels(stage)
    groups = np.arange(N) % 4
    expo = np.array([-100, -40, 0, 100])
    flags = 3 if trainable else 1

    def run(mult):
        ctx = make_ctx(sc, trainable=trainable)
        ctx.render_backward(stage, ro, rd, gd, -1.0, cu(g_rgb * mult[:, None]), cu(g_d * mult), None, flags=flags)
        ctx.sync()
        out = {k: ctx.grid_download(k, grad=True).astype(np.float64) for k in levels}
        if trainable:
            out["decoder"] = ctx.decoder_download("color", grad=True).astype(np.float64)
        return out

    total = None
    for gi in range(4):
        sel = (groups == gi).astype(np.float32)
        base = run(sel)                                              # this group's rays alone, unscaled
        assert all(np.abs(v).max() > 0 for v in base.values())
        f = np.ldexp(np.float32(1), int(expo[gi]))
        got = run(sel * f)
        for k, v in got.items():
            assert np.isfinite(v).all(), (k, expo[gi])
            e = rel_l2(v / float(f), base[k])
            assert e < 1e-5, "upstream gradient x 2^%d: %s differs from the unscaled run by %.2e" % (expo[gi], k, e)
        total = {k: v.copy() for k, v in got.items()} if total is None else {k: total[k] + got[k] for k in got}
    mixed = run(np.ldexp(np.float32(1), expo[groups]).astype(np.float32))
    for k, v in mixed.items():
        assert np.isfinite(v).all()
        assert rel_l2(v, total[k]) < 1e-5, (k, rel_l2(v, total[k]))


def test_eval_points_matches_oracle(oracle32):
    """Renderer::eval_points: raw = (rgb, occ), occ = 100 outside the bound"""
    sc = _scene(5)
    rng = np.random.default_rng(0)
    b = sc["bound"]
    pts = (b[:, 0] + (b[:, 1] - b[:, 0]) * rng.uniform(-0.1, 1.1, (500, 3))).astype(np.float32)
    ctx = make_ctx(sc)
    # oracle: a ray with origin = point, direction unit z, n_samples=1 would change z; use the aux raw of 1-sample rays
    op = oracle32.opts(b, n_samples=1, n_surface=0)
    ro = pts - np.array([0, 0, 0.01], np.float32) * 0  # placeholder: compare through render of degenerate rays below
    for stage in ("coarse", "middle", "fine", "color"):
        raw = ctx.eval_points(stage, cu(pts)).cpu().numpy()
        inb = np.all((pts < b[:, 1]) & (pts > b[:, 0]), axis=1)
        assert (raw[~inb, 3] == 100).all() and (raw[inb, 3] != 100).all()
        if stage != "color":
            assert np.abs(raw[:, :3]).max() == 0
    # value check against the oracle: samples of real rays are points too
    rays = scenes.make_rays(8, 20, b)
    fw = oracle32.render_forward(oracle32.opts(b), sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"], want_aux=True)
    p = (rays["rays_o"][:, None, :] + rays["rays_d"][:, None, :] * fw["z"][:, :, None]).reshape(-1, 3).astype(np.float32)
    raw = ctx.eval_points("color", cu(p)).cpu().numpy()
    assert rel_l2(raw, fw["raw"].reshape(-1, 4)) < TOL


def _backward_case(stage, with_gt, occupancy, oracle32, oracle64, trainable, n_rays=96, seed=3, tau=2e-5, filtered=True):
    sc = _scene(seed)
    rays = scenes.make_rays(seed + 1, n_rays, sc["bound"], n_frames=2, zero_frac=0.1)
    gd = rays["gt_depth"] if with_gt else None
    rng = np.random.default_rng(seed + 2)
    N = rays["rays_o"].shape[0]
    g_rgb, g_d, g_v = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    # drop rays that sit on a ReLU kink (their gradient is not a function of the inputs to within rounding)
    frag = oracle64.ray_fragility(oracle64.opts(sc["bound"], occupancy=occupancy), sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], gd)
    keep = frag > tau if filtered else np.ones(N, bool)
    assert keep.mean() > 0.5
    g_rgb[~keep] = 0; g_d[~keep] = 0; g_v[~keep] = 0
    op = oracle32.opts(sc["bound"], occupancy=occupancy)
    ref = oracle32.render_backward(op, sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], gd, -1.0, g_rgb, g_d, g_v)
    ref64 = oracle64.render_backward(oracle64.opts(sc["bound"], occupancy=occupancy), sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], gd, -1.0, g_rgb, g_d, g_v)
    ctx = make_ctx(sc, occupancy=occupancy, trainable=trainable)
    g_ro, g_rd = ctx.render_backward(stage, cu(rays["rays_o"]), cu(rays["rays_d"]), None if gd is None else cu(gd), -1.0,
                                     cu(g_rgb), cu(g_d), cu(g_v), flags=7)
    ctx.sync()
    out = {}
    for k in stage_levels(stage):
        out["grid_" + k] = (ctx.grid_download(k, grad=True), ref["g_grids"][k], ref64["g_grids"][k])
        if k in trainable:
            out["dec_" + k] = (ctx.decoder_download(k, grad=True), ref["g_decoders"][k], ref64["g_decoders"][k])
    out["rays_o"] = (g_ro.cpu().numpy(), ref["g_rays_o"], ref64["g_rays_o"])
    out["rays_d"] = (g_rd.cpu().numpy(), ref["g_rays_d"], ref64["g_rays_d"])
    out["_kept"] = float(keep.mean())
    return out, ctx, sc


@pytest.mark.parametrize("stage", ["coarse", "middle", "fine", "color"])
@pytest.mark.parametrize("with_gt,occupancy", [(True, False), (False, True)])
def test_backward_matches_oracle(stage, with_gt, occupancy, oracle32, oracle64):
    trainable = stage_levels(stage)
    out_all, _, _ = _backward_case(stage, with_gt, occupancy, oracle32, oracle64, trainable, filtered=False)
    _assert_gradients(out_all, "all rays")
    out, ctx, sc = _backward_case(stage, with_gt, occupancy, oracle32, oracle64, trainable)
    _assert_gradients(out, "filtered")
    # untouched levels / frozen decoders keep zero gradient
    for k in scenes.LEVELS:
        if k not in stage_levels(stage):
            assert np.abs(ctx.grid_download(k, grad=True)).max() == 0
            assert np.abs(ctx.decoder_download(k, grad=True)).max() == 0


def test_frozen_decoders_get_no_gradient_and_grads_accumulate(oracle32, oracle64):
    out, ctx, sc = _backward_case("color", True, False, oracle32, oracle64, trainable=["color"])
    out.pop("_kept")
    assert np.abs(ctx.decoder_download("middle", grad=True)).max() == 0
    assert np.abs(ctx.decoder_download("fine", grad=True)).max() == 0
    g1 = ctx.grid_download("fine", grad=True)
    ctx.zero_grads()
    assert np.abs(ctx.grid_download("fine", grad=True)).max() == 0
    assert np.abs(g1).max() > 0


def test_losses_and_pose_kernels(oracle32):
    rng = np.random.default_rng(0)
    N = 203
    depth, var = rng.uniform(0.5, 4, N).astype(np.float32), rng.uniform(1e-3, 0.5, N).astype(np.float32)
    rgb, gt_c = rng.uniform(0, 1, (N, 3)).astype(np.float32), rng.uniform(0, 1, (N, 3)).astype(np.float32)
    gt_d = (depth + rng.standard_normal(N) * 0.2).astype(np.float32)
    gt_d[::7] = 0.0
    gt_d[3] = depth[3] + 50.0
    sc = _scene()
    ctx = make_ctx(sc)
    for use_color in (True, False):
        loss, g_d, g_c = ctx.loss_map(cu(depth), cu(rgb), cu(gt_d), cu(gt_c), 0.5, use_color)
        l_ref, gd_ref, gc_ref = oracle32.loss_map(depth, rgb, gt_d, gt_c, 0.5, use_color)
        assert abs(float(loss) - l_ref) < 1e-4 * abs(l_ref)
        assert np.array_equal(g_d.cpu().numpy(), gd_ref) and np.array_equal(g_c.cpu().numpy(), gc_ref)
    for hd in (True, False):
        for detach in (True, False):
            loss, g_d, g_c, g_v = ctx.loss_track(cu(depth), cu(rgb), cu(var), cu(gt_d), cu(gt_c), 0.5, True, hd, detach)
            l_ref, gd_ref, gc_ref, gv_ref = oracle32.loss_track(depth, rgb, var, gt_d, gt_c, 0.5, True, hd, detach)
            assert abs(float(loss) - l_ref) < 1e-4 * abs(l_ref)
            assert rel_l2(g_d.cpu().numpy(), gd_ref) < 1e-6 and np.array_equal(g_c.cpu().numpy(), gc_ref)
            assert rel_l2(g_v.cpu().numpy(), gv_ref) < 1e-5
    # pose chain
    cam = np.concatenate([rng.standard_normal(4), rng.standard_normal(3)]).astype(np.float32)
    pi, pj = rng.integers(0, 640, 77).astype(np.int32), rng.integers(0, 480, 77).astype(np.int32)
    intr = (360.0, 360.0, 320.0, 240.0)
    c2w = ctx.camera_from_tensor(cu(cam))
    assert rel_l2(c2w.cpu().numpy(), oracle32.camera_from_tensor(cam)) < 1e-6
    for mode in (0, 1, 2, 3):
        ro, rd = ctx.rays_from_pixels(cu(pi, torch.int32), cu(pj, torch.int32), intr, c2w, mode)
        ro_ref, rd_ref = oracle32.rays_from_pixels(pi, pj, *intr, c2w.cpu().numpy(), mode)
        assert np.array_equal(ro.cpu().numpy(), ro_ref) and rel_l2(rd.cpu().numpy(), rd_ref) < 1e-6
        g_o, g_d = rng.standard_normal((77, 3)).astype(np.float32), rng.standard_normal((77, 3)).astype(np.float32)
        g_c2w = ctx.rays_backward(cu(pi, torch.int32), cu(pj, torch.int32), intr, cu(g_o), cu(g_d), mode)
        g_c2w_ref = oracle32.rays_backward(pi, pj, *intr, g_o, g_d, mode)
        assert rel_l2(g_c2w.cpu().numpy(), g_c2w_ref) < 1e-5
        g_cam = ctx.camera_backward(cu(cam), g_c2w)
        assert rel_l2(g_cam.cpu().numpy(), oracle32.camera_backward(cam, g_c2w_ref)) < 1e-4
    rays = scenes.make_rays(9, 300, sc["bound"], n_frames=2, shrink=-0.5)
    keep = ctx.inside_filter(cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]))
    assert np.array_equal(keep.cpu().numpy(), oracle32.inside_filter(sc["bound"], rays["rays_o"], rays["rays_d"], rays["gt_depth"]))


def test_edge_cases(oracle32, oracle64):
    """single ray; 16-sample coarse-only (K1 shape); ray leaving the bound; all-zero depth; N not a multiple of 4"""
    sc = _scene(7)
    b = sc["bound"]
    ctx = make_ctx(sc)
    ro = np.array([[b[0, 1] - 0.05, 0.0, 0.0]], np.float32)
    rd = np.array([[-0.3, 0.2, -1.0]], np.float32)
    for gtv in (9.0, 0.0):
        gt = np.array([gtv], np.float32)
        ref = oracle32.render_forward(oracle32.opts(b), sc["grids"], sc["decoders"], "color", ro, rd, gt)
        rgb, depth, var, w = ctx.render_forward("color", cu(ro), cu(rd), cu(gt))
        assert rel_l2(depth.cpu().numpy(), ref["depth"]) < TOL and rel_l2(rgb.cpu().numpy(), ref["rgb"]) < TOL
        # the ray leaving the bound, per ray: var and weights too, and the backward voxel row by voxel row (tests/local_parity.py)
        LP.compare_forward(dict(rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy(), var=var.cpu().numpy(), weights=w.cpu().numpy()), ref, "edge ray gt %.0f" % gtv)
        if gtv > 0:
            g_c, g_d, g_v = np.array([[0.3, -0.2, 0.5]], np.float32), np.array([1.0], np.float32), np.array([0.25], np.float32)
            ctx.zero_grads()
            g_ro, g_rd = ctx.render_backward("color", cu(ro), cu(rd), cu(gt), -1.0, cu(g_c), cu(g_d), cu(g_v), flags=5)
            levels = ["middle", "fine", "color"]
            hip = dict(g_grids={k: ctx.grid_download(k, grad=True) for k in levels}, g_rays_o=g_ro.cpu().numpy(), g_rays_d=g_rd.cpu().numpy())
            bits = {k: ctx.debug_relu_bits(k, 48) for k in levels}
            sig_on = (ctx.debug_fetch("occ1", 48) + ctx.debug_fetch("occ2", 48)) > 0
            rays1 = dict(rays_o=ro, rays_d=rd, gt_depth=gt)
            r32, r64 = [LP.forced_reference(o, sc, rays1, "color", -1.0, g_c, g_d, g_v, bits, sig_on, decoders=False) for o in (oracle32, oracle64)]
            LP.compare_backward(hip, r32, r64, levels, "edge ray backward")
    ctx16 = make_ctx(sc, n_samples=16, n_surface=0)
    rays = scenes.make_rays(1, 203, b)
    ref = oracle32.render_forward(oracle32.opts(b, n_samples=16, n_surface=0), sc["grids"], sc["decoders"], "coarse", rays["rays_o"], rays["rays_d"], None)
    rgb, depth, var, w = ctx16.render_forward("coarse", cu(rays["rays_o"]), cu(rays["rays_d"]), None)
    assert w.shape == (203, 16) and rel_l2(depth.cpu().numpy(), ref["depth"]) < TOL
    import nice_slam_cpp_amd as pkg
    with pytest.raises(pkg.NskError):
        ctx.set_render_opts(n_samples=60, n_surface=16)
    empty = pkg.Context(0)
    with pytest.raises(pkg.NskError):
        empty.render_forward("color", cu(ro), cu(rd), None)


def test_reference_sized_scene_forward(oracle32):
    """reference grid shapes and init (src/main.cpp:33-78), 1000 rays x 48 samples (K2 size)"""
    sc = scenes.make_scene(11)
    rays = scenes.make_rays(12, 1000, sc["bound"], n_frames=5)
    ref = oracle32.render_forward(oracle32.opts(sc["bound"]), sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"])
    ctx = make_ctx(sc)
    rgb, depth, var, w = ctx.render_forward("color", cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]))
    assert rel_l2(depth.cpu().numpy(), ref["depth"]) < TOL
    assert rel_l2(rgb.cpu().numpy(), ref["rgb"]) < TOL
    assert rel_l2(var.cpu().numpy(), ref["var"]) < TOL
    # size-independent properties: weights in [0,1], sum <= 1, depth inside the sampled range
    wn = w.cpu().numpy()
    assert wn.min() >= 0 and wn.sum(1).max() <= 1 + 1e-5


@pytest.mark.parametrize("matmul_mode", [2, 1, 0])
def test_mapping_steps_match_oracle(matmul_mode, oracle32):
    """north_star metric: optimised grids (and colour decoder) after Adam steps, 1e-4 relative L2; every forward
    matrix path (2 = fp16 2-piece split, the default; 1 = bf16 3-piece split -- the fused Adam kernel refreshes the fragment image of
    either; 0 = fp32 MFMA)"""
    sc = _scene(21, grid_std=0.05)
    rays = scenes.make_rays(22, 200, sc["bound"], n_frames=2)
    ctx = make_ctx(sc, trainable=["color"])
    ctx.set_matmul_mode(matmul_mode)
    rng = np.random.default_rng(5)
    masks = {k: rng.random(sc["grids"][k].shape[1:]) < 0.7 for k in ("middle", "fine", "color")}
    for k, m in masks.items():
        ctx.set_mask(k, m)
    lr = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]          # config/nice_slam.yaml:90-95 colour stage
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    # oracle state
    o = oracle32
    grids = {k: v.copy() for k, v in sc["grids"].items()}
    decs = {k: v.copy() for k, v in sc["decoders"].items()}
    mom = {k: (np.zeros_like(grids[k]), np.zeros_like(grids[k])) for k in masks}
    dm, dv = np.zeros_like(decs["color"]), np.zeros_like(decs["color"])
    loss_t = torch.zeros(1, device="cuda")
    for step in range(1, 4):
        ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, loss=loss_t)
        ctx.adam_step(lr)
        op = o.opts(sc["bound"])
        fw = o.render_forward(op, grids, decs, "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"])
        l_ref, g_d, g_c = o.loss_map(fw["depth"], fw["rgb"], rays["gt_depth"], rays["gt_color"], 0.2, True)
        assert abs(float(loss_t) - l_ref) < 2e-4 * abs(l_ref)
        bw = o.render_backward(op, grids, decs, "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"], -1.0, g_c, g_d, None,
                               want_rays=False)
        for k in masks:
            vm = np.broadcast_to(masks[k][None], grids[k].shape)
            o.adam_step(grids[k], bw["g_grids"][k], mom[k][0], mom[k][1], 0.005, step, mask=vm)
        o.adam_step(decs["color"], bw["g_decoders"]["color"], dm, dv, 0.005, step)
    ctx.sync()
    for k in masks:
        got = ctx.grid_download(k)
        assert rel_l2(got, grids[k]) < TOL, k
        assert np.array_equal(got[:, ~masks[k]], sc["grids"][k][:, ~masks[k]])      # unmasked voxels never move
    assert rel_l2(ctx.decoder_download("color"), decs["color"]) < TOL
    assert np.array_equal(ctx.decoder_download("fine"), sc["decoders"]["fine"])


def test_tracking_steps_match_oracle(oracle32, oracle64):
    """Tracker::optimize_cam_in_batch (src/Tracker.cpp:41-89): pose 7-vector after Adam iterations, 1e-4 relative L2.
    Pixel indices are an input (torch::randint cannot be matched)."""
    sc = _scene(31, grid_std=0.3)
    b = sc["bound"]
    rays0 = scenes.make_rays(32, 200, b, H=480, W=640, fx=360.0, fy=360.0, cx=320.0, cy=240.0, n_frames=1, edge=20)
    intr = rays0["intr"]
    c2w0 = rays0["c2w"][0]
    # start from a slightly perturbed pose (quaternion of a small rotation composed with the true one is overkill here:
    # the test needs identical inputs on both sides, not a converging tracker)
    R = c2w0[:3, :3].astype(np.float64)
    qw = np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])
    cam0 = np.concatenate([q * 1.3, c2w0[:3, 3] + np.array([0.02, -0.01, 0.015])]).astype(np.float32)   # un-normalised q is allowed
    pi, pj = rays0["pix_i"], rays0["pix_j"]
    gt_d, gt_c = rays0["gt_depth"], rays0["gt_color"]
    ctx = make_ctx(sc)
    cam = cu(cam0); m = torch.zeros(7, device="cuda"); v = torch.zeros(7, device="cuda")
    pi_t, pj_t = cu(pi, torch.int32), cu(pj, torch.int32)
    loss_t = torch.zeros(1, device="cuda")
    losses, g_first = [], None
    for step in range(1, 4):
        c2w = ctx.camera_from_tensor(cam)
        ro, rd = ctx.rays_from_pixels(pi_t, pj_t, intr, c2w)
        keep = ctx.inside_filter(ro, rd, cu(gt_d))
        idx = torch.nonzero(keep).squeeze(1)
        ro_k, rd_k = ro[idx].contiguous(), rd[idx].contiguous()
        gd_k, gc_k = cu(gt_d)[idx].contiguous(), cu(gt_c)[idx].contiguous()
        g_ro = torch.empty_like(ro_k); g_rd = torch.empty_like(rd_k)
        ctx.track_step("color", ro_k, rd_k, gd_k, gc_k, -1.0, 0.5, True, True, True, flags=4, loss=loss_t, g_rays=(g_ro, g_rd))
        g_c2w = ctx.rays_backward(pi_t[idx].contiguous(), pj_t[idx].contiguous(), intr, g_ro, g_rd)
        g_cam = ctx.camera_backward(cam, g_c2w)
        ctx.adam_vector(cam, g_cam, m, v, 1e-2, step)
        losses.append(float(loss_t))
        if step == 1:
            g_first = g_cam.cpu().numpy()

    def oracle_track(o):
        cam_ref = cam0.astype(o.dt); m_ref = np.zeros(7, o.dt); v_ref = np.zeros(7, o.dt)
        ls, g1 = [], None
        for step in range(1, 4):
            c2w_r = o.camera_from_tensor(cam_ref)
            ro_r, rd_r = o.rays_from_pixels(pi, pj, *intr, c2w_r)
            keep_r = o.inside_filter(b, ro_r, rd_r, gt_d)
            op = o.opts(b)
            fw = o.render_forward(op, sc["grids"], sc["decoders"], "color", ro_r[keep_r], rd_r[keep_r], gt_d[keep_r])
            l_ref, gD, gC, gV = o.loss_track(fw["depth"], fw["rgb"], fw["var"], gt_d[keep_r], gt_c[keep_r], 0.5, True, True, True)
            bw = o.render_backward(op, sc["grids"], sc["decoders"], "color", ro_r[keep_r], rd_r[keep_r], gt_d[keep_r], -1.0, gC, gD, None,
                                   want_grids=False, want_decoders=False)
            g_c2w_r = o.rays_backward(pi[keep_r], pj[keep_r], *intr, bw["g_rays_o"], bw["g_rays_d"])
            g_cam_r = o.camera_backward(cam_ref, g_c2w_r)
            if step == 1:
                g1 = g_cam_r.copy()
            o.adam_step(cam_ref, g_cam_r, m_ref, v_ref, 1e-2, step)
            ls.append(l_ref)
        return cam_ref, ls, g1

    cam32, l32, g32 = oracle_track(oracle32)
    cam64, l64, g64 = oracle_track(oracle64)
    for a, r in zip(losses, l32):
        assert abs(a - r) < 1e-3 * abs(r), (a, r)
    # the pose gradient sums ReLU-kinked per-sample terms over ~10^4 samples: two fp32 evaluations differ by whatever
    # the fp32 oracle differs from the fp64 one; the HIP path must be at least that close to the fp64 truth
    e_g, e_g_ref = rel_l2(g_first, g64), rel_l2(g32, g64)
    assert e_g < max(5 * TOL, 3 * e_g_ref), (e_g, e_g_ref)
    e_p, e_p_ref = rel_l2(cam.cpu().numpy(), cam64), rel_l2(cam32, cam64)
    assert e_p < max(TOL, 3 * e_p_ref), (e_p, e_p_ref)
    print("tracking: grad err hip %.2e oracle32 %.2e | pose err hip %.2e oracle32 %.2e" % (e_g, e_g_ref, e_p, e_p_ref))


@pytest.mark.parametrize("n_rays,masked", [(200, False), (37, True), (1023, False), (1500, False), (1, False), (2, True), (5, False), (1000, True)])
def test_tracker_median_in_the_composite_launch(n_rays, masked):
    """Tracker.cpp:67-71: the 10 x median threshold in its three forms -- found by every workgroup of the BACKWARD launch from residuals the
    compositing left (composite mode 5 + k_decode_bwd_track: the default with ray gradients, no barrier anywhere), found inside the loss launch
    behind a grid barrier (k_composite mode 4: round 3's form, still what a call without ray gradients takes), and the three-launch form
    (composite, k_median_thr, composite) -- gives the same loss bits and the same ray gradients; ray counts that are not a multiple of the four
    rays of a workgroup, a ray mask, and a batch above the fused forms' limit (1500 rays: all runs take the three launches)"""
    sc = _scene(33, grid_std=0.3)
    rays = scenes.make_rays(34, n_rays, sc["bound"], n_frames=1, zero_frac=0.1)
    out = {}
    forms = {"deferred": {}, "barrier": {"no_deferred_median": 1}, "three": {"no_fused_median": 1}}
    for form, tune in forms.items():
        ctx = make_ctx(sc)
        for k, v in tune.items():
            ctx.set_tuning(k, v)
        if masked:
            keep = (np.arange(n_rays) % 3 != 0).astype(np.uint8)
            ctx.set_ray_mask(cu(keep, torch.uint8))
        ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
        g_ro = torch.empty_like(ro); g_rd = torch.empty_like(rd); loss = torch.zeros(1, device="cuda")
        for _ in range(3):          # the barrier re-arms itself: three launches in a row
            ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, True, True, True, flags=4, loss=loss, g_rays=(g_ro, g_rd))
        ctx.sync()
        out[form] = (float(loss), g_ro.cpu().numpy().copy(), g_rd.cpu().numpy().copy())
    for form in ("deferred", "barrier"):
        assert out[form][0] == out["three"][0], (form, out[form][0], out["three"][0])
        # the ray gradients are sums of atomics over the samples' tiles: equal up to the order of those adds
        assert rel_l2(out[form][1], out["three"][1]) < 1e-6 and rel_l2(out[form][2], out["three"][2]) < 1e-6, form
        # and a ray the threshold drops has an exactly zero gradient in every form
        assert np.array_equal(np.all(out[form][2] == 0, axis=1), np.all(out["three"][2] == 0, axis=1)), form


@pytest.mark.parametrize("stage", ["fine", "color"])
def test_forward_bf16_split_mode_matches_oracle(stage, oracle32, oracle64):
    """matmul modes 1 (fp32 operands as three bf16 pieces, six bf16 MFMAs per product) and 2 (two fp16 pieces, 22 significant
    bits, three MFMAs) -- both must stay inside the same 1e-4 contract, and stay close to the fp64 truth: mode 1 as close as the plain
    fp32 path, mode 2 within 1e-5 of it (measured: see the assert message)"""
    sc = _scene()
    rays = scenes.make_rays(4, 100, sc["bound"], n_frames=2, zero_frac=0.1)
    gd = rays["gt_depth"]
    ref = oracle32.render_forward(oracle32.opts(sc["bound"]), sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], gd)
    ref64 = oracle64.render_forward(oracle64.opts(sc["bound"]), sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], gd)
    errs = {}
    for mode in (0, 1, 2):
        ctx = make_ctx(sc)
        ctx.set_matmul_mode(mode)
        rgb, depth, var, w = ctx.render_forward(stage, cu(rays["rays_o"]), cu(rays["rays_d"]), cu(gd))
        ctx.sync()
        assert rel_l2(depth.cpu().numpy(), ref["depth"]) < TOL and rel_l2(w.cpu().numpy(), ref["weights"]) < TOL
        if stage == "color":
            assert rel_l2(rgb.cpu().numpy(), ref["rgb"]) < TOL
        errs[mode] = rel_l2(w.cpu().numpy(), ref64["weights"])
    print("rel L2 of the weights against the fp64 oracle per matmul mode:", errs)
    assert errs[1] < 3 * errs[0] + 1e-6, errs
    assert errs[2] < 1e-5, errs


def test_frustum_mask_matches_oracle(oracle32):
    """next row N2: Mapper::get_mask_from_c2w (src/Mapper.cpp:42-130) on the device, bit-exact against the restatement"""
    sc = scenes.make_scene(41)
    b = sc["bound"]
    H, W, fx, fy, cx, cy = 120, 160, 80.0, 80.0, 79.5, 59.5
    rng = np.random.default_rng(3)
    c2w = scenes.make_camera(rng, b)
    # depth image of the room walls + a band of zeros (invalid depth)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dirs = np.stack([(ii - cx) / fx, -(jj - cy) / fy, -np.ones_like(ii, dtype=np.float64)], -1).reshape(-1, 3) @ c2w[:3, :3].T.astype(np.float64)
    o = np.broadcast_to(c2w[:3, 3].astype(np.float64), dirs.shape)
    room = b.astype(np.float64).copy(); room[:, 0] += 0.3; room[:, 1] -= 0.3
    depth = scenes._ray_box_far(room, o, dirs).reshape(H, W).astype(np.float32)
    depth[40:50, :] = 0.0
    ctx = make_ctx(sc)
    total = 0
    for level in ("coarse", "middle", "fine", "color"):
        shape = sc["grids"][level].shape[1:]
        ref = oracle32.frustum_mask(b, shape, depth, (fx, fy, cx, cy), c2w, is_coarse=(level == "coarse"))
        got = ctx.frustum_mask(level, cu(depth), (fx, fy, cx, cy), c2w)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (level, int((got != ref).sum()))
        if level != "coarse":
            assert 0 < ref.sum() < ref.size
        total += int(ref.sum())
    # the installed mask is what Adam honours: voxels outside never move
    rays = scenes.make_rays(5, 200, b, n_frames=1)
    ctx.map_step("color", cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"]), -1.0, 0.5, True, flags=1)
    ctx.adam_step([0.0, 0.0, 0.005, 0.005, 0.005, 0.0])
    fine_mask = oracle32.frustum_mask(b, sc["grids"]["fine"].shape[1:], depth, (fx, fy, cx, cy), c2w)
    new = ctx.grid_download("fine")
    assert np.array_equal(new[:, ~fine_mask], sc["grids"]["fine"][:, ~fine_mask]) and np.abs(new - sc["grids"]["fine"]).max() > 0


def test_keyframe_overlap_matches_oracle(oracle32):
    """next row N3: Mapper::keyframe_selection_overlap (src/Mapper.cpp:132-196): the per-keyframe fractions are counts over the
    same fp32 arithmetic, so they must agree exactly; the ranking the Mapper derives from them follows"""
    from test_oracle import _overlap_case
    r, cams, intr, HW = _overlap_case(seed=5, n=100, K=9)
    ref = oracle32.keyframe_overlap(r["rays_o"], r["rays_d"], r["gt_depth"], intr, HW, cams)
    sc = scenes.make_scene(1, grid_shapes=scenes.SMALL_GRID_SHAPES)
    ctx = make_ctx(sc)
    got = ctx.keyframe_overlap(cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), intr, HW, cams)
    assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float32)), (got, ref)
    assert len(set(np.argsort(-got, kind="stable")[:3])) == 3 and got.max() > 0.5


def test_sample_and_gather_pixels_match_oracle(oracle32):
    """next row N1: raySampler's pixel draw + ground-truth gather on the device (utils.h:13-43), index-exact against the oracle's
    restatement of the same hash; rays from those pixels through nsk_rays_from_pixels as before"""
    H, W = 96, 128
    rng = np.random.default_rng(2)
    depth = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    color = rng.random((H, W, 3)).astype(np.float32)
    sc = scenes.make_scene(1, grid_shapes=scenes.SMALL_GRID_SHAPES)
    ctx = make_ctx(sc)
    for seed, n, win in ((11, 1000, (0, H, 0, W)), (12, 333, (10, H - 10, 20, W - 20)), (13, 1, (5, 6, 7, 8))):
        pi, pj = ctx.sample_pixels(seed, n, *win)
        ri, rj = oracle32.sample_pixels(seed, n, *win)
        assert np.array_equal(pi.cpu().numpy(), ri) and np.array_equal(pj.cpu().numpy(), rj)
        gd, gc = ctx.gather_pixels(pi, pj, cu(depth), cu(color))
        rgd, rgc = oracle32.gather_pixels(ri, rj, depth, color)
        assert np.array_equal(gd.cpu().numpy(), rgd) and np.array_equal(gc.cpu().numpy(), rgc)
    c2w = scenes.make_camera(rng, sc["bound"])
    ro, rd = ctx.rays_from_pixels(pi, pj, (80.0, 80.0, 63.5, 47.5), cu(np.ascontiguousarray(c2w[:3, :4])))
    rro, rrd = oracle32.rays_from_pixels(ri, rj, 80.0, 80.0, 63.5, 47.5, c2w)
    assert np.array_equal(ro.cpu().numpy(), rro) and rel_l2(rd.cpu().numpy(), rrd) < 1e-6


def test_backward_with_several_iterations_per_workgroup(oracle32, oracle64):
    """5000 rays = 15000 tiles: the trainable role runs more than two panel iterations per workgroup (staged loads, image
    swaps, resident embedding rows and the scatter all cross iteration boundaries); colour decoder trainable only, as in
    the mapping step"""
    out_all, _, _ = _backward_case("color", True, False, oracle32, oracle64, ["color"], n_rays=5000, seed=31, filtered=False)
    _assert_gradients(out_all, "all rays")
    out, ctx, sc = _backward_case("color", True, False, oracle32, oracle64, ["color"], n_rays=5000, seed=31)
    _assert_gradients(out, "filtered")


def test_graph_replay_matches_eager_steps(oracle32):
    """hipGraph capture of a mapping step (nsk_graph_begin / end / launch): three replays must leave the same optimised state as
    three eager steps (up to the order of the atomic adds), including Adam's per-step bias correction"""
    sc = _scene(23, grid_std=0.05)
    rays = scenes.make_rays(24, 300, sc["bound"], n_frames=2)
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    lr = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]
    out = {}
    for mode in ("eager", "graph"):
        ctx = make_ctx(sc, trainable=["color"])
        loss = torch.zeros(1, device="cuda")
        with torch.cuda.stream(ctx.tstream):
            def step():
                ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, loss=loss)
                ctx.adam_step(lr)
            step()                                   # step 1 eagerly in both (sizes the workspaces)
            if mode == "eager":
                step(); step(); step()
            else:
                ctx.graph_begin(); step(); gid = ctx.graph_end()
                for _ in range(3):
                    ctx.graph_launch(gid)
                ctx.graph_destroy(gid)
        ctx.sync()
        out[mode] = ({k: ctx.grid_download(k) for k in ("middle", "fine", "color")}, ctx.decoder_download("color"), float(loss))
    for k in ("middle", "fine", "color"):
        assert np.abs(out["eager"][0][k] - sc["grids"][k]).max() > 1e-3
        assert rel_l2(out["graph"][0][k], out["eager"][0][k]) < 1e-5, k
    assert rel_l2(out["graph"][1], out["eager"][1]) < 1e-5
    assert abs(out["graph"][2] - out["eager"][2]) < 1e-4 * abs(out["eager"][2])


def test_graph_is_refused_after_a_mask_change(oracle32):
    """A captured step holds the optimiser masks' voxel lists as kernel arguments (k_adam_multi walks the marked voxels): new mask
    CONTENTS must make nsk_graph_launch refuse the replay (it used to replay onto the old list silently), and a fresh capture must
    equal the eager steps under the new mask"""
    sc = _scene(27, grid_std=0.05)
    rays = scenes.make_rays(28, 300, sc["bound"], n_frames=2)
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    lr = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]
    rng = np.random.default_rng(5)
    masks_a = {k: (rng.random(sc["grids"][k].shape[1:]) < 0.5).astype(np.uint8) for k in ("middle", "fine", "color")}
    masks_b = {k: (1 - v).astype(np.uint8) for k, v in masks_a.items()}
    out = {}
    for mode in ("eager", "graph"):
        ctx = make_ctx(sc, trainable=["color"])
        loss = torch.zeros(1, device="cuda")
        with torch.cuda.stream(ctx.tstream):
            def step():
                ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, loss=loss)
                ctx.adam_step(lr)
            for k, v in masks_a.items():
                ctx.set_mask(k, v)
            step()
            if mode == "graph":
                ctx.graph_begin(); step(); gid = ctx.graph_end()
                ctx.graph_launch(gid)
            else:
                step()
            for k, v in masks_b.items():             # same allocation, new contents
                ctx.set_mask(k, v)
            if mode == "graph":
                with pytest.raises(RuntimeError, match="stale"):
                    ctx.graph_launch(gid)
                step()                               # eager once (rebuilds the voxel lists), then capture again
                ctx.graph_begin(); step(); gid2 = ctx.graph_end()
                ctx.graph_launch(gid2)
            else:
                step(); step()
        ctx.sync()
        out[mode] = {k: ctx.grid_download(k) for k in ("middle", "fine", "color")}
    for k in ("middle", "fine", "color"):
        moved = np.abs(out["eager"][k] - sc["grids"][k]).max(axis=0)
        assert (moved[masks_a[k] > 0] > 0).any() and (moved[masks_b[k] > 0] > 0).any()
        assert rel_l2(out["graph"][k], out["eager"][k]) < 1e-5, k


def test_fused_pose_kernels_equal_their_parts():
    """nsk_rays_from_camera = camera_from_tensor + rays_from_pixels and nsk_pose_step = rays_backward + camera_backward +
    adam_vector: same arithmetic, so the same bits.  One camera and one batch here; the parts themselves are checked in tests/test_gpu_pose.py
    (forward to the bit, the two backward kernels component by component inside derived fp64 bounds), which also repeats this claim across
    quaternion kinds, batch sizes and consecutive steps"""
    sc = scenes.make_scene(1, grid_shapes=scenes.SMALL_GRID_SHAPES)
    ctx = make_ctx(sc)
    rng = np.random.default_rng(9)
    n = 333
    pi = cu(rng.integers(0, 640, n), torch.int32); pj = cu(rng.integers(0, 480, n), torch.int32)
    intr = (360.0, 355.0, 320.5, 239.5)
    cam = cu(np.array([0.9, 0.2, -0.3, 0.1, 0.5, -0.2, 0.4], np.float32))
    for mode in (0, 1, 2):
        c2w = ctx.camera_from_tensor(cam)
        ro, rd = ctx.rays_from_pixels(pi, pj, intr, c2w, mode)
        ro2, rd2 = ctx.rays_from_camera(pi, pj, intr, cam, mode)
        assert torch.equal(ro, ro2) and torch.equal(rd, rd2)
    g_ro = cu(rng.standard_normal((n, 3))); g_rd = cu(rng.standard_normal((n, 3)))
    cam_a, m_a, v_a = cam.clone(), cu(rng.random(7) * 0.1), cu(rng.random(7) * 0.01)
    cam_b, m_b, v_b = cam_a.clone(), m_a.clone(), v_a.clone()
    for step in (3, 4):
        g_cam = ctx.camera_backward(cam_a, ctx.rays_backward(pi, pj, intr, g_ro, g_rd))
        ctx.adam_vector(cam_a, g_cam, m_a, v_a, 1e-2, step)
        g_out = torch.zeros(7, device="cuda")
        ctx.pose_step(pi, pj, intr, g_ro, g_rd, cam_b, m_b, v_b, 1e-2, step, g_cam_out=g_out)
        assert torch.equal(g_out, g_cam)
        assert torch.equal(cam_a, cam_b) and torch.equal(m_a, m_b) and torch.equal(v_a, v_b)


def test_prepare_rays_equals_the_separate_entry_points():
    """nsk_prepare_rays (one launch for a window of frames) against nsk_sample_pixels + nsk_gather_pixels + nsk_rays_from_pixels /
    nsk_rays_from_camera + nsk_inside_filter frame by frame: every output bit for bit (two frames, one posed by a 7-vector, one by a
    c2w matrix; 300 rays each, a cropped window as the Tracker uses)"""
    import torch
    sc = scenes.make_scene(3, scenes.SMALL_GRID_SHAPES)
    ctx = make_ctx(sc)
    rng = np.random.default_rng(5)
    H, W = 96, 128
    intr = (110.0, 108.0, 63.5, 47.5)
    frames = []
    for k in range(2):
        depth = torch.tensor(rng.uniform(0.5, 6.0, (H, W)).astype(np.float32), device="cuda")
        color = torch.tensor(rng.random((H, W, 3)).astype(np.float32), device="cuda")
        if k == 0:
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            pose = torch.tensor(np.concatenate([q, rng.uniform(-1, 1, 3)]).astype(np.float32), device="cuda")
        else:
            c2w = np.asarray(scenes.make_camera(np.random.default_rng(7), sc["bound"], "y"), np.float32).reshape(-1)[:12]
            pose = torch.tensor(np.ascontiguousarray(c2w), device="cuda")
        frames.append(dict(depth=depth, color=color, pose=pose, seed=1000 + 17 * k))
    n = 300
    win = (8, H - 8, 12, W - 12)
    got = ctx.prepare_rays(frames, n, win, intr)
    ctx.sync()
    for k, f in enumerate(frames):
        pi, pj = ctx.sample_pixels(f["seed"], n, *win)
        gd, gc = ctx.gather_pixels(pi, pj, f["depth"], f["color"])
        if f["pose"].numel() == 7:
            ro, rd = ctx.rays_from_camera(pi, pj, intr, f["pose"])
        else:
            ro, rd = ctx.rays_from_pixels(pi, pj, intr, f["pose"])
        keep = ctx.inside_filter(ro, rd, gd)
        ctx.sync()
        sl = slice(k * n, (k + 1) * n)
        for name, a, b in (("pix_i", got["pix_i"][sl], pi), ("pix_j", got["pix_j"][sl], pj), ("gt_depth", got["gt_depth"][sl], gd), ("gt_color", got["gt_color"][sl], gc),
                           ("rays_o", got["rays_o"][sl], ro), ("rays_d", got["rays_d"][sl], rd), ("keep", got["keep"][sl].bool(), keep)):
            assert torch.equal(a.cpu().reshape(-1), b.cpu().reshape(-1)), (k, name)
    # more frames than one launch's table holds (16): the call splits, outputs stay frame-major
    many = [dict(depth=frames[k % 2]["depth"], color=frames[k % 2]["color"], pose=frames[k % 2]["pose"], seed=5000 + k) for k in range(19)]
    got = ctx.prepare_rays(many, 40, win, intr)
    ctx.sync()
    for k in (0, 15, 16, 18):
        pi, pj = ctx.sample_pixels(5000 + k, 40, *win)
        gd, _ = ctx.gather_pixels(pi, pj, many[k]["depth"], many[k]["color"])
        ctx.sync()
        sl = slice(k * 40, (k + 1) * 40)
        assert torch.equal(got["pix_i"][sl].cpu(), pi.cpu()) and torch.equal(got["gt_depth"][sl].cpu(), gd.cpu()), k
    ctx.close()


@pytest.mark.parametrize("n_samples,n_surface", [(24, 16), (20, 0), (32, 5)])
def test_sample_counts_that_are_not_multiples_of_the_tile(n_samples, n_surface, oracle32, oracle64):
    """S = 40, 20, 37 samples per ray: 16-sample tiles straddle rays (the per-tile ray-gradient sum falls back to per-sample adds, the
    last tile of the batch is partly empty).  Forward outputs and the full backward (grids, trainable decoders, rays) against the oracle."""
    sc = _scene(51)
    rays = scenes.make_rays(52, 77, sc["bound"], n_frames=2, zero_frac=0.1)
    gd = rays["gt_depth"]
    N = rays["rays_o"].shape[0]                 # 76: two frames of 38
    rng = np.random.default_rng(53)
    g_rgb, g_d = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    kw = dict(n_samples=n_samples, n_surface=n_surface)
    frag = oracle64.ray_fragility(oracle64.opts(sc["bound"], **kw), sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], gd)
    keep = frag > 2e-5
    assert keep.mean() > 0.5
    g_rgb[~keep] = 0; g_d[~keep] = 0
    ctx = make_ctx(sc, trainable=["color"], **kw)
    rgb, depth, var, w = ctx.render_forward("color", cu(rays["rays_o"]), cu(rays["rays_d"]), cu(gd))
    fw = oracle32.render_forward(oracle32.opts(sc["bound"], **kw), sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], gd)
    assert w.shape == (N, n_samples + n_surface)
    assert rel_l2(depth.cpu().numpy(), fw["depth"]) < TOL and rel_l2(rgb.cpu().numpy(), fw["rgb"]) < TOL and rel_l2(w.cpu().numpy(), fw["weights"]) < TOL
    ref = oracle32.render_backward(oracle32.opts(sc["bound"], **kw), sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], gd, -1.0, g_rgb, g_d, None)
    g_ro, g_rd = ctx.render_backward("color", cu(rays["rays_o"]), cu(rays["rays_d"]), cu(gd), -1.0, cu(g_rgb), cu(g_d), None, flags=7)
    ctx.sync()
    for k in ("middle", "fine", "color"):
        assert rel_l2(ctx.grid_download(k, grad=True), ref["g_grids"][k]) < TOL, k
    assert rel_l2(ctx.decoder_download("color", grad=True), ref["g_decoders"]["color"]) < TOL
    assert rel_l2(g_ro.cpu().numpy(), ref["g_rays_o"]) < TOL and rel_l2(g_rd.cpu().numpy(), ref["g_rays_d"]) < TOL
    ctx.close()


@pytest.mark.parametrize("stage", ["fine", "color"])
@pytest.mark.parametrize("n_rays", [1, 7, 100, 333])
def test_forward_merged_occupancy_role_has_the_bits_of_the_separate_roles(stage, n_rays):
    """The forward's middle and fine decoders as ONE workgroup role (decode_fwd_occ_body: the middle level looked up once, both weight images in
    LDS) against the three-role launch, each forced by nsk_set_tuning("no_occ_role", 2 | 1) -- the host otherwise takes whichever split
    predicts the shorter launch, so at these ragged sizes (a single ray, partial tiles, rays without depth, both sample orders) the merged body
    would not run by itself.  Each decoder's arithmetic is the same instruction sequence in both forms: rendered arrays, the per-sample decoder
    outputs and the ReLU bits a mapping step saves must agree bit for bit."""
    sc = _scene(41, grid_std=0.3)
    rays = scenes.make_rays(42, n_rays, sc["bound"], n_frames=1, zero_frac=0.2)
    got = {}
    for form in (1, 2):
        for sort_mode in (0, 1):
            ctx = make_ctx(sc, trainable=["color"] if stage == "color" else [])
            ctx.set_tuning("no_occ_role", form)
            ctx.set_sort_mode(sort_mode)
            ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
            rgb, depth, var, w = ctx.render_forward(stage, ro, rd, gd)
            loss = torch.zeros(1, device="cuda")
            ctx.map_step(stage, ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss)
            ctx.sync()
            M = n_rays * w.shape[1]
            got[form, sort_mode] = [rgb.cpu().numpy(), depth.cpu().numpy(), var.cpu().numpy(), w.cpu().numpy(), np.float32(float(loss)),
                                    ctx.debug_fetch("occ1", M), ctx.debug_fetch("occ2", M), ctx.debug_relu_bits("middle", M), ctx.debug_relu_bits("fine", M)]
    for sort_mode in (0, 1):
        for a, b in zip(got[1, sort_mode], got[2, sort_mode]):
            assert np.array_equal(a, b, equal_nan=True), (stage, n_rays, sort_mode)

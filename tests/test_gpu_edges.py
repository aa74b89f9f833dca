"""GPU parity (-m gpu) per ray and per voxel row on the scenes built at the geometric edges (tests/edge_scenes.py), with the localised
comparison of tests/local_parity.py: the worst ray against RAY_TOL = 1e-4, the worst voxel row against 8 x kappa_ref, kappa_ref being the fp32
oracle against the fp64 oracle on the SAME forced branches (the HIP forward's hidden-ReLU bits, its relu(sigma) branches, the L1 signs of its
residuals), measured inside the test on the very batch; voxels no sample touches must be exactly zero.

Every scene: forward on all rays (the non-finite rays must be the fp32 oracle's, which tests/test_local_parity_cpu.py shows to be exactly the
constructed ones); then, with the ray mask dropping those rays, nsk_map_step as the Mapper runs it (flags 3), with ray gradients (flags 7), and
nsk_render_backward with a depth-variance seed and every decoder of the stage trainable (flags 7), against the oracles on the compacted batch.
The coarse stage (thin-grid scene, a 1-voxel axis) has no ReLU dump (nsk_debug_relu_bits covers the three MLP decoders): both oracles take the fp32
oracle's own hidden-ReLU branches there, relu(sigma) and the L1 signs are the HIP forward's; its decoder has no embedding, so the HIP ReLU inputs differ
from the oracle's by the rounding of the matrix products only.

Measured on an MI355X (worst grid level over stages, sort and matmul modes; kappa's denominator is R_v + 2^-24 max R, tests/local_parity.py;
every test prints its own figures):
    scene              kappa (GPU)   kappa_ref   ratio (limit 8)
    lattice            3.6e-5        3.6e-5      1.4
    outside-on-bound   2.0e-4        2.0e-4      2.0
    thin-grids         2.6e-5        2.1e-5      4.2
    one-cell           2.5e-6        5.5e-7      6.2
    max-spread         6.5e-3        6.5e-3      1.0
    principal-point    2.1e-5        2.1e-5      1.2
  worst ray: forward <= 1e-5 of its magnitude, ray gradients <= 9.6e-5 of their scale (the fp32 oracle's own: 9.6e-5, outside-on-bound colour stage).
Mutation check (done once on scratch builds, nothing of it committed; every address stays inside the grid):
  (i)   scatter_tile's flush with sv[3] = s2 for runs whose first voxel lies on the lower x face: test_edge_scene fails in all six lattice / outside
        cases at map_step flags 3, grid middle, kappa 1.4 .. 3.5 (limit 8 x 3.6e-6 .. 1.3e-4) at voxel (5, 4, 0) (edge) / (1, 4, 0) (edge) / (4, 1, 0)
        (face).  The parent's suite notices this form too (19 failures in test_gpu_parity / test_gpu_relu / test_gpu_configs: a ninth of all runs
        start on that face), contrary to what the issue expected;
  (ii)  dropping `mul = 0.f` in tri_setup's `x >= mx` clip changes NO result, in any test old or new: it is an equivalent mutant.  At the upper
        clip t = 0 and the +1 neighbour is clamped to the same voxel, so tri_grad_p's pairs (-dot, +dot) cancel exactly and gi[k] is 0 before it meets
        gmul.  The statement that can be wrong is the LOWER clip's (x <= 0: voxel 0 and voxel 1 differ);
  (ii') dropping `mul = 0.f` in the `x <= 0` clip: test_edge_scene[lattice-color] fails at g_rays_o ray 120 (8.9e-2 of its scale, limit 1e-4) and
        [outside-on-bound-color] at ray 52 (4.4e-2); the middle / fine stages cannot see it (a clipped sample is outside the bound and sends
        no occupancy gradient: only the colour reaches it).  Whether the parent's suite notices (ii') was not run.
Two kernel defects these scenes exposed are fixed with them (nsk_device.h): k_sample's rank sort gave every NaN z rank 0 and read the empty slots back
from uninitialised LDS (an upper-x-face ray rendered finite garbage or NaN from run to run); the compositing backward formed its exclusive suffix sum
as "inclusive minus own", which is 0 behind a masked sample of weight 1 (d loss / d rays_d of rays entering from outside: wrong sign).
"""
import numpy as np
import pytest
import torch

import edge_scenes as E
import local_parity as LP
from gpu_util import cu, make_ctx, stage_levels

pytestmark = pytest.mark.gpu
W_COLOR = 0.5
GRAD_ALL = 7


def _ctx(e, trainable):
    return make_ctx(e["sc"], n_samples=e["n_samples"], n_surface=e["n_surface"], trainable=trainable)


def _bits(ctx, o32, e, kept, stage, gmax, M, ks):
    """the hidden-ReLU branches the HIP forward took, by decoder; coarse: the fp32 oracle's own (no dump for that decoder)"""
    if stage == "coarse":
        op = o32.opts(e["sc"]["bound"], n_samples=e["n_samples"], n_surface=e["n_surface"])
        return {"coarse": o32.preacts(op, e["sc"]["grids"], e["sc"]["decoders"], "coarse", "coarse", kept["rays_o"], kept["rays_d"], kept["gt_depth"], gmax) > 0}
    return {k: ctx.debug_relu_bits(k, M)[ks] for k in stage_levels(stage)}


def _sigma(ctx, stage, M):
    if stage == "coarse":
        return ctx.debug_fetch("occ0", M)
    sig = ctx.debug_fetch("occ1", M)
    if stage in ("fine", "color"):
        sig = ctx.debug_fetch("occ2", M) + sig
    return sig


def _grads(ctx, stage, trainable):
    g = dict(g_grids={k: ctx.grid_download(k, grad=True) for k in stage_levels(stage)}, g_decoders={k: ctx.decoder_download(k, grad=True) for k in trainable})
    return g


def _references(o32, o64, e, rays, stage, gmax, g_c, g_d, g_v, bits, sig_on, decoders):
    kw = dict(n_samples=e["n_samples"], n_surface=e["n_surface"], decoders=decoders)
    return [LP.forced_reference(o, e["sc"], rays, stage, gmax, g_c, g_d, g_v, bits, sig_on, **kw) for o in (o32, o64)]


def check_scene(e, stage, oracle32, oracle64, sort_modes=(0, 1), matmul_modes=(2, 0), render_backward=True, profile=None):
    sc, rays = e["sc"], e["rays"]
    N = rays["rays_o"].shape[0]
    S = e["n_samples"] + e["n_surface"]
    M = N * S
    gmax = float(rays["gt_depth"].max())
    keep = ~e["made_nonfinite"]
    kept = {k: v[keep] for k, v in rays.items()}
    ks = np.repeat(keep, S)
    levels = stage_levels(stage)
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    mask = None if keep.all() else cu(keep.astype(np.uint8), torch.uint8)
    op32 = oracle32.opts(sc["bound"], n_samples=e["n_samples"], n_surface=e["n_surface"])
    with np.errstate(all="ignore"):
        ref_fw = oracle32.render_forward(op32, sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], rays["gt_depth"], gmax)
    figures = {}
    for mm in matmul_modes:
        for sm in sort_modes:
            label = "%s/%s sort %d matmul %d" % (e["name"], stage, sm, mm)
            trainable = ["color"] if stage == "color" else []
            ctx = _ctx(e, trainable)
            ctx.set_sort_mode(sm)
            ctx.set_matmul_mode(mm)
            # ---- forward, all rays: same non-finite rays as the fp32 oracle, every other ray within RAY_TOL ------------------------------
            rgb, depth, var, w = ctx.render_forward(stage, ro, rd, gd, gmax)
            got = dict(rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy(), var=var.cpu().numpy(), weights=w.cpu().numpy())
            bad = ~np.isfinite(got["depth"])
            assert (bad == e["made_nonfinite"]).all(), (label, np.flatnonzero(bad), np.flatnonzero(e["made_nonfinite"]))
            figures[label + " fwd"] = LP.compare_forward(got, ref_fw, label + " forward")
            ctx.set_ray_mask(mask)
            # ---- the Mapper's step (flags 3: the frozen / trainable-colour backward kernels), then with ray gradients (flags 7) -----------
            for flags in (3, GRAD_ALL):
                ctx.zero_grads()
                loss_t = torch.zeros(1, device="cuda")
                out = (torch.zeros(N, 3, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"))
                g_rays = (torch.zeros(N, 3, device="cuda"), torch.zeros(N, 3, device="cuda")) if flags & 4 else None
                if profile is not None:
                    ctx.profile_begin()
                ctx.map_step(stage, ro, rd, gd, gc, gmax, W_COLOR, stage == "color", flags=flags, loss=loss_t, outputs=out, g_rays=g_rays)
                if profile is not None:
                    profile.update(ctx.profile_end())
                hip = _grads(ctx, stage, trainable)
                # a masked ray whose box exit is NaN is sampled with far = 0 (include/nsk.h): it renders finite and takes no part in anything
                assert all(np.isfinite(t.cpu().numpy()[~keep]).all() for t in out), label
                if g_rays is not None:
                    assert not g_rays[0].cpu().numpy()[~keep].any() and not g_rays[1].cpu().numpy()[~keep].any(), label
                if g_rays is not None:
                    hip.update(g_rays_o=g_rays[0].cpu().numpy()[keep], g_rays_d=g_rays[1].cpu().numpy()[keep])
                bits = _bits(ctx, oracle32, e, kept, stage, gmax, M, ks)
                sig_on = (_sigma(ctx, stage, M) > 0)[ks]
                _, g_d, g_c = oracle32.loss_map(out[1].cpu().numpy()[keep], out[0].cpu().numpy()[keep], kept["gt_depth"], kept["gt_color"], W_COLOR, stage == "color")
                r32, r64 = _references(oracle32, oracle64, e, kept, stage, gmax, g_c, g_d, None, bits, sig_on, bool(trainable))
                for k in levels:
                    assert np.isfinite(hip["g_grids"][k]).all(), (label, k)
                figures[label + " map_step flags %d" % flags] = LP.compare_backward(hip, r32, r64, levels, label + " map_step flags %d" % flags, decoders=trainable)
            ctx.close()
    if render_backward:
        # ---- nsk_render_backward: given seeds with a depth-variance term, every decoder of the stage trainable ---------------------------
        label = "%s/%s render_backward" % (e["name"], stage)
        ctx = _ctx(e, levels)
        ctx.set_sort_mode(0)
        ctx.set_ray_mask(mask)
        rng = np.random.default_rng(11)
        g_c = (rng.standard_normal((N, 3)) * (stage == "color")).astype(np.float32)
        g_d, g_v = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
        g_ro, g_rd = ctx.render_backward(stage, ro, rd, gd, gmax, cu(g_c), cu(g_d), cu(g_v), flags=GRAD_ALL)
        hip = _grads(ctx, stage, levels)
        hip.update(g_rays_o=g_ro.cpu().numpy()[keep], g_rays_d=g_rd.cpu().numpy()[keep])
        bits = _bits(ctx, oracle32, e, kept, stage, gmax, M, ks)
        sig_on = (_sigma(ctx, stage, M) > 0)[ks]
        r32, r64 = _references(oracle32, oracle64, e, kept, stage, gmax, g_c[keep], g_d[keep], g_v[keep], bits, sig_on, True)
        figures[label] = LP.compare_backward(hip, r32, r64, levels, label, decoders=levels)
        ctx.close()
    return figures


_SMALL = {"lattice": E.lattice, "outside-on-bound": E.outside_and_on_bound, "thin-grids": E.thin_grids}


@pytest.mark.parametrize("stage", ["middle", "fine", "color"])
@pytest.mark.parametrize("name", list(_SMALL))
def test_edge_scene(name, stage, oracle32, oracle64):
    """lattice: zero direction components, samples on voxel planes, rays inside faces and along edges, every border voxel touched;
    outside-on-bound: origins outside / on the bound, misses, ground truth beyond the exit, the ray mask dropping the 0/0 rays;
    thin-grids: levels with dimensions of 1 and 2.  Sort modes 0 and 1, matmul modes 2 and 0."""
    check_scene(_SMALL[name](), stage, oracle32, oracle64)


def test_thin_grids_coarse_stage(oracle32, oracle64):
    """coarse level (32, 1, 2, 3): forward, map_step and render_backward on a level with a 1-voxel axis"""
    check_scene(E.thin_grids(), "coarse", oracle32, oracle64, sort_modes=(0, 1), matmul_modes=(2,))


def test_miss_rays_without_ground_truth(oracle32, oracle64):
    """gt_depth == NULL on rays that miss the bound: far < 0 is not clamped, z descends from 0.01 to far, every sample is outside (occupancy
    100) and the negative distances make alpha = 1 - exp(+100 |dist|) negative: ATen and the fp32 oracle render weights of 1e21, depths of -1e21 and
    var = inf, NaN on half of these rays (pinned to each other on the CPU).  The GPU must give the same non-finite entries ray by ray and agree on the
    finite ones; the backward (no ground truth, 32 samples) is compared on the rays whose every output is finite: the eight ordinary ones."""
    sc, ro, rd = E.misses_without_gt()
    e = dict(sc=sc, n_samples=32, n_surface=0)
    N, S = len(ro), 32
    with np.errstate(all="ignore"):
        ref = oracle32.render_forward(oracle32.opts(sc["bound"]), sc["grids"], sc["decoders"], "color", ro, rd, None)
    ctx = make_ctx(sc)
    rgb, depth, var, w = ctx.render_forward("color", cu(ro), cu(rd), None)
    got = dict(rgb=rgb.cpu().numpy(), depth=depth.cpu().numpy(), var=var.cpu().numpy(), weights=w.cpu().numpy())
    LP.compare_forward(got, ref, "misses without gt, forward")
    fin = np.isfinite(ref["depth"]) & np.isfinite(ref["var"]) & np.isfinite(ref["rgb"]).all(axis=1) & np.isfinite(ref["weights"]).all(axis=1)
    assert (~fin[:24]).all() and fin[-8:].all()          # every miss ray overflows somewhere (var = inf at the least); the eight ordinary rays render
    rays = dict(rays_o=ro[fin], rays_d=rd[fin], gt_depth=None)
    n = int(fin.sum())
    rng = np.random.default_rng(3)
    g_c, g_d, g_v = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    g_ro, g_rd = ctx.render_backward("color", cu(rays["rays_o"]), cu(rays["rays_d"]), None, -1.0, cu(g_c), cu(g_d), cu(g_v), flags=5)
    levels = stage_levels("color")
    hip = dict(g_grids={k: ctx.grid_download(k, grad=True) for k in levels}, g_rays_o=g_ro.cpu().numpy(), g_rays_d=g_rd.cpu().numpy())
    bits = {k: ctx.debug_relu_bits(k, n * S) for k in levels}
    sig_on = _sigma(ctx, "color", n * S) > 0
    r32, r64 = _references(oracle32, oracle64, e, rays, "color", -1.0, g_c, g_d, g_v, bits, sig_on, False)
    LP.compare_backward(hip, r32, r64, levels, "misses without gt, render_backward")
    ctx.close()


def test_one_cell_takes_the_cell_sort(oracle32, oracle64):
    """4096 rays x 48 samples in a 2 x 2 x 2 fine level: one run per tile, one key in k_sample's table; the automatic sort mode must pick the cell
    sort (>= 4 samples per cell); per-voxel check on the 8 voxels"""
    prof = {}
    check_scene(E.one_cell(4096), "fine", oracle32, oracle64, sort_modes=(-1,), matmul_modes=(2,), render_backward=False, profile=prof)
    print("one-cell: launches", {k: v[0] for k, v in prof.items()})
    assert prof.get("cell_sort", (0, 0.0))[0] >= 1, prof


def test_max_spread_fills_the_cell_table(oracle32, oracle64):
    """a k_sample workgroup (8 rays x 48 samples) meets > 300 distinct fine cells (asserted on the CPU: tests/test_local_parity_cpu.py): table
    probing and the one-add-per-thread path, cell sort forced and automatic"""
    check_scene(E.max_spread(), "fine", oracle32, oracle64, sort_modes=(1, -1), matmul_modes=(2,), render_backward=False)


def test_principal_point_rays_through_the_product_path(oracle32, oracle64):
    """identity pose, integer cx, cy: the principal-point row and column give directions with exact zeros (equal to the oracle's), through
    nsk_rays_from_pixels and nsk_rays_from_camera; nsk_inside_filter, a render and a Tracker step with forced branches on them"""
    pi, pj, intr, c2w = E.principal_point()
    e = E.outside_and_on_bound()
    sc = e["sc"]
    ctx = make_ctx(sc)
    o_ro, o_rd = oracle32.rays_from_pixels(pi, pj, *intr, c2w, 0)
    ro, rd = ctx.rays_from_pixels(cu(pi, torch.int32), cu(pj, torch.int32), intr, cu(c2w[:3]))
    cam = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
    ro2, rd2 = ctx.rays_from_camera(cu(pi, torch.int32), cu(pj, torch.int32), intr, cu(cam))
    for a, b in ((ro, o_ro), (rd, o_rd), (ro2, o_ro), (rd2, o_rd)):
        assert (a.cpu().numpy().view(np.uint32) == b.view(np.uint32)).all()                 # bit-equal, the sign of a zero component included
    # ---- the same through nsk_prepare_rays: a window one row (j = cy) / one column (i = cx) wide, so that every drawn pixel lies on it --------
    H, W = 480, 640
    rng = np.random.default_rng(2)
    frame = dict(depth=cu(rng.uniform(0.5, 6.0, (H, W)).astype(np.float32)), color=cu(rng.random((H, W, 3)).astype(np.float32)), pose=cu(cam), seed=77)
    for win, axis in (((int(intr[3]), int(intr[3]) + 1, 20, W - 20), 1), ((20, H - 20, int(intr[2]), int(intr[2]) + 1), 0)):
        for pose in (cu(cam), cu(np.ascontiguousarray(c2w[:3].reshape(-1)))):
            pr = ctx.prepare_rays([dict(frame, pose=pose)], 256, win, intr)
            ctx.sync()
            ppi, ppj = pr["pix_i"].cpu().numpy(), pr["pix_j"].cpu().numpy()
            assert (ppj == int(intr[3])).all() if axis == 1 else (ppi == int(intr[2])).all()
            p_ro, p_rd = oracle32.rays_from_pixels(ppi, ppj, *intr, c2w, 0)
            assert (pr["rays_d"].cpu().numpy().view(np.uint32) == p_rd.view(np.uint32)).all() and (pr["rays_o"].cpu().numpy() == p_ro).all()
            assert (pr["rays_d"].cpu().numpy()[:, axis] == 0).all()
            gdp = pr["gt_depth"].cpu().numpy()
            assert (pr["keep"].cpu().numpy().astype(bool) == oracle32.inside_filter(sc["bound"], p_ro, p_rd, gdp)).all()
            assert 0 < pr["keep"].sum() < 256
    rdn = rd.cpu().numpy()
    assert (rdn[pi == int(intr[2]), 0] == 0).all() and (rdn[pj == int(intr[3]), 1] == 0).all()
    ex = E._exit(sc["bound"], o_ro, o_rd)
    gt = (ex * np.where(np.arange(len(ex)) % 7 == 0, 1.3, 0.7)).astype(np.float32)          # every seventh beyond the exit: the filter drops it
    keep = ctx.inside_filter(ro, rd, cu(gt)).cpu().numpy()
    assert (keep == oracle32.inside_filter(sc["bound"], o_ro, o_rd, gt)).all() and (~keep).sum() >= 10
    n = 200
    rays = dict(rays_o=o_ro[keep][:n], rays_d=o_rd[keep][:n], gt_depth=gt[keep][:n])
    hit = rays["rays_o"] + rays["rays_d"] * rays["gt_depth"][:, None]
    rays["gt_color"] = (0.5 + 0.5 * np.sin(hit * np.array([1.3, 2.1, 0.7]) + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
    e2 = dict(e, name="principal-point", rays=rays, made_nonfinite=np.zeros(n, bool))
    check_scene(e2, "color", oracle32, oracle64, sort_modes=(0,), matmul_modes=(2,))
    # ---- one Tracker step (no dynamic mask, variance detached) and the pose gradient against the fp64 chain ----------------------------
    S, M = 48, n * 48
    gmax = float(rays["gt_depth"].max())
    loss_t = torch.zeros(1, device="cuda")
    g_rays = (torch.zeros(n, 3, device="cuda"), torch.zeros(n, 3, device="cuda"))
    dro, drd = cu(rays["rays_o"]), cu(rays["rays_d"])
    ctx.track_step("color", dro, drd, cu(rays["gt_depth"]), cu(rays["gt_color"]), gmax, W_COLOR, True, False, True, flags=4, loss=loss_t, g_rays=g_rays)
    bits = {k: ctx.debug_relu_bits(k, M) for k in ("middle", "fine", "color")}
    sig_on = _sigma(ctx, "color", M) > 0
    rgb, depth, var, _ = ctx.render_forward("color", dro, drd, cu(rays["gt_depth"]), gmax)
    _, g_d, g_c, g_v = oracle64.loss_track(depth.cpu().numpy(), rgb.cpu().numpy(), var.cpu().numpy(), rays["gt_depth"], rays["gt_color"], W_COLOR, True, False, True)
    r32, r64 = _references(oracle32, oracle64, e2, rays, "color", gmax, g_c, g_d, None, bits, sig_on, False)
    hip = dict(g_rays_o=g_rays[0].cpu().numpy(), g_rays_d=g_rays[1].cpu().numpy())
    LP.compare_backward(hip, r32, r64, [], "principal-point track_step", decoders=[])
    pi_k, pj_k = pi[keep][:n], pj[keep][:n]
    g_c2w = ctx.rays_backward(cu(pi_k, torch.int32), cu(pj_k, torch.int32), intr, g_rays[0], g_rays[1])
    g_cam = ctx.camera_backward(cu(cam), g_c2w).cpu().numpy()
    ref = oracle64.camera_backward(cam, oracle64.rays_backward(pi_k, pj_k, *intr, r64["g_rays_o"], r64["g_rays_d"]))
    err = np.abs(g_cam - ref).max() / np.abs(ref).max()
    print("principal-point track_step: pose gradient off by %.2e of its largest component" % err)
    assert err < LP.RAY_TOL
    ctx.close()

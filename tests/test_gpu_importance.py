"""GPU tests (-m gpu) of hierarchical importance sampling (include/nsk.h: nsk_set_importance, nsk_importance_resample): the resampling launch
against the numpy restatement of the rule (tests/importance_checks.py) to the bit, the fused two-pass path against its parts and against
the reference's op sequence on ATen-CPU (oracle/torch_ref.py), and what surrounds it: the cell sort, gradients, the switch, non-finite
maps, whole frames, the C++ Renderer and captured graphs.

Shapes: 37 rays (not a multiple of the 8 rays of a sampling workgroup), some with depth 0, on the small two-level scene;
(n_samples, n_surface, n_importance) = (32, 16, 16) (a full wave), (8, 5, 5), (3, 0, 1) (the minimum) and (32, 16, 16) without depths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import aten_chains as A
import importance_checks as IC
import scenes
from gpu_util import cu, make_ctx
from oracle import torch_ref as T
from scenes import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
N = 37
SHAPES = [(32, 16, 16, True), (8, 5, 5, True), (3, 0, 1, True), (32, 16, 16, False)]
IDS = ["32+16+16", "8+5+5", "3+0+1", "32+16-nogt"]
SEED = 5
_CACHE = {}


def same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _scene():
    if "sc" not in _CACHE:
        _CACHE["sc"] = scenes.make_scene(3, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    return _CACHE["sc"]


def _rays(n=N, seed=4):
    key = ("rays", n, seed)
    if key not in _CACHE:
        r = scenes.make_rays(seed, n, _scene()["bound"], n_frames=1, zero_frac=0.0)
        r["gt_depth"][::9] = 0.0                       # a depth vector with zeros in it
        _CACHE[key] = r
    return _CACHE[key]


def _dev(r, with_gt=True):
    return cu(r["rays_o"]), cu(r["rays_d"]), (cu(r["gt_depth"]) if with_gt else None), cu(r["gt_color"])


def _ctx(shape, ni=None, sc=None, **kw):
    ns, nsurf, Ni, _ = shape
    ctx = make_ctx(sc or _scene(), n_samples=ns, n_surface=nsurf, **kw)
    if ni is None:
        ni = Ni
    if ni:
        ctx.set_importance(ni)
    return ctx


def _first_pass(shape):
    """the one-pass rendering of the shape (n_importance = 0): z and weights [N, S1] as numpy, and the numpy restatement's z2 for both u"""
    if shape not in _CACHE:
        ns, nsurf, Ni, with_gt = shape
        S1 = ns + (nsurf if with_gt else 0)
        ro, rd, gd, _ = _dev(_rays(), with_gt)
        ctx = _ctx(shape, 0)
        _, _, _, w = ctx.render_forward("color", ro, rd, gd)
        ctx.sync()
        z = ctx.debug_fetch("z", N * S1).reshape(N, S1)
        ctx.close()
        w = w.cpu().numpy()
        assert np.isfinite(z).all() and np.isfinite(w).all() and (np.diff(z, axis=1) >= 0).all()
        _CACHE[shape] = dict(z=z, w=w, z2={det: IC.resample(z, w, Ni, det, SEED) for det in (True, False)})
    return _CACHE[shape]


# ---- 1. the resampling launch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [True, False], ids=["det", "hash"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_resampling_equals_the_restated_rule_to_the_bit(shape, det):
    f = _first_pass(shape)
    ctx = _ctx(shape, 0)
    z2 = ctx.importance_resample(cu(f["z"]), cu(f["w"]), shape[2], det=det, seed=SEED)
    ctx.sync()
    ctx.close()
    want = f["z2"][det]
    got = z2.cpu().numpy()
    assert got.shape == want.shape == (N, f["z"].shape[1] + shape[2])
    assert same(got, want), "worst |difference| %.3e in %d of %d depths" % (np.abs(got - want).max(), (got != want).sum(), got.size)
    assert not same(f["z2"][True], f["z2"][False])


# ---- 2. the fused path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_path_equals_its_parts(shape):
    """render_forward with n_importance set leaves the restated rule's z2 (bytes); its outputs agree within 1e-4 with the device's own
    eval_points + raw2outputs on that z2 (the single-decoder launches against the stage launch) and with oracle/torch_ref.py's on ATen-CPU"""
    ns, nsurf, Ni, with_gt = shape
    f = _first_pass(shape)
    S2 = f["z"].shape[1] + Ni
    sc, r = _scene(), _rays()
    ro, rd, gd, _ = _dev(r, with_gt)
    ctx = _ctx(shape)
    rgb, depth, var, w = ctx.render_forward("color", ro, rd, gd)
    ctx.sync()
    assert w.shape == (N, S2)
    zf = ctx.debug_fetch("z", N * S2).reshape(N, S2)
    assert same(zf, f["z2"][True])
    _, _, samples = ctx.last_call_stats()
    assert samples == N * (S2 + S2 - Ni)                # both passes are counted
    z2 = cu(zf)
    pts = (ro[:, None, :] + rd[:, None, :] * z2[:, :, None]).reshape(-1, 3).contiguous()
    parts = ctx.raw2outputs(ctx.eval_points("color", pts).view(N, S2, 4).contiguous(), z2, rd)
    ctx.sync()
    ctx.close()
    bound, grids, decs = A.torch_scene(sc)
    torch.set_num_threads(16)
    with torch.no_grad():
        tz = torch.tensor(zf)
        tp = torch.tensor(r["rays_o"])[:, None, :] + torch.tensor(r["rays_d"])[:, None, :] * tz[:, :, None]
        ref = T.raw2outputs_nerf_color(T.eval_points(tp.reshape(-1, 3), "color", decs, grids, bound).reshape(N, S2, 4), tz, False, torch.tensor(r["rays_d"]))
    for name, got, a, b in zip(("rgb", "depth", "var", "weights"), (rgb, depth, var, w), parts, ref):
        e_parts, e_ref = rel_l2(got.cpu().numpy(), a.cpu().numpy()), rel_l2(got.cpu().numpy(), b.numpy())
        print("%s %s: against the parts %.1e, against ATen %.1e" % (IDS[SHAPES.index(shape)], name, e_parts, e_ref))
        assert e_parts < TOL and e_ref < TOL, (name, e_parts, e_ref)


# ---- 3. the cell sort ----------------------------------------------------------------------------------------------------------------
def test_sorted_step_equals_unsorted_step():
    shape = SHAPES[0]
    ro, rd, gd, gc = _dev(_rays())
    out = {}
    for mode in (0, 1):
        ctx = _ctx(shape)
        ctx.set_sort_mode(mode)
        o = (torch.zeros(N, 3, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"))
        ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=1, outputs=o)
        ctx.sync()
        out[mode] = (o, {k: ctx.grid_download(k, grad=True) for k in ("middle", "fine", "color")})
        ctx.close()
    for a, b in zip(out[0][0], out[1][0]):
        assert same(a, b)
    for k in ("middle", "fine", "color"):
        assert np.abs(out[0][1][k]).max() > 0
        e = rel_l2(out[1][1][k], out[0][1][k])
        assert e < TOL, (k, e)


# ---- 4. gradients --------------------------------------------------------------------------------------------------------------------
def _aten_second_pass(sc, r, z2, leaves):
    """the second pass on ATen-CPU with the device's z2 as constants: points, eval_points, raw2outputs (oracle/torch_ref.py)"""
    bound, grids, decs = A.torch_scene(sc)
    t = {k: torch.tensor(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")}
    for k in leaves:
        if k in ("rays_o", "rays_d"):
            t[k].requires_grad_(True)
        elif k == "decoder":
            decs["color"].requires_grad_(True)
        else:
            grids[k].requires_grad_(True)
    tz = torch.tensor(z2)
    n, S2 = z2.shape
    pts = t["rays_o"][:, None, :] + t["rays_d"][:, None, :] * tz[:, :, None]
    raw = T.eval_points(pts.reshape(-1, 3), "color", decs, grids, bound).reshape(n, S2, 4)
    rgb, depth, var, _ = T.raw2outputs_nerf_color(raw, tz, False, t["rays_d"])
    return t, grids, decs, rgb, depth, var


def test_map_step_gradients_against_aten_autograd():
    """colour-stage map_step, 64 rays x (32 + 16 + 16), the colour decoder trainable: loss, grid and decoder gradients against ATen autograd
    through the second pass on the device's z2, 1e-4 relative L2"""
    sc, r = _scene(), _rays(64, 14)
    ro, rd, gd, gc = _dev(r)
    ctx = _ctx(SHAPES[0], trainable=["color"])
    loss = torch.zeros(1, device="cuda")
    ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss)
    ctx.sync()
    z2 = ctx.debug_fetch("z", 64 * 64).reshape(64, 64)
    got = {k: ctx.grid_download(k, grad=True) for k in ("middle", "fine", "color")}
    got["decoder"] = ctx.decoder_download("color", grad=True)
    ctx.close()
    torch.set_num_threads(16)
    t, grids, decs, rgb, depth, var = _aten_second_pass(sc, r, z2, ("middle", "fine", "color", "decoder"))
    ref_loss = T.loss_map(depth, rgb, t["gt_depth"], t["gt_color"], 0.5, True)
    ref_loss.backward()
    ref = {k: grids[k].grad[0].numpy() for k in ("middle", "fine", "color")}
    ref["decoder"] = decs["color"].grad.numpy()
    e_l = abs(float(loss) - float(ref_loss.detach())) / float(ref_loss.detach())
    errs = {k: rel_l2(got[k], ref[k]) for k in ref}
    print("map_step with n_importance = 16 against ATen autograd: loss %.1e, gradients %s" % (e_l, {k: "%.1e" % e for k, e in errs.items()}))
    assert e_l < 2e-5
    for k, e in errs.items():
        assert e < TOL, (k, e)


def test_track_step_ray_gradients_against_aten_autograd():
    """track_step with NSK_GRAD_RAYS, 64 rays x (32 + 16 + 16), the dynamic mask and the detached variance on: loss and d loss / d rays
    against ATen autograd through the second pass on the device's z2 (a constant, as upstream detaches it), 1e-4 relative L2"""
    sc, r = _scene(), _rays(64, 14)
    ro, rd, gd, gc = _dev(r)
    ctx = _ctx(SHAPES[0])
    loss = torch.zeros(1, device="cuda")
    g_ro, g_rd = torch.empty_like(ro), torch.empty_like(rd)
    ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, True, True, True, flags=4, loss=loss, g_rays=(g_ro, g_rd))
    ctx.sync()
    z2 = ctx.debug_fetch("z", 64 * 64).reshape(64, 64)
    ctx.close()
    torch.set_num_threads(16)
    t, _, _, rgb, depth, var = _aten_second_pass(sc, r, z2, ("rays_o", "rays_d"))
    ref_loss = T.loss_track(depth, rgb, var, t["gt_depth"], t["gt_color"], 0.5, True, True, True)
    ref_loss.backward()
    e_l = abs(float(loss) - float(ref_loss.detach())) / float(ref_loss.detach())
    e_o, e_d = rel_l2(g_ro.cpu().numpy(), t["rays_o"].grad.numpy()), rel_l2(g_rd.cpu().numpy(), t["rays_d"].grad.numpy())
    print("track_step with n_importance = 16 against ATen autograd: loss %.1e, d rays_o %.1e, d rays_d %.1e" % (e_l, e_o, e_d))
    assert e_l < 2e-5 and e_o < TOL and e_d < TOL, (e_l, e_o, e_d)


# ---- 5. the switch -------------------------------------------------------------------------------------------------------------------
def _forward_and_step(ctx, prepare=False):
    ro, rd, gd, gc = _dev(_rays())
    fwd = ctx.render_forward("color", ro, rd, gd)
    o = (torch.zeros(N, 3, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"))
    loss = torch.zeros(1, device="cuda")
    if prepare:
        ctx.map_prepare("color", ro, rd, gd, -1.0, flags=3)
    ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss, outputs=o)
    ctx.sync()
    g = [ctx.grid_download(k, grad=True) for k in ("middle", "fine", "color")] + [ctx.decoder_download("color", grad=True)]
    return [t.cpu().numpy() for t in fwd] + [t.cpu().numpy() for t in o] + [loss.cpu().numpy()] + g


def test_off_means_off():
    """set_importance(16) (and a rendering with it) followed by set_importance(0) gives the bytes of a context that never set it: the
    forward, a map_step's outputs, loss and gradients in the deterministic mode"""
    shape = SHAPES[0]
    ctx = _ctx(shape, 0, trainable=["color"])
    ctx.set_tuning("deterministic", 1)
    want = _forward_and_step(ctx)
    ctx.close()
    ctx = _ctx(shape, 16, trainable=["color"])
    ctx.set_tuning("deterministic", 1)
    with_it = _forward_and_step(ctx)
    ctx.zero_grads()
    ctx.set_importance(0)
    got = _forward_and_step(ctx)
    ctx.close()
    assert with_it[3].shape == (N, 64) and not same(with_it[1], want[1])
    assert len(got) == len(want) == 12
    for i, (a, b) in enumerate(zip(got, want)):
        assert same(a, b), i


def test_prepare_registers_nothing_with_importance():
    """map_prepare with n_importance > 0 succeeds and registers nothing: the step after it has the bytes of the step alone"""
    out = []
    for prepare in (False, True):
        ctx = _ctx(SHAPES[0], trainable=["color"])
        ctx.set_tuning("deterministic", 1)
        out.append(_forward_and_step(ctx, prepare))
        ctx.close()
    for i, (a, b) in enumerate(zip(out[1], out[0])):
        assert same(a, b), i


def test_refusals():
    import nice_slam_cpp_amd as pkg
    ctx = make_ctx(_scene())
    for bad, word in ((-1, ">= 0"), (17, "<= 64")):
        with pytest.raises(pkg.NskError, match=word):
            ctx.set_importance(bad)
    ctx.set_importance(16)
    with pytest.raises(pkg.NskError, match="<= 64"):
        ctx.set_render_opts(n_samples=33, n_surface=16)
    with pytest.raises(pkg.NskError, match="n_samples >= 3"):
        ctx.set_render_opts(n_samples=2, n_surface=16)
    ctx.set_render_opts(n_samples=32, n_surface=16)
    ctx.set_importance(0)
    ctx.set_render_opts(n_samples=2, n_surface=0)
    with pytest.raises(pkg.NskError, match="n_samples >= 3"):
        ctx.set_importance(1)
    z = torch.zeros(4, 2, device="cuda")
    with pytest.raises(pkg.NskError, match="S >= 3"):
        ctx.importance_resample(z, z, 1)
    z = torch.zeros(4, 60, device="cuda")
    with pytest.raises(pkg.NskError, match="<= 64"):
        ctx.importance_resample(z, z, 5)
    # the output may not overlap an input (the strides differ): refused before any launch
    L, P = pkg.nsk.lib(), (lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off))
    buf, w = torch.zeros(4 * 12 + 4 * 8, device="cuda"), torch.zeros(4, 8, device="cuda")
    for zin, win, zout, word in ((P(buf), P(w), P(buf), "d_z"), (P(w), P(buf, 40), P(buf), "d_weights"), (P(buf, 47), P(w), P(buf), "d_z")):
        assert L.nsk_importance_resample(ctx.h, 4, 8, zin, win, 4, 1, C.c_uint64(0), zout) != 0
        assert ("d_z_out overlaps " + word).encode() in L.nsk_last_error()
    assert L.nsk_importance_resample(ctx.h, 4, 8, P(buf, 48), P(w), 4, 1, C.c_uint64(0), P(buf)) == 0       # adjacent is not overlapping
    ctx.set_render_opts(n_samples=32, n_surface=16)
    assert ctx.get_importance() == 0
    ctx.set_importance(7)
    assert ctx.get_importance() == 7
    ctx.close()


# ---- 6. non-finite maps --------------------------------------------------------------------------------------------------------------
def test_nan_voxel_stays_with_its_rays():
    """one middle-level voxel set to NaN: the rays whose first-pass weights are NaN render non-finite, every other ray has the bytes it has
    in a batch without those rays, and the call succeeds"""
    shape = SHAPES[0]
    sc0, r = _scene(), _rays()
    f = _first_pass(shape)
    p = r["rays_o"][1] + r["rays_d"][1] * f["z"][1, 20]
    b = sc0["bound"]
    dims = np.array(sc0["grids"]["middle"].shape[1:][::-1])          # X, Y, Z
    ix, iy, iz = np.clip(np.round((p - b[:, 0]) / (b[:, 1] - b[:, 0]) * (dims - 1)).astype(int), 0, dims - 1)
    sc = dict(bound=sc0["bound"], decoders=sc0["decoders"], grids={k: v.copy() for k, v in sc0["grids"].items()})
    sc["grids"]["middle"][:, iz, iy, ix] = np.nan
    gmax = float(r["gt_depth"].max())
    ro, rd, gd, _ = _dev(r)
    ctx = _ctx(shape, 0, sc=sc)
    w1 = ctx.render_forward("color", ro, rd, gd, gmax)[3].cpu().numpy()
    bad = ~np.isfinite(w1).all(1)
    assert bad[1] and 0 < bad.sum() < N, bad.sum()
    ctx.set_importance(16)
    full = [t.cpu().numpy() for t in ctx.render_forward("color", ro, rd, gd, gmax)]
    for n in np.flatnonzero(bad):
        assert not (np.isfinite(full[0][n]).all() and np.isfinite(full[1][n]) and np.isfinite(full[2][n])), n
    keep = torch.tensor(~bad, device="cuda")
    part = [t.cpu().numpy() for t in ctx.render_forward("color", ro[keep].contiguous(), rd[keep].contiguous(), gd[keep].contiguous(), gmax)]
    ctx.close()
    for a, b_ in zip(full, part):
        assert same(a[~bad], b_)


# ---- 7. whole frames and the C++ Renderer -----------------------------------------------------------------------------------------------
def test_render_image_equals_render_forward():
    sc = _scene()
    H, W, intr = 24, 40, (30.0, 30.0, 19.5, 11.5)
    c2w = scenes.make_camera(np.random.default_rng(7), sc["bound"])
    depth_img = cu(scenes.frame_depth_image(sc["bound"], c2w, H, W, *intr))
    pose = cu(np.ascontiguousarray(c2w[:3, :4]).reshape(12))
    ctx = _ctx(SHAPES[0])
    for dimg in (depth_img, None):
        rgb, depth, var = ctx.render_image("color", (H, W), intr, pose, dimg)
        ro, rd, gd = ctx.image_rays((H, W), intr, pose, dimg)
        want = ctx.render_forward("color", ro, rd, gd, want_weights=False)
        ctx.sync()
        assert same(rgb.view(-1, 3), want[0]) and same(depth.view(-1), want[1]) and same(var.view(-1), want[2])
        assert bool(torch.isfinite(depth).all())
    ctx.close()


@pytest.mark.parametrize("with_gt", [True, False], ids=["gt", "nogt"])
def test_cpp_renderer_equals_the_python_context(with_gt, tmp_path):
    exe = os.path.join(HOST, "importance_test")
    if not os.path.exists(exe):
        pytest.fail("importance_test is not built (run __graft_entry__.build())")
    d, sc, r = str(tmp_path), _scene(), _rays()
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    np.save(os.path.join(d, "rays_o.npy"), r["rays_o"])
    np.save(os.path.join(d, "rays_d.npy"), r["rays_d"])
    if with_gt:
        np.save(os.path.join(d, "gt_depth.npy"), r["gt_depth"])
    run = subprocess.run([exe, d, "color", "16"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "importance_test ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    ro, rd, gd, _ = _dev(r, with_gt)
    ctx = _ctx(SHAPES[0])
    want = ctx.render_forward("color", ro, rd, gd)
    ctx.sync()
    ctx.close()
    for name, t in zip(("imp_rgb", "imp_depth", "imp_var", "imp_weights"), want):
        assert same(np.load(os.path.join(d, name + ".npy")), t), name




# ---- 8. captured graphs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two-replays", "sorted-one-replay"])
def test_graph_replay_matches_eager_steps_with_importance(form):
    """A captured map_step + adam_step with n_importance = 16 against eager steps, within the tolerances of
    tests/test_gpu_parity.py::test_graph_replay_matches_eager_steps (1e-5 on the optimised grids and decoder, 1e-4 on the loss).

    two-replays: one eager step, then two replays against two eager steps, in the deterministic mode, where they agree exactly (measured 0).
    Outside it no two runs of the EAGER steps agree within 1e-5 on this scene: measured eager against eager after two steps 7e-5 / 1.2e-3 /
    1.7e-4 (middle / fine / colour grid), against 3e-8 with n_importance = 0.  The atomic adds' order moves the first step's map by ~1e-8,
    and upstream's rule is ill-conditioned where the cdf is flat: a bin of weight ~0 has pdf ~1e-5, so the inverse cdf has a slope of
    bin width / 1e-5 there, and the last u = 1 either meets a cdf that ends at or an ulp below 1 (bins[S1-2] exactly) or one that ends an ulp
    above (t = (1 - cdf[S1-3]) / ~1e-5, its numerator a rounding residue): a depth moves by ~1e-3 of a bin and the second step's gradients follow.
    sorted-one-replay: the launches the deterministic mode does not have (the cell sort's keys from the resampling, the parallel backward):
    both contexts come to the compared step with identical maps (the first eager step has no optimiser step), one replay against one eager step."""
    sc = scenes.make_scene(23, scenes.SMALL_GRID_SHAPES, grid_std=0.05, bias_std=0.1)
    rays = scenes.make_rays(24, 300, sc["bound"], n_frames=2)
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    lr = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]
    two = form == "two-replays"
    out = {}
    for mode in ("eager", "graph"):
        ctx = _ctx(SHAPES[0], sc=sc, trainable=["color"])
        if two:
            ctx.set_tuning("deterministic", 1)
        else:
            ctx.set_sort_mode(1)
        loss = torch.zeros(1, device="cuda")
        with torch.cuda.stream(ctx.tstream):
            def step():
                ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, loss=loss)
                ctx.adam_step(lr)
            if two:
                step()                               # step 1 eagerly in both (sizes the workspaces)
            else:
                ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, loss=loss)      # sizes the workspaces, moves nothing
                ctx.zero_grads()
            if mode == "eager":
                for _ in range(2 if two else 1):
                    step()
            else:
                ctx.graph_begin(); step(); gid = ctx.graph_end()
                for _ in range(2 if two else 1):
                    ctx.graph_launch(gid)
                ctx.graph_destroy(gid)
        ctx.sync()
        out[mode] = ({k: ctx.grid_download(k) for k in ("middle", "fine", "color")}, ctx.decoder_download("color"), float(loss))
        ctx.close()
    errs = {k: rel_l2(out["graph"][0][k], out["eager"][0][k]) for k in ("middle", "fine", "color")}
    errs["decoder"] = rel_l2(out["graph"][1], out["eager"][1])
    print("graph against eager, %s: %s, loss %.6f / %.6f" % (form, {k: "%.1e" % e for k, e in errs.items()}, out["graph"][2], out["eager"][2]))
    for k in ("middle", "fine", "color"):
        assert np.abs(out["eager"][0][k] - sc["grids"][k]).max() > 1e-3
    for k, e in errs.items():
        assert e < 1e-5, (k, e)
    assert abs(out["graph"][2] - out["eager"][2]) < 1e-4 * abs(out["eager"][2])


def test_first_eager_step_renders_the_same_bytes_twice():
    """What the docstring above rests on: outside the deterministic mode two eager runs start to differ only behind the first optimiser step
    (the order of the gradients' atomic adds).  Before it nothing is order-dependent: the first map_step of two contexts on the graph test's
    scene renders identical bytes, first pass, resampling and second pass included."""
    sc = scenes.make_scene(23, scenes.SMALL_GRID_SHAPES, grid_std=0.05, bias_std=0.1)
    rays = scenes.make_rays(24, 300, sc["bound"], n_frames=2)
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    out = []
    for _ in range(2):
        ctx = _ctx(SHAPES[0], sc=sc, trainable=["color"])
        o = (torch.zeros(300, 3, device="cuda"), torch.zeros(300, device="cuda"), torch.zeros(300, device="cuda"))
        with torch.cuda.stream(ctx.tstream):
            ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, outputs=o)
        ctx.sync()
        out.append(o)
        ctx.close()
    assert bool(torch.isfinite(out[0][1]).all()) and float(out[0][1].abs().max()) > 0
    for a, b in zip(out[0], out[1]):
        assert same(a, b)

"""GPU tests of whole-frame rendering (nsk_image_rays, nsk_render_image, nsk_image_metrics, Renderer::render_img) on the 24 x 32 frame of
tests/image_views.py: rays against the explicit-index entry points, chunks against nsk_render_forward on the same rays (bytes) and against
the fp32 oracle (1e-4 relative L2), the two gt_depth_max semantics, the relation to other context state, the metrics, the errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import image_views as iv
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
TOL = 1e-4                                   # the project's contract (include/nsk.h)
WINDOW, WSTRIDE = (3, 22, 5, 30), 2          # odd extents: 19 x 25 pixels, every second one -> a 10 x 13 view
CAM7 = np.array([0.9, 0.1, -0.3, 0.2, 0.4, -0.2, 0.3], np.float32)      # an unnormalised quaternion + translation


def same(a, b):
    return a.contiguous().cpu().numpy().tobytes() == b.contiguous().cpu().numpy().tobytes()


class Env:
    def __init__(self):
        self.fr = iv.make_frame()
        self.sc = self.fr["scene"]
        self.ctx = make_ctx(self.sc)
        self.c2w = cu(self.fr["c2w"])
        self.depth = cu(self.fr["depth"])
        self.color = cu(self.fr["color"])
        self.ro, self.rd, self.gd = self.ctx.image_rays((iv.H, iv.W), iv.INTR, self.c2w, self.depth)
        self._fwd, self._img = {}, {}

    def forward_chunks(self, stage, with_depth, chunk, gtmax=-1.0):
        """nsk_render_forward over the chunks of the frame's rays, concatenated (computed once per case)"""
        key = (stage, with_depth, min(chunk, 768), gtmax)
        if key not in self._fwd:
            parts = [self.ctx.render_forward(stage, self.ro[a:a + n].contiguous(), self.rd[a:a + n].contiguous(),
                                             self.gd[a:a + n].contiguous() if with_depth else None, gtmax, want_weights=False)[:3]
                     for a, n in iv.chunk_ranges(768, chunk)]
            self._fwd[key] = tuple(torch.cat([p[k] for p in parts]) for k in range(3))
        return self._fwd[key]

    def image(self, stage, with_depth, chunk, gtmax=-1.0):
        return self.ctx.render_image(stage, (iv.H, iv.W), iv.INTR, self.c2w, self.depth if with_depth else None, gt_depth_max=gtmax, chunk_rays=chunk)


@pytest.fixture(scope="module")
def env():
    return Env()


@pytest.fixture(scope="module")
def oracle_images(oracle32):
    """the fp32 oracle's render of the frame, chunk by chunk, once per (stage, depth image, chunk, maximum)"""
    fr = iv.make_frame()
    ro, rd, gd = iv.frame_rays(oracle32, fr)
    cache = {}

    def get(stage, with_depth, chunk, gtmax=-1.0):
        key = (stage, with_depth, min(chunk, 768), gtmax)
        if key not in cache:
            cache[key] = iv.oracle_render(oracle32, fr["scene"], stage, ro, rd, gd if with_depth else None, chunk, gtmax)
        return cache[key]
    return get


# ---- 1. rays -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("view", ["full", "window"])
def test_image_rays_equal_the_explicit_index_entry_points(env, view, mode):
    ctx = env.ctx
    window, stride = (None, 1) if view == "full" else (WINDOW, WSTRIDE)
    pi, pj = iv.view_pixels(iv.H, iv.W, window, stride)
    total = pi.size
    assert total == (768 if view == "full" else 130)
    dpi, dpj = cu(pi, torch.int32), cu(pj, torch.int32)
    cam = cu(CAM7)
    ro_p, rd_p = ctx.rays_from_pixels(dpi, dpj, iv.INTR, env.c2w, mode)
    ro_c, rd_c = ctx.rays_from_camera(dpi, dpj, iv.INTR, cam, mode)
    gd_p, _ = ctx.gather_pixels(dpi, dpj, env.depth)
    assert not same(rd_p, rd_c) and float(gd_p.max()) > 0 and int((gd_p == 0).sum()) > 0
    ranges = [(0, 768), (200, 200), (600, 168), (767, 1)] if view == "full" else [(0, 130), (50, 37), (129, 1)]
    for first, n in ranges:
        ro, rd, gd = ctx.image_rays((iv.H, iv.W), iv.INTR, env.c2w, env.depth, window, stride, first, n, mode)
        assert ro.shape == (n, 3) and gd.shape == (n,)
        assert same(ro, ro_p[first:first + n]) and same(rd, rd_p[first:first + n]) and same(gd, gd_p[first:first + n]), (view, mode, first, n, "c2w")
        ro, rd, gd = ctx.image_rays((iv.H, iv.W), iv.INTR, cam, None, window, stride, first, n, mode)
        assert gd is None and same(ro, ro_c[first:first + n]) and same(rd, rd_c[first:first + n]), (view, mode, first, n, "cam7")
    if mode == 0 and view == "full":                  # D10: intrinsics truncated to integers (mode bit 1)
        intr = (30.7, 29.2, 15.5, 11.5)
        a = ctx.rays_from_pixels(dpi, dpj, intr, env.c2w, 2)[1]
        b = ctx.image_rays((iv.H, iv.W), intr, env.c2w, None, mode=2)[1]
        assert same(a, b) and not same(a, ctx.rays_from_pixels(dpi, dpj, intr, env.c2w, 0)[1])


# ---- 2. chunks are batches --------------------------------------------------------------------------------------------
def test_render_forward_is_reproducible(env):
    """the premise of every byte comparison below: two nsk_render_forward calls on one chunk give equal bytes"""
    a, n = 200, 200
    args = ("color", env.ro[a:a + n].contiguous(), env.rd[a:a + n].contiguous(), env.gd[a:a + n].contiguous())
    x = env.ctx.render_forward(*args, want_weights=False)
    y = env.ctx.render_forward(*args, want_weights=False)
    assert all(same(x[k], y[k]) for k in range(3))


@pytest.mark.parametrize("chunk", iv.CHUNKS)
@pytest.mark.parametrize("case", ["color", "color_nodepth", "fine"])
def test_chunks_equal_render_forward_on_the_same_rays(env, case, chunk):
    stage, with_depth = case.split("_")[0], not case.endswith("nodepth")
    rgb, depth, var = env.image(stage, with_depth, chunk)
    assert rgb.shape == (iv.H, iv.W, 3) and depth.shape == (iv.H, iv.W) and var.shape == (iv.H, iv.W)
    w_rgb, w_depth, w_var = env.forward_chunks(stage, with_depth, chunk)
    assert same(rgb.reshape(-1, 3), w_rgb) and same(depth.reshape(-1), w_depth) and same(var.reshape(-1), w_var)
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(rgb).all())


def test_window_and_stride_render_the_view(env):
    """a strided window, a 7-vector pose and a ragged chunk at once: the bytes of nsk_render_forward on the view's rays"""
    ctx = env.ctx
    cam = cu(np.concatenate([[1.0, 0.02, -0.05, 0.01], env.fr["c2w"][:, 3]]).astype(np.float32))
    ro, rd, gd = ctx.image_rays((iv.H, iv.W), iv.INTR, cam, env.depth, WINDOW, WSTRIDE)
    rgb, depth, var = ctx.render_image("color", (iv.H, iv.W), iv.INTR, cam, env.depth, WINDOW, WSTRIDE, chunk_rays=50)
    assert depth.shape == (10, 13)
    for a, n in iv.chunk_ranges(130, 50):
        w = ctx.render_forward("color", ro[a:a + n].contiguous(), rd[a:a + n].contiguous(), gd[a:a + n].contiguous(), want_weights=False)
        assert same(rgb.reshape(-1, 3)[a:a + n], w[0]) and same(depth.reshape(-1)[a:a + n], w[1]) and same(var.reshape(-1)[a:a + n], w[2])


# ---- 3. oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", iv.CHUNKS)
@pytest.mark.parametrize("case", ["color", "color_nodepth", "fine"])
def test_images_match_the_oracle_chunk_by_chunk(env, oracle_images, case, chunk):
    stage, with_depth = case.split("_")[0], not case.endswith("nodepth")
    rgb, depth, var = env.image(stage, with_depth, chunk)
    ref = oracle_images(stage, with_depth, chunk)
    e_d = scenes.rel_l2(depth.cpu().numpy(), ref["depth"])
    e_v = scenes.rel_l2(var.cpu().numpy(), ref["var"])
    e_c = scenes.rel_l2(rgb.cpu().numpy(), ref["rgb"]) if stage == "color" else 0.0
    print("%s chunk %d: rel-L2 depth %.2e, colour %.2e, variance %.2e" % (case, chunk, e_d, e_c, e_v))
    assert e_d < TOL and e_c < TOL and e_v < TOL, (e_d, e_c, e_v)


# ---- 4. global maximum ---------------------------------------------------------------------------------------------------
def test_global_maximum_makes_the_frame_independent_of_the_chunking(env, oracle_images):
    gmax = float(env.fr["depth"].max())
    a = env.image("color", True, 200, gmax)
    b = env.image("color", True, 768, gmax)
    ref = oracle_images("color", True, 768, gmax)
    for k, name in enumerate(("rgb", "depth", "var")):
        e_ab = scenes.rel_l2(a[k].cpu().numpy(), b[k].cpu().numpy())
        e_a, e_b = scenes.rel_l2(a[k].cpu().numpy(), ref[name]), scenes.rel_l2(b[k].cpu().numpy(), ref[name])
        print("global maximum, %s: chunks of 200 against 768 rel-L2 %.2e (bit-equal: %s), against the oracle %.2e / %.2e" % (name, e_ab, same(a[k], b[k]), e_a, e_b))
        assert e_ab < TOL and e_a < TOL and e_b < TOL
    per_chunk = env.image("color", True, 200)
    e = scenes.rel_l2(per_chunk[1].cpu().numpy(), a[1].cpu().numpy())
    print("per-chunk maxima against the global maximum: depth rel-L2 %.3e" % e)
    assert e >= 1e-3, e


# ---- 5. context state -------------------------------------------------------------------------------------------------------
def test_render_ignores_ray_mask_and_depth_max_batch(env):
    ctx = env.ctx
    want = env.forward_chunks("color", True, 200)
    keep = cu((np.arange(768) % 2).astype(np.uint8), torch.uint8)
    huge = cu(np.array([1.0e6, 1.0, 2.0, 3.0], np.float32))
    ctx.set_ray_mask(keep)
    ctx.set_depth_max_batch(huge)
    try:
        rgb, depth, var = env.image("color", True, 200)
    finally:
        ctx.set_ray_mask(None)
        ctx.set_depth_max_batch(None)
    assert same(rgb.reshape(-1, 3), want[0]) and same(depth.reshape(-1), want[1]) and same(var.reshape(-1), want[2])


@pytest.mark.parametrize("ride", [False, True])
def test_render_leaves_a_prepared_batch_intact(env, ride):
    """map_prepare -> render_image -> map_step gives the loss and outputs of map_prepare -> map_step, to the bit.  ride: another batch's
    step runs after the registration and carries the registered batch's sampling in its launches, so the render meets a batch that is
    already sampled into the workspace's second set (without: one that is only registered)"""
    ctx = env.ctx
    rays = [scenes.make_rays(s, 256, env.sc["bound"]) for s in (21, 22)]
    dev = [{k: cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")} for r in rays]
    env.image("color", True, 200)                       # the workspace has its size before anything is registered

    def run(render):
        ctx.zero_grads()
        out = (torch.zeros(256, 3, device="cuda"), torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda"))
        loss = torch.zeros(1, device="cuda")
        b0, b1 = dev
        ctx.map_prepare("color", b1["rays_o"], b1["rays_d"], b1["gt_depth"], -1.0, flags=1)
        if ride:
            ctx.map_step("color", b0["rays_o"], b0["rays_d"], b0["gt_depth"], b0["gt_color"], -1.0, 0.2, True, flags=1)
        img = env.image("color", True, 200) if render else None
        ctx.map_step("color", b1["rays_o"], b1["rays_d"], b1["gt_depth"], b1["gt_color"], -1.0, 0.2, True, flags=1, loss=loss, outputs=out)
        ctx.sync()
        return loss, out, img
    l0, o0, _ = run(False)
    l1, o1, img = run(True)
    assert float(l0) > 0 and same(l0, l1) and all(same(o0[k], o1[k]) for k in range(3))
    want = env.forward_chunks("color", True, 200)
    assert same(img[1].reshape(-1), want[1]) and same(img[0].reshape(-1, 3), want[0])
    ctx.zero_grads()


# ---- 6. metrics ---------------------------------------------------------------------------------------------------------------
def check_metrics(ctx, rgb, depth, gt_d, gt_c, residual_bytes=True, tol=1e-12):
    m = ctx.image_metrics(rgb, depth, gt_d, gt_c, want_residuals=True)
    h, rd, rc = iv.metrics_ref(rgb.cpu().numpy(), depth.cpu().numpy(), None if gt_d is None else gt_d.cpu().numpy(), None if gt_c is None else gt_c.cpu().numpy())
    got = np.array(m["h_out"])
    print("metrics %s: device %s, numpy %s" % (tuple(depth.shape), got[:6], h[:6]))
    for k in (0, 1, 3, 5, 6, 7):
        assert got[k] == h[k], (k, got, h)                      # counts are exact
    for k in (2, 4):                                            # the same fp32 terms added in fp64 in another order: at most n 2^-53 relative
        assert abs(got[k] - h[k]) <= tol * abs(h[k]), (k, got[k], h[k])
    if residual_bytes:
        assert (rd is None and m["res_depth"] is None) or m["res_depth"].cpu().numpy().tobytes() == rd.reshape(depth.shape).tobytes()
        assert (rc is None and m["res_color"] is None) or m["res_color"].cpu().numpy().tobytes() == rc.reshape(rgb.shape).tobytes()
    m2 = ctx.image_metrics(rgb, depth, gt_d, gt_c)
    assert np.array(m2["h_out"]).tobytes() == got.tobytes()     # two runs, the same bytes
    return m, h


def test_metrics_of_the_rendered_frame(env):
    ctx = env.ctx
    rgb, depth, var = env.image("color", True, 200)
    m, h = check_metrics(ctx, rgb, depth, env.depth, env.color)
    assert m["pixels"] == 768 and m["nonfinite"] == 0 and 0 < m["depth_pixels"] == int((env.fr["depth"] > 0).sum()) and m["color_terms"] == 3 * 768
    assert m["depth_l1"] == m["depth_sum"] / m["depth_pixels"] and abs(m["psnr"] - iv.psnr(h)) < 1e-9
    print("rendered frame against the input frame: depth L1 %.4f, PSNR %.2f dB" % (m["depth_l1"], m["psnr"]))
    # ground truth absent: the corresponding sums and counts are zero
    m, _ = check_metrics(ctx, rgb, depth, None, env.color)
    assert m["depth_pixels"] == 0 and m["depth_sum"] == 0 and m["depth_l1"] is None and m["res_depth"] is None and m["color_terms"] == 3 * 768
    m, _ = check_metrics(ctx, rgb, depth, env.depth, None)
    assert m["color_terms"] == 0 and m["color_sum"] == 0 and m["psnr"] is None and m["res_color"] is None and m["depth_pixels"] > 0
    # a NaN pixel and a +inf pixel are left out of every sum and counted
    rgb2, depth2 = rgb.clone(), depth.clone()
    depth2[5, 7] = float("nan")
    rgb2[17, 3, 1] = float("inf")
    m, _ = check_metrics(ctx, rgb2, depth2, env.depth, env.color, residual_bytes=False)
    assert m["nonfinite"] == 2 and np.isfinite(m["h_out"]).all() and m["color_terms"] == 3 * 766
    assert bool(torch.isnan(m["res_depth"][5, 7])) or float(env.depth[5, 7]) == 0.0


def test_metrics_beyond_one_pass_of_the_grid(env):
    """more pixels than the 1024 workgroups cover in one pass (262144): threads walk several pixels; odd sizes, zero depths, non-finite values"""
    rng = np.random.default_rng(9)
    Hh, Ww = 521, 517
    depth = rng.uniform(0.5, 4.0, (Hh, Ww)).astype(np.float32)
    gt = (depth + rng.normal(0, 0.1, (Hh, Ww))).astype(np.float32)
    gt[rng.random((Hh, Ww)) < 0.07] = 0.0
    rgb = rng.random((Hh, Ww, 3)).astype(np.float32)
    gc = rng.random((Hh, Ww, 3)).astype(np.float32)
    depth[rng.random((Hh, Ww)) < 0.001] = np.inf
    rgb[rng.random((Hh, Ww, 3)) < 0.0005] = -np.inf
    assert Hh * Ww > 1024 * 256
    # n non-negative terms added in fp64 in two different orders: each sum is within (n - 1) 2^-53 relative of the exact one
    m, h = check_metrics(env.ctx, cu(rgb), cu(depth), cu(gt), cu(gc), residual_bytes=False, tol=2 * 3 * Hh * Ww * 2.0 ** -53)
    assert m["nonfinite"] > 100 and m["depth_pixels"] > 200000
    fin = np.isfinite(depth)
    assert (m["res_depth"].cpu().numpy()[fin] == np.where(gt > 0, np.abs(gt - depth), 0).astype(np.float32)[fin]).all()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument_and_launch_nothing(env):
    import nice_slam_cpp_amd as pkg
    ctx = env.ctx
    ctx.sync()
    ctx.profile_begin()
    hw, intr = (iv.H, iv.W), iv.INTR
    for window, pat in (((0, 25, 0, 32), "H1"), ((0, 24, 5, 33), "W1"), ((-1, 24, 0, 32), "H0"), ((0, 24, 32, 32), "W0"), ((5, 5, 0, 32), "H0")):
        with pytest.raises(pkg.NskError, match=pat):
            ctx.render_image("color", hw, intr, env.c2w, env.depth, window=window)
        with pytest.raises(pkg.NskError, match=pat):
            ctx.image_rays(hw, intr, env.c2w, env.depth, window=window, n=1)
    with pytest.raises(pkg.NskError, match="stride"):
        ctx.render_image("color", hw, intr, env.c2w, env.depth, stride=0)
    with pytest.raises(pkg.NskError, match="stride"):
        ctx.image_rays(hw, intr, env.c2w, env.depth, stride=0, n=1)
    with pytest.raises(pkg.NskError, match="first, n"):
        ctx.image_rays(hw, intr, env.c2w, env.depth, first=700, n=69)
    S = 48
    largest = ((1 << 26) - 1) // S
    assert (largest + 1) * S >= 1 << 26 > largest * S
    with pytest.raises(pkg.NskError, match=r"chunk_rays.*\b%d\b" % largest):
        ctx.render_image("color", hw, intr, env.c2w, env.depth, chunk_rays=largest + 1)
    with pytest.raises(pkg.NskError, match=r"chunk_rays.*\b%d\b" % (((1 << 26) - 1) // 32)):
        ctx.render_image("color", hw, intr, env.c2w, None, chunk_rays=((1 << 26) - 1) // 32 + 1)
    with pytest.raises(pkg.NskError, match="chunk_rays"):
        ctx.render_image("color", hw, intr, env.c2w, env.depth, chunk_rays=0)
    # residual images asked for without the ground truth they need (the Python method cannot ask for that: through the C interface)
    rgb, depth = torch.zeros(4, 5, 3, device="cuda"), torch.zeros(4, 5, device="cuda")
    res_d, res_c = torch.zeros(4, 5, device="cuda"), torch.zeros(4, 5, 3, device="cuda")
    L, h = pkg.nsk.lib(), (C.c_double * 8)()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.nsk_image_metrics(ctx.h, 4, 5, p(rgb), p(depth), None, p(rgb), p(res_d), None, h) != 0 and b"d_res_depth" in L.nsk_last_error()
    assert L.nsk_image_metrics(ctx.h, 4, 5, p(rgb), p(depth), p(depth), None, None, p(res_c), h) != 0 and b"d_res_color" in L.nsk_last_error()
    assert L.nsk_image_metrics(ctx.h, 4, 5, p(rgb), None, p(depth), None, None, None, h) != 0 and b"d_depth" in L.nsk_last_error()
    assert L.nsk_image_metrics(ctx.h, 0, 5, p(rgb), p(depth), None, None, None, None, h) != 0 and b"Hv" in L.nsk_last_error()
    assert ctx.profile_end() == {}                      # nothing was launched
    env.image("color", True, largest)                   # the largest allowed value is allowed


# ---- 8. C++ ------------------------------------------------------------------------------------------------------------------------
def test_cpp_render_img_equals_render_image(env, tmp_path):
    exe = os.path.join(HOST, "render_img_test")
    if not os.path.exists(exe):
        pytest.fail("render_img_test is not built (run __graft_entry__.build())")
    d, sc = str(tmp_path), env.sc
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    np.save(os.path.join(d, "c2w.npy"), env.fr["c2w"])
    np.save(os.path.join(d, "depth.npy"), env.fr["depth"])
    args = [exe, d, "color", str(iv.H), str(iv.W)] + [repr(float(x)) for x in iv.INTR]
    ray_batch_size = 500000                              # Renderer::Renderer (src/Renderer.cpp:5)
    for with_depth in (True, False):
        if not with_depth:
            os.remove(os.path.join(d, "depth.npy"))
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "render_img_test ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        rgb, depth, var = env.image("color", with_depth, ray_batch_size)
        for name, t in (("img_depth", depth), ("img_var", var), ("img_rgb", rgb)):
            got = np.load(os.path.join(d, name + ".npy"))
            assert got.dtype == np.float32 and got.shape == tuple(t.shape) and got.tobytes() == t.cpu().numpy().tobytes(), (name, with_depth)

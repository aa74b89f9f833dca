"""GPU tests (-m gpu) of the frame-level Mapper and Tracker kernels at their edges: k_frustum_pass1 / _pass2, k_keyframe_overlap,
k_sample_pixels / k_gather_pixels, k_inside_filter and the filter inside k_prepare_rays, k_median_thr and the fused median forms,
k_loss_map / k_loss_track.  The device against the fp32 oracle to the bit and against the fp64 evaluations of tests/keyframe_checks.py
under the margin rule stated there, over the case tables that tests/test_keyframe_cpu.py proves on the CPU; against ATen on the CPU where
the operation is an ATen expression upstream."""
import ctypes as C

import numpy as np
import pytest
import torch

import keyframe_checks as K
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu
LEVELS3 = ("middle", "fine", "color")
_CTX = {}


def _ctx(bound, shape, fresh=False, shapes=None):
    """one context per lattice shape: the shape installed as the middle, fine and color level"""
    key = (np.asarray(bound, np.float32).tobytes(), tuple(shape))
    if fresh or shapes or key not in _CTX:
        gs = dict(coarse=(32, 3, 2, 4), **{k: (32,) + tuple(shape) for k in LEVELS3})
        gs.update(shapes or {})
        ctx = make_ctx(scenes.make_scene(1, gs, bound=bound))
        if fresh or shapes:
            return ctx
        _CTX[key] = ctx
    return _CTX[key]


_FRUSTUM = K.frustum_cases() + K.dyadic_cases()


@pytest.mark.parametrize("k", range(len(_FRUSTUM)), ids=[c["name"] for c in _FRUSTUM])
def test_frustum_mask_cases(k, oracle32):
    """nsk_frustum_mask over the case table x {room walls, all zeros, every third row zero}: byte for byte the fp32 oracle, the fp64 evaluation
    under the margin rule (dyadic cases: at every voxel, exact ties included), coarse all ones.  Excluded shares are those of the fp32 oracle
    (tests/test_keyframe_cpu.py: at most 0.39 % of a case, one voxel of 257; 0 in 30 of the 36 case x image pairs), since the device has its bits."""
    case = _FRUSTUM[k]
    ctx = _ctx(case["bound"], case["shape"])
    level = LEVELS3[k % 3]
    for kind in K.FRUSTUM_KINDS:
        img = K.frustum_image(case, kind)
        got = ctx.frustum_mask(level, cu(img), case["intr"], case["c2w"])
        ref32 = oracle32.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"])
        assert got.shape == ref32.shape and np.array_equal(got, ref32), (case["name"], kind, int((got != ref32).sum()))
        ref = K.frustum64(case["bound"], case["shape"], img, case["intr"], case["c2w"])
        share = K.check_frustum(got, case, kind, ref)
        kept = int(got.sum())
        print("frustum %s/%s on %s: kept %d of %d, excluded %.4f %%, ties %s" % (case["name"], kind, level, kept, got.size, 100 * share, ref["ties"]))
        if kind in case["some"]:
            assert 0 < kept < got.size, (case["name"], kind, kept)
        if case["name"] == "outside-turned":
            assert kept == 0
        if case["dyadic"] and kind == "walls":
            assert sum(ref["ties"].values()) > 0, ref["ties"]
    assert ctx.frustum_mask("coarse", cu(img), case["intr"], case["c2w"]).all()


def test_frustum_maximum_has_the_floor_zero(oracle32):
    """an image whose samples are all negative: max(0, .) on both sides (include/nsk.h)"""
    case = K.frustum_cases()[5]
    img = K.frustum_image(case, "negative")
    got = _ctx(case["bound"], case["shape"]).frustum_mask("fine", cu(img), case["intr"], case["c2w"])
    assert np.array_equal(got, oracle32.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"]))
    K.check_frustum(got, case, "negative", K.frustum64(case["bound"], case["shape"], img, case["intr"], case["c2w"]))


@pytest.mark.parametrize("between", ["nothing", "overlap"])
def test_frustum_mask_carries_nothing_from_call_to_call(between, oracle32):
    """a deep room image, then a shallow image with zero rows, on ONE context: the second mask is a fresh context's (the sampled maximum is
    reset: the zero rows take the SHALLOW maximum); the same with an nsk_keyframe_overlap call in between and a 4 080-voxel level followed by a
    6-voxel level (both calls share one scratch buffer)"""
    big, small = K.frustum_cases()[4], K.frustum_cases()[0]
    assert big["shape"] == (17, 16, 15) and small["shape"] == (1, 2, 3)
    first, second = (big, big) if between == "nothing" else (big, small)
    shapes = dict(middle=(32,) + first["shape"], fine=(32,) + second["shape"])
    deep, shallow = K.frustum_image(first, "walls"), K.frustum_image(second, "shallow")
    assert deep.max() > 4 * shallow.max() and (shallow == 0).any()
    used, fresh = _ctx(K.REF_BOUND, first["shape"], shapes=shapes), _ctx(K.REF_BOUND, first["shape"], shapes=shapes)
    m1 = used.frustum_mask("middle", cu(deep), first["intr"], first["c2w"])
    assert np.array_equal(m1, oracle32.frustum_mask(K.REF_BOUND, first["shape"], deep, first["intr"], first["c2w"]))
    if between == "overlap":
        oc = K.overlap_case(100, 16, 33)
        r = oc["rays"]
        p = used.keyframe_overlap(cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), oc["intr"], oc["HW"], oc["cams"])
        assert np.array_equal(p, oracle32.keyframe_overlap(r["rays_o"], r["rays_d"], r["gt_depth"], oc["intr"], oc["HW"], oc["cams"]).astype(np.float32))
    m2 = used.frustum_mask("fine", cu(shallow), second["intr"], second["c2w"])
    ref = oracle32.frustum_mask(K.REF_BOUND, second["shape"], shallow, second["intr"], second["c2w"])
    assert np.array_equal(m2, fresh.frustum_mask("fine", cu(shallow), second["intr"], second["c2w"])) and np.array_equal(m2, ref)
    # the case bites: with the deep image's maximum left in place the zero rows would reach further
    carried = np.where(shallow == 0, deep.max(), shallow).astype(np.float32)
    assert between == "overlap" or not np.array_equal(ref, oracle32.frustum_mask(K.REF_BOUND, second["shape"], carried, second["intr"], second["c2w"]))


@pytest.mark.parametrize("N,ns,Kf", K.OVERLAP_SIZES)
def test_keyframe_overlap_sizes(N, ns, Kf, oracle32):
    """nsk_keyframe_overlap: the float32 fractions carry the fp32 oracle's bits; round(p N ns) equals the fp64 count up to the points below the
    margin bound (none in these six cases, cap 2 per keyframe); the own pose ranks first, the turned pose sees exactly nothing"""
    case = K.overlap_case(N, ns, Kf)
    r = case["rays"]
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    got = ctx.keyframe_overlap(cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), case["intr"], case["HW"], case["cams"], n_samples=ns)
    ref = oracle32.keyframe_overlap(r["rays_o"], r["rays_d"], r["gt_depth"], case["intr"], case["HW"], case["cams"], n_samples=ns).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got, ref)
    off, low = K.check_overlap(got, case, K.overlap64(case))
    print("overlap (%d, %d, %d): %d low-margin points, %d count differences" % (N, ns, Kf, low, off))


@pytest.mark.parametrize("size", [39, 41])
def test_keyframe_overlap_of_an_image_narrower_than_the_edge_is_zero(size):
    case = K.overlap_case(100, 16, 9, HW=(size, size))
    r = case["rays"]
    got = _ctx(K.REF_BOUND, (9, 8, 11)).keyframe_overlap(cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), case["intr"], case["HW"], case["cams"])
    assert got.shape == (9,) and (got == 0).all(), got


# ---- pixel draw and gather ------------------------------------------------------------------------------------------------------------------
_IMG = {}


def _images():
    if not _IMG:
        depth, color = K.pixel_images()
        _IMG.update(depth=depth, color=color, d_depth=cu(depth), d_color=cu(color))
    return _IMG


@pytest.mark.parametrize("w", range(len(K.WINDOWS)), ids=["%d-%d-%d-%d" % w for w in K.WINDOWS])
def test_pixel_draw_and_gather_windows(w, oracle32):
    """nsk_sample_pixels index-exact against the oracle and inside the window, nsk_gather_pixels with and without colour against numpy indexing,
    n = 0 a success that writes nothing"""
    import nice_slam_cpp_amd as pkg
    win, im = K.WINDOWS[w], _images()
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    for n in K.PIXEL_COUNTS:
        if n == 0:
            pi, pj = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda")
            gd, gc = torch.full((4,), -7.0, device="cuda"), torch.full((4, 3), -7.0, device="cuda")
            torch.cuda.synchronize()
            p = lambda t: C.c_void_p(t.data_ptr())
            assert pkg.nsk.lib().nsk_sample_pixels(ctx.h, C.c_ulonglong(40 + w), 0, *win, p(pi), p(pj)) == 0
            assert pkg.nsk.lib().nsk_gather_pixels(ctx.h, 0, p(pi), p(pj), K.PIXEL_HW[0], K.PIXEL_HW[1], p(im["d_depth"]), p(im["d_color"]), p(gd), p(gc)) == 0
            ctx.sync()
            assert (pi == -7).all() and (pj == -7).all() and (gd == -7).all() and (gc == -7).all()
            continue
        pi, pj = ctx.sample_pixels(40 + w, n, *win)
        ri, rj = oracle32.sample_pixels(40 + w, n, *win)
        K.check_pixels(pi.cpu().numpy(), pj.cpu().numpy(), win, (ri, rj))
        rd, rc = K.gather_np(ri, rj, im["depth"], im["color"])
        gd, gc = ctx.gather_pixels(pi, pj, im["d_depth"], im["d_color"])
        assert np.array_equal(gd.cpu().numpy(), rd) and np.array_equal(gc.cpu().numpy(), rc)
        gd, gc = ctx.gather_pixels(pi, pj, im["d_depth"])
        assert gc is None and np.array_equal(gd.cpu().numpy(), rd)


def test_pixel_draw_decodes_row_major():
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    pi, pj = ctx.sample_pixels(9, 256, 3, 4, 10, 12)                      # a 1 x 2 window shows both pixels within 256 draws
    assert set(pi.cpu().tolist()) == {10, 11} and (pj == 3).all()
    a, b = ctx.sample_pixels(77, 1000, 0, 1, 0, 64), ctx.sample_pixels(77, 1000, 0, 64, 3, 4)      # one row of 64, one column of 64
    assert torch.equal(a[0], b[1]) and (a[1] == 0).all() and (b[0] == 3).all() and len(set(a[0].cpu().tolist())) == 64


@pytest.mark.parametrize("nframes", [1, 3])
def test_prepare_rays_is_the_separate_entry_points(nframes):
    """nsk_prepare_rays on the same windows: the indices of nsk_sample_pixels, the ground truth of nsk_gather_pixels and the keep of
    nsk_inside_filter on its own rays, frame by frame"""
    im = _images()
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    H, W = K.PIXEL_HW
    intr = (600.0, 600.0, 599.5, 339.5)
    rng = np.random.default_rng(5)
    poses = [cu(np.ascontiguousarray(scenes.make_camera(rng, K.REF_BOUND)[:3].reshape(-1))) for _ in range(nframes)]
    shallow = cu((K.pixel_images()[0] * np.float32(1.5)).astype(np.float32))      # depths up to 6 m: the filter drops part of the rays
    for w, win in enumerate(K.WINDOWS):
        for n in K.PIXEL_COUNTS[1:]:
            frames = [dict(depth=im["d_depth"] if f != 1 else shallow, color=im["d_color"], pose=poses[f], seed=900 + 10 * w + f) for f in range(nframes)]
            pr = ctx.prepare_rays(frames, n, win, intr)
            for f, fr in enumerate(frames):
                sl = slice(f * n, (f + 1) * n)
                pi, pj = ctx.sample_pixels(fr["seed"], n, *win)
                assert torch.equal(pr["pix_i"][sl], pi) and torch.equal(pr["pix_j"][sl], pj)
                gd, gc = ctx.gather_pixels(pi, pj, fr["depth"], fr["color"])
                assert torch.equal(pr["gt_depth"][sl], gd) and torch.equal(pr["gt_color"][sl], gc)
                keep = ctx._inside_filter_u8(pr["rays_o"][sl].contiguous(), pr["rays_d"][sl].contiguous(), gd)
                assert torch.equal(pr["keep"][sl], keep)
    assert 0 < int(pr["keep"].sum()) < pr["keep"].numel() or nframes == 1


# ---- inside filter ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [K.REF_BOUND, K.DYADIC_BOUND], ids=["ref", "dyadic"])
def test_inside_filter_is_the_aten_expression(bound, oracle32):
    """nsk_inside_filter == the ATen expression on the CPU, bit for bit: zero direction components (+-0), origins on faces, edges and corners,
    gt == t exactly, one ulp above, 0, +inf, NaN.  A NaN in any of the six quotients drops the ray (include/nsk.h)."""
    ctx = _ctx(bound, (9, 5, 9))
    rays = K.filter_rays(bound)
    for n in K.FILTER_COUNTS + [len(rays[0])]:
        ro, rd, gt = K.filter_tiled(rays, n)
        ref = K.aten_filter(bound, ro, rd, gt)
        got = ctx.inside_filter(cu(ro), cu(rd), cu(gt)).cpu().numpy()
        assert np.array_equal(got, ref), (n, np.flatnonzero(got != ref)[:8])
        assert np.array_equal(oracle32.inside_filter(bound, ro, rd, gt), ref)
    assert not got[:2].any() and 0 < got.sum() < len(got)
    if bound is K.DYADIC_BOUND:
        d, o = cu(np.array([[0, 0, -1]], np.float32)), cu(np.zeros((1, 3), np.float32))
        for g, keep in ((3.0, True), (np.nextafter(np.float32(3), np.float32(4)), False), (0.0, True), (np.inf, False), (np.nan, False)):
            assert bool(ctx.inside_filter(o, d, cu(np.array([g], np.float32)))[0]) == keep, g


def test_prepare_rays_filter_drops_the_rays_inside_a_face():
    """the filter inside nsk_prepare_rays on 0/0 rays: identity rotation, integer principal point, a window one column wide at i = cx (d_x = 0
    exactly) and the camera ON the lower / upper x face; every such ray is dropped, as ATen drops it; a camera inside keeps some"""
    b = K.REF_BOUND
    ctx = _ctx(b, (9, 8, 11))
    H, W, intr = 120, 160, (80.0, 80.0, 80.0, 60.0)
    rng = np.random.default_rng(8)
    depth = cu(rng.uniform(0.5, 4.0, (H, W)).astype(np.float32))
    frames = []
    for ox in (b[0, 0], b[0, 1], np.float32(0.25)):
        c2w = np.concatenate([np.eye(3, dtype=np.float32), np.array([[ox], [0.1], [0.2]], np.float32)], 1)
        frames.append(dict(depth=depth, color=None, pose=cu(np.ascontiguousarray(c2w.reshape(-1))), seed=31))
    pr = ctx.prepare_rays(frames, 256, (0, H, 80, 81), intr)
    ro, rd, gd = (pr[k].cpu().numpy() for k in ("rays_o", "rays_d", "gt_depth"))
    assert (rd[:, 0] == 0).all()
    keep = pr["keep"].cpu().numpy().astype(bool)
    assert np.array_equal(keep, K.aten_filter(b, ro, rd, gd))
    assert not keep[:512].any() and 0 < keep[512:].sum() < 256
    assert np.array_equal(ctx.inside_filter(pr["rays_o"], pr["rays_d"], pr["gt_depth"]).cpu().numpy(), keep)


# ---- Tracker median ---------------------------------------------------------------------------------------------------------------------------
def _loss_track(ctx, B, handle_dynamic=True, use_color=True, detach=False):
    loss, g_d, g_c, g_v = ctx.loss_track(cu(B["depth"]), cu(B["rgb"]), cu(B["var"]), cu(B["gt_depth"]), cu(B["gt_color"]), B.get("w_color", 0.5),
                                         use_color, handle_dynamic, detach)
    return float(loss), g_d.cpu().numpy(), g_c.cpu().numpy(), g_v.cpu().numpy()


@pytest.mark.parametrize("kind", K.MEDIAN_LISTS)
def test_planted_median_through_loss_track(kind):
    """nsk_loss_track(handle_dynamic = 1), the path through k_median_thr, on planted residuals that are exact in fp32: thr = 10 x the lower
    median over the rays the ray mask keeps (numpy sort, equal to torch.median on the CPU), a ray counts iff gt > 0 and r < thr.  The exact set
    of counted rays, the gradients, and the loss against the fp64 sum of the per-ray terms within n 2^-24 sum|l|; ties, all-equal, all-zero
    lists; N at the power-of-two padding switches and the limit of 16 384; with and without a ray mask."""
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    try:
        for N in K.MEDIAN_COUNTS:
            B = K.planted_batch(kind, N)
            r = np.abs(B["gt_depth"] - B["depth"])
            for keep in (None, K.ray_mask(N)):
                assert K.lower_median_x10(r, keep) == K.aten_median_x10(r, keep)
                ctx.set_ray_mask(None if keep is None else cu(keep, torch.uint8))
                ref = K.track_terms64(B, keep, True, True, False)
                K.check_track(*_loss_track(ctx, B), ref, (kind, N, keep is not None))
                if kind == "zero" and (keep is None or keep.any()):      # (N = 1 under the mask keeps no ray: see the fully masked batch)
                    assert not ref["counted"].any() and ref["loss"] == 0.0
    finally:
        ctx.set_ray_mask(None)


def test_median_limit_and_the_fully_masked_batch():
    """N = 16 385 is refused with a message that names the limit of 16 384, and the context works afterwards.  A batch whose ray mask keeps no
    ray: every residual sorts as +inf, the threshold is +inf, and every ray with gt > 0 counts (nsk_loss_track applies the mask to the median
    only) -- pinned here as it is."""
    import nice_slam_cpp_amd as pkg
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    B = K.planted_batch("distinct", K.MEDIAN_LIMIT + 1)
    with pytest.raises(pkg.nsk.NskError, match=str(K.MEDIAN_LIMIT)):
        _loss_track(ctx, B)
    B = K.planted_batch("outliers", 257)
    K.check_track(*_loss_track(ctx, B), K.track_terms64(B, None, True, True, False), "after the refusal")
    try:
        ctx.set_ray_mask(cu(np.zeros(257, np.uint8), torch.uint8))
        ref = K.track_terms64(B, np.zeros(257, np.uint8), True, True, False)
        assert ref["thr"] == np.inf and np.array_equal(ref["counted"], B["gt_depth"] > 0)
        K.check_track(*_loss_track(ctx, B), ref, "fully masked")
    finally:
        ctx.set_ray_mask(None)


@pytest.mark.parametrize("N", K.FUSED_COUNTS)
def test_fused_median_forms_drop_the_expected_rays(N, oracle32):
    """nsk_track_step with ray gradients in its three forms (deferred: every workgroup of the backward selects the median; barrier: inside the
    loss launch; three: k_median_thr) on batches with exact ties at the switches of lower_median_x10 and the fused limit, and at 250 and 258
    rays, where the median is the first of its pair, so that a select one rank low returns another value.  Expected dropped
    set: numpy fp32 |gt - D| with D from nsk_render_forward of the same rays, the lower median, r >= 10 x median, united with gt = 0.  Every
    form drops exactly that set (rows of zero gradient); a ray within a relative 1e-5 of the threshold may differ (none is that close: cap 2),
    and the copies of a ray share their fate.  nsk_render_forward and the step's forward share their bits here: the threshold the step
    applied (debug_fetch "median_thr") equals the one computed from render_forward's depth -- asserted below."""
    sc, rays, idx, off = K.fused_case(N, oracle32)
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    forms = {"deferred": {}, "barrier": {"no_deferred_median": 1}, "three": {"no_fused_median": 1}}
    for form, tune in forms.items():
        ctx = make_ctx(sc)
        for k, v in tune.items():
            ctx.set_tuning(k, v)
        _, depth, _, _ = ctx.render_forward("color", ro, rd, gd)
        dropped, near, thr = K.dropped_by_median(rays["gt_depth"], depth.cpu().numpy())
        assert near.sum() <= 2, (form, int(near.sum()))
        g_ro, g_rd, loss = torch.empty_like(ro), torch.empty_like(rd), torch.zeros(1, device="cuda")
        for _ in range(2):
            ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, True, True, True, flags=4, loss=loss, g_rays=(g_ro, g_rd))
        ctx.sync()
        zero = np.all(g_rd.cpu().numpy() == 0, axis=1) & np.all(g_ro.cpu().numpy() == 0, axis=1)
        applied = ctx.debug_fetch("median_thr", N * 48)[0]
        print("fused %s N=%d: thr %.9g (step applied %.9g), dropped %d, near %d" % (form, N, thr, applied, int(zero.sum()), int(near.sum())))
        assert not ((zero != dropped) & ~near).any(), (form, np.flatnonzero(zero != dropped)[:8])
        assert applied == thr, (form, applied, thr)
        assert set(idx[zero & (rays["gt_depth"] > 0)]) >= set(off.tolist()) and zero.sum() < N // 2
        first = {}
        for i, k in enumerate(idx):
            assert zero[i] == first.setdefault(k, zero[i]), (form, i)
        ctx.close()


# ---- losses at exact zeros ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", K.LOSS_COUNTS)
def test_losses_at_exact_zeros_against_autograd(N):
    """nsk_loss_map / nsk_loss_track against ATen autograd of src/Mapper.cpp:435-442 and src/Tracker.cpp:67-82 on the CPU: depth and colour
    residuals exactly 0 (|.|'s gradient at 0 is 0), gt_depth = 0, var = 0 and 1e-12, colour off, variance detached or not; gradients
    elementwise to the tolerances of test_losses_and_pose_kernels, signs exact"""
    ctx = _ctx(K.REF_BOUND, (9, 8, 11))
    B = K.zero_batch(N)
    for use_color in (True, False):
        l_ref, gd_ref, gc_ref = K.aten_loss_map(B, 0.5, use_color)
        loss, g_d, g_c = ctx.loss_map(cu(B["depth"]), cu(B["rgb"]), cu(B["gt_depth"]), cu(B["gt_color"]), 0.5, use_color)
        assert abs(float(loss) - l_ref) <= 1e-4 * abs(l_ref)
        assert np.array_equal(g_d.cpu().numpy(), gd_ref) and np.array_equal(g_c.cpu().numpy(), gc_ref)
        for hd in (False, True):
            for detach in (True, False):
                l_ref, *g_ref = K.aten_loss_track(B, 0.5, use_color, hd, detach)
                loss, *got = _loss_track(ctx, B, hd, use_color, detach)
                assert abs(loss - l_ref) <= 1e-4 * abs(l_ref), (N, use_color, hd, detach, loss, l_ref)
                K.check_loss_grads(got, g_ref, (N, use_color, hd, detach))

"""The case tables of tests/keyframe_checks.py proven on the CPU before a GPU sees them: the fp32 and fp64 oracles against the independent
fp64 numpy evaluations (frustum mask, keyframe overlap, Tracker median and loss), against ATen on the CPU where the operation is an ATen
expression upstream (inside filter, torch.median, the two losses through autograd), and the caps of the margin rule met by the fp32 oracle
alone.  tests/test_gpu_keyframe.py runs the same tables on the device."""
import numpy as np
import pytest

import keyframe_checks as K
import scenes


def test_frustum_tables_meet_the_margin_caps(oracle32, oracle64):
    """Every frustum case x depth image: the fp32 oracle differs from the fp64 evaluation only at voxels whose margin is below 1, and at most
    1 % of a case's voxels are that close.  Excluded shares measured with the fp32 oracle (walls / zeros / every third row zero): 0 in 30 of
    the 36 case x image pairs; inside-1x1x257 rows 0.39 % (one voxel), inside-17x16x15 walls and rows 0.025 % (one voxel), outside-looking-in
    walls 0.098 % and rows 0.12 %, scaled-rotation rows 0.13 %.  No voxel of any case differs between the two; the fp64 oracle is held to the
    same rule."""
    shares = {}
    for case in K.frustum_cases():
        for kind in K.FRUSTUM_KINDS:
            img = K.frustum_image(case, kind)
            ref = K.frustum64(case["bound"], case["shape"], img, case["intr"], case["c2w"])
            got32 = oracle32.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"])
            got64 = oracle64.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"])
            shares[case["name"], kind] = (K.check_frustum(got32, case, kind, ref), int((got32 != ref["mask"]).sum()))
            assert not ((got64 != ref["mask"]) & (ref["margin"] >= 1)).any()
            kept = int(ref["mask"].sum())
            if kind in case["some"]:
                assert 0 < kept < ref["mask"].size, (case["name"], kind, kept)
            if case["name"] == "outside-turned":
                assert kept == 0 and not got32.any()                     # the ball misses the lattice, and nothing else can mark a voxel
            if case["name"] == "on-a-voxel":
                on = np.unravel_index((4 * 8 + 3) * 11 + 5, case["shape"])
                assert ref["mask"][on] and got32[on]                     # z = 1e-5 > 0 fails the depth test; the ball keeps the voxel
        assert oracle32.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"], is_coarse=True).all()
    for k, v in shares.items():
        print("frustum %-28s %-6s excluded %.4f %%, differing voxels %d" % (k[0], k[1], 100 * v[0], v[1]))


def test_frustum_is_exact_on_dyadic_lattices(oracle32, oracle64):
    """The eight dyadic cases: fp32 == fp64 at EVERY voxel, no exclusion, the voxels exactly on u = 0, v = 0, z_cam = 0 and |p - c|^2 = 0.25
    included.  Ties per case (u = 0 / v = 0 / z_cam = 0 / ball; shapes 9x5x9 and 5x3x17): t (0,0,1.5) 10/9/45/0 and 12/17/51/2, t (0,0,0)
    15/9/45/0 and 15/17/51/2, t (1,0,3) 10/9/45/0 and 12/17/51/2, t (0,0,4.5) 5/0/0/0 and 6/0/0/0 (the camera plane and row lie between
    lattice planes); 85 / 78 / 288 / 6 in all, each set non-empty (asserted)."""
    total = dict(u0=0, v0=0, z0=0, ball=0)
    for case in K.dyadic_cases():
        for kind in K.FRUSTUM_KINDS:
            img = K.frustum_image(case, kind)
            ref = K.frustum64(case["bound"], case["shape"], img, case["intr"], case["c2w"])
            for o in (oracle32, oracle64):
                K.check_frustum(o.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"]), case, kind, ref)
        print("dyadic %-32s ties %s kept %d" % (case["name"], ref["ties"], int(ref["mask"].sum())))
        for k in total:
            total[k] += ref["ties"][k]
    assert all(v > 0 for v in total.values()), total
    print("dyadic tie totals", total)


def test_frustum_maximum_has_the_floor_zero(oracle32, oracle64):
    """an image whose samples are all negative: the maximum is 0 (include/nsk.h), not the largest negative sample"""
    case = K.frustum_cases()[5]
    img = K.frustum_image(case, "negative")
    assert (img < 0).all()
    ref = K.frustum64(case["bound"], case["shape"], img, case["intr"], case["c2w"])
    assert ref["dmax"] == 0.0
    for o in (oracle32, oracle64):
        K.check_frustum(o.frustum_mask(case["bound"], case["shape"], img, case["intr"], case["c2w"]), case, "negative", ref)


@pytest.mark.parametrize("N,ns,Kf", K.OVERLAP_SIZES)
def test_overlap_counts_equal_the_fp64_counts(N, ns, Kf, oracle32, oracle64):
    """round(p N ns) of the fp32 (and fp64) oracle against the fp64 count per keyframe.  Measured: equal in all six size cases, and no point of
    any case has a margin below 1 (cap: 2 per keyframe)."""
    case = K.overlap_case(N, ns, Kf)
    ref = K.overlap64(case)
    r = case["rays"]
    for o in (oracle32, oracle64):
        got = o.keyframe_overlap(r["rays_o"], r["rays_d"], r["gt_depth"], case["intr"], case["HW"], case["cams"], n_samples=ns)
        off, low = K.check_overlap(got, case, ref)
    print("overlap (%d, %d, %d): counts %s, low-margin points %d, count differences %d" % (N, ns, Kf, ref[0].tolist(), low, off))


@pytest.mark.parametrize("size", [39, 41])
def test_overlap_of_an_image_narrower_than_the_edge_is_zero(size, oracle32):
    """20 < u < W - 20 is empty at 39 and one pixel wide at 41: no sample point of these rays falls into it"""
    case = K.overlap_case(100, 16, 9, HW=(size, size))
    assert (K.overlap64(case)[0] == 0).all()
    r = case["rays"]
    assert (oracle32.keyframe_overlap(r["rays_o"], r["rays_d"], r["gt_depth"], case["intr"], case["HW"], case["cams"]) == 0).all()


def test_pixel_draw_tables(oracle32):
    depth, color = K.pixel_images()
    for w, win in enumerate(K.WINDOWS):
        for n in K.PIXEL_COUNTS:
            pi, pj = oracle32.sample_pixels(40 + w, n, *win)
            assert pi.shape == (n,)
            K.check_pixels(pi, pj, win)
            if n:
                gd, gc = oracle32.gather_pixels(pi, pj, depth, color)
                rd, rc = K.gather_np(pi, pj, depth, color)
                assert np.array_equal(gd, rd) and np.array_equal(gc, rc)
    pi, pj = oracle32.sample_pixels(9, 256, 3, 4, 10, 12)                 # a 1 x 2 window shows both pixels within 256 draws
    assert set(pi.tolist()) == {10, 11} and (pj == 3).all()
    # the index is floor(hash * total / 2^32), decoded row-major: one row of 64 and one column of 64 draw the same numbers
    a, b = oracle32.sample_pixels(77, 1000, 0, 1, 0, 64), oracle32.sample_pixels(77, 1000, 0, 64, 3, 4)
    assert np.array_equal(a[0], b[1]) and (a[1] == 0).all() and (b[0] == 3).all() and len(set(a[0].tolist())) == 64


@pytest.mark.parametrize("bound", [K.REF_BOUND, K.DYADIC_BOUND], ids=["ref", "dyadic"])
def test_inside_filter_is_the_aten_expression(bound, oracle32):
    """nso_inside_filter == torch.min(torch.max((bound - o) / d, 2), 1) >= gt on the CPU, bit for bit, the 0/0 rays included.  Before the NaN
    rule the comparison form kept o = (b_x.lo, 0, 0), d = (0, 0.3, -1) and dropped o = (b_x.hi, b_y.hi, 0), d = (0, 0, -1); ATen drops both."""
    rays = K.filter_rays(bound)
    assert rays[3] > 100                                                 # rays with a NaN exit in the list
    for n in K.FILTER_COUNTS + [len(rays[0])]:
        ro, rd, gt = K.filter_tiled(rays, n)
        ref = K.aten_filter(bound, ro, rd, gt)
        assert np.array_equal(K.filter_np(bound, ro, rd, gt)[0], ref)
        assert np.array_equal(oracle32.inside_filter(bound, ro, rd, gt), ref), n
    ro, rd, gt = K.filter_tiled(rays, len(rays[0]))
    ref = K.aten_filter(bound, ro, rd, gt)
    assert not ref[:2].any() and 0 < ref.sum() < len(ref)
    d = np.array([[0, 0, -1]], np.float32)
    if bound is K.DYADIC_BOUND:                                          # gt == t exactly (t = 3), and one ulp above it
        for g, keep in ((3.0, True), (np.nextafter(np.float32(3), np.float32(4)), False), (0.0, True), (np.inf, False), (np.nan, False)):
            got = oracle32.inside_filter(bound, np.zeros((1, 3), np.float32), d, np.array([g], np.float32))
            assert got[0] == keep == K.aten_filter(bound, np.zeros((1, 3), np.float32), d, np.array([g], np.float32))[0], g


@pytest.mark.parametrize("kind", K.MEDIAN_LISTS)
def test_planted_median_against_numpy_and_torch(kind, oracle32, oracle64):
    """10 x lower median of planted, exact residuals: numpy sort == torch.median == the oracle's loss, set of counted rays included"""
    for N in K.MEDIAN_COUNTS:
        B = K.planted_batch(kind, N)
        r = np.abs(B["gt_depth"] - B["depth"])
        for keep in (None, K.ray_mask(N)):
            assert K.lower_median_x10(r, keep) == K.aten_median_x10(r, keep), (kind, N)
        for detach in (True, False):
            ref = K.track_terms64(B, None, True, True, detach)
            for o in (oracle32, oracle64):
                loss, g_d, g_c, g_v = o.loss_track(B["depth"], B["rgb"], B["var"], B["gt_depth"], B["gt_color"], B["w_color"], True, True, detach)
                K.check_track(loss, g_d, g_c, g_v, ref, (kind, N, detach))
        if kind == "zero":
            assert not ref["counted"].any() and ref["loss"] == 0.0
        if kind == "half" and N > 1:
            assert ref["counted"].any() == (N % 2 == 1)                   # the LOWER median: 0 for even N
        if kind in ("distinct", "outliers") and N >= 16:
            assert 0 < (~ref["counted"]).sum() < N
    assert K.lower_median_x10(np.ones(4, np.float32), np.zeros(4, np.uint8)) == np.inf


@pytest.mark.parametrize("N", K.FUSED_COUNTS)
def test_fused_median_batches_have_no_ray_at_the_threshold(N, oracle32):
    """the batches of the fused-form test: with the fp32 oracle's depth no ray lies within a relative 1e-5 of 10 x median, five distinct rays
    (and their copies) are dropped by it, and the copies of a ray tie exactly"""
    sc, rays, idx, off = K.fused_case(N, oracle32)
    fw = oracle32.render_forward(oracle32.opts(sc["bound"]), sc["grids"], sc["decoders"], "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"])
    dropped, near, thr = K.dropped_by_median(rays["gt_depth"], fw["depth"])
    assert not near.any(), (N, int(near.sum()))
    by_median = dropped & (rays["gt_depth"] > 0)
    assert set(idx[by_median]) >= set(off.tolist()) and 0 < by_median.sum() < N // 4
    first = {}
    for i, k in enumerate(idx):
        assert dropped[i] == first.setdefault(k, dropped[i])


@pytest.mark.parametrize("N", K.LOSS_COUNTS)
def test_losses_at_exact_zeros_against_autograd(N, oracle32):
    """nso_loss_map / nso_loss_track against ATen autograd of src/Mapper.cpp:435-442 and src/Tracker.cpp:67-82 on batches with exact zeros"""
    B = K.zero_batch(N)
    for use_color in (True, False):
        l_ref, gd_ref, gc_ref = K.aten_loss_map(B, 0.5, use_color)
        loss, g_d, g_c = oracle32.loss_map(B["depth"], B["rgb"], B["gt_depth"], B["gt_color"], 0.5, use_color)
        assert abs(loss - l_ref) <= 1e-4 * abs(l_ref)
        assert np.array_equal(g_d, gd_ref) and np.array_equal(g_c, gc_ref)
        for hd in (False, True):
            for detach in (True, False):
                l_ref, *g_ref = K.aten_loss_track(B, 0.5, use_color, hd, detach)
                loss, *got = oracle32.loss_track(B["depth"], B["rgb"], B["var"], B["gt_depth"], B["gt_color"], 0.5, use_color, hd, detach)
                assert abs(loss - l_ref) <= 1e-4 * abs(l_ref), (N, use_color, hd, detach)
                K.check_loss_grads(got, g_ref, (N, use_color, hd, detach))

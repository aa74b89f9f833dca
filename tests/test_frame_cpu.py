"""CPU tests (-m "not gpu") of the frame preparation's rule: the numpy restatement in tests/frame_checks.py against torch's CPU
F.interpolate, its S1 against the fp64 form with a derived per-pixel bound, that form against scipy.ndimage.map_coordinates, the rule's
properties, and nsk_frame_plan through ctypes (the library loads without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import frame_checks as fc

F = np.float32
SIZE_PAIRS = [((480, 640), (384, 512)), ((13, 17), (9, 11)), ((9, 11), (13, 17)), ((97, 129), (48, 64)), ((2, 3), (7, 1))]


def _u8(rng, H, W, C3=3):
    return rng.integers(0, 256, size=(H, W, C3), dtype=np.uint8)


def _torch_resize(img, size, mode, **kw):
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None]
    return TF.interpolate(t, size=size, mode=mode, **kw)[0].permute(1, 2, 0).numpy()


# ---- the restatement against torch's CPU F.interpolate -----------------------------------------------------------------------------------
def test_nearest_index_equals_torch_for_every_size_pair():
    for n_in in range(1, 70):
        src = torch.arange(n_in, dtype=torch.float32)[None, None, None, :]
        for n_out in range(1, 70):
            got = fc.nearest_index(n_in, n_out)
            want = TF.interpolate(src, size=(1, n_out), mode="nearest")[0, 0, 0].numpy().astype(np.int32)
            assert np.array_equal(got, want), (n_in, n_out)
    for n_in, n_out in ((480, 384), (640, 512)):
        src = torch.arange(n_in, dtype=torch.float32)[None, None, None, :]
        want = TF.interpolate(src, size=(1, n_out), mode="nearest")[0, 0, 0].numpy().astype(np.int32)
        assert np.array_equal(fc.nearest_index(n_in, n_out), want)


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_depth_nearest_equals_torch(pair):
    (H, W), (Ho, Wo) = pair
    d = np.random.default_rng(3).random((H, W, 1), dtype=F)
    assert np.array_equal(fc.resize_nearest(d[None, :, :, 0], Ho, Wo)[0], _torch_resize(d, (Ho, Wo), "nearest")[:, :, 0])


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_bilinear_forms_within_1e6_of_torch(pair):
    """each side is a convex combination of values <= 1 with at most 8 roundings of 2^-24: 2 x 8 x 2^-24 = 9.5e-7 < 1e-6"""
    (H, W), (Ho, Wo) = pair
    img = fc.convert_color(_u8(np.random.default_rng(H * 1000 + W), H, W))
    e_half = float(np.abs(fc.resize_half(img, Ho, Wo) - _torch_resize(img, (Ho, Wo), "bilinear", align_corners=False)).max())
    e_al = float(np.abs(fc.resize_aligned(img, Ho, Wo) - _torch_resize(img, (Ho, Wo), "bilinear", align_corners=True)).max())
    print("S2 (half-pixel) max |diff| %.3g, S3 (aligned) max |diff| %.3g" % (e_half, e_al))
    assert e_half <= 1e-6 and e_al <= 1e-6


# ---- S1 ---------------------------------------------------------------------------------------------------------------------------------
def _tum_images():
    H, W = 480, 640
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = np.stack([0.5 + 0.5 * np.sin(u / 37.0) * np.cos(v / 23.0), u / W, 0.5 + 0.5 * np.cos((u + v) / 51.0)], -1).astype(F)
    rnd = fc.convert_color(_u8(np.random.default_rng(7), H, W))
    return dict(smooth=smooth, random=rnd)


@pytest.fixture(scope="module")
def tum_images():
    return _tum_images()


@pytest.mark.parametrize("which", ["smooth", "random"])
def test_undistort_f32_within_the_bound_of_its_f64_form(tum_images, which):
    img = tum_images[which]
    cam = fc.TUM_CAM
    out, border = fc.undistort_f32(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], fc.TUM_DIST)
    val, bound = fc.undistort_f64(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], fc.TUM_DIST)
    err = np.abs(out.astype(np.float64) - val)
    print("%s: largest bound %.3g, largest error %.3g, largest error / bound %.3g, border pixels %d"
          % (which, bound.max(), err.max(), (err / np.maximum(bound, 1e-300)).max(), int(border.sum())))
    assert out.dtype == np.float32 and np.isfinite(bound).all()
    assert (err <= bound).all()                      # every pixel: bilinear sampling is continuous across tap changes
    assert 0 < int(border.sum()) < border.size       # TUM's undistortion does leave a rim


@pytest.mark.parametrize("which", ["smooth", "random"])
def test_f64_form_equals_scipy_map_coordinates(tum_images, which):
    from scipy.ndimage import map_coordinates
    img = tum_images[which].astype(np.float64)
    cam = fc.TUM_CAM
    us, vs, _, _ = fc.source_coords_f64(480, 640, cam["fx"], cam["fy"], cam["cx"], cam["cy"], fc.TUM_DIST)
    val = fc.bilinear_zero_f64(img, us, vs)
    for ch in range(3):
        ref = map_coordinates(img[:, :, ch], [vs, us], order=1, mode="grid-constant", cval=0.0)
        assert float(np.abs(ref - val[:, :, ch]).max()) <= 1e-12


def test_border_count_small_case_by_hand():
    """a 3 x 3 image under the identity map: the last column and the last row read their second tap at index 3, outside the image"""
    img = np.arange(27, dtype=F).reshape(3, 3, 3)
    out, border = fc.undistort_f32(img, 1.0, 1.0, 0.0, 0.0, [0.0, 0.0, 0.0, 0.0])
    assert np.array_equal(out, img) and int(border.sum()) == 5       # zero coefficients: us = u exactly, the taps at 3 lie outside (weight 0 counts)
    assert border[:, 2].all() and border[2, :].all() and not border[:2, :2].any()


def test_three_operation_division_by_255_is_the_division_for_every_byte():
    """the kernel's float(v) / 255: q = RN(a y), r = a - 255 q (exact), RN(q + r y) with y = RN(1 / 255), in exact rational arithmetic
    with one rounding to fp32 per operation, against numpy's correctly rounded fp32 division, for all 256 bytes"""
    from fractions import Fraction as Fr

    def rn32(fr):
        d = float(fr)
        if Fr(d) == fr:
            return F(d)                  # a double converts to fp32 with one correct rounding, ties to even
        c = F(d)
        cands = [c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(-np.inf))]
        dist = sorted((abs(Fr(float(x)) - fr), i) for i, x in enumerate(cands))
        assert dist[0][0] < dist[1][0]
        return cands[dist[0][1]]
    y = rn32(Fr(1, 255))
    assert float(y).hex() == "0x1.0101020000000p-8"
    for a in range(256):
        q = rn32(Fr(a) * Fr(float(y)))
        r = Fr(a) - 255 * Fr(float(q))
        assert Fr(float(F(float(r)))) == r                       # the residual is an fp32 number: the FMA delivers it exactly
        assert rn32(Fr(float(q)) + r * Fr(float(y))) == F(a) / F(255), a


# ---- properties -------------------------------------------------------------------------------------------------------------------------
def test_linear_image_stays_linear_through_crop_size():
    H, W, Ho, Wo = 97, 129, 48, 64
    v, u = np.mgrid[0:H, 0:W].astype(F)
    img = (F(0.25) * u + F(0.5) * v + F(3))[..., None].repeat(3, -1)       # exact in fp32
    out = fc.resize_aligned(img, Ho, Wo)
    vo, uo = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    want = 0.25 * uo * ((W - 1) / (Wo - 1)) + 0.5 * vo * ((H - 1) / (Ho - 1)) + 3
    # the coordinate carries 2 roundings (the scale, the product) of up to 2^-24 x 128, the value 8 more of its magnitude (<= 84)
    tol = 2 * 2.0 ** -24 * 128 * 0.5 + 8 * 2.0 ** -24 * 84
    assert float(np.abs(out[..., 0] - want).max()) <= tol


def test_all_stages_off_is_the_conversion_alone():
    rng = np.random.default_rng(5)
    c = _u8(rng, 5, 7)[None]
    d = rng.integers(0, 65536, size=(1, 5, 7), dtype=np.uint16)
    co, do, intr, nb = fc.prepare(c, d, fc.options(fx=3.0, fy=4.0, cx=1.0, cy=2.0, png_depth_scale=5000.0, scale=1.5))
    assert co.tobytes() == (c.astype(F) / F(255)).tobytes()
    assert do.tobytes() == ((d.astype(F) / F(5000)) * F(1.5)).tobytes()
    assert intr.tolist() == [3.0, 4.0, 1.0, 2.0] and nb == 0
    cf = rng.random((1, 5, 7, 3), dtype=F)
    co, _, _, _ = fc.prepare(cf, None, fc.options(swap_rb=True))
    assert co.tobytes() == np.ascontiguousarray(cf[..., ::-1]).tobytes()


def test_no_coefficients_against_explicit_zeros():
    img = fc.convert_color(_u8(np.random.default_rng(9), 23, 31))
    o = fc.tum_options(23, 31)
    out, border = fc.undistort_f32(img, o["fx"], o["fy"], o["cx"], o["cy"], [0.0] * 5)
    val, bound = fc.undistort_f64(img, o["fx"], o["fy"], o["cx"], o["cy"], [0.0] * 5)
    assert (np.abs(out - val) <= bound).all()
    # in doubles the zero coefficients give the image itself up to the coordinate's own roundings, which the bound holds
    assert (np.abs(img.astype(np.float64) - val) <= bound).all()
    # so the two fp32 results, n_dist = 0 (the image) and five zeros, are within the bound of each other through the doubles; not byte-equal
    # in general (us = fx ((u - cx) / fx) + cx does not round back to u at every pixel)
    assert (np.abs(out.astype(np.float64) - img) <= 2 * bound).all()
    c = (img * F(255)).astype(np.uint8)[None]
    off = fc.prepare(c, None, fc.tum_options(23, 31, dist=[], crop_size=None, crop_edge=0))[0]
    assert off.tobytes() == fc.convert_color(c).tobytes()


def test_crop_edge_commutes_with_slicing():
    rng = np.random.default_rng(11)
    c = _u8(rng, 23, 31)[None].repeat(2, 0)
    d = rng.integers(0, 65536, size=(2, 23, 31), dtype=np.uint16)
    o = fc.tum_options(23, 31, crop_size=(17, 19), crop_edge=0)
    c0, d0, i0, _ = fc.prepare(c, d, o)
    o2 = dict(o, crop_edge=2)
    c2, d2, i2, _ = fc.prepare(c, d, o2)
    assert c2.tobytes() == np.ascontiguousarray(c0[:, 2:-2, 2:-2]).tobytes()
    assert d2.tobytes() == np.ascontiguousarray(d0[:, 2:-2, 2:-2]).tobytes()
    assert i2[0] == i0[0] and i2[1] == i0[1] and i2[2] == i0[2] - F(2) and i2[3] == i0[3] - F(2)


def test_tum_intrinsics_equal_upstream_to_one_ulp():
    cam = fc.TUM_CAM
    p = fc.plan(fc.tum_options(), 480, 640, 480, 640)
    H, W, fx, fy, cx, cy = fc.intrinsics_upstream(480, 640, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["crop_size"], cam["crop_edge"])
    assert (p["H"], p["W"]) == (H, W) == (368, 496)
    for got, want in zip(p["intr"], (fx, fy, cx, cy)):
        assert abs(float(got) - want) <= float(np.spacing(F(want))), (got, want)


# ---- nsk_frame_plan through ctypes ----------------------------------------------------------------------------------------------------------
CASES = [
    (dict(fc.tum_options()), (480, 640), (480, 640)),
    (dict(fc.tum_options(23, 31, crop_size=(17, 19), crop_edge=2)), (23, 31), (23, 31)),
    (dict(fc.options(fx=577.87, fy=577.87, cx=319.5, cy=239.5, crop_edge=10, png_depth_scale=1000.0)), (968, 1296), (480, 640)),
    (dict(fc.options(fx=600.0, fy=600.0, cx=599.5, cy=339.5, png_depth_scale=6553.5)), (680, 1200), (680, 1200)),
    (dict(fc.options(fx=7.0, fy=5.0, cx=1.3, cy=0.7, crop_size=(7, 1))), (2, 3), (2, 3)),
]


def _plan(o, cs, ds):
    import nice_slam_cpp_amd as pkg
    return pkg.nsk.frame_plan(cs, ds, (o["fx"], o["fy"], o["cx"], o["cy"]), o["dist"], o["crop_size"], o["crop_edge"], o["png_depth_scale"],
                              o["scale"], o["swap_rb"])


def test_frame_plan_equals_the_restatement():
    import nice_slam_cpp_amd as pkg
    pkg.build()
    for o, cs, ds in CASES:
        H, W, intr = _plan(o, cs, ds)
        p = fc.plan(o, cs[0], cs[1], ds[0], ds[1])
        assert (H, W) == (p["H"], p["W"])
        assert intr.dtype == np.float32 and intr.tobytes() == p["intr"].tobytes()


@pytest.mark.parametrize("change,sizes,word", [
    (dict(crop_edge=9, crop_size=(17, 19)), ((23, 31), (23, 31)), "crop_edge"),
    (dict(crop_edge=12, crop_size=None), ((23, 31), (23, 31)), "crop_edge"),
    (dict(dist=[0.1, 0.2, 0.3]), ((23, 31), (23, 31)), "n_dist"),
    (dict(), ((29, 37), (23, 31)), "undistort"),
    (dict(crop_size=(17, 0)), ((23, 31), (23, 31)), "crop_size"),
    (dict(crop_size=(0, 19)), ((23, 31), (23, 31)), "crop_size"),
])
def test_frame_plan_names_the_invalid_option(change, sizes, word):
    import nice_slam_cpp_amd as pkg
    pkg.build()
    o = dict(fc.tum_options(23, 31, crop_size=(17, 19), crop_edge=2), **change)
    with pytest.raises(ValueError):
        fc.plan(o, *sizes[0], *sizes[1])
    with pytest.raises(pkg.NskError) as ei:
        _plan(o, *sizes)
    assert word in str(ei.value), str(ei.value)


def test_frame_plan_null_outputs_and_null_opts():
    import nice_slam_cpp_amd as pkg
    pkg.build()
    L = pkg.nsk.lib()
    o = pkg.nsk.frame_opts((1.0, 1.0, 0.0, 0.0))
    assert L.nsk_frame_plan(C.byref(o), 4, 5, 4, 5, None, None, None) == 0
    assert L.nsk_frame_plan(None, 4, 5, 4, 5, None, None, None) != 0 and b"opts" in L.nsk_last_error()
    assert L.nsk_version() >= 101

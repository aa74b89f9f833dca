"""CPU tests of the whole-frame helpers (tests/image_views.py): the view's pixel lists against the oracle's explicit-index functions, the
metrics restatement on hand-made images, and that the frame the GPU tests render can tell the two gt_depth_max semantics apart."""
import numpy as np
import pytest

import image_views as iv
import scenes


@pytest.fixture(scope="module")
def frame():
    return iv.make_frame()


@pytest.mark.parametrize("window,stride", [(None, 1), ((3, 22, 5, 30), 2), ((3, 22, 5, 30), 3), ((0, 24, 31, 32), 1), ((23, 24, 0, 32), 5)])
def test_view_pixels_order_and_gather(oracle32, frame, window, stride):
    pi, pj = iv.view_pixels(iv.H, iv.W, window, stride)
    Hv, Wv = iv.view_shape(iv.H, iv.W, window, stride)
    H0, H1, W0, W1 = window or (0, iv.H, 0, iv.W)
    assert pi.size == Hv * Wv and Hv == -(-(H1 - H0) // stride) and Wv == -(-(W1 - W0) // stride)
    n = np.arange(Hv * Wv)
    assert (pi == W0 + stride * (n % Wv)).all() and (pj == H0 + stride * (n // Wv)).all()          # row-major: n = row Wv + col
    assert pi.max() < W1 and pj.max() < H1 and pi.max() + stride >= W1 and pj.max() + stride >= H1
    # the oracle's gather on the list is the strided slice of the images
    gd, gc = oracle32.gather_pixels(pi, pj, frame["depth"], frame["color"])
    assert (gd.reshape(Hv, Wv) == frame["depth"][H0:H1:stride, W0:W1:stride]).all()
    assert (gc.reshape(Hv, Wv, 3) == frame["color"][H0:H1:stride, W0:W1:stride]).all()
    # upstream's get_rays order: directions of the meshgrid, row-major (utils.h:44-52), for the ragged sub-range too
    fx, fy, cx, cy = frame["intr"]
    ro, rd = oracle32.rays_from_pixels(pi, pj, fx, fy, cx, cy, frame["c2w"])
    f32 = np.float32
    dirs = np.stack([(pi.astype(f32) - f32(cx)) / f32(fx), -((pj.astype(f32) - f32(cy)) / f32(fy)), -np.ones(pi.size, f32)], -1)
    want = (dirs[:, None, :].astype(np.float64) * frame["c2w"][None, :3, :3].astype(np.float64)).sum(-1)
    assert np.abs(rd - want).max() < 1e-5 and (ro == frame["c2w"][:3, 3]).all()
    a, k = min(200, pi.size - 1), min(168, pi.size - min(200, pi.size - 1))
    ro2, rd2 = oracle32.rays_from_pixels(pi[a:a + k], pj[a:a + k], fx, fy, cx, cy, frame["c2w"])
    assert rd2.tobytes() == rd[a:a + k].tobytes()


def test_metrics_restatement_on_hand_made_images():
    f32 = np.float32
    depth = np.arange(12, dtype=f32).reshape(3, 4) * f32(0.25) + f32(1)
    gt = depth + np.array([[0.5, -0.25, 0, 1], [0.125, 0, -2, 0.75], [0, 0, 0.0625, -0.5]], f32)
    gt[1, 1] = 0.0                                   # no measurement: no residual, not in the sum
    rgb = np.linspace(0, 1, 36, dtype=f32).reshape(3, 4, 3)
    gc = rgb + f32(0.125)
    gc[0, 0] = rgb[0, 0] - np.array([0.5, 0.25, 0], f32)
    depth[2, 3] = np.nan                             # a non-finite pixel: left out of every sum, counted
    h, rd, rc = iv.metrics_ref(rgb, depth, gt, gc)
    assert h[0] == 12 and h[5] == 1 and h[6] == 0 and h[7] == 0
    assert h[1] == 10                                # 12 - zero depth - NaN
    want_d = [0.5, 0.25, 0, 1, 0.125, 2, 0.75, 0, 0, 0.0625]
    assert h[2] == sum(want_d)                       # (exact: dyadic numbers)
    assert rd.dtype == np.float32 and rc.dtype == np.float32
    rd = rd.reshape(3, 4)
    assert rd[1, 1] == 0 and np.isnan(rd[2, 3]) and rd[0, 3] == 1
    assert h[3] == 33                                # 36 components - the NaN pixel's 3
    d = np.full((3, 4, 3), f32(0.125))
    d[0, 0] = [0.5, 0.25, 0]
    want_c = np.abs((gc - rgb).astype(f32))
    assert (rc.reshape(3, 4, 3) == want_c).all()
    good = np.ones((3, 4), bool); good[2, 3] = False
    assert h[4] == (want_c[good].astype(np.float64) ** 2).sum()
    assert abs(h[4] - ((d[good].astype(np.float64)) ** 2).sum()) < 1e-6
    assert abs(iv.psnr(h) - (-10 * np.log10(h[4] / 33))) < 1e-12 and 15 < iv.psnr(h) < 19       # errors of 0.125: about 18 dB, less for the 0.5 pixel
    # a non-finite colour component drops the whole pixel (depth term included); +inf counts like NaN
    rgb2 = rgb.copy(); rgb2[0, 1, 2] = np.inf
    h2, _, _ = iv.metrics_ref(rgb2, depth, gt, gc)
    assert h2[5] == 2 and h2[1] == 9 and h2[3] == 30 and np.isfinite(h2).all()
    # absent ground truth: the corresponding sums and counts are zero
    h3, rd3, rc3 = iv.metrics_ref(rgb, depth, None, gc)
    assert h3[1] == 0 and h3[2] == 0 and rd3 is None and h3[3] == 33
    h4, rd4, rc4 = iv.metrics_ref(rgb, depth, gt, None)
    assert h4[3] == 0 and h4[4] == 0 and rc4 is None and h4[1] == 10


def test_frame_tells_the_depth_max_semantics_apart(oracle32, frame):
    """on the fp32 oracle alone: chunks of 200 pixels see another max(gt_depth) than the frame, and rendering with it moves the depth image by
    at least 1e-3 relative L2 -- ten times the 1e-4 contract, so a wrong maximum cannot hide under the tolerance"""
    gd_img = frame["depth"]
    zero = float((gd_img == 0).mean())
    assert 0.02 < zero < 0.20, zero
    assert (gd_img[9:14, 11:18] == 0).all()
    ro, rd, gd = iv.frame_rays(oracle32, frame)
    assert gd.tobytes() == gd_img.tobytes()
    gmax = float(gd.max())
    cmax = [float(gd[a:a + n].max()) for a, n in iv.chunk_ranges(gd.size, 200)]
    assert all((gd[a:a + n] == 0).any() for a, n in iv.chunk_ranges(gd.size, 200))          # every chunk holds pixels without a measurement
    assert max(abs(m - gmax) / gmax for m in cmax) > 0.01, (cmax, gmax)
    per_chunk = iv.oracle_render(oracle32, frame["scene"], "color", ro, rd, gd, 200)
    glob = iv.oracle_render(oracle32, frame["scene"], "color", ro, rd, gd, 768, gmax)
    e = scenes.rel_l2(per_chunk["depth"], glob["depth"])
    print("chunk maxima %s, frame maximum %.4f, zero-depth pixels %.3f, depth rel-L2 between the semantics %.3e" % (np.round(cmax, 4), gmax, zero, e))
    assert e >= 1e-3, e
    assert np.isfinite(per_chunk["depth"]).all() and np.isfinite(glob["rgb"]).all()
    # with the global maximum the chunking does not matter (the oracle renders rays independently given the maximum)
    glob200 = iv.oracle_render(oracle32, frame["scene"], "color", ro, rd, gd, 200, gmax)
    assert glob200["depth"].tobytes() == glob["depth"].tobytes()

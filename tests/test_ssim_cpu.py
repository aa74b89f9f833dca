"""CPU tests (-m "not gpu") of the structural-similarity rule (include/nsk.h: nsk_image_ssim): tests/ssim_checks.py's float64 restatement
against two independent forms of the published definition, the pooling against avg_pool2d, the exact identity, constant images, and
the entry point's presence in the header and in the built library.

The 1e-9 of the comparisons: about 50 roundings of 1.1e-16 on moments <= 1, divided by sx + sy + C2 >= 9e-4, give about 1e-11 on a map
value (1.8e-12 at worst was seen); 1e-9 leaves two orders of margin and is five orders below the error of the same arithmetic in fp32."""
import os
import re

import numpy as np
import pytest
import torch

import ssim_checks as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


@pytest.mark.parametrize("kind", sk.KINDS)
@pytest.mark.parametrize("shape", sk.SHAPES, ids=lambda s: "%dx%dx%d_w%d_l%d" % (s[0], s[1], s[2], s[3], s[5]))
def test_restatement_agrees_with_both_independent_forms(shape, kind):
    H, W, C, win, sigma, levels = shape
    a, b, r = sk.case(kind, shape)
    assert r["map"].shape == (H - win + 1, W - win + 1, C) and r["left_out"] == 0
    for name, form in (("torch", sk.torch_form), ("scipy", sk.scipy_form)):
        result, ssim0, map0 = form(a, b, win=win, sigma=sigma, levels=levels)
        e_map = float(np.abs(r["maps"][0][0] - map0).max())
        print("%s %s %s: map %.3g, ssim %.3g, result %.3g" % (shape, kind, name, e_map, abs(r["ssim"] - ssim0), abs(r["result"] - result)))
        assert e_map <= TOL and abs(r["ssim"] - ssim0) <= TOL and abs(r["result"] - result) <= TOL
    if levels == 1:
        assert r["result"] == r["ssim"]


def test_fp32_arithmetic_would_not_do():
    """the reason for fp64: the same arithmetic in float32 on the flat bright pair is wrong by far more than the tolerance above"""
    a, b, r = sk.case("flat", sk.SHAPES[4])
    g = sk.window(11, 1.5).astype(np.float32)
    C1, C2 = (np.float32(v) for v in sk.constants(1.0, 0.01, 0.03))
    s32, _ = sk.level_maps(a, b, g, C1, C2)
    assert s32.dtype == np.float32
    assert float(np.abs(s32.astype(np.float64) - r["maps"][0][0]).max()) > 1e-5


@pytest.mark.parametrize("kind", sk.KINDS)
def test_pooling_equals_avg_pool2d_bit_for_bit(kind):
    """161 x 176 -> 81 x 88 -> 41 x 44 -> 21 x 22 -> 11 x 11, every level of both images.  (The rule adds the rows' pair sums, avg_pool2d adds
    the four in row-major order; on pixels that began as float32 both sums are exact, so the bits agree.  On arbitrary doubles they need not.)"""
    for v in sk.case(kind, sk.SHAPES[4])[:2]:
        v = v.astype(np.float64)
        for want_hw in ((81, 88), (41, 44), (21, 22), (11, 11)):
            H, W = v.shape[:2]
            t = torch.tensor(v).permute(2, 0, 1)[None].contiguous()
            want = torch.nn.functional.avg_pool2d(t, kernel_size=2, padding=(H % 2, W % 2))[0].permute(1, 2, 0).numpy()
            v = sk.pool(v)
            assert v.shape == want.shape == want_hw + (3,)
            assert np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(want).tobytes()


def test_pooling_pads_odd_sides_with_zeros():
    v = np.arange(1.0, 16.0).reshape(5, 3, 1)
    got = sk.pool(v)[:, :, 0]
    assert got.shape == (3, 2)                              # (5 + 2) // 2, (3 + 2) // 2: the last padded row and column are not read
    assert got[0, 0] == 1.0 * 0.25 and got[0, 1] == (2.0 + 3.0) * 0.25 and got[1, 0] == (4.0 + 7.0) * 0.25
    assert got[2, 1] == ((11.0 + 12.0) + (14.0 + 15.0)) * 0.25


def test_pyramid_sizes():
    sizes = [(161, 176)]
    for _ in range(4):
        sizes.append(sk.pool(np.zeros(sizes[-1] + (1,))).shape[:2])
    assert sizes == [(161, 176), (81, 88), (41, 44), (21, 22), (11, 11)]


@pytest.mark.parametrize("kind", sk.KINDS)
@pytest.mark.parametrize("shape", sk.SHAPES, ids=lambda s: "%dx%dx%d_w%d_l%d" % (s[0], s[1], s[2], s[3], s[5]))
def test_identity_is_exactly_one(shape, kind):
    H, W, C, win, sigma, levels = shape
    for x in sk.case(kind, shape)[:2]:
        r = sk.restate(x, x, win=win, sigma=sigma, levels=levels)
        assert r["result"] == 1.0 and r["ssim"] == 1.0 and (r["map"] == np.float32(1)).all()
        assert all((s == 1.0).all() and (cs == 1.0).all() for s, cs in r["maps"])


@pytest.mark.parametrize("va,vb", [(0.25, 0.75), (0.999, 0.001), (0.0, 1.0), (0.5, 0.5)])
def test_constant_images(va, vb):
    a, b = np.full((23, 19, 2), va, np.float32), np.full((23, 19, 2), vb, np.float32)
    x, y = float(np.float32(va)), float(np.float32(vb))
    C1 = 0.01 ** 2
    want = (2 * x * y + C1) / (x * x + y * y + C1)
    r = sk.restate(a, b)
    assert np.abs(r["maps"][0][0] - want).max() <= TOL and abs(r["ssim"] - want) <= TOL


def test_non_finite_windows_are_left_out():
    a, b = (v.copy() for v in sk.case("noise", sk.SHAPES[3])[:2])
    a[20, 30, 1] = np.nan
    b[50, 10, 0] = np.inf
    r = sk.restate(a, b)
    bad = ~np.isfinite(r["maps"][0][0])
    assert r["left_out"] == int(bad.sum()) == 2 * 11 * 11 and bad[:, :, 2].sum() == 0
    assert np.isfinite(r["sums"]).all() and np.isfinite(r["result"])


def test_entry_point_is_declared_and_exported():
    import nice_slam_cpp_amd as pkg
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+nsk_image_ssim\s*\(", txt), "include/nsk.h does not declare nsk_image_ssim"
    pkg.build()
    assert hasattr(pkg.nsk.lib(), "nsk_image_ssim"), "libnsk.so does not export nsk_image_ssim"
    assert "nsk_image_ssim" in pkg.nsk.SYMBOLS and hasattr(pkg.Context, "image_ssim")

"""GPU tests of nsk_image_ssim (csrc/nsk_ssim.h): the device against tests/ssim_checks.py's float64 restatement -- the level-0 map and every
sum bytes for bytes, the host's combine within 1e-12 relative (only its pow and its division may differ) -- and against the torch
float64 form of the published definition within the 1e-9 tests/test_ssim_cpu.py derives.  Shapes: those of the CPU file, the edges of
the kernel's tile (SSIM_TILE = 8 x 32 windows per workgroup: a map of exactly one tile, one tile plus a row and a column, one window),
the pyramid with odd sizes at several levels, non-finite pixels, the identity, a rendered frame, the argument errors, the host program."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_views as iv
import rows_checks as rw
import scenes
import ssim_checks as sk
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
TILE_H, TILE_W = 8, 32                                     # csrc/nsk_ssim.h (test_tile_constants holds them to the header and the binding)
IDS = lambda s: "%dx%dx%d_w%d_l%d" % (s[0], s[1], s[2], s[3], s[5])


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def close(got, want, tol):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= tol * abs(want)


def check(ctx, a, b, r=None, torch_too=False, **kw):
    """one call against the restatement r (computed when not given): map, sums, counts, combine; a second call gives the same bytes"""
    if r is None:
        r = sk.restate(a, b, **kw)
    levels = kw.get("levels", 1)
    m = ctx.image_ssim(a, b, want_map=True, **kw)
    got_map = m["map"].cpu().numpy().reshape(r["map"].shape)
    h = m["per_level"]
    nan = np.isnan(r["map"])
    print("ssim %r (restated %r), result %r (restated %r), left out %d of %d" % (m["ssim"], r["ssim"], m["h_out"][0], r["result"], m["left_out"], r["windows"]))
    assert (np.isnan(got_map) == nan).all() and got_map[~nan].tobytes() == r["map"][~nan].tobytes()
    assert (rw.bits(h[:, :, :3]) == rw.bits(r["sums"])).all()
    assert close(m["h_out"][0], r["result"], 1e-12) and close(m["h_out"][1], r["ssim"], 1e-12)
    assert all(close(h[l, c, 3], r["h_levels"][l, c, 3], 1e-12) for l in range(levels) for c in range(h.shape[1]))
    assert m["left_out"] == r["left_out"] and m["h_out"][2] == r["windows"] - r["left_out"] and m["h_out"][4] == levels
    assert (m["h_out"][5], m["h_out"][6], m["h_out"][7]) == (r["map"].shape[0], r["map"].shape[1], 0.0)
    assert (m["ms_ssim"] is None) == (levels == 1) and (levels == 1 or close(m["ms_ssim"], r["result"], 1e-12))
    if torch_too:
        result, ssim0, _ = sk.torch_form(a, b, **kw)
        assert abs(m["h_out"][0] - result) <= 1e-9 and abs(m["h_out"][1] - ssim0) <= 1e-9
    m2 = ctx.image_ssim(a, b, want_map=True, **kw)                       # two runs, the same bytes
    assert m2["map"].cpu().numpy().tobytes() == m["map"].cpu().numpy().tobytes() and m2["per_level"].tobytes() == h.tobytes()
    assert m2["h_out"][:2] == m["h_out"][:2] or np.isnan(m["h_out"][0])
    return m, r


def test_tile_constants():
    import nice_slam_cpp_amd as pkg
    txt = open(os.path.join(ROOT, "nice-slam-cpp_amd", "csrc", "nsk_ssim.h")).read()
    hw = tuple(int(re.search(r"#define SSIM_TILE_%s (\d+)" % k, txt).group(1)) for k in "HW")
    assert hw == (TILE_H, TILE_W) == tuple(pkg.nsk.SSIM_TILE)


@pytest.mark.parametrize("kind", sk.KINDS)
@pytest.mark.parametrize("shape", sk.SHAPES, ids=IDS)
def test_shapes_and_kinds(ctx, shape, kind):
    H, W, C, win, sigma, levels = shape
    a, b, r = sk.case(kind, shape)
    m, _ = check(ctx, a, b, r, torch_too=True, win=win, sigma=sigma, levels=levels)
    assert m["left_out"] == 0 and m["map"].shape == (H - win + 1, W - win + 1, C)


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("hm,wm", [(TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (1, 1), (1, TILE_W + 1), (TILE_H + 1, 1), (2 * TILE_H, 2 * TILE_W)])
def test_tile_edges(ctx, hm, wm, C):
    """maps of exactly one tile, one tile plus one row and one column, one window, a row and a column of windows that cross a tile's edge, and
    exactly four tiles; 1 and 4 channels"""
    win = 11
    a, b = sk.make_pair("noise", hm + win - 1, wm + win - 1, C, seed=3)
    m, _ = check(ctx, a, b, torch_too=True, win=win)
    assert m["map"].shape == (hm, wm, C)


def test_two_dimensional_input_and_numpy_or_tensors(ctx):
    a, b = sk.make_pair("smooth", 30, 41, 1)
    r = sk.restate(a, b)
    for x, y in ((a[:, :, 0], b[:, :, 0]), (torch.tensor(a[:, :, 0]), cu(b[:, :, 0])), (cu(a).double(), torch.tensor(b))):
        m = ctx.image_ssim(x, y, want_map=True)
        assert m["map"].shape == ((20, 31) if x.ndim == 2 else (20, 31, 1)) and m["map"].cpu().numpy().tobytes() == r["map"].tobytes()
        assert (rw.bits(m["per_level"][:, :, :3]) == rw.bits(r["sums"])).all()
    assert ctx.image_ssim(a, b)["map"] is None


# ---- MS-SSIM ---------------------------------------------------------------------------------------------------------------------------
def test_ms_ssim_single_channel_odd_sizes(ctx):
    """161 -> 81 -> 41 -> 21 -> 11 on both sides: odd at every level, the last level a single window"""
    a, b = sk.make_pair("noise", 161, 161, 1)
    m, r = check(ctx, a, b, torch_too=True, levels=5)
    assert r["maps"][4][0].shape == (1, 1, 1) and m["per_level"][4, 0, 2] == 1.0
    assert sk.case("noise", sk.SHAPES[4])[2]["maps"][4][0].shape == (1, 1, 3)       # (161, 176, 3) of test_shapes_and_kinds as well


def test_ms_ssim_too_small_names_the_side_that_would_do(ctx):
    import nice_slam_cpp_amd as pkg
    a, b = sk.make_pair("noise", 160, 176, 3)
    with pytest.raises(pkg.NskError, match=r"\b161\b"):
        ctx.image_ssim(a, b, levels=5)
    with pytest.raises(pkg.NskError, match=r"\b161\b"):
        ctx.image_ssim(a.transpose(1, 0, 2), b.transpose(1, 0, 2), levels=5)


@pytest.mark.parametrize("kind", sk.KINDS)
def test_three_levels_with_caller_weights(ctx, kind):
    a, b = sk.case(kind, sk.SHAPES[3])[:2]
    check(ctx, a, b, torch_too=True, win=7, levels=3, weights=(0.2, 0.3, 0.5))


# ---- non-finite values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,win", [(1, 11), (3, 7)])
def test_non_finite_pixels_are_left_out_and_counted(ctx, levels, win):
    a, b = (v.copy() for v in sk.case("noise", sk.SHAPES[3])[:2])
    a[5, 7, 0], a[40, 33, 1], a[70, 2, 2] = np.nan, np.inf, -np.inf
    b[20, 60, 0], b[41, 34, 1], b[3, 3, 2] = np.inf, -np.inf, np.nan
    kw = dict(win=win, levels=levels, weights=None if levels == 1 else (0.3, 0.3, 0.4))
    m, r = check(ctx, a, b, **kw)
    assert 0 < m["left_out"] == r["left_out"] < r["windows"]
    assert np.isnan(r["map"]).sum() > 0 and np.isfinite(m["per_level"]).all() and np.isfinite(m["h_out"][0])
    # a channel without a finite window: NaN, and no error
    a[:, :, 1] = np.nan
    m, r = check(ctx, a, b, **kw)
    assert np.isnan(m["h_out"][0]) and np.isnan(m["ssim"]) and m["per_level"][0, 1, 2] == 0 and m["per_level"][0, 0, 2] > 0


# ---- identity and determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sk.SHAPES, ids=IDS)
def test_identity_is_exactly_one(ctx, shape):
    H, W, C, win, sigma, levels = shape
    for kind in sk.KINDS:
        x = sk.case(kind, shape)[1]
        m = ctx.image_ssim(x, x, win=win, sigma=sigma, levels=levels, want_map=True)
        assert m["h_out"][0] == 1.0 and m["ssim"] == 1.0 and bool((m["map"] == 1.0).all())
        assert (m["per_level"][:, :, 0] == m["per_level"][:, :, 2]).all() and (m["per_level"][:, :, 1] == m["per_level"][:, :, 2]).all()


# ---- after a render --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    fr = iv.make_frame()
    return dict(fr=fr, sc=fr["scene"], ctx=make_ctx(fr["scene"]), c2w=cu(fr["c2w"]), depth=cu(fr["depth"]), color=cu(fr["color"]))


def test_ssim_of_a_rendered_frame(env):
    c = env["ctx"]
    rgb, depth, var = c.render_image("color", (iv.H, iv.W), iv.INTR, env["c2w"], env["depth"], chunk_rays=200)
    m, r = check(c, rgb.cpu().numpy(), env["fr"]["color"], torch_too=True)
    assert m["map"].shape == (14, 22, 3) and m["left_out"] == 0 and -1.0 <= m["ssim"] <= 1.0
    got = c.image_ssim(rgb, env["color"])                               # device tensors, as a caller has them after the render
    assert got["h_out"] == m["h_out"]
    check(c, depth.cpu().numpy(), env["fr"]["depth"], data_range=float(env["fr"]["depth"].max()))       # a depth image is C = 1


@pytest.mark.parametrize("ride", [False, True])
def test_ssim_leaves_a_prepared_batch_intact(env, ride):
    """map_prepare -> image_ssim -> map_step gives the loss and outputs of map_prepare -> map_step, to the bit (the guarantee of
    nsk_render_image).  ride: another batch's step runs after the registration and carries the registered batch's sampling."""
    c = env["ctx"]
    rays = [scenes.make_rays(s, 256, env["sc"]["bound"]) for s in (21, 22)]
    dev = [{k: cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")} for r in rays]
    a, b = (cu(v) for v in sk.case("smooth", sk.SHAPES[4])[:2])
    want = sk.case("smooth", sk.SHAPES[4])[2]

    def run(ssim):
        c.zero_grads()
        out = (torch.zeros(256, 3, device="cuda"), torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda"))
        loss = torch.zeros(1, device="cuda")
        b0, b1 = dev
        c.map_prepare("color", b1["rays_o"], b1["rays_d"], b1["gt_depth"], -1.0, flags=1)
        if ride:
            c.map_step("color", b0["rays_o"], b0["rays_d"], b0["gt_depth"], b0["gt_color"], -1.0, 0.2, True, flags=1)
        m = c.image_ssim(a, b, levels=5) if ssim else None              # (the first one grows the call's workspace)
        c.map_step("color", b1["rays_o"], b1["rays_d"], b1["gt_depth"], b1["gt_color"], -1.0, 0.2, True, flags=1, loss=loss, outputs=out)
        c.sync()
        return loss, out, m
    same = lambda x, y: x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    l0, o0, _ = run(False)
    l1, o1, m = run(True)
    assert float(l0) > 0 and same(l0, l1) and all(same(o0[k], o1[k]) for k in range(3))
    assert (rw.bits(m["per_level"][:, :, :3]) == rw.bits(want["sums"])).all()
    c.zero_grads()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument_and_launch_nothing(ctx):
    import nice_slam_cpp_amd as pkg
    L = pkg.nsk.lib()
    a, b = (cu(v) for v in sk.make_pair("noise", 40, 50, 3))
    dmap = torch.full((30, 40, 3), 9.0, device="cuda")
    h, hl = (C.c_double * 8)(), (C.c_double * 96)()
    w3 = (C.c_double * 3)(0.2, 0.3, 0.5)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    err = lambda: L.nsk_last_error().decode()
    good = dict(ctx=ctx.h, Hv=40, Wv=50, C=3, a=a, b=b, win=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, levels=1, weights=None, out=h)

    def call(**kw):
        k = dict(good, **kw)
        return L.nsk_image_ssim(k["ctx"], k["Hv"], k["Wv"], k["C"], p(k["a"]), p(k["b"]), k["win"], k["sigma"], k["data_range"], k["k1"], k["k2"],
                                k["levels"], k["weights"], p(dmap), k["out"], hl)
    ctx.sync()
    torch.cuda.synchronize()
    ctx.profile_begin()
    assert call(ctx=None) != 0 and "ctx" in err()
    assert call(a=None) != 0 and "d_a" in err()
    assert call(b=None) != 0 and "d_b" in err()
    assert call(out=None) != 0 and "h_out" in err()
    for bad in (0, 5, -1):
        assert call(C=bad) != 0 and re.search(r"\bC = ", err()), bad
    for bad in (1, 10, 17, -3, 0):
        assert call(win=bad) != 0 and "win" in err(), bad
    for name in ("sigma", "data_range", "k1", "k2"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(**{name: bad}) != 0 and name in err(), (name, bad)
    assert call(Hv=10) != 0 and "Hv" in err()
    assert call(Wv=10) != 0 and "Wv" in err()
    for bad in (0, 9, -1):
        assert call(levels=bad) != 0 and "levels" in err(), bad
    for bad in (2, 3, 4, 6, 8):
        assert call(levels=bad) != 0 and "h_weights" in err(), bad
    assert call(levels=3, weights=w3) != 0 and "smaller than win" in err() and re.search(r"\b41\b", err())         # 40 -> 20 -> 10 < 11
    assert call(levels=5) != 0 and re.search(r"\b161\b", err())
    assert ctx.profile_end() == {}                          # nothing was launched
    # inside a capture (which records one small launch, so that the graph is not empty) the call is refused
    q, g, m, v = (torch.zeros(8, device="cuda") for _ in range(4))
    torch.cuda.synchronize()
    with torch.cuda.stream(ctx.tstream):
        ctx.graph_begin()
        try:
            ctx.adam_vector(q, g, m, v, 1e-3, 1)
            rc = call()
            msg = err()
        finally:
            ctx.graph_end()
    assert rc != 0 and "captured" in msg
    ctx.sync()
    assert bool((dmap == 9.0).all()), "a refused call wrote to the map"
    assert call() == 0 and h[5] == 30 and h[6] == 40 and bool((dmap != 9.0).all())      # and a good call follows, on the same context


# ---- the host program -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 5])
def test_cpp_eval_img_test_equals_image_ssim(ctx, tmp_path, levels):
    exe = os.path.join(HOST, "eval_img_test")
    if not os.path.exists(exe):
        pytest.fail("eval_img_test is not built (run __graft_entry__.build())")
    a, b = sk.case("smooth", sk.SHAPES[4])[:2]
    pa, pb = os.path.join(str(tmp_path), "a.npy"), os.path.join(str(tmp_path), "b.npy")
    np.save(pa, 2.0 * a); np.save(pb, 2.0 * b)
    r = subprocess.run([exe, pa, pb, str(levels), "2.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    m = ctx.image_ssim(2.0 * a, 2.0 * b, data_range=2.0, levels=levels)
    assert got["ssim"] == m["ssim"] and got["ms_ssim"] == m["ms_ssim"] and got["left_out"] == m["left_out"] == 0
    assert (got["Hm"], got["Wm"]) == (151, 166)

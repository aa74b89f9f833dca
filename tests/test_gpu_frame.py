"""GPU tests of the frame preparation: nsk_frame_prepare / Context.prepare_frames, nskh::FramePrep through host/test/frame_prep_test.
What the device must give, byte for byte, is tests/frame_checks.py's numpy restatement of the rule (tests/test_frame_cpu.py proves it)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import frame_checks as fc
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
F = np.float32
DIST8 = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633, 0.05, -0.11, 0.3]


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def raw(seed, n, Hc, Wc, Hd=None, Wd=None, floats=False):
    rng = np.random.default_rng(seed)
    Hd, Wd = Hd or Hc, Wd or Wc
    c = rng.integers(0, 256, size=(n, Hc, Wc, 3), dtype=np.uint8)
    d = rng.integers(0, 65536, size=(n, Hd, Wd), dtype=np.uint16)
    if floats:
        return rng.random((n, Hc, Wc, 3), dtype=F), (rng.random((n, Hd, Wd), dtype=F) * F(6)).astype(F)
    return c, d


def dev(a):
    if a is None:
        return None
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).cuda()          # the same bits
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, c, d, o, depth_size=None):
    return ctx.prepare_frames(dev(c), dev(d), (o["fx"], o["fy"], o["cx"], o["cy"]), o["dist"] or None, o["crop_size"], o["crop_edge"],
                              o["png_depth_scale"], o["scale"], o["swap_rb"], depth_size=depth_size)


def same(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes() and tuple(t.shape) == a.shape


def check(ctx, c, d, o):
    got_c, got_d, got_i, got_b = run(ctx, c, d, o)
    ref_c, ref_d, ref_i, ref_b = fc.prepare(c, d, o)
    assert same(got_c, ref_c), "colour differs in %d values" % int((got_c.cpu().numpy().view(np.uint32) != ref_c.view(np.uint32)).sum())
    assert same(got_d, ref_d)
    assert got_i.tobytes() == ref_i.tobytes() and got_b == ref_b
    return ref_c, ref_d, ref_i, ref_b


CASE1 = fc.tum_options(23, 31, crop_size=(17, 19), crop_edge=2)


def test_small_tum_case_three_frames(ctx):
    """23 x 31, five coefficients, crop_size (17, 19), edge 2: odd sizes, every row less than a wave"""
    c, d = raw(1, 3, 23, 31)
    ref_c, _, _, nb = check(ctx, c, d, CASE1)
    assert ref_c.shape == (3, 13, 15, 3)


def test_colour_resized_to_the_depth_size(ctx):
    """29 x 37 colour over 13 x 17 depth, crop_size, edge 1: S2 + S3 + S4"""
    c, d = raw(2, 2, 29, 37, 13, 17)
    o = fc.options(fx=15.0, fy=14.0, cx=8.2, cy=6.1, crop_size=(9, 11), crop_edge=1, png_depth_scale=1000.0)
    check(ctx, c, d, o)
    check(ctx, c, d, dict(o, crop_size=None))          # S2 + S4 alone


def test_eight_coefficients_float_inputs_swap(ctx):
    c, d = raw(3, 2, 23, 31, floats=True)
    o = fc.tum_options(23, 31, dist=DIST8, crop_size=(17, 19), crop_edge=2, swap_rb=True, png_depth_scale=1.0, scale=0.5)
    check(ctx, c, d, o)
    check(ctx, c, d, dict(o, dist=DIST8[:4], crop_size=None, crop_edge=0))      # four coefficients, S1 alone


def test_upsampling_and_an_output_of_width_one(ctx):
    c, d = raw(4, 2, 9, 11)
    check(ctx, c, d, fc.options(fx=9.0, fy=9.0, cx=5.0, cy=4.0, crop_size=(13, 17)))
    c, d = raw(5, 2, 2, 3)
    check(ctx, c, d, fc.options(fx=2.0, fy=2.0, cx=1.0, cy=1.0, crop_size=(7, 1)))


def test_everything_off(ctx):
    for H, W in ((1, 1), (5, 7)):
        c, d = raw(6 + H, 2, H, W)
        ref_c, ref_d, _, nb = check(ctx, c, d, fc.options(fx=3.0, fy=3.0, cx=0.5, cy=0.5, png_depth_scale=5000.0))
        assert ref_c.tobytes() == (c.astype(F) / F(255)).tobytes() and nb == 0


def test_every_byte_and_every_sixteenth_depth_value_convert_exactly(ctx):
    c = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 1, 256, 3)
    d = np.arange(0, 65536, 16, dtype=np.uint16).reshape(1, 64, 64)
    got_c, _, _, _ = run(ctx, c, None, fc.options())
    _, got_d, _, _ = run(ctx, None, d, fc.options(png_depth_scale=6553.5, scale=1.25))
    assert same(got_c, c.astype(F) / F(255))
    assert same(got_d, (d.astype(F) / F(6553.5)) * F(1.25))


def test_rows_across_wave_boundaries(ctx):
    c, d = raw(8, 2, 65, 130)
    check(ctx, c, d, fc.tum_options(65, 130, crop_size=None, crop_edge=0))
    check(ctx, c, d, fc.tum_options(65, 130, crop_size=(70, 129), crop_edge=1))


def test_coordinates_that_leave_the_image_and_non_finite_ones(ctx):
    c, d = raw(9, 2, 23, 31)
    # k4 = -1 puts the pole of the rational model on the circle r2 = 1, which passes through four pixels exactly (x, y multiples of 1 / 4):
    # there rad = num / 0 is infinite and 0 * rad is NaN; around the circle the coordinates leave the image, far from it they stay inside
    o = fc.options(fx=4.0, fy=4.0, cx=15.0, cy=11.0, dist=[0.05, 0.0, 0.01, -0.02, 0.0, -1.0, 0.0, 0.0])
    us, vs = fc.source_coords(23, 31, o["fx"], o["fy"], o["cx"], o["cy"], o["dist"])
    assert np.isnan(us).any() and np.isinf(us).any() and np.isnan(vs).any() and np.isinf(vs).any()
    _, _, _, nb = check(ctx, c, d, o)
    o2 = fc.tum_options(23, 31, dist=[4.0, 0.0, 0.1, 0.0], crop_size=(17, 19), crop_edge=1)
    _, _, _, nb2 = check(ctx, c, d, o2)
    assert 0 < nb < 2 * 23 * 31 and 0 < nb2 < 2 * 15 * 17


def test_one_tum_frame(ctx):
    c, d = raw(10, 1, 480, 640)
    ref_c, _, intr, nb = check(ctx, c, d, fc.tum_options())
    assert ref_c.shape == (1, 368, 496, 3)
    print("TUM frame: n_border %d of %d pixels" % (nb, 368 * 496))


def test_batch_equals_single_calls_and_two_runs_agree(ctx):
    c, d = raw(11, 3, 23, 31)
    gc, gd, _, gb = run(ctx, c, d, CASE1)
    gc2, gd2, _, gb2 = run(ctx, c, d, CASE1)
    assert torch.equal(gc, gc2) and torch.equal(gd, gd2) and gb == gb2
    tot = 0
    for k in range(3):
        sc, sd, _, sb = run(ctx, c[k:k + 1], d[k:k + 1], CASE1)
        assert torch.equal(sc[0], gc[k]) and torch.equal(sd[0], gd[k])
        tot += sb
    assert tot == gb


def test_colour_only_and_depth_only(ctx):
    c, d = raw(12, 2, 29, 37, 13, 17)
    o = fc.options(fx=15.0, fy=14.0, cx=8.2, cy=6.1, crop_size=(9, 11), crop_edge=1, png_depth_scale=1000.0)
    gc, gd, gi, _ = run(ctx, c, d, o)
    oc, none_d, ci, _ = run(ctx, c, None, o, depth_size=(13, 17))
    none_c, od, di, _ = run(ctx, None, d, o)
    assert none_d is None and none_c is None and torch.equal(oc, gc) and torch.equal(od, gd)
    assert ci.tobytes() == gi.tobytes()
    c, d = raw(13, 2, 23, 31)
    gc, gd, _, gb = run(ctx, c, d, CASE1)
    oc, _, _, ob = run(ctx, c, None, CASE1)
    _, od, _, db = run(ctx, None, d, CASE1)
    assert torch.equal(oc, gc) and torch.equal(od, gd) and ob == gb and db == 0


def test_errors_leave_the_outputs_untouched(ctx):
    import nice_slam_cpp_amd as pkg
    L = pkg.nsk.lib()
    err = lambda: L.nsk_last_error().decode()
    c, d = raw(14, 1, 23, 31)
    tc, td = dev(c), dev(d)
    out_c = torch.full((1, 23, 31, 3), 7.0, device="cuda")
    out_d = torch.full((1, 23, 31), 7.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    intr = (CASE1["fx"], CASE1["fy"], CASE1["cx"], CASE1["cy"])

    def call(o, Hc=23, Wc=31, Hd=23, Wd=31, ct=0, dt=1, n=1):
        nb = C.c_int(-5)
        return L.nsk_frame_prepare(ctx.h, C.byref(o), n, p(tc), ct, Hc, Wc, p(td), dt, Hd, Wd, p(out_c), p(out_d), C.byref(nb))
    FO = pkg.nsk.frame_opts
    for o, kw, word in ((FO(intr, fc.TUM_DIST, (17, 19), 9), {}, "crop_edge"),
                        (FO(intr, fc.TUM_DIST, None, 12), {}, "crop_edge"),
                        (FO(intr, [0.1, 0.2, 0.3]), {}, "n_dist"),
                        (FO(intr, fc.TUM_DIST), dict(Hd=13, Wd=17), "undistort"),
                        (FO(intr, None, (17, 0)), {}, "crop_size"),
                        (FO(intr), dict(ct=1), "color_type"),
                        (FO(intr), dict(dt=0), "depth_type"),
                        (FO(intr), dict(n=-1), "n = -1")):
        assert call(o, **kw) != 0 and word in err(), (word, err())
    ctx.sync()
    assert bool((out_c == 7.0).all()) and bool((out_d == 7.0).all())
    with pytest.raises(pkg.NskError):
        ctx.prepare_frames(tc, dev(raw(15, 1, 13, 17)[1]), intr, fc.TUM_DIST)
    # and the context still works
    check(ctx, c, d, CASE1)


def test_frame_prep_test_program(ctx, tmp_path):
    """host/test/frame_prep_test (nskh::FramePrep on a cam block from a YAML file) on the first case's arrays writes the bytes and the
    intrinsics Context.prepare_frames gives"""
    exe = os.path.join(HOST, "frame_prep_test")
    if not os.path.exists(exe):
        pytest.fail("frame_prep_test is not built (run __graft_entry__.build())")
    c, d = raw(1, 3, 23, 31)
    dd = str(tmp_path)
    np.save(os.path.join(dd, "color.npy"), c[0])
    np.save(os.path.join(dd, "depth.npy"), d[0])
    o = CASE1
    with open(os.path.join(dd, "cam.yaml"), "w") as f:
        f.write("cam:\n  H: 23\n  W: 31\n  fx: %r\n  fy: %r\n  cx: %r\n  cy: %r\n  png_depth_scale: 5000.0 #for depth image in png format\n"
                "  crop_edge: 2\n  crop_size: [17, 19]\n  distortion: [%s]\n" % (o["fx"], o["fy"], o["cx"], o["cy"], ", ".join(repr(v) for v in o["dist"])))
    r = subprocess.run([exe, dd, os.path.join(dd, "cam.yaml")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    gc, gd, gi, gb = run(ctx, c[:1], d[:1], o)
    pc, pd = np.load(os.path.join(dd, "prep_color.npy")), np.load(os.path.join(dd, "prep_depth.npy"))
    assert pc.dtype == np.float32 and pd.dtype == np.float32
    assert same(gc[0], pc) and same(gd[0], pd)
    assert (rep["H"], rep["W"], rep["n_border"]) == (13, 15, gb)
    assert [F(rep[k]) for k in ("fx", "fy", "cx", "cy")] == list(gi)


def test_prepare_rays_gathers_the_prepared_pixels():
    """nsk_prepare_rays on the prepared frame with intr_out: the ground truth it gathers is the restatement's pixel, and the ray
    through a pixel is the one nsk_rays_from_pixels gives for the moved intrinsics"""
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    c, d = raw(16, 1, 23, 31)
    gc, gd, gi, _ = run(ctx, c, d, CASE1)
    ref_c, ref_d, ref_i, _ = fc.prepare(c, d, CASE1)
    H, W = ref_d.shape[1:]
    cam = cu(np.array([1, 0, 0, 0, 0, 0, 0], F))
    intr = tuple(float(v) for v in gi)
    pr = ctx.prepare_rays([dict(depth=gd[0], color=gc[0], pose=cam, seed=5)], 128, (0, H, 0, W), intr)
    ctx.sync()
    pi, pj = pr["pix_i"].cpu().numpy(), pr["pix_j"].cpu().numpy()
    assert pr["gt_depth"].cpu().numpy().tobytes() == ref_d[0][pj, pi].tobytes()
    assert pr["gt_color"].cpu().numpy().tobytes() == np.ascontiguousarray(ref_c[0][pj, pi]).tobytes()
    ro, rd = ctx.rays_from_camera(pr["pix_i"], pr["pix_j"], tuple(float(v) for v in ref_i), cam)
    assert torch.equal(rd, pr["rays_d"]) and torch.equal(ro, pr["rays_o"])


def test_slam_loop_prepares_frames_when_the_cam_block_asks(tmp_path):
    """host/test/slam_loop on a three-frame synthetic TUM-layout sequence whose cam block carries a crop_size and a crop_edge: the frames go
    through nskh::FramePrep (the line it prints names the prepared camera, which is nsk_frame_plan's), the loop runs end to end, the losses
    are finite and the poses stay near the truth -- resizing with the intrinsics moved along and cutting the rim keep the geometry"""
    from test_gpu_host_cpp import NS_YAML
    from test_host_io import _png
    import nice_slam_cpp_amd as pkg
    exe = os.path.join(HOST, "slam_loop")
    if not os.path.exists(exe):
        pytest.fail("slam_loop is not built (run __graft_entry__.build())")
    seq = tmp_path / "tum"
    (seq / "rgb").mkdir(parents=True); (seq / "depth").mkdir()
    H, W, fx, fy, cx, cy = 48, 64, 40.0, 40.0, 32.0, 24.0
    bound = np.array([[-2.0, 2.0], [-1.5, 1.5], [-2.0, 2.2]], np.float32)
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    gts = []
    with open(seq / "rgb.txt", "w") as fr, open(seq / "depth.txt", "w") as fd, open(seq / "groundtruth.txt", "w") as fg:
        for i in range(3):
            t = 1.0 + 0.1 * i
            p_tum = np.eye(4); p_tum[:3, 3] = [0.02 * i, 0.01 * i, 0.015 * i]
            c2w = (p_tum @ flip).astype(np.float32)
            gts.append(c2w)
            depth = scenes.frame_depth_image(bound, c2w, H, W, fx, fy, cx, cy)
            jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            dirs = np.stack([(ii - cx) / fx, -(jj - cy) / fy, -np.ones_like(ii, dtype=np.float64)], -1) @ c2w[:3, :3].T.astype(np.float64)
            hit = c2w[:3, 3] + dirs * depth[..., None]
            col = np.clip(255 * (0.5 + 0.5 * np.sin(hit * np.array([1.3, 2.1, 0.7]))), 0, 255).astype(np.uint8)
            _png(str(seq / "rgb" / ("%.6f.png" % t)), col)
            _png(str(seq / "depth" / ("%.6f.png" % t)), np.round(depth * 5000).astype(np.uint16))
            fr.write("%.6f rgb/%.6f.png\n" % (t, t)); fd.write("%.6f depth/%.6f.png\n" % (t, t))
            fg.write("%.6f %.9g %.9g %.9g 0 0 0 1\n" % ((t,) + tuple(p_tum[:3, 3])))
    (seq / "bound.txt").write_text(" ".join("%g" % v for v in bound.reshape(-1)))
    ns, cf = tmp_path / "ns.yaml", tmp_path / "cf.yaml"
    ns.write_text(NS_YAML)
    cf.write_text("mapping:\n  pixels: 500\ncam:\n  H: %d\n  W: %d\n  fx: %g\n  fy: %g\n  cx: %g\n  cy: %g\n  crop_size: [42, 56]\n  crop_edge: 3\n"
                  % (H, W, fx, fy, cx, cy))
    out = tmp_path / "out"; out.mkdir()
    r = subprocess.run([exe, "tum", str(seq), str(ns), str(cf), str(out), "3", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "slam_loop ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    Hp, Wp, intr = pkg.nsk.frame_plan((H, W), (H, W), (fx, fy, cx, cy), None, (42, 56), 3)
    assert (Hp, Wp) == (36, 50)
    assert "frames are prepared on the device: 36 x 50, fx %.3f fy %.3f cx %.3f cy %.3f" % tuple(float(v) for v in intr) in r.stdout, r.stdout[:2000]
    est, gt = np.load(out / "est_poses.npy"), np.load(out / "gt_poses.npy")
    tl, ml = np.load(out / "track_loss.npy"), np.load(out / "map_loss.npy")
    assert est.shape == (3, 4, 4) and np.allclose(gt, np.stack(gts), atol=1e-5)
    assert np.isfinite(est).all() and np.isfinite(tl).all() and np.isfinite(ml).all() and (ml > 0).all() and (tl[1:] > 0).all()
    assert np.linalg.norm(est[:, :3, 3] - gt[:, :3, 3], axis=1).max() < 0.15

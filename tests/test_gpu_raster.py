"""GPU tests of the mesh depth views: nsk_mesh_depth, nsk_depth_pair_stats, nsk_depth_views, Context.recon_depth_l1 and
Mesher::eval_recon_depth.  The device's images must equal the numpy float32 restatement of the rule (tests/raster_checks.py, proved on
analytic scenes by tests/test_raster_cpu.py) on every pixel of every view, bit for bit, under every setting of the tuning keys."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import raster_checks as rk
from gpu_util import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
H, W, F = 48, 64, 40.0
CAM = (F, F, W / 2.0 - 0.5, H / 2.0 - 0.5)
DEFAULTS = {"raster_inline_max": 64, "raster_queue_cap": 1 << 18, "raster_load_first": 1}


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def cui(a):
    return cu(a, torch.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene(name):
    """(verts, tris, views) of the named scene"""
    if name == "sheet":
        v, t, _ = rk.sheet()
        return v, t, rk.sheet_views()
    if name == "floor":
        return rk.floor() + (np.stack([rk.look(), rk.look(rk.rot_x(0.5) @ rk.rot_y(0.8), (0.2, 0.3, 0.1))]),)
    if name == "room_inside":
        return rk.cube_room() + (rk.room_views_inside(),)
    if name == "room_outside":
        return rk.cube_room() + (rk.room_views_outside(),)
    if name == "blob33":
        return rk.blob() + (rk.orbit_views(33),)
    if name == "on_plane":              # vertices exactly on the camera plane (d = 0) of the identity view, one triangle wholly in it
        v = np.array([[0, 0, 0], [1, -1, -3], [-1, -1, -3], [0.5, 0.2, 0], [2, 1, -4], [-2, 1.5, -4], [1, 0, 0], [0, 1, 0]], np.float32)
        return v, np.array([[0, 1, 2], [3, 4, 5], [0, 6, 7]], np.int32), rk.look()[None]
    if name == "behind":
        v, t = rk.cube_room()
        return (v + np.float32([0, 0, 10])).astype(np.float32), t, rk.look()[None]
    if name == "hostile":               # a repeated index, collinear vertices, a NaN vertex, indices out of range
        v, t = rk.cube_room()
        v = np.concatenate([v, [[np.nan, 0, 0], [0, 0, -1], [0.5, 0.5, -1.5], [1, 1, -2]]]).astype(np.float32)
        t = np.concatenate([[[0, 0, 1], [9, 10, 11], [0, 1, 8], [0, 1, 12]], t, [[-1, 2, 3], [9, 9, 9]]]).astype(np.int32)
        return v, t, rk.room_views_inside()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, h=H, w=W, cam=CAM):
    v, t, views = scene(name)
    dep, skipped = rk.render(v, t, views, h, w, *cam)
    dep.setflags(write=False)
    return dep, skipped


def device(ctx, name, h=H, w=W, cam=CAM):
    v, t, views = scene(name)
    d = ctx.mesh_depth(cu(v), cui(t), views, h, w, *cam, want_skipped=True)
    return d.cpu().numpy(), ctx.last_skipped


def set_all(ctx, **kw):
    for k, val in {**DEFAULTS, **kw}.items():
        ctx.set_tuning(k, val)


@pytest.mark.parametrize("name", ["sheet", "floor", "room_inside", "room_outside", "blob33", "on_plane", "behind", "hostile"])
def test_images_equal_the_rule_bit_for_bit(ctx, name):
    want, want_skipped = reference(name)
    got, skipped = device(ctx, name)
    nd = int((bits(got) != bits(want)).sum())
    print("%s: %d views, %d of %d pixels hit, %d pixels differ, skipped %d" % (name, len(want), int((want > 0).sum()), want.size, nd, skipped))
    assert got.shape == want.shape and nd == 0 and skipped == want_skipped
    if name == "sheet":
        assert len(scene(name)[1]) == 3042 and (want[0] > 0).all()
    if name == "room_inside":
        assert (want > 0).all()
    if name == "behind":
        assert (want == 0).all()
    if name == "hostile":
        assert want_skipped == 2
    if name == "blob33":
        assert len(want) == 33 and (want[32] > 0).any()
    again, _ = device(ctx, name)
    assert (bits(again) == bits(got)).all()


@pytest.mark.parametrize("name", ["sheet", "floor", "room_inside"])
def test_every_tuning_gives_the_same_bytes(ctx, name):
    want, _ = reference(name)
    try:
        for kw in (dict(raster_inline_max=0), dict(raster_inline_max=1 << 30), dict(), dict(raster_inline_max=0, raster_queue_cap=4),
                   dict(raster_load_first=0), dict(raster_inline_max=7, raster_load_first=0)):
            set_all(ctx, **kw)
            got, _ = device(ctx, name)
            nd = int((bits(got) != bits(want)).sum())
            print("%s %s: %d pixels differ" % (name, kw, nd))
            assert nd == 0
    finally:
        set_all(ctx)


def test_image_that_is_no_multiple_of_the_tiles(ctx):
    cam = (35.0, 33.0, 26.0, 18.0)
    for name in ("blob33", "room_inside"):
        want, _ = reference(name, 37, 53, cam)
        got, _ = device(ctx, name, 37, 53, cam)
        assert got.shape[1:] == (37, 53) and (bits(got) == bits(want)).all()
    try:
        set_all(ctx, raster_inline_max=0)
        assert (bits(device(ctx, "room_inside", 37, 53, cam)[0]) == bits(reference("room_inside", 37, 53, cam)[0])).all()
    finally:
        set_all(ctx)


def test_marching_cubes_mesh(ctx):
    """the welded mesh of Context.extract_mesh on a small lattice: a sphere of radius 1.1 cut by the lattice's border"""
    n = 12
    g = np.linspace(-1.2, 1.2, n).astype(np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    vol = (np.float32(1.1) - np.sqrt(x * x + 1.3 * y * y + z * z)).astype(np.float32)
    origin = np.full(3, g[0], np.float32); step = np.full(3, g[1] - g[0], np.float32)
    verts, tris = ctx.extract_mesh(cu(vol), origin, step, 0.0)
    v, t = verts.cpu().numpy(), tris.cpu().numpy()
    assert 100 < len(t) <= 3200
    views = np.concatenate([rk.orbit_views(2, radius=3.0, seed=4), rk.look(None, (0.1, 0.0, 0.2))[None]])      # the last one from inside
    want, _ = rk.render(v, t, views, H, W, *CAM)
    got = ctx.mesh_depth(verts, tris, views, H, W, *CAM).cpu().numpy()
    print("marching cubes: %d triangles, %d pixels hit" % (len(t), int((want > 0).sum())))
    assert (want[2] > 0).all() and (want[0] > 0).any() and (bits(got) == bits(want)).all()


def test_empty_inputs(ctx):
    v, t = rk.cube_room()
    d = ctx.mesh_depth(cu(v), cui(t[:0]), rk.room_views_inside(), H, W, *CAM, want_skipped=True)
    assert d.shape == (3, H, W) and bool((d == 0).all()) and ctx.last_skipped == 0
    d = ctx.mesh_depth(cu(v), cui(t), np.zeros((0, 4, 4), np.float32), H, W, *CAM)
    assert d.shape == (0, H, W)
    bad = np.concatenate([t, [[0, 1, 99]]]).astype(np.int32)
    ctx.mesh_depth(cu(v), cui(bad), np.zeros((0, 4, 4), np.float32), H, W, *CAM, want_skipped=True)
    assert ctx.last_skipped == 1
    assert ctx.depth_pair_stats(d, d).shape == (0, 4)


def close(got, want):
    return np.abs(got - want) <= 1e-12 * np.abs(want)


def test_pair_stats(ctx):
    v, t = rk.cube_room()
    a = np.array(reference("room_outside")[0])                  # zeros where the room is missed
    views = scene("room_outside")[2]
    b, _ = rk.render((v * np.float32(0.9)).astype(np.float32), t, views, H, W, *CAM)
    assert (a == 0).any() and (b == 0).any() and ((a > 0) & (b == 0)).any()
    want = rk.pair_stats(a, b)
    got = ctx.depth_pair_stats(cu(a), cu(b))
    print(got, want)
    assert close(got[:, [0, 2]], want[:, [0, 2]]).all() and (got[:, [1, 3]] == want[:, [1, 3]]).all()
    assert (ctx.depth_pair_stats(cu(a), cu(b)) == got).all()
    # NaN and inf on either side, a 37 x 53 stack of 5 views
    rng = np.random.default_rng(2)
    a = rng.uniform(0, 4, (5, 37, 53)).astype(np.float32); b = rng.uniform(0, 4, (5, 37, 53)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = 0; b[rng.random(a.shape) < 0.2] = 0
    for arr, val in ((a, np.nan), (a, np.inf), (b, np.nan), (b, np.inf), (b, -np.inf)):
        arr[rng.random(arr.shape) < 0.03] = val
    want = rk.pair_stats(a, b)
    got = ctx.depth_pair_stats(cu(a), cu(b))
    assert np.isfinite(got).all() and close(got[:, [0, 2]], want[:, [0, 2]]).all() and (got[:, [1, 3]] == want[:, [1, 3]]).all()


def test_view_draw_on_the_device_box(ctx):
    v, _ = rk.cube_room()
    v = np.concatenate([v, [[np.nan, 50, 0], [np.inf, 0, 0]]]).astype(np.float32)
    w = ctx.depth_views(cu(v), 40, seed=9, shrink=0.6)
    assert (bits(ctx.last_box) == bits(rk.finite_box(v))).all()
    assert (bits(w) == bits(rk.draw_views(rk.finite_box(v), 40, 9, 0.6))).all()


N_VIEWS, SEED = 8, 3


def room_pair():
    gv, gt = rk.cube_room()
    return ((gv * np.float32(0.99)).astype(np.float32), gt), (gv, gt)


def test_recon_depth_l1(ctx):
    rec, gt = room_pair()
    m = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n_views=N_VIEWS, HW=(H, W), focal=F, seed=SEED)
    l1, n_used, restricted, st = rk.depth_l1(rec, gt, N_VIEWS, H, W, F, seed=SEED)
    print("depth L1 %.6f cm (restated %.6f), restricted %.6f cm, %d views used" % (m["depth_l1_cm"], l1, m["restricted_l1_cm"], m["n_used"]))
    assert m["n_used"] == n_used == N_VIEWS
    assert abs(m["depth_l1_cm"] - l1) <= 1e-12 * l1 and abs(m["restricted_l1_cm"] - restricted) <= 1e-12 * restricted
    assert close(m["stats"][:, [0, 2]], st[:, [0, 2]]).all() and (m["stats"][:, [1, 3]] == st[:, [1, 3]]).all()
    assert 0.5 < m["depth_l1_cm"] < 5.0
    # a cover no view reaches: no view is used
    none = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n_views=2, HW=(H, W), focal=F, seed=SEED, min_cover=1.5)
    assert none["n_used"] == 0 and np.isnan(none["depth_l1_cm"])


def write_ply(path, v, t):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t))).encode())
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        rec = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)]); rec["n"] = 3; rec["i"] = t
        f.write(rec.tobytes())


def test_host_class_gives_the_same_number(ctx, tmp_path):
    exe = os.path.join(HOST, "eval_depth_test")
    assert os.path.exists(exe), "build() makes host/eval_depth_test"
    rec, gt = room_pair()
    write_ply(str(tmp_path / "rec.ply"), *rec); write_ply(str(tmp_path / "gt.ply"), *gt)
    out = subprocess.run([exe, str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), str(N_VIEWS), str(H), str(W), str(F), str(SEED)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n_views=N_VIEWS, HW=(H, W), focal=F, seed=SEED)
    print(got["depth_l1_cm"], want["depth_l1_cm"])
    assert got["n_used"] == want["n_used"] == N_VIEWS
    assert abs(got["depth_l1_cm"] - want["depth_l1_cm"]) <= 1e-9 * want["depth_l1_cm"]
    assert abs(got["restricted_l1_cm"] - want["restricted_l1_cm"]) <= 1e-9 * want["restricted_l1_cm"]
    assert (np.asarray(got["w2c0"], np.float32) == want["w2c"][0].reshape(-1)).all()

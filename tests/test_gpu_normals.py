"""GPU tests of the vertex normals and the colouring along them (nsk_mesh_vertex_normals, nsk_normal_rays, nsk_mesh_vertex_colors, the
Mesher's color_method): the device against the numpy restatement of tests/normals_checks.py bytes for bytes, the colours against
render_forward and eval_points bytes for bytes, the PLY of host/normals_mesh_test against the Python binding."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_cull_checks as mcc
import normals_checks as nc
import raster_checks as rc
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
LENGTH = 0.1


def b32(a):
    return nc.bits32(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)


def same(a, b):
    return b32(a).tobytes() == b32(b).tobytes()


@pytest.fixture(scope="module")
def scene_ctx():
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    return make_ctx(sc), sc


@pytest.fixture(scope="module")
def spheres_mesh(scene_ctx):
    """the device's own mesh of the three spheres and the blob on the 40^3 lattice, as cuda tensors and as arrays"""
    ctx, _ = scene_ctx
    vt, tt = ctx.extract_mesh(cu(mcc.spheres_volume()), mcc.SPHERES_ORIGIN, mcc.SPHERES_STEP, 0.0)
    assert vt.shape[0] > 2000 and tt.shape[0] > 4000
    return vt, tt, vt.cpu().numpy(), tt.cpu().numpy()


def device_normals(ctx, v, t):
    n, info = ctx.mesh_vertex_normals(cu(v), cu(np.asarray(t).reshape(-1, 3), torch.int32), want_info=True)
    return n.cpu().numpy(), [info["left_out"], info["zero"], info["max_valence"], 0]


MESHES = {
    "sphere": nc.uv_sphere, "fan": nc.fan, "sheet": lambda: rc.sheet(40)[:2], "cube_room": rc.cube_room, "dirty": nc.dirty_mesh,
    "sphere_shuffled": lambda: (nc.uv_sphere()[0], nc.shuffled(nc.uv_sphere()[1])),
}


# ---- 1. the normals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_normals_equal_the_restatement_bytes_for_bytes(scene_ctx, name):
    ctx, _ = scene_ctx
    v, t = MESHES[name]()
    want, want_info = nc.vertex_normals(v, t)
    got, info = device_normals(ctx, v, t)
    assert info == want_info, (info, want_info)
    diff = (b32(got) != b32(want)).any(axis=1)
    assert not diff.any(), "%d of %d vertices differ, first %d" % (diff.sum(), len(v), int(np.nonzero(diff)[0][0]))
    if name == "dirty":
        assert info == nc.DIRTY_INFO
    if name == "fan":
        assert info[2] == 1000                              # the hub's list is longer than a workgroup


def test_normals_of_the_devices_own_mesh(scene_ctx, spheres_mesh):
    ctx, _ = scene_ctx
    vt, tt, v, t = spheres_mesh
    want, want_info = nc.vertex_normals(v, t)
    n, info = ctx.mesh_vertex_normals(vt, tt, want_info=True)
    assert [info["left_out"], info["zero"], info["max_valence"], 0] == want_info and want_info[0] == 0
    assert same(n, want)
    # (a surface through a lattice node leaves triangles without an area, and a few vertices named by such triangles alone)
    has = (want != 0).any(axis=1)
    assert has.sum() == len(v) - want_info[1] and want_info[1] < 0.01 * len(v)
    # wound towards free space: out of the balls
    centres = np.array([c for c, _ in mcc.SPHERES + (mcc.BLOB,)])
    near = centres[np.argmin(np.linalg.norm(v[:, None, :] - centres[None], axis=2), axis=1)]
    assert ((want * (v - near)).sum(axis=1) > 0)[has].all()


# ---- 2. determinism, empty inputs, errors -----------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [%r, %r]
import hashlib, numpy as np, torch
import nice_slam_cpp_amd as pkg
import mesh_cull_checks as mcc, normals_checks as nc
ctx = pkg.Context(0)
cu = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
v, t = nc.fan()
a = ctx.mesh_vertex_normals(cu(v), cu(t, torch.int32))
vt, tt = ctx.extract_mesh(cu(mcc.spheres_volume()), mcc.SPHERES_ORIGIN, mcc.SPHERES_STEP, 0.0)
b = ctx.mesh_vertex_normals(vt, tt)
print("DIGEST", hashlib.sha256(a.cpu().numpy().tobytes()).hexdigest(), hashlib.sha256(b.cpu().numpy().tobytes()).hexdigest())
"""


def test_two_runs_and_a_fresh_process_give_the_same_bytes(scene_ctx, spheres_mesh):
    ctx, _ = scene_ctx
    vt, tt, _, _ = spheres_mesh
    v, t = nc.fan()
    fv, ft = cu(v), cu(t, torch.int32)
    a1, b1 = ctx.mesh_vertex_normals(fv, ft).cpu().numpy(), ctx.mesh_vertex_normals(vt, tt).cpu().numpy()
    a2, b2 = ctx.mesh_vertex_normals(fv, ft).cpu().numpy(), ctx.mesh_vertex_normals(vt, tt).cpu().numpy()       # (the scratch is reused)
    assert a1.tobytes() == a2.tobytes() and b1.tobytes() == b2.tobytes()
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    da, db = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1:]
    assert da == hashlib.sha256(a1.tobytes()).hexdigest() and db == hashlib.sha256(b1.tobytes()).hexdigest()


def test_empty_inputs_and_errors_leave_the_context_usable(scene_ctx):
    import nice_slam_cpp_amd as pkg
    ctx, _ = scene_ctx
    v, t = nc.uv_sphere()
    want = nc.vertex_normals(v, t)[0]
    got, info = device_normals(ctx, v, np.zeros((0, 3), np.int32))
    assert info == [0, len(v), 0, 0] and (b32(got) == 0).all()
    got, info = device_normals(ctx, np.zeros((0, 3), np.float32), t)
    assert got.shape == (0, 3) and info == [len(t), 0, 0, 0]
    vt, nt = cu(v), cu(want)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(pkg.NskError, match="length"):
            ctx.normal_rays(vt, nt, bad)
        with pytest.raises(pkg.NskError, match="length"):
            ctx.mesh_vertex_colors(vt, nt, bad)
    with pytest.raises(pkg.NskError, match="chunk_rays"):
        ctx.mesh_vertex_colors(vt, nt, LENGTH, chunk_rays=1 << 30)
    with pytest.raises(pkg.NskError, match="chunk_rays"):
        ctx.mesh_vertex_colors(vt, None, LENGTH, chunk_rays=-5)
    assert ctx.mesh_vertex_colors(vt[:0], nt[:0], LENGTH, want_fallback=True)[1] == 0
    assert same(device_normals(ctx, v, t)[0], want)


# ---- 3. the rays ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0.1, 0.037])
def test_normal_rays_equal_the_restatement(scene_ctx, length):
    ctx, _ = scene_ctx
    v, t = nc.dirty_mesh()
    n = nc.vertex_normals(v, t)[0]
    n[3] = [np.nan, 0.0, 1.0]                                # a normal with a non-finite component: no ray either
    n[4] = [0.0, -0.0, 0.0]
    want = nc.normal_rays(v, n, length)
    assert want[3].sum() == len(v) - 8 and not want[3][[3, 4, 121, 122]].any()
    got = ctx.normal_rays(cu(v), cu(n), length)
    for g, w in zip(got[:3], want[:3]):
        assert same(g, w)
    assert (got[3].cpu().numpy() == want[3]).all()
    assert np.isnan(got[0].cpu().numpy()[122, 0])            # the NaN vertex's origin is the vertex


# ---- 4. / 5. the colours ----------------------------------------------------------------------------------------------------------
def clamp255(rgb):
    with np.errstate(invalid="ignore"):
        x = np.where(rgb > 0, np.minimum(rgb, np.float32(1)), np.float32(0)).astype(np.float32) * np.float32(255)
    return np.floor(x.astype(np.float64) + 0.5).astype(np.uint8)


@pytest.fixture(scope="module")
def scaled_mesh(scene_ctx, spheres_mesh):
    """the 40^3 mesh's vertices (inside [0, 2]^3) scaled into the middle 80 % of the scene's bound, their normals from the device"""
    ctx, sc = scene_ctx
    _, tt, v, _ = spheres_mesh
    lo, ext = sc["bound"][:, 0], sc["bound"][:, 1] - sc["bound"][:, 0]
    vs = (lo + ext * (np.float32(0.1) + np.float32(0.4) * v)).astype(np.float32)
    vt = cu(vs)
    nt = ctx.mesh_vertex_normals(vt, tt)
    return vt, nt, vs, nt.cpu().numpy()


def check_colors(ctx, v, n, **kw):
    """mesh_vertex_colors against render_forward on the restated rays where has_ray, against eval_points elsewhere -> (rgb, fallback)"""
    o, d, g, has = nc.normal_rays(v, n, LENGTH)
    ref = ctx.render_forward("color", cu(o), cu(d), cu(g), gt_depth_max=LENGTH, want_weights=False)[0].cpu().numpy()
    pts = ctx.eval_points("color", cu(v)).cpu().numpy()[:, :3]
    rgb, fb = ctx.mesh_vertex_colors(cu(v), cu(n), LENGTH, want_fallback=True, **kw)
    rgb = rgb.cpu().numpy()
    want = np.where(has[:, None] != 0, ref, pts)
    diff = (b32(rgb) != b32(want)).any(axis=1)
    assert not diff.any(), "%d of %d vertices differ (%d of them with a ray)" % (diff.sum(), len(v), int((diff & (has != 0)).sum()))
    assert fb == int((has == 0).sum())
    return rgb, fb, ref, pts


def test_colors_equal_render_forward_on_the_rays(scene_ctx, scaled_mesh):
    ctx, _ = scene_ctx
    _, _, vs, ns = scaled_mesh
    rgb, fb, ref, pts = check_colors(ctx, vs, ns)
    assert fb == int((ns == 0).all(axis=1).sum()) < 0.01 * len(vs) and np.isfinite(rgb).all()
    # the two methods are two different colours: the ray composites the field across the surface
    assert (b32(rgb) != b32(pts)).any(axis=1).mean() > 0.5


def test_colors_fall_back_to_the_point_query(scene_ctx):
    ctx, _ = scene_ctx
    v, t = nc.dirty_mesh()
    n, info = device_normals(ctx, v, t)
    rgb, fb, _, _ = check_colors(ctx, v, n)
    assert fb == info[1] == 6


def test_chunks_and_the_point_query_path(scene_ctx, scaled_mesh):
    ctx, _ = scene_ctx
    vt, nt, vs, _ = scaled_mesh
    a = ctx.mesh_vertex_colors(vt, nt, LENGTH)
    b = ctx.mesh_vertex_colors(vt, nt, LENGTH, chunk_rays=1000)
    assert same(a, b)
    pts = ctx.eval_points("color", vt)[:, :3]
    c, fb = ctx.mesh_vertex_colors(vt, None, LENGTH, want_fallback=True)
    assert same(c, pts) and fb == len(vs)
    d = ctx.mesh_vertex_colors(vt, None, LENGTH, chunk_rays=7)              # 7 rays' worth of samples per chunk of points
    assert same(d, pts)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def test_mesher_end_to_end(tmp_path):
    """host/normals_mesh_test on the reference-bound scene at resolution 48: with render_ray_along_normal and normals in the PLY, the normals
    and colours are the Python binding's on the file's own vertices and triangles; with direct_point_query and no normals the file is
    mesh_test's, byte for byte"""
    sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    exe, old = os.path.join(HOST, "normals_mesh_test"), os.path.join(HOST, "mesh_test")
    if not os.path.exists(exe) or not os.path.exists(old):
        pytest.fail("normals_mesh_test / mesh_test is not built (run __graft_entry__.build())")
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    out = os.path.join(d, "along.ply")
    r = subprocess.run([exe, d, out, "48", "render_ray_along_normal", "0.1", "1", "0.1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    pv, pn, pc, pt = nc.read_ply(out)
    assert rep["vertices"] == len(pv) > 10000 and rep["triangles"] == len(pt) and rep["method"] == "render_ray_along_normal"
    vt, tt = cu(pv), cu(pt, torch.int32)
    n, info = ctx.mesh_vertex_normals(vt, tt, want_info=True)
    assert same(n, pn) and info["left_out"] == 0 and info["zero"] == rep["without_normal"]
    rgb, fb = ctx.mesh_vertex_colors(vt, n, 0.1, want_fallback=True)
    assert fb == rep["fallback"] == rep["without_normal"]
    assert (pc == clamp255(rgb.cpu().numpy())).all()
    print("end to end: %d vertices, %d triangles, %d without a normal, most namings %d" % (len(pv), len(pt), info["zero"], info["max_valence"]))
    # the defaults: the file mesh_test writes
    out2 = os.path.join(d, "point.ply")
    r = subprocess.run([exe, d, out2, "48", "direct_point_query", "0.1", "0", "0.1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["fallback"] == len(pv)
    r = subprocess.run([old, "scene", d, "48", "1", "0.1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert open(out2, "rb").read() == open(os.path.join(d, "mesh.ply"), "rb").read()
    qv, qn, qc, qt = nc.read_ply(out2)
    assert qn is None and qv.tobytes() == pv.tobytes() and qt.tobytes() == pt.tobytes() and (qc != pc).any()

"""GPU tests of the mesh culling: the seen mask of a lattice (nsk_lattice_seen), the component filter (nsk_mesh_filter), Mesher::get_clean_mesh.
What they must give is computed by tests/mesh_cull_checks.py and tests/mesh_checks.py in numpy (tests/test_mesh_cull_cpu.py proves those helpers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_checks as mc
import mesh_cull_checks as cc
import scenes
from gpu_util import cu, make_ctx
from test_gpu_mesh import ORIGIN, STEP, noise_volume

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


@pytest.fixture(scope="module")
def scene():
    sc = cc.cull_scene(scenes.REF_BOUND)
    sc["want"] = {p: cc.seen_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], *p) for p in sc["params"]}
    return sc


def seen(ctx, sc, edge, trunc, ks=None, valid=None):
    ks = list(range(len(sc["depths"]))) if ks is None else ks
    d = cu(sc["depths"][ks]) if ks else torch.empty((0,) + sc["depths"].shape[1:], device="cuda")
    return ctx.lattice_seen(sc["origin"], sc["step"], sc["nx"], sc["ny"], sc["nz"], d, sc["intr"], sc["w2c"][ks], edge, trunc, valid)


# ---- 1. byte for byte -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge,trunc", [(0, 0.0), (0, 0.5), (3, 0.0), (3, 0.5)])
def test_seen_mask_equals_the_float32_rule_at_every_node(ctx, scene, edge, trunc):
    want = scene["want"][(edge, trunc)]
    valid, n_seen = seen(ctx, scene, edge, trunc)
    got = valid.cpu().numpy().reshape(-1)
    assert valid.shape == (scene["nz"], scene["ny"], scene["nx"]) and valid.dtype == torch.uint8
    print("edge %d trunc %.1f: %d nodes seen (rule: %d), %d differ" % (edge, trunc, n_seen, int(want.sum()), int((got != want).sum())))
    assert (got == want).all()
    assert n_seen == int(want.sum()) and set(np.unique(got).tolist()) <= {0, 1}


# ---- 2. accumulate ----------------------------------------------------------------------------------------------
def test_accumulate_batches_and_clear(ctx, scene):
    want = scene["want"][(0, 0.5)]
    one, n1 = seen(ctx, scene, 0, 0.5)
    valid = None
    for k in range(3):
        valid, n3 = seen(ctx, scene, 0, 0.5, [k], valid)
    assert (valid == one).all() and n3 == n1 == int(want.sum())
    # K = 0 without a mask to accumulate into clears; with one it keeps
    kept, nk = seen(ctx, scene, 0, 0.5, [], valid)
    assert (kept == one).all() and nk == n1
    junk = torch.full_like(one, 7)
    L = __import__("nice_slam_cpp_amd").nsk.lib()
    o = np.ascontiguousarray(scene["origin"], np.float32); s = np.ascontiguousarray(scene["step"], np.float32)
    n = C.c_longlong(-1)
    rc = L.nsk_lattice_seen(ctx.h, o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), scene["nx"], scene["ny"], scene["nz"], 0, None, 24, 32,
                            C.c_float(40), C.c_float(40), C.c_float(15.5), C.c_float(11.5), None, 0, C.c_float(0.5), 0, C.c_void_p(junk.data_ptr()), C.byref(n))
    assert rc == 0 and n.value == 0 and int(junk.sum()) == 0
    # onto all ones: stays all ones (any non-zero byte counts as set and comes back as 1)
    ones = torch.full_like(one, 1)
    ones, n_all = seen(ctx, scene, 0, 0.5, None, ones)
    assert bool((ones == 1).all()) and n_all == ones.numel()
    # more keyframes than one launch holds (32), poses repeated, the keyframe that sees most last: the union
    ks = [2] * 30 + [1] * 5 + [2] * 20 + [0] * 3
    many, nm = seen(ctx, scene, 0, 0.5, ks)
    assert len(ks) > 32 and (many == one).all() and nm == n1
    part, _ = seen(ctx, scene, 0, 0.5, [2] * 33 + [1])
    assert (part.cpu().numpy().reshape(-1) == cc.seen_f32(scene["pts"], scene["depths"][1:2], scene["intr"], scene["w2c"][1:2], 0, 0.5)).all()


# ---- 3. mask into extract ---------------------------------------------------------------------------------------
def test_seen_mask_as_valid_of_extract(ctx):
    """the noise volume of tests/test_gpu_mesh.py on its lattice, seen from a camera outside it: the mesh is what mesh_checks predicts for
    that mask"""
    vol = noise_volume()
    nz, ny, nx = vol.shape
    o, s = np.array(ORIGIN, np.float32), np.array(STEP, np.float32)
    ctr = o + 0.5 * s * np.array([nx - 1, ny - 1, nz - 1], np.float32)
    c2w = cc.look_at(ctr + np.array([-5.0, 0.4, 0.9]), ctr + np.array([0.0, 0.1, -0.2]), 0.03)
    depth = cc.depth_image(cc.IMG_H, cc.IMG_W, 4.0, 8.5)[None]
    valid, n_seen = ctx.lattice_seen(o, s, nx, ny, nz, cu(depth), cc.INTR, cc.w2c_of(c2w)[None], 0, 0.25)
    mask = valid.cpu().numpy()
    assert (mask.reshape(-1) == cc.seen_f32(mc.lattice_points(o, s, nx, ny, nz), depth, cc.INTR, cc.w2c_of(c2w)[None], 0, 0.25)).all()
    proc = mc.processed_cells(vol, mask)
    assert 0.05 < proc.mean() < 0.9, proc.mean()
    v, t = ctx.extract_mesh(cu(vol), o, s, 0.0, valid)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    keys = mc.check_vertices(v, vol, o, s, 0.0, mask, max_ulp=0)
    nb = mc.check_topology(t, keys, vol, mask)
    print("seen mask into extract: %d of %d nodes seen, %d vertices, %d triangles, %d border sides" % (n_seen, mask.size, len(v), len(t), nb))
    assert len(v) > 1000 and nb > 0


# ---- 4. the filter, exact ---------------------------------------------------------------------------------------
def filter_volumes():
    return {"noise level 0": (noise_volume(), ORIGIN, STEP, 0.0), "noise level 0.4": (noise_volume(), ORIGIN, STEP, 0.4),
            "spheres": (cc.spheres_volume(), cc.SPHERES_ORIGIN, cc.SPHERES_STEP, 0.0),
            "serpentine": (cc.serpentine_volume(), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0)}


def thresholds_between(area):
    """two min_area values between component areas: geometric means of neighbours a third and two thirds up the sorted list (with two
    distinct areas: between them, and half the smaller; with one: a quarter and a half of it)"""
    a = np.unique(area)
    if len(a) == 1:
        return [float(a[0]) / 4, float(a[0]) / 2]
    k0, k1 = (len(a) - 1) // 3, (2 * (len(a) - 1)) // 3
    if k0 == k1:
        return [float(a[0]) / 2, float(np.sqrt(a[0] * a[1]))]
    return [float(np.sqrt(a[k0] * a[k0 + 1])), float(np.sqrt(a[k1] * a[k1 + 1]))]


@pytest.mark.parametrize("name", ["noise level 0", "noise level 0.4", "spheres", "serpentine"])
def test_filter_equals_numpy_components_byte_for_byte(ctx, name):
    vol, origin, step, level = filter_volumes()[name]
    dv = cu(vol)
    v0, t0 = ctx.extract_mesh(dv, origin, step, level)
    v0, t0 = v0.cpu().numpy(), t0.cpu().numpy()
    base = cc.components(v0, t0)
    area = base["area"]
    th = thresholds_between(area)
    above = float(area.max()) * 2
    print("%s: %d vertices, %d triangles, %d components, areas %.4g .. %.4g, thresholds %s" % (name, len(v0), len(t0), base["n_components"], area.min(), area.max(), th))
    if name == "serpentine":
        assert base["n_components"] == 1 and len(t0) > 5000
    if name == "spheres":
        assert base["n_components"] == 4
    # conditions of the inputs (not tolerances of the code): no area near a threshold, the two largest apart
    assert cc.areas_clear_of(area, th + [above], largest_only=True)
    assert len(th) == 2 and th[0] != th[1]
    for min_area, largest in [(0.0, True), (th[0], False), (th[1], False), (0.0, False), (above, False)]:
        want = cc.components(v0, t0, min_area, largest)
        runs = []
        for _ in range(2):
            ctx.extract_mesh(dv, origin, step, level)
            v, t, nc, nk = ctx.filter_mesh(min_area, largest)
            runs.append((v.cpu().numpy(), t.cpu().numpy()))
            assert nc == want["n_components"] and nk == want["n_kept"], (min_area, largest, nc, nk, want["n_components"], want["n_kept"])
        v, t = runs[0]
        assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape == want["verts"].shape and t.shape == want["tris"].shape
        assert v.tobytes() == want["verts"].tobytes() and t.tobytes() == want["tris"].tobytes(), (min_area, largest)
        assert runs[1][0].tobytes() == v.tobytes() and runs[1][1].tobytes() == t.tobytes()
        if min_area == above:
            L = __import__("nice_slam_cpp_amd").nsk.lib()
            pv, pt = C.c_void_p(1), C.c_void_p(1)
            assert L.nsk_mesh_buffers(ctx.h, C.byref(pv), C.byref(pt)) == 0 and pv.value is None and pt.value is None
            assert len(v) == 0 and len(t) == 0 and nk == 0
            v2, t2, nc2, nk2 = ctx.filter_mesh(0.0, False)          # the empty mesh again: not an error, no components
            assert len(v2) == 0 and nc2 == 0 and nk2 == 0
        elif not largest and min_area > 0:
            assert 0 < nk < nc or nc == 1
    # filtering what is already filtered changes nothing
    ctx.extract_mesh(dv, origin, step, level)
    a = ctx.filter_mesh(th[1], False)
    b = ctx.filter_mesh(th[1], False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[2] == b[3] == a[3]


# ---- 5. errors --------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable(scene):
    import nice_slam_cpp_amd as pkg
    ctx = pkg.Context(0)                                    # a context of its own: no mesh extracted yet
    L = pkg.nsk.lib()
    err = lambda: L.nsk_last_error().decode()
    nv, nt, nc, nk = C.c_int(7), C.c_int(7), C.c_int(7), C.c_int(7)
    refs = [C.byref(x) for x in (nv, nt, nc, nk)]
    assert L.nsk_mesh_filter(ctx.h, C.c_float(0), 0, *refs) < 0 and "nsk_mesh_extract first" in err()
    vol = cu(noise_volume())
    v0, t0 = ctx.extract_mesh(vol, ORIGIN, STEP, 0.0)
    assert L.nsk_mesh_filter(ctx.h, C.c_float(0), 0, None, refs[1], refs[2], refs[3]) < 0 and "NULL" in err()
    assert L.nsk_mesh_filter(ctx.h, C.c_float(0), 0, refs[0], refs[1], refs[2], None) < 0 and "NULL" in err()
    assert L.nsk_mesh_filter(ctx.h, C.c_float(float("nan")), 0, *refs) < 0 and "NaN" in err()
    assert L.nsk_mesh_filter(None, C.c_float(0), 0, *refs) < 0
    v, t, ncomp, nkept = ctx.filter_mesh(0.0, False)        # nothing was touched by the failed calls
    assert torch.equal(v, v0) and torch.equal(t, t0) and ncomp == nkept > 1
    sc = scene
    o = np.ascontiguousarray(sc["origin"], np.float32); s = np.ascontiguousarray(sc["step"], np.float32)
    op, sp = o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)
    d = cu(sc["depths"]); w = np.ascontiguousarray(sc["w2c"].reshape(3, 16)); wp = w.ctypes.data_as(C.c_void_p)
    valid = torch.full((sc["nz"], sc["ny"], sc["nx"]), 9, dtype=torch.uint8, device="cuda")
    n = C.c_longlong(-1)
    f = C.c_float

    def call(nx=sc["nx"], ny=sc["ny"], nz=sc["nz"], K=3, dp=C.c_void_p(d.data_ptr()), H=24, W=32, wq=wp, edge=0, vp=C.c_void_p(valid.data_ptr()), org=op):
        return L.nsk_lattice_seen(ctx.h, org, sp, nx, ny, nz, K, dp, H, W, f(40), f(40), f(15.5), f(11.5), wq, edge, f(0.5), 0, vp, C.byref(n))
    assert call(vp=None) < 0 and "d_valid is NULL" in err()
    assert call(dp=None) < 0 and "NULL" in err()
    assert call(wq=None) < 0 and "NULL" in err()
    assert call(org=None) < 0 and "null" in err()
    assert call(H=0) < 0 and "image" in err()
    assert call(W=-3) < 0 and "image" in err()
    assert call(K=-1) < 0 and call(edge=-1) < 0 and "edge" in err()
    assert call(nx=1 << 10, ny=1 << 10, nz=(1 << 8) + 1) < 0 and "at most" in err()
    assert call(nx=0) < 0
    assert int((valid != 9).sum()) == 0, "a refused call wrote to the mask"
    # an edge that leaves no pixel is valid: nothing is seen
    assert call(edge=16) == 0 and n.value == 0 and int(valid.sum()) == 0
    assert call(edge=2 ** 31 - 1) == 0 and n.value == 0
    # and a good call follows
    assert call() == 0 and n.value == int(sc["want"][(0, 0.5)].sum())
    assert (valid.cpu().numpy().reshape(-1) == sc["want"][(0, 0.5)]).all()


# ---- 6. C++ -----------------------------------------------------------------------------------------------------
def test_clean_mesh_cpp_equals_the_python_path(tmp_path):
    """Mesher::get_clean_mesh on the small scene with two synthetic keyframes against eval_lattice -> lattice_seen -> extract_mesh -> filter_mesh
    -> eval_points (color) here: the PLY parses back to the same arrays; seen nodes, components and kept components match"""
    exe = os.path.join(HOST, "clean_mesh_test")
    if not os.path.exists(exe):
        pytest.fail("clean_mesh_test is not built (run __graft_entry__.build())")
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    ks = cc.mesher_scene(sc["bound"])
    n, pad = cc.MESHER_N, np.float32(cc.MESHER_PAD)
    b = sc["bound"]
    lo, hi = (b[:, 0] - pad).astype(np.float32), (b[:, 1] + pad).astype(np.float32)
    origin, step = lo, ((hi - lo) / np.float32(n - 1)).astype(np.float32)
    assert (origin == ks["origin"]).all() and (step == ks["step"]).all()
    vol = ctx.eval_lattice("fine", origin, step, n, n, n)
    valid, n_seen = ctx.lattice_seen(origin, step, n, n, n, cu(ks["depths"]), ks["intr"], ks["w2c"], 0, 0.5)
    assert (valid.cpu().numpy().reshape(-1) == cc.seen_f32(ks["pts"], ks["depths"], ks["intr"], ks["w2c"], 0, 0.5)).all()
    v0, t0 = ctx.extract_mesh(vol, origin, step, 0.0, valid)
    base = cc.components(v0.cpu().numpy(), t0.cpu().numpy())
    th = thresholds_between(base["area"])[1]
    assert base["n_components"] > 2 and cc.areas_clear_of(base["area"], [th], largest_only=True)
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    np.save(os.path.join(d, "depths.npy"), ks["depths"].astype(np.float32))
    np.save(os.path.join(d, "c2ws.npy"), ks["c2w"].astype(np.float32))
    np.save(os.path.join(d, "intr.npy"), np.array(ks["intr"], np.float32))
    for min_area, largest, color in ((th, 0, 1), (0.0, 1, 0)):
        ctx.extract_mesh(vol, origin, step, 0.0, valid)       # (the driver inverts the float32 c2w in double: ks["w2c"])
        v, t, nc, nk = ctx.filter_mesh(min_area, bool(largest))
        want = cc.components(v0.cpu().numpy(), t0.cpu().numpy(), min_area, bool(largest))
        r = subprocess.run([exe, d, str(n), str(color), "0.1", repr(float(np.float32(min_area))), str(largest)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "clean_mesh_test ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
        m = re.search(r"ok: (\d+) vertices, (\d+) triangles, (\d+) components, (\d+) kept, (\d+) seen", r.stdout)
        assert [int(x) for x in m.groups()] == [len(v), len(t), nc, nk, n_seen], (r.stdout, len(v), len(t), nc, nk, n_seen)
        pv, pc, pf = mc.read_ply(os.path.join(d, "clean_mesh.ply"))
        assert pv.tobytes() == v.cpu().numpy().tobytes() and pf.tobytes() == t.cpu().numpy().tobytes()
        assert 0 < nk < nc and len(v) > 0
        assert pv.tobytes() == want["verts"].tobytes() and pf.tobytes() == want["tris"].tobytes()
        if color:
            rgb = ctx.eval_points("color", v).cpu().numpy()[:, :3]
            with np.errstate(invalid="ignore"):
                x = np.where(rgb > 0, np.minimum(rgb, np.float32(1)), np.float32(0)).astype(np.float32) * np.float32(255)
            assert (pc == np.floor(x.astype(np.float64) + 0.5).astype(np.uint8)).all()
        else:
            assert pc is None


def test_clean_mesh_cpp_streams_more_keyframes_than_a_batch(tmp_path):
    """17 keyframes cross the 16-frame batch of Mesher::get_clean_mesh on a 24^3 lattice: sixteen views from outside, no two alike, and,
    alone in the second batch, the view from inside.  Each batch sees nodes the other does not (a condition of the input), and the PLY
    and the counts are those of the Python path, whose result does not depend on its own batch (test_accumulate_batches_and_clear)."""
    exe = os.path.join(HOST, "clean_mesh_test")
    if not os.path.exists(exe):
        pytest.fail("clean_mesh_test is not built (run __graft_entry__.build())")
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    n, pad = 24, np.float32(0.1)
    ks = cc.cull_scene(sc["bound"], (n,) * 3, float(pad), keyframes=(0, 1), params=((0, 0.5),))
    tr = cc.long_trajectory(ks, [0] * 16 + [1])
    b = sc["bound"]
    lo, hi = (b[:, 0] - pad).astype(np.float32), (b[:, 1] + pad).astype(np.float32)
    origin, step = lo, ((hi - lo) / np.float32(n - 1)).astype(np.float32)          # the Mesher's own expressions
    seen_of = lambda sl: ctx.lattice_seen(origin, step, n, n, n, cu(tr["depths"][sl]), ks["intr"], tr["w2c"][sl], 0, 0.5)
    valid, n_seen = seen_of(slice(None))
    n_first, n_last = seen_of(slice(0, 16))[1], seen_of(slice(16, 17))[1]
    print("17 keyframes: %d nodes seen, %d by the first batch alone, %d by the second alone" % (n_seen, n_first, n_last))
    assert len(tr["w2c"]) == 17 and 0 < n_first < n_seen and 0 < n_last < n_seen
    vol = ctx.eval_lattice("fine", origin, step, n, n, n)
    ctx.extract_mesh(vol, origin, step, 0.0, valid)
    v, t, nc, nk = ctx.filter_mesh(0.0, False)
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    np.save(os.path.join(d, "depths.npy"), tr["depths"])
    np.save(os.path.join(d, "c2ws.npy"), tr["c2w"].astype(np.float32))
    np.save(os.path.join(d, "intr.npy"), np.array(ks["intr"], np.float32))
    r = subprocess.run([exe, d, str(n), "0", "0.1", "0.0", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "clean_mesh_test ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"ok: (\d+) vertices, (\d+) triangles, (\d+) components, (\d+) kept, (\d+) seen", r.stdout)
    assert [int(x) for x in m.groups()] == [len(v), len(t), nc, nk, n_seen], (r.stdout, len(v), len(t), nc, nk, n_seen)
    pv, pc, pf = mc.read_ply(os.path.join(d, "clean_mesh.ply"))
    assert len(v) > 0 and pc is None
    assert pv.tobytes() == v.cpu().numpy().tobytes() and pf.tobytes() == t.cpu().numpy().tobytes()

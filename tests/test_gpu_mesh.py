"""GPU tests of the mesh extraction (nsk_eval_lattice, nsk_mesh_extract, Mesher).  Every property of a mesh is computed by
tests/mesh_checks.py from the VOLUME alone: nothing here reads the library's case table."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_checks as mc
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def small_ctx():
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    return make_ctx(sc), sc


@pytest.fixture(scope="module")
def bare_ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def extract(ctx, vol, origin, step, level, valid=None):
    v, t = ctx.extract_mesh(cu(vol), origin, step, level, None if valid is None else cu(valid, torch.uint8))
    return v.cpu().numpy(), t.cpu().numpy()


# ---- 1. lattice evaluation --------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["coarse", "middle", "fine"])
def test_eval_lattice_equals_eval_points_bit_for_bit(small_ctx, stage):
    """a lattice that sticks out of the bound on every side, node counts that are multiples neither of 16 nor of the slab, walked in one
    slab (automatic) and in five slabs of 5000 nodes (tuning key "lattice_slab"): channel 3 of eval_points on the numpy float32 lattice"""
    ctx, sc = small_ctx
    b = sc["bound"]
    nx, ny, nz = 37, 23, 29
    origin = (b[:, 0] - np.float32(0.3)).astype(np.float32)
    step = ((b[:, 1] - b[:, 0] + np.float32(0.6)) / np.array([nx - 1, ny - 1, nz - 1], np.float32)).astype(np.float32)
    pts = mc.lattice_points(origin, step, nx, ny, nz)
    want = ctx.eval_points(stage, cu(pts))[:, 3].cpu().numpy().reshape(nz, ny, nx)
    inb = ((pts > b[:, 0]) & (pts < b[:, 1])).all(axis=1).reshape(nz, ny, nx)
    assert inb.any() and (~inb).any() and (want[~inb] == 100.0).all() and (want[inb] != 100.0).any()
    for axis in range(3):                                # outside on both sides of every axis
        assert not inb.take(0, axis=axis).any() and not inb.take(-1, axis=axis).any()
    for slab in (0, 5000):
        ctx.set_tuning("lattice_slab", slab)
        got = ctx.eval_lattice(stage, origin, step, nx, ny, nz).cpu().numpy()
        ndiff = int((bits(got) != bits(want)).sum())
        print("stage %s slab %d: %d of %d nodes differ" % (stage, slab, ndiff, got.size))
        assert ndiff == 0
    ctx.set_tuning("lattice_slab", 0)
    if stage == "fine":
        assert (bits(ctx.eval_lattice("color", origin, step, nx, ny, nz).cpu().numpy()) == bits(want)).all()


# ---- 2 / 3. vertices and topology ------------------------------------------------------------------------------
def noise_volume(seed=11, shape=(33, 31, 35)):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def hostile_volume(level, seed=12, shape=(27, 30, 25)):
    """noise with plateaus exactly on the level, +-inf, NaN and a random validity mask"""
    rng = np.random.default_rng(seed)
    vol = rng.standard_normal(shape).astype(np.float32)
    r = rng.random(shape)
    vol[r < 0.15] = np.float32(level)
    vol[2:9, 3:7, 4:12] = np.float32(level)               # a block of cells that lie on the level entirely
    vol[(r > 0.15) & (r < 0.17)] = np.inf
    vol[(r > 0.17) & (r < 0.19)] = -np.inf
    vol[(r > 0.19) & (r < 0.21)] = np.nan
    valid = (rng.random(shape) < 0.93).astype(np.uint8)
    return vol, valid


ORIGIN, STEP = (-1.3, 0.7, 2.1), (0.1, 0.037, 0.25)


def test_noise_volume_vertices_and_topology(bare_ctx):
    """Vertex bijection and positions: the roundings are pinned (t = (level - v0) / (v1 - v0), p0 + t * (p1 - p0), node = origin + i * step:
    every operation an fp32 operation of its own, no FMA), so the positions are asserted BIT-EQUAL to the numpy float32 formula (0 ulp),
    not merely within 1 ulp.  Topology per mesh_checks.check_topology.  All 256 cases occur in this volume."""
    vol = noise_volume()
    for level in (0.0, 0.4):
        cases = mc.cell_cases(vol, level, mc.processed_cells(vol))
        assert len(np.unique(cases)) == 256
        v, t = extract(bare_ctx, vol, ORIGIN, STEP, level)
        keys = mc.check_vertices(v, vol, ORIGIN, STEP, level, max_ulp=0)
        nb = mc.check_topology(t, keys, vol)
        print("noise level %.1f: %d vertices, %d triangles, %d border sides" % (level, len(v), len(t), nb))
        assert nb > 0 and t.dtype == np.int32 and v.dtype == np.float32


def test_plateaus_nonfinite_and_valid_mask(bare_ctx):
    level = 0.25
    vol, valid = hostile_volume(level)
    proc = mc.processed_cells(vol, valid)
    assert 0.2 < proc.mean() < 0.9 and (vol == np.float32(level)).mean() > 0.1
    for msk in (valid, None):
        v, t = extract(bare_ctx, vol, ORIGIN, STEP, level, msk)
        keys = mc.check_vertices(v, vol, ORIGIN, STEP, level, msk, max_ulp=0)
        nb = mc.check_topology(t, keys, vol, msk)
        print("hostile volume, mask %s: %d vertices, %d triangles, %d border sides" % (msk is not None, len(v), len(t), nb))
        assert len(v) > 1000 and nb > 0


def test_level_outside_the_value_range(bare_ctx):
    vol = noise_volume()
    for level in (1e9, -1e9):
        v, t = extract(bare_ctx, vol, ORIGIN, STEP, level)
        assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = extract(bare_ctx, vol, ORIGIN, STEP, 0.0)           # the context goes on working
    assert len(v) > 0


# ---- 4. analytic surfaces ---------------------------------------------------------------------------------------
def sampled(fn, origin, step, n):
    """fn at the float32 lattice nodes, evaluated in float64, cast to float32"""
    cx, cy, cz = [c.astype(np.float64) for c in mc.lattice_coords(origin, step, (n, n, n))]
    return fn(cx[None, None, :], cy[None, :, None], cz[:, None, None]).astype(np.float32)


def test_sphere_converges_at_second_order(bare_ctx):
    """value = r - |p - c|, r = 0.8, spacings h = 0.1, 0.05, 0.025.  Closed, Euler characteristic 2, signed volume positive (winding).
    Every vertex within h^2 / (8 (r - h)) of the sphere radially, plus the fp32 margin 16 * 2^-24 = 9.5e-7 (coordinates below 1.1 in
    magnitude, a handful of fp32 operations; measured between the float32 numpy restatement and a float64 one of the same vertices:
    3.5e-8 at most).  |V - 4/3 pi r^3| <= 4 pi (r + e)^2 (e + 3 h^2 / (8 (r - h))), e the vertex bound.
    Measured (printed by the test, not gated): max radial error 1.547e-3 / 3.897e-4 / 9.743e-5 against bounds 1.787e-3 / 4.176e-4 /
    1.018e-4, ratios 3.97 and 4.00 per halving; volume error 2.000e-2 / 5.013e-3 / 1.254e-3 against bounds 5.77e-2 / 1.34e-2 / 3.25e-3,
    ratios 3.99 and 4.00 (second order predicts 4)."""
    r, c = 0.8, np.array([0.05, -0.02, 0.03])
    fn = lambda x, y, z: r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    prev = None
    for h in (0.1, 0.05, 0.025):
        n = int(round(2.0 / h)) + 1
        origin, step = (-1.0, -1.0, -1.0), (h, h, h)
        hh = float(np.float32(h))
        vol = sampled(fn, origin, step, n)
        v, t = extract(bare_ctx, vol, origin, step, 0.0)
        keys = mc.check_vertices(v, vol, origin, step, 0.0, max_ulp=0)
        assert mc.check_topology(t, keys, vol) == 0, "the sphere's mesh is not closed"
        assert mc.euler_characteristic(t, len(v)) == 2
        e = hh * hh / (8 * (r - hh)) + 16 * 2.0 ** -24
        rad = np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - r).max()
        vol_mesh = mc.signed_volume(v, t)
        dv = abs(vol_mesh - 4.0 / 3.0 * np.pi * r ** 3)
        dv_max = 4 * np.pi * (r + e) ** 2 * (e + 3 * hh * hh / (8 * (r - hh)))
        line = "sphere h %.3f: %d vertices, radial error %.3e (bound %.3e), volume error %.3e (bound %.3e)" % (h, len(v), rad, e, dv, dv_max)
        if prev:
            line += ", ratios %.2f %.2f" % (prev[0] / rad, prev[1] / dv)
        print(line)
        prev = (rad, dv)
        assert vol_mesh > 0, "normals point inwards"
        assert rad <= e
        assert dv <= dv_max


def test_torus_and_two_spheres(bare_ctx):
    h, n = 0.05, 41
    origin, step = (-1.0, -1.0, -1.0), (h, h, h)
    torus = lambda x, y, z: 0.22 - np.sqrt((np.sqrt((x - 0.01) ** 2 + (y + 0.02) ** 2) - 0.6) ** 2 + (z - 0.013) ** 2)
    two = lambda x, y, z: np.maximum(0.3 - np.sqrt((x + 0.45) ** 2 + y ** 2 + z ** 2), 0.35 - np.sqrt((x - 0.5) ** 2 + (y - 0.1) ** 2 + (z + 0.2) ** 2))
    both = lambda x, y, z: np.maximum(0.2 - np.sqrt((np.sqrt(x ** 2 + y ** 2) - 0.7) ** 2 + z ** 2), 0.25 - np.sqrt(x ** 2 + y ** 2 + (z - 0.02) ** 2))
    for name, fn, chi in (("torus", torus, 0), ("two spheres", two, 4), ("torus around a sphere", both, 2)):
        vol = sampled(fn, origin, step, n)
        v, t = extract(bare_ctx, vol, origin, step, 0.0)
        keys = mc.check_vertices(v, vol, origin, step, 0.0, max_ulp=0)
        assert mc.check_topology(t, keys, vol) == 0
        assert mc.euler_characteristic(t, len(v)) == chi, name
        assert mc.signed_volume(v, t) > 0


# ---- 5. determinism -------------------------------------------------------------------------------------------
CHILD = """
import sys
sys.path[:0] = [%r, %r]
import hashlib, numpy as np, torch
import nice_slam_cpp_amd as pkg
from test_gpu_mesh import hostile_volume, ORIGIN, STEP
vol, valid = hostile_volume(0.25)
ctx = pkg.Context(0)
v, t = ctx.extract_mesh(torch.tensor(vol, device="cuda"), ORIGIN, STEP, 0.25, torch.tensor(valid, device="cuda"))
print("DIGEST", hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest(), hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest())
"""


def test_two_runs_and_a_fresh_process_give_the_same_bytes(bare_ctx):
    vol, valid = hostile_volume(0.25)
    v1, t1 = extract(bare_ctx, vol, ORIGIN, STEP, 0.25, valid)
    extract(bare_ctx, noise_volume(), ORIGIN, STEP, 0.0)                     # another mesh in between (the buffers are reused)
    v2, t2 = extract(bare_ctx, vol, ORIGIN, STEP, 0.25, valid)
    assert v1.tobytes() == v2.tobytes() and t1.tobytes() == t2.tobytes()
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    dv, dt = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1:]
    assert dv == hashlib.sha256(v1.tobytes()).hexdigest() and dt == hashlib.sha256(t1.tobytes()).hexdigest()


# ---- 6. end to end ----------------------------------------------------------------------------------------------
def test_scene_mesh_end_to_end_and_ply(tmp_path):
    """the reference-bound scene of tests/scenes.py with grids of std 0.3: eval_lattice (fine) -> extract at level 0 -> colour query;
    the vertex and topology checks hold on the real volume; colours equal eval_points (color) on the downloaded vertices bit for bit;
    the PLY of Mesher::get_mesh (C++ driver, same scene from .npy files) parses back to the same arrays"""
    sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    n, pad = 48, np.float32(0.1)
    b = sc["bound"]
    lo, hi = (b[:, 0] - pad).astype(np.float32), (b[:, 1] + pad).astype(np.float32)
    origin, step = lo, ((hi - lo) / np.float32(n - 1)).astype(np.float32)
    vol_t = ctx.eval_lattice("fine", origin, step, n, n, n)
    vol = vol_t.cpu().numpy()
    verts_t, tris_t = ctx.extract_mesh(vol_t, origin, step, 0.0)
    v, t = verts_t.cpu().numpy(), tris_t.cpu().numpy()
    keys = mc.check_vertices(v, vol, origin, step, 0.0, max_ulp=0)
    nb = mc.check_topology(t, keys, vol)
    assert len(v) > 10000 and (vol == 100.0).any()
    raw = ctx.eval_points("color", verts_t)
    raw2 = ctx.eval_points("color", cu(v))
    assert (bits(raw.cpu().numpy()) == bits(raw2.cpu().numpy())).all()
    rgb = raw.cpu().numpy()[:, :3]
    print("scene mesh: %d vertices, %d triangles, %d border sides, Euler characteristic %d" % (len(v), len(t), nb, mc.euler_characteristic(t, len(v))))
    # the same through the C++ Mesher
    exe = os.path.join(HOST, "mesh_test")
    if not os.path.exists(exe):
        pytest.fail("mesh_test is not built (run __graft_entry__.build())")
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    r = subprocess.run([exe, "scene", d, str(n), "1", "0.1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mesh_test scene ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    pv, pc, pf = mc.read_ply(os.path.join(d, "mesh.ply"))
    assert pv.tobytes() == v.tobytes() and pf.tobytes() == t.tobytes()
    with np.errstate(invalid="ignore"):
        x = np.where(rgb > 0, np.minimum(rgb, np.float32(1)), np.float32(0)).astype(np.float32) * np.float32(255)
    want_c = np.floor(x.astype(np.float64) + 0.5).astype(np.uint8)
    assert (pc == want_c).all()
    # and without colours, with a validity mask
    valid = (np.random.default_rng(4).random(n ** 3) < 0.9)
    np.save(os.path.join(d, "valid.npy"), valid.astype(np.float32))
    r = subprocess.run([exe, "scene", d, str(n), "0", "0.1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    pv, pc, pf = mc.read_ply(os.path.join(d, "mesh.ply"))
    assert pc is None
    vm = valid.astype(np.uint8).reshape(n, n, n)
    keys = mc.check_vertices(pv, vol, origin, step, 0.0, vm, max_ulp=0)
    mc.check_topology(pf, keys, vol, vm)


# ---- 7. error paths ---------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable(small_ctx):
    import ctypes as C
    import nice_slam_cpp_amd as pkg
    ctx, sc = small_ctx
    L = pkg.nsk.lib()
    vol = cu(noise_volume())
    nz, ny, nx = vol.shape
    o = (C.c_float * 3)(0, 0, 0); s = (C.c_float * 3)(1, 1, 1); neg = (C.c_float * 3)(1, -1, 1)
    nv, nt = C.c_int(7), C.c_int(7)
    p = C.c_void_p(vol.data_ptr())
    err = lambda: L.nsk_last_error().decode()
    assert L.nsk_mesh_extract(ctx.h, p, None, 1, ny, nz, o, s, C.c_float(0), C.byref(nv), C.byref(nt)) < 0 and "at least 2 nodes" in err()
    assert L.nsk_mesh_extract(ctx.h, None, None, nx, ny, nz, o, s, C.c_float(0), C.byref(nv), C.byref(nt)) < 0 and "NULL" in err()
    assert L.nsk_mesh_extract(ctx.h, p, None, nx, ny, nz, o, neg, C.c_float(0), C.byref(nv), C.byref(nt)) < 0 and "step[1]" in err()
    assert L.nsk_mesh_extract(ctx.h, p, None, nx, ny, nz, o, s, C.c_float(0), None, C.byref(nt)) < 0
    assert L.nsk_eval_lattice(ctx.h, 2, o, neg, 4, 4, 4, p) < 0 and "step[1]" in err()
    assert L.nsk_eval_lattice(ctx.h, 2, o, s, 4, 4, 4, None) < 0 and "NULL" in err()
    assert L.nsk_eval_lattice(ctx.h, 2, o, s, 0, 4, 4, p) < 0
    assert L.nsk_eval_lattice(ctx.h, 5, o, s, 4, 4, 4, p) < 0 and "stage" in err()
    with pytest.raises(pkg.NskError):
        ctx.set_tuning("lattice_slab", -1)
    v, t = ctx.extract_mesh(vol, ORIGIN, STEP, 0.0)
    keys = mc.check_vertices(v.cpu().numpy(), vol.cpu().numpy(), ORIGIN, STEP, 0.0, max_ulp=0)
    mc.check_topology(t.cpu().numpy(), keys, vol.cpu().numpy())
    b = sc["bound"]
    assert np.isfinite(ctx.eval_lattice("fine", b[:, 0] + 0.1, (0.05, 0.05, 0.05), 5, 6, 7).cpu().numpy()).all()

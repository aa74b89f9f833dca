"""GPU tests of mesh simplification by vertex clustering: nsk_mesh_simplify through Context.simplify_mesh, Mesher::simplify_mesh
(host/test/simplify_mesh_test) and Mesher::simplify_cell (host/test/mesh_test).  What the device must give is computed by
tests/simplify_checks.py in numpy (int64 / float64 as include/nsk.h states the rule; tests/test_simplify_cpu.py checks that restatement's
properties); the device's bytes equal it: vertices, triangles, vertex map and info."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_checks as mc
import scenes
import simplify_checks as sc
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
F = np.float32
N = 24
STEP = F(1) / F(N - 1)


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


@pytest.fixture(scope="module")
def sphere(ctx):
    """the marching-cubes sphere on a 24^3 lattice over the unit cube, extracted once -> (verts, tris) as numpy arrays"""
    v, t = ctx.extract_mesh(cu(sc.sphere_volume(N)), F([0, 0, 0]), F([STEP] * 3), 0.0)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert len(v) > 1000 and len(t) > 2000 and sc.directed_edge_excess(t) == {}
    return v, t


def device(ctx, v, t, cell, keep=False):
    v, t = np.ascontiguousarray(v, F).reshape(-1, 3), np.ascontiguousarray(t, np.int32).reshape(-1, 3)
    ov, ot, vm, info = ctx.simplify_mesh(cu(v), cu(t, torch.int32), cell, keep_duplicates=keep, want_map=True, want_info=True)
    return ov.cpu().numpy(), ot.cpu().numpy(), vm.cpu().numpy(), info


def check(ctx, v, t, cell, keep=False):
    """the device against the restatement, bytes for bytes -> (the restatement's result, info)"""
    want = sc.simplify(v, t, cell, keep_duplicates=keep)
    ov, ot, vm, info = device(ctx, v, t, cell, keep)
    print("cell %.6g%s: %d -> %d vertices, %d -> %d triangles; info %s (rule: %s)"
          % (cell, " keeping duplicates" if keep else "", len(v), len(ov), len(t), len(ot), info.tolist(), want["info"].tolist()))
    assert info.tobytes() == want["info"].tobytes()
    assert ov.dtype == F and ot.dtype == np.int32 and vm.dtype == np.int32 and ov.shape == want["verts"].shape and ot.shape == want["tris"].shape
    assert ot.tobytes() == want["tris"].tobytes()
    assert ov.tobytes() == want["verts"].tobytes()
    assert vm.tobytes() == want["vertex_map"].tobytes()
    sc.check_output(want, keep)
    return want, info


# ---- 1. the rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True])
def test_sphere(ctx, sphere, keep):
    v, t = sphere
    want, info = check(ctx, v, t, F(2.5) * STEP, keep)
    assert 0 < len(want["tris"]) < len(t) and info[3] > 0 and info[1] == 0 and info[2] == 0
    if keep:
        assert info[4] == 0 and sc.directed_edge_excess(want["tris"]) == {}       # a closed mesh stays balanced


def test_scan_boundaries(ctx, sphere):
    """more than 65 536 cells: the scan over the occupancy flags takes three levels; the occupied count is no multiple of 256, so the
    scans over the lists' counts and the referenced flags end inside a workgroup"""
    v, t = sphere
    want, info = check(ctx, v, t, F(0.018))
    assert info[6] > 65536 and info[5] % 256 != 0 and info[5] > 256
    assert len(want["tris"]) > 0


def test_vertices_on_cell_planes_one_cell_wide(ctx):
    k = np.arange(6)
    X, Y = np.meshgrid(k, k, indexing="xy")
    v = np.stack([1000.0 + 0.25 * X.reshape(-1), -1000.0 + 0.25 * Y.reshape(-1), np.full(36, 7.0)], 1).astype(F)
    q = (Y[:-1, :-1] * 6 + X[:-1, :-1]).reshape(-1)
    t = np.concatenate([np.stack([q, q + 1, q + 7], 1), np.stack([q, q + 7, q + 6], 1)]).astype(np.int32)
    want, info = check(ctx, v, t, 0.25)
    assert sc.unpack_dims(info) == (6, 6, 1) and want["verts"].tobytes() == v.tobytes() and want["tris"].tobytes() == t.tobytes()
    want, info = check(ctx, v, t, 0.5)
    assert sc.unpack_dims(info) == (3, 3, 1) and len(want["verts"]) == 9 and len(want["tris"]) == 8
    for axes in ((2, 0, 1), (1, 2, 0)):                                            # one cell wide along x, along y
        want, info = check(ctx, v[:, axes], t, 0.5)
        assert sorted(sc.unpack_dims(info)) == [1, 3, 3] and len(want["tris"]) == 8


def test_all_in_one_cell_and_empty_inputs(ctx, sphere):
    v, t = sphere
    want, info = check(ctx, v, t, 5.0)
    assert info[6] == 1 and info[5] == 1 and info[3] == len(t) and len(want["verts"]) == 0 and len(want["tris"]) == 0
    want, info = check(ctx, np.zeros((0, 3), F), np.zeros((0, 3), np.int32), 1.0)
    assert info.tolist() == [0] * 8
    want, info = check(ctx, v, np.zeros((0, 3), np.int32), 0.1)                    # vertices without a triangle: cells, no output
    assert info[0] == len(v) and info[5] > 0 and len(want["verts"]) == 0 and (want["vertex_map"] == -1).all()
    want, info = check(ctx, np.zeros((0, 3), F), np.array([[0, 1, 2]], np.int32), 1.0)
    assert info[2] == 1


def test_long_list_with_planted_duplicates_and_mirrored_pairs(ctx):
    import nice_slam_cpp_amd as pkg
    T = pkg.nsk.simplify_list_threshold()
    n_rim = max(300, 2 * T + 7)                                                    # one list longer than the threshold and than a workgroup
    v, fan = sc.fan(n_rim)
    assert len(fan) > T and len(fan) > 256
    picks = [0, 1, T - 1, T, T + 1, 255, 256, len(fan) - 1]
    dup_rot = np.array([[2 + i, 0, 1 + i] for i in picks], np.int32)               # the fan's own triple, rotated: same cells, same order
    mirrored = np.array([[0, 2 + i, 1 + i] for i in picks[::2]], np.int32)         # the other side of the wall
    # a second sheet through vertices of its own in the same cells: every triangle of it repeats the fan's
    v2 = (v + F([0.125, 0.0625, 0.03125])).astype(F)
    sheet = (fan[[3, 40, 41, 257]] + len(v)).astype(np.int32)
    early = np.array([[0, 1 + 100, 2 + 100]], np.int32)                            # in front of the fan: fan triangle 100 is then the duplicate
    vv = np.concatenate([v, v2])
    tt = np.concatenate([early, fan, dup_rot, mirrored, sheet, mirrored[:2, [1, 2, 0]]])
    planted = len(dup_rot) + len(sheet) + 1 + 2                                    # rotated, the sheet, triangle 100, the repeated mirrored pair
    want, info = check(ctx, vv, tt, 1.0)
    assert info[4] == planted and planted > 0 and info[3] == 0 and info[2] == 0
    assert info[5] == n_rim + 1 and len(want["tris"]) == len(tt) - planted
    out = set(map(tuple, want["tris"].tolist()))
    vm = want["vertex_map"]
    for m in mirrored:
        assert tuple(vm[m].tolist()) in out, "a mirrored triangle went"
    assert tuple(vm[early[0]].tolist()) == tuple(want["tris"][0].tolist())
    # and with the duplicates kept nothing goes
    want, info = check(ctx, vv, tt, 1.0, keep=True)
    assert info[4] == 0 and len(want["tris"]) == len(tt)


def test_short_lists_duplicates_by_one_thread(ctx):
    v = F([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [0.15, 0.12, 0.1], [1.2, 0.2, 0.1], [0.2, 1.2, 0.1]])
    t = np.array([[0, 1, 2], [3, 5, 4], [4, 5, 3], [2, 0, 1], [5, 3, 4]], np.int32)
    want, info = check(ctx, v, t, 1.0)
    assert info[4] == 3 and want["tris"].tolist() == [[0, 1, 2], [0, 2, 1]]
    v, t = sc.two_tetrahedra()
    want, info = check(ctx, v, t, 1.0)
    assert info[4] == 1 and len(want["tris"]) == 7
    check(ctx, v, t, 1.0, keep=True)


def test_bad_inputs_are_counted(ctx, sphere):
    v, t = sphere[0].copy(), sphere[1].copy()
    v[5, 1] = np.nan; v[77, 0] = np.inf; v[300, 2] = -np.inf
    t[10, 0] = -1; t[11, 2] = len(v); t[12, 1] = np.iinfo(np.int32).max; t[13, 0] = np.iinfo(np.int32).min
    want, info = check(ctx, v, t, F(2.5) * STEP)
    bad = (np.isin(t, [5, 77, 300]).any(1))
    bad[[10, 11, 12, 13]] = True
    assert info[0] == len(v) - 3 and info[1] == 3 and info[2] == bad.sum() and info[2] > 4
    assert (want["vertex_map"][[5, 77, 300]] == -1).all() and np.isfinite(want["verts"]).all()
    nothing = np.full((4, 3), np.nan, F)
    want, info = check(ctx, nothing, np.array([[0, 1, 2]], np.int32), 1.0)
    assert info.tolist() == [0, 4, 1, 0, 0, 0, 0, 0]


def test_two_runs_and_a_fresh_context_give_the_same_bytes(ctx, sphere):
    import nice_slam_cpp_amd as pkg
    v, t = sphere
    cell = F(1.7) * STEP
    a = device(ctx, v, t, cell)
    device(ctx, *sc.icosphere(2), 0.3)                                             # another mesh in between (the scratch is reused)
    b = device(ctx, v, t, cell)
    c = device(pkg.Context(0), v, t, cell)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert len(a[0]) > 0


def test_errors_leave_the_context_usable(ctx, sphere):
    import nice_slam_cpp_amd as pkg
    v, t = sphere
    with pytest.raises(pkg.NskError, match="cells, at most 2\\^28"):
        device(ctx, v, t, 1e-4)                                                    # 0.74 / 1e-4 cells per axis
    check(ctx, v, t, F(3) * STEP)
    with pytest.raises(pkg.NskError, match="along an axis"):
        device(ctx, F([[0, 0, 0], [3e6, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32), 1.0)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(pkg.NskError, match="must be positive and finite"):
            device(ctx, v, t, bad)
    check(ctx, v, t, F(3) * STEP)


# ---- 2. the Mesher --------------------------------------------------------------------------------------------------------------------
def run(exe, *args):
    path = os.path.join(HOST, exe)
    if not os.path.exists(path):
        pytest.fail("%s is not built (run __graft_entry__.build())" % exe)
    r = subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("keep", [0, 1])
def test_mesher_simplify_mesh_ply_to_ply(ctx, sphere, tmp_path, keep):
    v, t = sphere
    cell = float(F(2.5) * STEP)
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    sc.write_ply(src, v, t)
    js = json.loads(run("simplify_mesh_test", src, out, "%.9g" % cell, keep).strip().splitlines()[-1])
    ov, ot, vm, info = device(ctx, v, t, cell, bool(keep))
    pv, pc, pf = mc.read_ply(out)
    assert pc is None and pv.tobytes() == ov.tobytes() and pf.tobytes() == ot.tobytes()
    assert F(js["cell"]) == F(cell) and js["keep_duplicates"] == keep and js["in_vertices"] == len(v)
    assert (js["vertices"], js["triangles"], js["mapped"]) == (len(ov), len(ot), int((vm >= 0).sum()))
    assert [js[k] for k in ("finite", "left_out", "invalid", "collapsed", "duplicates", "occupied", "cells")] == info[:7].tolist()
    assert tuple(js["dims"]) == sc.unpack_dims(info)


def test_mesher_simplify_cell_zero_is_off_and_a_cell_is_the_python_path(tmp_path):
    s = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    c = make_ctx(s)
    n = 32
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), s["bound"].astype(F))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), s["grids"][k][None].astype(F))
        np.save(os.path.join(d, "dec_%s.npy" % k), s["decoders"][k].astype(F))
    ply = os.path.join(d, "mesh.ply")
    run("mesh_test", "scene", d, n, 1, 0)                                          # the member never touched
    untouched = open(ply, "rb").read()
    out = run("mesh_test", "scene", d, n, 1, 0, 0)                                 # the member set to 0
    assert open(ply, "rb").read() == untouched and len(untouched) > 10000
    b = s["bound"].astype(F)
    origin, step = b[:, 0].copy(), ((b[:, 1] - b[:, 0]) / F(n - 1)).astype(F)      # the Mesher's own expressions, padding 0
    cell = float(F(2) * step.max())
    out = run("mesh_test", "scene", d, n, 1, 0, "%.9g" % cell)
    verts, tris = c.extract_mesh(c.eval_lattice("fine", origin, step, n, n, n), origin, step, 0.0)
    ov, ot = c.simplify_mesh(verts, tris, cell)
    pv, pc, pf = mc.read_ply(ply)
    assert pv.tobytes() == ov.cpu().numpy().tobytes() and pf.tobytes() == ot.cpu().numpy().tobytes() and 0 < len(pf) < len(tris)
    assert "simplified: %d vertices, %d triangles" % (len(ov), len(ot)) in out and "scene ok: %d vertices, %d triangles" % (len(verts), len(tris)) in out
    # colours are those of the written mesh: the colour query at the representatives
    raw = c.eval_points("color", ov).cpu().numpy()[:, :3]
    with np.errstate(invalid="ignore"):
        x = np.where(raw > 0, np.minimum(raw, F(1)), F(0)).astype(F) * F(255)
    assert (pc == np.floor(x.astype(np.float64) + 0.5).astype(np.uint8)).all()

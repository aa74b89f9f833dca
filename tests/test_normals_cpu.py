"""CPU tests (-m "not gpu") of the vertex normals: the numpy restatement of nsk_mesh_vertex_normals (tests/normals_checks.py) against its own
fp64 evaluation, its orientation on a meshed ball, its counts on a mesh with every defect, its dependence on the triangle order; the PLY
overloads with normals and the Mesher's colouring key through host/normals_mesh_test."""
import json
import os
import subprocess

import numpy as np
import pytest

import mesh_cull_checks as mcc
import normals_checks as nc
import raster_checks as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")

# The largest |n32 - n64| over the vertices in units of 2^-23, as the restatement gives it on these meshes, and the bound: four times that.
# The error grows with the number of namings and with how thin a triangle is; a bound derived from the operation count would be far looser.
MEASURED = {"sphere": 0.8815, "blob": 0.7531, "cube_room": 0.4658, "sheet": 0.9337}
MESHES = {"sphere": nc.uv_sphere, "blob": rc.blob, "cube_room": rc.cube_room, "sheet": lambda: rc.sheet(40)[:2]}


def exe():
    p = os.path.join(HOST, "normals_mesh_test")
    if not os.path.exists(p):
        pytest.fail("normals_mesh_test is not built (run __graft_entry__.build())")
    return p


@pytest.mark.parametrize("name", sorted(MESHES))
def test_fp32_restatement_against_its_fp64_evaluation(name):
    v, t = MESHES[name]()
    assert len(v) == {"sphere": 362, "blob": 121, "cube_room": 8, "sheet": 1600}[name]
    n32, i32 = nc.vertex_normals(v, t, np.float32)
    n64, i64 = nc.vertex_normals(v, t, np.float64)
    assert n32.dtype == np.float32 and n64.dtype == np.float64
    assert i32[:2] == [0, 0] and i64[:2] == [0, 0] and i32[2] == i64[2]              # every triangle takes part, no vertex is without a normal
    assert np.abs(np.linalg.norm(n64, axis=1) - 1.0).max() < 1e-15
    err = float(np.abs(n32.astype(np.float64) - n64).max()) * 2.0 ** 23
    print("%s: %d vertices, %d triangles, most namings %d, max |n32 - n64| = %.4f x 2^-23" % (name, len(v), len(t), i32[2], err))
    assert err <= 4.0 * MEASURED[name]


def test_normals_of_a_meshed_ball_point_to_free_space():
    """the ball is meshed by hand (mesh_cull_checks.numpy_mesh) with the library's own case table, which needs no device: inside is positive
    (radius - distance, as spheres_volume), so free space is outside the ball and every normal has n . (v - centre) > 0"""
    import nice_slam_cpp_amd as pkg
    table = [pkg.nsk.mesh_table(c) for c in range(256)]
    n, centre, radius = 20, np.array([0.93, 1.02, 0.97]), 0.61
    origin, step = (0.0, 0.0, 0.0), (0.1, 0.1, 0.1)
    g = np.arange(n) * 0.1
    x, y, z = g[None, None, :], g[None, :, None], g[:, None, None]
    vol = (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)
    v, t = mcc.numpy_mesh(table, vol, origin, step)
    assert len(v) > 200 and len(t) > 400
    nrm, info = nc.vertex_normals(v, t)
    assert info[:2] == [0, 0]
    dots = (nrm.astype(np.float64) * (v.astype(np.float64) - centre)).sum(axis=1)
    assert (dots > 0).all(), int((dots <= 0).sum())
    assert dots.min() > 0.9 * radius * 0.9                  # and nearly radial: the ball is smooth at this step


def test_dirty_mesh_counts_and_zero_bits():
    v, t = nc.dirty_mesh()
    n, info = nc.vertex_normals(v, t)
    assert info == nc.DIRTY_INFO == [3, 6, 8, 0]
    zero = [121, 122, 123, 124, 125, 126]
    assert (nc.bits32(n[zero]) == 0).all()                  # +0, not -0
    rest = np.setdiff1d(np.arange(len(v)), zero)
    assert np.abs(np.linalg.norm(n[rest].astype(np.float64), axis=1) - 1.0).max() < 3e-7
    # the triangle that names vertex 60 twice adds an exact zero: the other vertices' normals are the clean blob's
    vb, tb = rc.blob()
    assert nc.bits32(n[:121]).tobytes() == nc.bits32(nc.vertex_normals(vb, tb)[0]).tobytes()
    o, d, gd, has = nc.normal_rays(v, n, 0.1)
    assert has.sum() == len(v) - 6 and not has[zero].any()
    assert nc.bits32(o[zero]).tobytes() == nc.bits32(v[zero]).tobytes() and (d[zero] == np.array([0, 0, -1], np.float32)).all()
    assert (gd == np.float32(0.1)).all()


def test_the_sum_depends_on_the_triangle_order():
    """the premise of the byte tests: the same triangles in another order give other bits, so the device must walk them in index order"""
    v, t = nc.uv_sphere()
    a, b = nc.vertex_normals(v, t)[0], nc.vertex_normals(v, nc.shuffled(t))[0]
    changed = int((nc.bits32(a) != nc.bits32(b)).any(axis=1).sum())
    print("shuffled triangle list: %d of %d vertices change bits" % (changed, len(v)))
    assert changed > 100
    assert np.abs(a.astype(np.float64) - b).max() < 4 * 2.0 ** -23


def test_ply_with_normals_round_trip(tmp_path):
    """host/normals_mesh_test ply: the new write_ply / read_ply overloads, the old pair and read_ply_mesh on each other's files (the program
    compares bytes); here the file's layout, its bytes against the arrays, and the old writer's bytes against what it always wrote"""
    v, t = nc.dirty_mesh()
    t = t[((t >= 0) & (t < len(v))).all(axis=1)]            # (read_ply_mesh refuses an index out of range)
    n = nc.vertex_normals(v, t)[0]
    n[7] = [-0.0, np.inf, np.float32(1e-42)]                # bits a conversion could lose
    rgb = np.random.default_rng(2).integers(0, 256, (len(v), 3)).astype(np.uint8)
    d = str(tmp_path)
    for name, a in (("xyz", v), ("normals", n), ("rgb", rgb), ("tris", t)):
        np.save(os.path.join(d, name + ".npy"), np.ascontiguousarray(a, np.float32))
    r = subprocess.run([exe(), "ply", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "normals_mesh_test ply ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    pv, pn, pc, pt = nc.read_ply(os.path.join(d, "with_normals.ply"))
    assert nc.bits32(pv).tobytes() == nc.bits32(v).tobytes() and nc.bits32(pn).tobytes() == nc.bits32(n).tobytes()
    assert pc.tobytes() == rgb.tobytes() and pt.tobytes() == t.tobytes()
    head = open(os.path.join(d, "with_normals.ply"), "rb").read(400).split(b"end_header\n")[0].decode().splitlines()
    assert [ln.split()[-1] for ln in head if ln.startswith("property")][:9] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    pv, pn, pc, pt = nc.read_ply(os.path.join(d, "normals_only.ply"))
    assert pc is None and nc.bits32(pn).tobytes() == nc.bits32(n).tobytes() and pt.tobytes() == t.tobytes()
    # the old writer: byte for byte what it wrote before there were normals, and the new one without normals writes the same file
    header = ("ply\nformat binary_little_endian 1.0\ncomment nice-slam-cpp_amd Mesher\nelement vertex %d\nproperty float x\nproperty float y\n"
              "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (len(v), len(t))).encode()
    vrec = np.zeros(len(v), np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    vrec["p"], vrec["c"] = v, rgb
    frec = np.zeros(len(t), np.dtype([("k", "u1"), ("i", "<i4", 3)]))
    frec["k"], frec["i"] = 3, t
    want = header + vrec.tobytes() + frec.tobytes()
    assert open(os.path.join(d, "old.ply"), "rb").read() == want
    assert open(os.path.join(d, "no_normals.ply"), "rb").read() == want


def test_color_method_key():
    """absent: the point query; the two values upstream knows; anything else throws and names the key"""
    for arg, want in (("-", "direct_point_query"), ("direct_point_query", "direct_point_query"), ("render_ray_along_normal", "render_ray_along_normal")):
        r = subprocess.run([exe(), "config", arg], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-1])
        assert got["color_method"] == want and got["write_normals"] == 0 and abs(got["color_ray_length"] - 0.1) < 1e-8
    r = subprocess.run([exe(), "config", "render_ray_query"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "color_mesh_extraction_method" in r.stderr and "render_ray_query" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]

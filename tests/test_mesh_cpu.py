"""CPU tests (-m "not gpu") of the mesh extraction: the 256-case marching-cubes table the library derives (through nsk_mesh_table, which
needs no device) and the PLY writer / reader of the C++ Mesher.  What the table must satisfy is in tests/mesh_checks.py."""
import os
import subprocess

import numpy as np

import mesh_checks as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


def _table():
    import nice_slam_cpp_amd as pkg
    pkg.build()
    return [pkg.nsk.mesh_table(c) for c in range(256)]


def test_table_is_crack_free_closed_and_oriented():
    """every case: triangle corners on exactly the crossing edges; inner sides paired in opposite directions, sides in a cube face used
    once; the segments on a face are a function of the face's four corner signs and the reverse of what any neighbour with those signs
    leaves (all 256 x 6 x 16 pairs); cases 0 / 255 empty; complements agree on every unambiguous face; one-corner normals point away from
    the inside corner.  Row capacity: the largest case has 5 triangles (the classic table's figure), asserted below."""
    table = _table()
    most = mc.check_table(table)
    counts = [len(t) for t in table]
    assert most == 5 and most == max(counts)
    print("largest case: %d triangles; %d triangles over the 256 cases" % (most, sum(counts)))


def test_table_error_paths():
    import ctypes as C
    import nice_slam_cpp_amd as pkg
    L = pkg.nsk.lib()
    buf = (C.c_int8 * 64)()
    assert L.nsk_mesh_table(256, buf, 64) < 0 and b"out of range" in L.nsk_last_error()
    assert L.nsk_mesh_table(-1, buf, 64) < 0
    assert L.nsk_mesh_table(1, buf, 2) < 0 and b"capacity" in L.nsk_last_error()
    assert L.nsk_mesh_table(1, None, 0) == 1                   # the count alone
    assert L.nsk_mesh_table(0, buf, 0) == 0


def test_table_matches_a_small_volume_in_numpy():
    """the table applied by hand (numpy) to a seeded 5 x 4 x 6 noise volume gives a mesh that passes the volume-only checks: the helpers and
    the table agree on the numbering before any GPU is involved"""
    table = _table()
    rng = np.random.default_rng(5)
    nz, ny, nx = 6, 4, 5
    vol = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    origin, step = (-1.0, 0.5, 2.0), (0.25, 0.5, 0.125)
    keys, pos = mc.reference_vertices(vol, origin, step, 0.0)
    vid = {int(k): n for n, k in enumerate(keys)}
    tris = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                case = sum(int(vol[k + dz, j + dy, i + dx] > 0) << c for c, (dx, dy, dz) in enumerate(mc.CORNER))
                for t in table[case]:
                    tri = []
                    for e in t:
                        dx, dy, dz = mc.CORNER[mc.edge_ends(e)[0]]
                        tri.append(vid[(((k + dz) * ny + j + dy) * nx + i + dx) * 3 + (e >> 2)])
                    tris.append(tri)
    tris = np.array(tris, np.int32)
    nb = mc.check_topology(tris, keys, vol)
    assert nb > 0                                               # noise reaches the lattice border
    assert len(mc.cell_cases(vol, 0.0, mc.processed_cells(vol))) == (nz - 1) * (ny - 1) * (nx - 1)


def test_ply_round_trip(tmp_path):
    """Mesher::write_ply -> Mesher::read_ply inside the C++ driver (it compares the arrays itself), and the same file parsed here:
    binary little-endian, float x y z, uchar red green blue, list uchar int vertex_indices"""
    import nice_slam_cpp_amd as pkg
    pkg.build()
    subprocess.check_call(["make", "-s", "-C", HOST, "mesh_test"])
    exe = os.path.join(HOST, "mesh_test")
    for color in (1, 0):
        path = str(tmp_path / ("m%d.ply" % color))
        r = subprocess.run([exe, "ply", path, str(color)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        v, c, f = mc.read_ply(path)
        n = 7
        k = np.arange(n, dtype=np.float32)
        want_v = np.stack([k * np.float32(0.5), k * k, -k], 1).astype(np.float32)
        assert v.tobytes() == want_v.tobytes()
        assert (f == np.stack([np.arange(5), np.arange(5) + 1, np.arange(5) + 2], 1)).all() and f.dtype == np.int32
        if color:
            assert (c == np.stack([np.arange(n) * 30, 255 - np.arange(n), np.full(n, 7)], 1).astype(np.uint8)).all()
        else:
            assert c is None

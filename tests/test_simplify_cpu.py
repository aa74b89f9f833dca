"""The simplification rule without a GPU: what tests/simplify_checks.py (the numpy restatement of nsk_mesh_simplify) leaves of a mesh, and
host/test/simplify_plan_test (csrc/nsk_simplify_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement's
grids, cell coordinates, fixed-point fractions and representatives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import simplify_checks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
F = np.float32

_sphere = sc.icosphere(3)                   # 642 vertices, 1280 triangles, radius 1


@pytest.mark.parametrize("cell", [0.2, 0.3, 0.77, 5.0])
def test_closed_mesh_stays_balanced_with_duplicates_kept(cell):
    """Why the balance holds: the boundary of a 2-chain is linear, and identifying vertices is a chain map -- it commutes with the
    boundary.  A closed oriented mesh has boundary zero (every directed side as often as its reverse), so its image has boundary zero
    too; a collapsed triangle's image contributes a side and its reverse (or a loop), so dropping it changes nothing.  Dropping a
    duplicate does: the test below shows it."""
    v, t = _sphere
    assert sc.directed_edge_excess(t) == {}
    res = sc.simplify(v, t, cell, keep_duplicates=True)
    sc.check_output(res, True)
    assert res["info"][4] == 0 and res["info"][2] == 0 and res["info"][3] + len(res["tris"]) == len(t)
    assert sc.directed_edge_excess(res["tris"]) == {}
    if cell == 5.0:
        assert len(res["tris"]) == 0 and len(res["verts"]) == 0 and res["info"][6] == 1 and res["info"][5] == 1
    else:
        assert 0 < len(res["tris"]) < len(t) and len(res["verts"]) < len(v)


def test_removing_a_duplicate_breaks_the_balance():
    v, t = sc.two_tetrahedra()
    assert sc.directed_edge_excess(t) == {}
    kept = sc.simplify(v, t, 1.0, keep_duplicates=True)
    sc.check_output(kept, True)
    assert len(kept["tris"]) == 8 and len(kept["verts"]) == 5 and sc.directed_edge_excess(kept["tris"]) == {}
    cut = sc.simplify(v, t, 1.0)
    sc.check_output(cut, False)
    assert cut["info"][4] == 1 and len(cut["tris"]) == 7 and cut["tris"].tolist() == np.delete(kept["tris"], 4, axis=0).tolist()
    ex = sc.directed_edge_excess(cut["tris"])
    a, b, c = kept["tris"][0].tolist()                      # the base that stayed: its sides are now short of one partner each
    assert ex == {(b, a): 1, (c, b): 1, (a, c): 1}


def test_mirrored_triangles_are_not_duplicates():
    v = F([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 1.1, 0.1], [0.15, 0.12, 0.1], [1.2, 0.2, 0.1], [0.2, 1.2, 0.1]])
    t = np.array([[0, 1, 2], [3, 5, 4], [4, 5, 3], [2, 0, 1], [5, 3, 4]], np.int32)        # front, back, back rotated, front rotated twice
    res = sc.simplify(v, t, 1.0)
    sc.check_output(res, False)
    assert res["info"][4] == 3 and res["tris"].tolist() == [[0, 1, 2], [0, 2, 1]]
    assert sc.directed_edge_excess(res["tris"]) == {}


@pytest.mark.parametrize("cell", [0.2, 0.3, 0.77])
@pytest.mark.parametrize("keep", [False, True])
def test_outputs_and_the_distance_a_vertex_moves(cell, keep):
    v, t = _sphere
    res = sc.simplify(v, t, cell, keep_duplicates=keep)
    sc.check_output(res, keep)
    vm = res["vertex_map"]
    on = vm >= 0
    assert on.any()
    # both lie in one closed cell; the slack covers the fp64 evaluation and one fp32 rounding
    d = np.abs(res["verts"][vm[on]].astype(np.float64) - v[on].astype(np.float64))
    bound = np.float64(F(cell)) + 2.0 ** -23 * np.abs(v).max()
    print("cell %g: %d -> %d vertices, %d -> %d triangles, largest move %.4g of %.4g allowed" % (cell, len(v), len(res["verts"]), len(t), len(res["tris"]), d.max(), bound))
    assert (d <= bound).all()
    # the representative lies in its cell, up to the same slack
    nx, ny, nz = sc.unpack_dims(res["info"])
    named = res["named_cells"]
    c = np.stack([named % nx, (named // nx) % ny, named // (nx * ny)], 1).astype(np.float64)
    lo = v.min(axis=0).astype(np.float64)
    rel = res["verts"].astype(np.float64) - (lo + c * np.float64(F(cell)))
    assert (rel >= -2.0 ** -23 * np.abs(v).max()).all() and (rel <= bound).all()


def test_far_from_the_origin_and_on_cell_planes():
    # vertices exactly on planes lo + k cell, one cell wide along z, 1000 units from the origin: every coordinate is reproduced exactly
    k = np.arange(6)
    X, Y = np.meshgrid(k, k, indexing="xy")
    v = np.stack([1000.0 + 0.25 * X.reshape(-1), -1000.0 + 0.25 * Y.reshape(-1), np.full(36, 7.0)], 1).astype(F)
    q = (Y[:-1, :-1] * 6 + X[:-1, :-1]).reshape(-1)
    t = np.concatenate([np.stack([q, q + 1, q + 7], 1), np.stack([q, q + 7, q + 6], 1)]).astype(np.int32)
    res = sc.simplify(v, t, 0.25)
    sc.check_output(res, False)
    assert sc.unpack_dims(res["info"]) == (6, 6, 1) and res["info"][5] == 36 and res["info"][3] == 0
    assert res["verts"].tobytes() == v.tobytes() and res["tris"].tobytes() == t.tobytes()
    res = sc.simplify(v, t, 0.5)
    sc.check_output(res, False)
    assert sc.unpack_dims(res["info"]) == (3, 3, 1) and len(res["verts"]) == 9 and len(res["tris"]) == 8


def test_bad_inputs_and_errors():
    v, t = sc.icosphere(1)
    v, t = v.copy(), t.copy()
    v[3, 1] = np.nan; v[7, 0] = np.inf; v[9, 2] = -np.inf
    t[0, 0] = -1; t[1, 2] = len(v)
    res = sc.simplify(v, t, 0.4)
    sc.check_output(res, False)
    named = set(np.flatnonzero((t == 3).any(1) | (t == 7).any(1) | (t == 9).any(1)).tolist()) | {0, 1}
    assert res["info"][0] == len(v) - 3 and res["info"][1] == 3 and res["info"][2] == len(named)
    assert (res["vertex_map"][[3, 7, 9]] == -1).all() and np.isfinite(res["verts"]).all()
    none = sc.simplify(np.full((4, 3), np.nan, F), np.array([[0, 1, 2]], np.int32), 1.0)
    assert none["info"].tolist() == [0, 4, 1, 0, 0, 0, 0, 0] and len(none["verts"]) == 0 and (none["vertex_map"] == -1).all()
    empty = sc.simplify(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), 1.0)
    assert empty["info"].tolist() == [0] * 8
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(sc.SimplifyError):
            sc.simplify(v, t, bad)
    with pytest.raises(sc.SimplifyError):
        sc.simplify(v, t, 1e-4)                                    # about 2.4e4 cells per axis: past 2^28 in all
    with pytest.raises(sc.SimplifyError):
        sc.simplify(F([[0, 0, 0], [3e6, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32), 1.0)       # 3e6 cells along x


def _case(v, cell, want_points=True):
    """one record of simplify_plan_test: the box, the cell, what the plan must answer, points and representatives"""
    v = np.ascontiguousarray(v, F)
    fin = np.isfinite(v).all(1)
    lo, hi = v[fin].min(0).astype(np.float64), v[fin].max(0).astype(np.float64)
    try:
        res = sc.simplify(v, np.zeros((0, 3), np.int32), cell)
        rc, n, cells = 0, sc.unpack_dims(res["info"]), int(res["info"][6])
    except sc.SimplifyError as e:
        rc, n, cells, want_points = (3 if "per axis" in str(e) else 2), (0, 0, 0), -1, False
    blob = struct.pack("<f", cell) + lo.astype("<f8").tobytes() + hi.astype("<f8").tobytes() + struct.pack("<qi3qq", int(fin.sum()), rc, *n, cells)
    if not want_points:
        return blob + struct.pack("<ii", 0, 0)
    cd = np.float64(F(cell))
    g = (v[fin].astype(np.float64) - lo) / cd
    c = np.floor(g)
    q = np.rint((g - c) * sc.FRAC).astype(np.int64)
    c = c.astype(np.int64)
    blob += struct.pack("<i", int(fin.sum()))
    for p, ci, qi in zip(v[fin], c, q):
        blob += p.astype("<f4").tobytes() + ci.astype("<i8").tobytes() + qi.astype("<i8").tobytes()
    # representatives per axis: the vertices grouped by their coordinate's cell along that axis alone
    reps = []
    for a in range(3):
        for ca in np.unique(c[:, a]):
            m = c[:, a] == ca
            s, k = int(q[m, a].sum()), int(m.sum())
            pos = F(lo[a] + (np.float64(ca) + (np.float64(s) / np.float64(k)) / sc.FRAC) * cd)
            reps.append(struct.pack("<iqQI", a, int(ca), s, k) + pos.tobytes())
    return blob + struct.pack("<i", len(reps)) + b"".join(reps)


def test_simplify_plan_test_under_the_sanitizers(tmp_path):
    v = _sphere[0]
    rng = np.random.default_rng(5)
    far = (rng.standard_normal((300, 3)) * [3.0, 0.01, 40.0] + [1e4, -2e3, 0.5]).astype(F)
    cases = [_case(v, 0.11), _case(v, 0.3), _case(v, F(1) / F(3)), _case(v, 5.0), _case(far, 0.37), _case(far, 1e-3), _case(v, 1e-4),
             _case(F([[0, 0, 0], [3e6, 0, 0]]), 1.0), _case(v[:1], 0.5), _case(np.concatenate([v[:50], [[np.nan, 0, 0]]]).astype(F), 0.2)]
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(cases)) + b"".join(cases))
    subprocess.check_call(["make", "-s", "-C", HOST, "simplify_plan_test"])
    r = subprocess.run([os.path.join(HOST, "simplify_plan_test"), str(path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "simplify_plan_test: ok" in r.stdout and "%d cases" % len(cases) in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]

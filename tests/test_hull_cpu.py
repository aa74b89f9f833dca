"""The hull rule without a GPU: tests/hull_checks.py (the numpy / Python integer restatement of nsk_points_hull and nsk_lattice_in_hull)
against scipy's Qhull on the quantised coordinates, and host/test/hull_plan_test (csrc/nsk_hull_plan.h over a CPU stand-in for the
device, under AddressSanitizer + UndefinedBehaviorSanitizer) against the restatement."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hull_checks as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")

_cache = {}


def _hull(name):
    if name not in _cache:
        _cache[name] = (hc.cloud(name), hc.hull(hc.cloud(name)))
    return _cache[name]


@pytest.mark.parametrize("name", hc.CLOUDS)
def test_restatement_against_qhull(name):
    from scipy.spatial import ConvexHull
    pts, h = _hull(name)
    q, finite, faces, verts = h["q"], h["finite"], h["faces"], h["vertices"]
    assert h["info"][2] == 3 and faces.shape[0] == h["info"][4] and verts.size == h["info"][3]
    assert hc.closed_manifold(faces)                                   # exact: every directed edge once, its twin once, V - E + F = 2
    assert hc.points_outside(q, finite, faces) == 0                    # exact containment
    ref = ConvexHull(q.astype(np.float64))
    v6 = hc.volume6(q, faces)
    assert v6 > 0 and abs(v6 - 6.0 * ref.volume) <= 1e-12 * v6, (v6, 6.0 * ref.volume)
    mine = set(map(tuple, q[verts].tolist()))
    theirs = set(map(tuple, q[ref.vertices].tolist()))
    assert mine >= theirs
    if name in hc.GENERAL:
        assert mine == theirs and set(verts.tolist()) == set(ref.vertices.tolist())
    if name == "repeated":                                             # the smallest index of each coordinate is the one used
        assert mine == theirs
        first = {}
        for i, row in enumerate(map(tuple, q.tolist())):
            first.setdefault(row, i)
        assert sorted(verts.tolist()) == sorted(first[r] for r in mine)
    assert h["info"][5] >= verts.size - 4                              # an insertion per vertex behind the simplex; some vertices die again


def test_restatement_degenerate_ranks():
    line, plane = hc.flat_cloud(1), hc.flat_cloud(2)
    for pts, rank, fin in ((np.zeros((0, 3), np.float32), 0, 0), (np.ones((3, 3), np.float32), 0, 3), (np.eye(3, dtype=np.float32), 2, 3),
                           (np.tile([[1.5, -2.0, 3.0]], (9, 1)).astype(np.float32), 0, 9), (line, 1, 16), (plane, 2, 136)):
        h = hc.hull(pts)
        assert h["info"][2] == rank and h["info"][0] == fin and h["faces"].shape[0] == 0 and h["vertices"].size == 0
    bad = hc.cloud("ball2000")[:40].copy()
    bad[3, 1] = np.nan; bad[17, 0] = np.inf; bad[18, 2] = -np.inf
    h, g = hc.hull(bad), hc.hull(np.delete(bad, [3, 17, 18], axis=0))
    assert h["info"][0] == 37 and h["info"][1] == 3 and h["info"][2] == 3
    keep = np.delete(np.arange(40), [3, 17, 18])
    assert np.array_equal(h["faces"], keep[g["faces"]]) and not set(h["vertices"].tolist()) & {3, 17, 18}


@pytest.mark.parametrize("name,scale", [("ball2000", 1.0), ("ball2000", 1.02), ("walls", 1.02), ("lattice5", 1.0)])
def test_mask_restatement_against_delaunay(name, scale):
    """an independent inside test: the simplices of a Delaunay triangulation of the scaled vertices.  Nodes closer than 1e-9 E to a
    plane are left out, so that agreement is a condition and not a tolerance; fewer than 1 % are."""
    from scipy.spatial import Delaunay
    pts, h = _hull(name)
    xyz = pts[h["vertices"]]
    E = float((pts.max(0).astype(np.float64) - pts.min(0).astype(np.float64)).max())
    lo, hi = pts.min(0) - np.float32(0.137 * E), pts.max(0) + np.float32(0.093 * E)      # (no node plane coincides with a wall)
    n = (17, 13, 9)
    step = (hi - lo) / (np.array(n, np.float32) - 1)
    mask, margin = hc.lattice_in_hull(lo, step, *n, xyz, hc.local_faces(h["vertices"], h["faces"]), scale, want_margin=True)
    V = xyz.astype(np.float64)
    c = V.mean(0)
    tri = Delaunay(c + scale * (V - c))
    P = hc.lattice_points(lo, step, *n)
    ref = tri.find_simplex(P.reshape(-1, 3), tol=0.0).reshape(mask.shape) >= 0
    keep = margin >= 1e-9 * E
    assert (~keep).sum() < 0.01 * keep.size
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(mask[keep] != 0, ref[keep])


def _record(pts, scale):
    h = hc.hull(pts)
    nv, nf = h["vertices"].size, h["faces"].shape[0]
    blob = struct.pack("<i", pts.shape[0]) + np.ascontiguousarray(pts, "<f4").tobytes() + h["info"].astype("<i8").tobytes()
    blob += struct.pack("<ii", nv, nf) + h["vertices"].astype("<i4").tobytes() + np.ascontiguousarray(h["faces"], "<i4").tobytes()
    blob += struct.pack("<d", scale)
    if nf:
        n, A, lo, hi = hc.mask_planes(pts[h["vertices"]], hc.local_faces(h["vertices"], h["faces"]), scale)
        blob += np.ascontiguousarray(np.concatenate([n, A], 1), "<f8").tobytes() + np.concatenate([lo, hi]).astype("<f8").tobytes()
    else:
        blob += np.zeros(6, "<f8").tobytes()
    return blob


def test_hull_plan_test_under_the_sanitizers(tmp_path):
    clouds = [hc.cloud(n) for n in hc.CLOUDS if n != "box70000"] + [hc.cloud("box70000")[:20000]]
    bad = hc.cloud("ball2000")[:40].copy()
    bad[3, 1] = np.nan; bad[17, 0] = np.inf
    clouds += [bad, np.zeros((0, 3), np.float32), np.ones((5, 3), np.float32), hc.flat_cloud(1), hc.flat_cloud(2),
               np.eye(4, 3, dtype=np.float32)]
    path = tmp_path / "clouds.bin"
    path.write_bytes(struct.pack("<i", len(clouds)) + b"".join(_record(p, 1.02) for p in clouds))
    subprocess.check_call(["make", "-s", "-C", HOST, "hull_plan_test"])
    r = subprocess.run([os.path.join(HOST, "hull_plan_test"), str(path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "hull_plan_test: ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]

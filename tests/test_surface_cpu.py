"""CPU tests (-m "not gpu") of the surface metrics' rule as tests/surface_checks.py restates it: hand-placed cases against their closed
forms, the float64 evaluation against an independent closest-point routine, the accuracy of the float32 rule, the property its stopping
bound rests on, a plain-numpy model of the grid walk, and the host-only grid sizing under the sanitizers.  The device is bound to
brute_mesh_nearest(float32) by byte equality in tests/test_gpu_surface.py, so the figures asserted here are the device's figures."""
import os
import subprocess

import numpy as np
import pytest

import recon_checks as rc
import surface_checks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
ULP = 2.0 ** -23


# ---- 1. hand-placed cases ---------------------------------------------------------------------------------------------------------------
V2 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
ONE = np.array([[0, 1, 2]], np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_placed_queries_have_their_closed_forms(dtype):
    q = np.array([[0.25, 0.25, 0.5],       # above the interior
                  [-1.0, -1.0, 0.0],       # beyond vertex a
                  [0.5, -2.0, 0.0],        # beyond edge ab
                  [1.0, 0.0, 0.0],         # on vertex b
                  [2.0, 2.0, 1.0]], np.float32)      # beyond edge bc, off the plane
    d, t, p = sc.brute_mesh_nearest(q, V2, ONE, dtype)
    assert d.dtype == dtype and p.dtype == dtype and t.dtype == np.int32 and (t == 0).all()
    assert (p[0] == [0.25, 0.25, 0.0]).all() and d[0] == 0.5
    assert (p[1] == [0, 0, 0]).all() and abs(d[1] - np.sqrt(2.0)) <= 2 * ULP
    assert (p[2] == [0.5, 0, 0]).all() and d[2] == 2.0
    assert (p[3] == [1, 0, 0]).all() and d[3] == 0.0
    assert (p[4] == [0.5, 0.5, 0]).all() and abs(d[4] - np.sqrt(1.5 ** 2 * 2 + 1)) <= 4 * ULP


@pytest.mark.parametrize("tris", [[[0, 1, 2], [1, 3, 2]], [[1, 3, 2], [0, 1, 2]], [[2, 1, 3], [2, 0, 1]]])
def test_on_a_shared_edge_the_lowest_triangle_wins(tris):
    q = np.array([[0.5, 0.5, 0.0], [0.25, 0.75, 0.0], [1.0, 0.0, 0.0], [0.625, 0.375, 0.25]], np.float32)
    d, t, p = sc.brute_mesh_nearest(q, V2, np.array(tris, np.int32))
    assert (t == 0).all() and (d[:3] == 0).all() and d[3] == 0.25
    assert (sc.bits32(p[:3]) == sc.bits32(q[:3])).all()


def test_triangles_that_do_not_take_part_and_queries_that_are_not_finite():
    v = np.concatenate([V2, [[np.nan, 0, 0]]]).astype(np.float32)
    t = np.array([[0, 0, 1], [0, 1, 4], [0, 1, 5], [-1, 0, 1], [0, 1, 2]], np.int32)
    assert list(sc.participating(v, t)) == [4]
    q = np.array([[0.25, 0.25, 1.0], [np.inf, 0, 0], [0, np.nan, 0]], np.float32)
    d, tri, p = sc.brute_mesh_nearest(q, v, t)
    assert d[0] == 1.0 and tri[0] == 4 and np.isnan(d[1:]).all() and (tri[1:] == -1).all() and np.isnan(p[1:]).all()
    d, tri, p = sc.brute_mesh_nearest(q, v, t[:4])
    assert d[0] == np.inf and np.isnan(d[1:]).all() and (tri == -1).all() and np.isnan(p).all()


# ---- 2. the rule in float64 against the region form -----------------------------------------------------------------------------------
SHEET = (sc.tilt(rc.sheet()[0]), rc.sheet()[1])


@pytest.mark.parametrize("name", ["tilted sheet", "slivers 1e-4", "slivers 1e-6"])
def test_the_rule_in_float64_equals_the_region_form(name):
    v, t = SHEET if name == "tilted sheet" else sc.slivers(float(name.split()[1]))
    q = sc.box_queries(v, 2000, 3.0, 21)
    d = sc.brute_mesh_nearest(q, v, t, np.float64)[0]
    e = sc.ericson_mesh_nearest(q, v, t)
    rel = np.abs(d - e) / e
    print("%s: 2000 queries, distances %.3g .. %.3g, worst relative difference to the region form %.3g" % (name, e.min(), e.max(), rel.max()))
    assert rel.max() <= 1e-12


# ---- 3. the accuracy of the float32 rule --------------------------------------------------------------------------------------------------
def _accuracy_scenes():
    S = {}
    for name, shift in (("tilted", (0.0, 0.0, 0.0)), ("tilted and shifted", (5.0, -3.0, 2.0))):
        (v, t), (v1, t1) = sc.tilted_sheets(0.03, shift)
        mid = 0.5 * (v.astype(np.float64).min(0) + v.astype(np.float64).max(0))
        box = (mid + np.random.default_rng(3).uniform(-3.5, 3.5, (800, 3))).astype(np.float32)
        S[name] = (v, t, [rc.sample_mesh(v, t, 800, 1)[0], rc.sample_mesh(v1, t1, 800, 2)[0], box])
    for hgt in (1e-4, 1e-6):
        v, t = sc.slivers(hgt)
        S["slivers %g" % hgt] = (v, t, [sc.box_queries(v, 800, 1.2, 5), sc.box_queries(v, 800, 7.0, 6)])
    v, t = rc.sheet(); v1, t1 = rc.sheet(nx=11, ny=13, origin=(0.0, 0.0, 0.03), seed=1)
    S["flat"] = (v, t, [rc.sample_mesh(v, t, 800, 1)[0], rc.sample_mesh(v1, t1, 800, 2)[0], sc.box_queries(v, 800, 7.0, 7)])
    return S


@pytest.mark.parametrize("name", ["tilted", "tilted and shifted", "slivers 0.0001", "slivers 1e-06", "flat"])
def test_the_float32_rule_is_within_four_ulp_of_the_scene(name):
    """measured (units of 2^-23 S, S the largest coordinate magnitude of scene and queries): tilted sheet 1.35, tilted and shifted 0.60,
    slivers 0.82, flat sheet 0.78 (the prototype of the rule, other seeds: 1.16 / 0.81 / 0.65); the bound is 4"""
    v, t, queries = _accuracy_scenes()[name]
    worst = 0.0
    for q in queries:
        S = max(np.abs(v).max(), np.abs(q).max())
        d32, t32, p32 = sc.brute_mesh_nearest(q, v, t, np.float32)
        d64 = sc.brute_mesh_nearest(q, v, t, np.float64)[0]
        err = np.abs(d32.astype(np.float64) - d64).max() / (ULP * S)
        worst = max(worst, err)
        # the property the stopping bound rests on: every returned point lies inside its triangle's box, exactly
        tv = v[np.asarray(t, np.int64)[t32]]
        assert ((p32 >= tv.min(1)) & (p32 <= tv.max(1))).all()
    print("%s: worst |d32 - d64| = %.3f x 2^-23 S" % (name, worst))
    assert worst <= 4.0


# ---- 4. the grid walk in plain numpy ---------------------------------------------------------------------------------------------------
def _same(got, want):
    return (sc.bits32(got[0]) == sc.bits32(want[0])).all() and (got[1] == want[1]).all() and (sc.bits32(got[2]) == sc.bits32(want[2])).all()


@pytest.mark.parametrize("h", [0.05, 0.11, 0.4])
def test_the_shell_walk_returns_the_brute_force_bytes_for_far_queries(h):
    v, t = SHEET
    q = np.concatenate([sc.box_queries(v, 150, 7.0, 9), rc.sample_mesh(v, t, 50, 3)[0]])
    got = sc.grid_mesh_nearest(q, v, t, h)
    print("h %.2f: dims %s, %d wide, the farthest walk reached radius %d" % (h, got[5], got[4], got[3]))
    assert got[4] == 0 and got[3] >= 2
    assert _same(got, sc.brute_mesh_nearest(q, v, t))


def test_the_shell_walk_with_a_wide_triangle():
    v, t = SHEET
    lo, hi = v.min(0), v.max(0)
    big = np.array([lo, [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]], np.float32)
    v2, t2 = rc.merge((v, t), (big, np.array([[0, 1, 2]], np.int32)))
    q = np.concatenate([sc.box_queries(v2, 150, 2.0, 10), rc.sample_mesh(v, t, 50, 4)[0]])
    got = sc.grid_mesh_nearest(q, v2, t2, 0.07)
    want = sc.brute_mesh_nearest(q, v2, t2)
    print("dims %s, %d wide, %d queries nearest to the wide triangle" % (got[5], got[4], int((want[1] == len(t)).sum())))
    assert got[4] == 1 and (want[1] == len(t)).sum() > 10
    assert _same(got, want)


# ---- 5. normals -------------------------------------------------------------------------------------------------------------------------
def test_normal_stats_restatement():
    va, ta = SHEET
    vb, tb = sc.tilt(rc.sheet(nx=11, ny=13, seed=1)[0], (0.3 + 0.4, -0.7, 1.1)), rc.sheet(nx=11, ny=13, seed=1)[1]
    rng = np.random.default_rng(0)
    ia = rng.integers(0, len(ta), 1000).astype(np.int32); ib = rng.integers(0, len(tb), 1000).astype(np.int32)
    ia[::50] = -1; ib[7::90] = len(tb); ia[3::200] = len(ta) + 5
    bad = (ia < 0) | (ia >= len(ta)) | (ib >= len(tb))
    s = sc.normal_stats(va, ta, ia, vb, tb, ib)
    terms = sc.normal_terms(va, ta, ia, vb, tb, ib)
    assert s["count"] == int((~bad).sum()) and s["skipped"] == int(bad.sum()) and s["count"] + s["skipped"] == 1000
    assert abs(s["sum"] - terms[:, 0].sum()) <= 1e-12 * s["sum"]
    # two sheets tilted alike, one turned by a further 0.4 rad about x before the common rotation: every pair has |cos| = cos 0.4
    assert np.abs(terms[~bad, 0] - np.cos(0.4)).max() < 1e-5
    assert sc.normal_stats(va, ta, ia[:0], vb, tb, ib[:0]) == dict(sum=0.0, count=0, skipped=0)
    # a degenerate triangle has no normal
    td = np.array([[0, 0, 1]], np.int32)
    assert sc.normal_stats(va, td, np.zeros(3, np.int32), vb, tb, np.zeros(3, np.int32)) == dict(sum=0.0, count=0, skipped=3)


# ---- 6. the grid sizing, host only ----------------------------------------------------------------------------------------------------
def test_surface_plan_test_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", HOST, "surface_plan_test"])
    r = subprocess.run([os.path.join(HOST, "surface_plan_test")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "surface_plan_test: ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]

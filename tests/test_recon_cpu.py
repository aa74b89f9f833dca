"""CPU tests (-m "not gpu") of tests/recon_checks.py: the numpy rules the GPU tests of the reconstruction metrics compare against."""
import numpy as np

import recon_checks as rc


def test_hash_matches_a_scalar_evaluation():
    def scalar(seed, a, b):
        m = (1 << 64) - 1
        x = seed ^ ((0x9E3779B97F4A7C15 * (a + 1)) & m) ^ ((0xC2B2AE3D27D4EB4F * (b + 1)) & m)
        x ^= x >> 33; x = (x * 0xFF51AFD7ED558CCD) & m
        x ^= x >> 33; x = (x * 0xC4CEB9FE1A85EC53) & m
        x ^= x >> 33
        return x >> 32
    for seed in (0, 1, 0xDEADBEEFCAFE, (1 << 64) - 1):
        a = np.array([0, 1, 77, 199999, (1 << 32) - 1])
        for b in (0, 1, 2):
            assert rc.hash_u32(seed, a, b).tolist() == [scalar(seed, int(x), b) for x in a]
    u = rc.sample_u(3, 1000)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()


def test_brute_force_agrees_with_a_float64_kd_tree():
    from scipy.spatial import cKDTree
    q, t = rc.sheet_clouds(6000, 5000)
    d, i = rc.brute_nearest(q, t)
    d64, i64 = cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
    rel = np.abs(d.astype(np.float64) - d64) / d64
    print("brute force against cKDTree: max relative %.2e, %d differing indices" % (rel.max(), int((i != i64).sum())))
    assert rel.max() < 1e-6
    assert (i == i64).all()


def test_brute_force_edge_rules():
    t = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [1, 0, 0], [np.inf, 1, 1]], np.float32)
    q = np.array([[0.9, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0]], np.float32)
    d, i = rc.brute_nearest(q, t)
    assert i.tolist() == [2, 0, -1, -1]                        # duplicates and the tie at 0.5: the lowest index
    assert d[0] == np.float32(np.sqrt(np.float32(np.float32(0.9) - np.float32(1)) ** 2)) and d[1] == np.float32(0.5) and np.isnan(d[2:]).all()
    d, i = rc.brute_nearest(q, t[[1, 4]])
    assert np.isinf(d[:2]).all() and np.isnan(d[2:]).all() and (i == -1).all()


def test_triangle_counts_follow_the_areas():
    v, t = rc.sheet()
    assert len(t) == 286
    ar, deg = rc.tri_areas(v, t)
    assert not deg.any() and abs(ar.sum() - 1.0) < 1e-6
    n = 20000
    _, tri, total, _ = rc.sample_mesh(v, t, n, 0)
    got = np.bincount(tri, minlength=len(t))
    want = n * ar / total
    chi = float((((got - want) ** 2) / want).sum() / (len(t) - 1))
    print("chi^2 / dof = %.2f" % chi)
    # chi^2 / dof of a multinomial draw has mean 1 and deviation sqrt(2 / dof) = 0.084: five deviations
    assert chi < 1.0 + 5.0 * np.sqrt(2.0 / (len(t) - 1))
    # every sample lies in its triangle's plane and inside the sheet
    p = rc.sample_points(v, t, tri, rc.sample_u(0, n))
    assert (p[:, 2] == 0).all() and p[:, :2].min() >= 0 and p[:, :2].max() <= 1


def test_two_associations_of_the_cumulative_area_choose_alike():
    v, t = rc.sheet()
    ar, _ = rc.tri_areas(v, t)
    u0 = rc.sample_u(0, 20000)[:, 0]
    a, gap = rc.choose_tris(rc.cum_sequential(ar), u0)
    b, _ = rc.choose_tris(rc.cum_blocked(ar, 64), u0)
    print("%d differing choices, smallest gap to a boundary %.1e A" % (int((a != b).sum()), gap.min() / ar.sum()))
    assert (a == b).all()
    assert a.min() >= 0 and a.max() < len(t)


def test_degenerate_triangles_have_no_area():
    v, t = rc.sheet(3, 3)
    v = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    t = np.concatenate([t, [[0, 0, 1], [0, 1, len(v) - 1], [0, 1, len(v)], [-1, 0, 1]]]).astype(np.int32)
    ar, deg = rc.tri_areas(v, t)
    assert deg.tolist() == [False] * 18 + [True] * 4 and (ar[-4:] == 0).all()
    _, tri, _, nd = rc.sample_mesh(v, t, 5000, 1)
    assert nd == 4 and tri.max() < 18


def test_stats_rule():
    d = np.array([0.01, 0.05, np.nan, np.inf, 0.2], np.float32)
    s = rc.stats(d, 0.05)
    assert s["count"] == 3 and s["below"] == 1 and s["max"] == float(np.float32(0.2))

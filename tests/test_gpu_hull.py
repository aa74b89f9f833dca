"""GPU tests of the convex hull and the inside mask: nsk_points_hull, nsk_hull_download, nsk_hull_upload, nsk_lattice_in_hull.  What they
must give is computed by tests/hull_checks.py in numpy and Python integers (tests/test_hull_cpu.py proves it against Qhull); the device's
bytes equal it: vertices, faces and counts."""
import numpy as np
import pytest
import torch

import hull_checks as hc
from gpu_util import cu

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


_rule = {}


def rule(name):
    """the restatement's hull of a named cloud, computed once"""
    if name not in _rule:
        _rule[name] = hc.hull(hc.cloud(name))
    return _rule[name]


def dev(points):
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    return cu(p) if p.shape[0] else None


def check(ctx, points, extra=None, want=None):
    want = hc.hull(points, extra) if want is None else want
    v, f, info = ctx.points_hull(dev(points), extra)
    print("points %d + %d: rank %d, %d vertices, %d faces, %d insertions, %d re-compactions (rule: %d, %d, %d, %d)"
          % (len(points), 0 if extra is None else len(extra), info[2], info[3], info[4], info[5], info[7], want["info"][2], want["info"][3],
             want["info"][4], want["info"][5]))
    assert v.dtype == np.int32 and f.dtype == np.int32 and f.shape == (info[4], 3)
    assert info[:7].tobytes() == want["info"][:7].tobytes()
    assert v.tobytes() == want["vertices"].tobytes() and f.tobytes() == np.ascontiguousarray(want["faces"]).tobytes()
    return v, f, info


# ---- 1. the hull ------------------------------------------------------------------------------------------------------------------
def test_four_points_and_a_fifth_outside(ctx):
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    v, f, info = check(ctx, p)
    assert info[2] == 3 and v.tolist() == [0, 1, 2, 3] and f.shape[0] == 4 and info[5] == 0
    v, f, info = check(ctx, np.concatenate([p, [[1, 1, 1]]]).astype(F))
    assert v.tolist() == [0, 1, 2, 3, 4] and f.shape[0] == 6 and info[5] == 1
    v, f, info = check(ctx, np.concatenate([p, [[0.2, 0.2, 0.2]]]).astype(F))
    assert v.tolist() == [0, 1, 2, 3] and info[5] == 0


@pytest.mark.parametrize("points,rank", [(np.eye(3, dtype=F), 2), (np.ones((3, 3), F), 0), (np.tile(F([[1.5, -2.0, 3.0]]), (9, 1)), 0),
                                         (hc.flat_cloud(1), 1), (hc.flat_cloud(2), 2), (np.array([[0, 0, 0], [1, 0, 0]], F), 1)],
                         ids=["three", "three-equal", "repeated-point", "line", "plane", "two"])
def test_no_hull_is_a_success_with_the_rank(ctx, points, rank):
    v, f, info = check(ctx, points)
    assert info[2] == rank and info[3] == 0 and info[4] == 0 and v.size == 0 and f.shape == (0, 3)
    # and the mask of no hull is empty
    valid, n = ctx.lattice_in_hull(F([-1, -1, -1]), F([0.5, 0.5, 0.5]), 9, 9, 9, 1.02)
    assert n == 0 and not bool(valid.any())


@pytest.mark.parametrize("name", ["lattice5", "sphere300", "ball2000", "walls", "repeated"])
def test_hull_equals_the_rule(ctx, name):
    v, f, info = check(ctx, hc.cloud(name), want=rule(name))
    assert info[2] == 3
    if name == "sphere300":
        assert info[3] == 300 and info[5] == 296                      # every point is an insertion


def test_non_finite_rows_are_skipped_and_counted(ctx):
    p = hc.cloud("ball2000")[:40].copy()
    p[3, 1] = np.nan; p[17, 0] = np.inf; p[18, 2] = -np.inf
    v, f, info = check(ctx, p)
    assert info[0] == 37 and info[1] == 3 and not set(v.tolist()) & {3, 17, 18}
    nothing = np.full((5, 3), np.nan, F)
    v, f, info = check(ctx, nothing)
    assert info[0] == 0 and info[1] == 5 and info[2] == 0


def test_host_points(ctx):
    p = hc.cloud("ball2000")[:500]
    far = np.array([[9, 9, 9], [-9, 8, 7], [1, -9, 2], [0, 1, -9], [np.nan, 0, 0]], F)
    v, f, info = check(ctx, p, far)                                   # the extreme ones
    assert {500, 501, 502, 503} <= set(v.tolist()) and info[1] == 1
    inner = (p[:7] * F(0.5) + p.mean(0) * F(0.5)).astype(F)
    v2, f2, info2 = check(ctx, p, inner)                              # all interior
    v0, f0, _ = check(ctx, p)
    assert v2.max() < 500 and v2.tobytes() == v0.tobytes() and f2.tobytes() == f0.tobytes()
    v3, f3, info3 = check(ctx, np.zeros((0, 3), F), p[:60])           # n = 0: the host points alone
    assert info3[2] == 3 and info3[0] == 60
    v4, f4, info4 = check(ctx, np.zeros((0, 3), F), None)
    assert not info4.any()


def test_many_workgroups_and_recompaction(ctx):
    p = hc.cloud("box70000")
    v, f, info = check(ctx, p, want=rule("box70000"))
    assert info[0] == 70000 and info[7] >= 1                          # 274 workgroups at first; the list was re-compacted


def test_two_runs_and_a_fresh_context_give_the_same_bytes(ctx):
    import nice_slam_cpp_amd as pkg
    p = dev(hc.cloud("walls"))
    a = ctx.points_hull(p)
    b = ctx.points_hull(p)
    other = pkg.Context(0)
    c = other.points_hull(p)
    other.close()
    for x in (b, c):
        assert all(u.tobytes() == w.tobytes() for u, w in zip(a, x))


# ---- 2. the mask ----------------------------------------------------------------------------------------------------------------
def lattice_for(points, n):
    lo, hi = points.min(0) - F(0.31), points.max(0) + F(0.27)
    return lo.astype(F), ((hi - lo) / (np.array(n, F) - F(1))).astype(F)


@pytest.mark.parametrize("n", [(17, 13, 9), (33, 33, 33)])
@pytest.mark.parametrize("scale", [1.0, 1.02])
def test_mask_equals_the_rule(ctx, n, scale):
    p = hc.cloud("ball2000")
    h = rule("ball2000")
    v, f, _ = check(ctx, p, want=h)
    o, s = lattice_for(p, n)
    want = hc.lattice_in_hull(o, s, *n, p[v], hc.local_faces(v, f), scale)
    valid, n_in = ctx.lattice_in_hull(o, s, *n, scale)
    got = valid.cpu().numpy()
    print("lattice %s scale %g: %d inside (rule %d), %d bytes differ" % (n, scale, n_in, int(want.sum()), int((got != want).sum())))
    assert got.shape == (n[2], n[1], n[0]) and got.tobytes() == want.tobytes() and n_in == int(want.sum()) and 0 < n_in < want.size


def test_mask_accumulates(ctx):
    p = hc.cloud("ball2000")
    v, f, _ = check(ctx, p, want=rule("ball2000"))
    n = (17, 13, 9)
    o, s = lattice_for(p, n)
    want = hc.lattice_in_hull(o, s, *n, p[v], hc.local_faces(v, f), 1.02)
    old = np.zeros(want.shape, np.uint8)
    old[::2, 1::3, ::4] = 7
    valid, n_in = ctx.lattice_in_hull(o, s, *n, 1.02, valid=cu(old, torch.uint8))
    both = ((old != 0) | (want != 0)).astype(np.uint8)
    assert valid.cpu().numpy().tobytes() == both.tobytes() and n_in == int(both.sum()) and both.sum() > want.sum()


def test_uploaded_cube(ctx):
    xyz = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F) * F([2.0, 1.5, 1.0]) + F([-1.0, -0.5, 0.25])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]          # wound outwards
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    ctx.hull_upload(xyz, faces)
    n = (21, 17, 13)
    o, s = F([-1.6, -1.1, -0.3]), F([0.16, 0.17, 0.15])
    valid, n_in = ctx.lattice_in_hull(o, s, *n, 1.0)
    P = hc.lattice_points(o, s, *n)
    want = ((P >= xyz.min(0).astype(np.float64)) & (P <= xyz.max(0).astype(np.float64))).all(-1).astype(np.uint8)
    assert valid.cpu().numpy().tobytes() == want.tobytes() and n_in == int(want.sum()) and 0 < n_in < want.size
    assert valid.cpu().numpy().tobytes() == hc.lattice_in_hull(o, s, *n, xyz, faces, 1.0).tobytes()
    with pytest.raises(Exception):
        ctx.hull_upload(xyz, np.array([[0, 1, 9]] * 4, np.int32))

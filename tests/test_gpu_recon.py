"""GPU tests of the reconstruction metrics: nsk_mesh_sample, nsk_cloud_nearest, nsk_cloud_stats, Context.recon_metrics and Mesher::eval_recon.
What they must give is computed by tests/recon_checks.py in numpy (tests/test_recon_cpu.py proves those helpers)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import recon_checks as rc
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def cui(a):
    return cu(a, torch.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. sampling ----------------------------------------------------------------------------------------------------------------
SHEET = rc.sheet()


@pytest.mark.parametrize("n", [1, 63, 1000, 20001])
def test_samples_equal_the_rule_bit_for_bit(ctx, n):
    v, t = SHEET
    dv, dt = cu(v), cui(t)
    pts, tri = ctx.sample_mesh(dv, dt, n, 5, want_tri=True)
    area = ctx.last_area
    assert pts.shape == (n, 3) and tri.shape == (n,) and tri.dtype == torch.int32 and ctx.last_degenerate == 0
    pts, tri = pts.cpu().numpy(), tri.cpu().numpy().astype(np.int64)
    ar, _ = rc.tri_areas(v, t)
    cum = rc.cum_sequential(ar)
    u = rc.sample_u(5, n)
    want_tri, gap = rc.choose_tris(cum, u[:, 0])
    sure = gap > 1e-9 * cum[-1]
    print("n %d: area %.15g (numpy %.15g), %d samples within 1e-9 A of a boundary, %d triangles differ, %d points differ" % (
        n, area, cum[-1], int((~sure).sum()), int((tri != want_tri)[sure].sum()), int((bits(pts) != bits(rc.sample_points(v, t, tri, u))).any(1).sum())))
    assert abs(area - cum[-1]) <= 1e-12 * cum[-1]
    assert (~sure).sum() <= 1e-3 * n
    assert (tri[sure] == want_tri[sure]).all()
    assert tri.min() >= 0 and tri.max() < len(t)
    assert (bits(pts) == bits(rc.sample_points(v, t, tri, u))).all()
    again = ctx.sample_mesh(dv, dt, n, 5).cpu().numpy()
    assert (bits(again) == bits(pts)).all()
    other = ctx.sample_mesh(dv, dt, n, 6).cpu().numpy()
    assert (bits(other) != bits(pts)).any()


def test_sampling_edges(ctx):
    import nice_slam_cpp_amd as pkg
    v, t = rc.sheet(3, 3)
    v = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    t = np.concatenate([[[0, 0, 1], [0, 1, len(v) - 1]], t, [[0, 1, len(v)], [-1, 0, 1]]]).astype(np.int32)
    pts, tri = ctx.sample_mesh(cu(v), cui(t), 5000, 1, want_tri=True)
    tri = tri.cpu().numpy()
    assert ctx.last_degenerate == 4 and tri.min() >= 2 and tri.max() < 20
    want = rc.sample_mesh(v, t, 5000, 1)
    assert (tri == want[1]).all() and (bits(pts.cpu().numpy()) == bits(want[0])).all() and abs(ctx.last_area - want[2]) <= 1e-12 * want[2]
    # one triangle; n = 0
    v1 = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32); t1 = np.array([[0, 1, 2]], np.int32)
    pts, tri = ctx.sample_mesh(cu(v1), cui(t1), 300, 9, want_tri=True)
    assert (tri == 0).all() and ctx.last_area == 1.0
    assert (bits(pts.cpu().numpy()) == bits(rc.sample_mesh(v1, t1, 300, 9)[0])).all()
    assert ctx.sample_mesh(cu(v1), cui(t1), 0, 9).shape == (0, 3) and ctx.last_area == 1.0
    # no triangle, no area: errors
    with pytest.raises(pkg.NskError):
        ctx.sample_mesh(cu(v1), cui(np.zeros((0, 3), np.int32)), 10, 0)
    with pytest.raises(pkg.NskError):
        ctx.sample_mesh(cu(v1), cui(np.array([[0, 0, 1]], np.int32)), 10, 0)
    assert ctx.last_area is None


# ---- 2. nearest -------------------------------------------------------------------------------------------------------------------
NQ, NT = 6000, 5000


def _scenes():
    rng = np.random.default_rng(11)
    f = np.float32
    uni = lambda n: rng.uniform(0, 1, (n, 3)).astype(f)
    S = {}
    S["sheets"] = rc.sheet_clouds(NQ, NT)
    # coordinates that are multiples of 2^-4: queries on the targets' planes and half way between them (cell faces, ties)
    S["lattice"] = ((rng.integers(-2, 35, (NQ, 3)) / 32.0).astype(f), (rng.integers(0, 17, (NT, 3)) / 16.0).astype(f))
    S["identical"] = (uni(NQ), np.tile(np.array([[0.3, 0.4, 0.5]], f), (NT, 1)))
    t = uni(NT); t[:, 2] = 0.25
    S["coplanar"] = (uni(NQ), t)
    t = uni(NT); t[:, 1] = -0.5; t[:, 2] = 0.25
    S["collinear"] = (uni(NQ), t)
    S["one_target"] = (uni(NQ), uni(1))
    S["one_query"] = (uni(1), uni(NT))
    t = uni(NT)
    d = rng.normal(size=(NQ, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    S["far"] = ((0.5 + d * np.sqrt(3.0) * rng.uniform(0.5, 1000.0, (NQ, 1))).astype(f), t)
    ball = rng.normal(size=(NT * 9 // 10, 3)); ball *= 1e-3 * rng.uniform(0, 1, (len(ball), 1)) ** (1 / 3) / np.linalg.norm(ball, axis=1, keepdims=True)
    t = np.concatenate([(0.37 + ball).astype(f), uni(NT - len(ball))])[rng.permutation(NT)]
    S["ball"] = (np.concatenate([uni(NQ - 1000), (0.37 + rng.uniform(-2e-3, 2e-3, (1000, 3))).astype(f)]), t)
    t = uni(NT // 2)
    S["duplicates"] = (uni(NQ), np.concatenate([t, t])[rng.permutation(NT)])
    t = uni(NT)
    S["query_is_target"] = (np.concatenate([t[rng.integers(0, NT, 1000)], uni(NQ - 1000)]), t)
    S["odd_small"] = (uni(257), uni(1023))
    S["odd"] = (uni(6001), uni(4999) * np.array([3.0, 1.0, 0.2], f))
    q = uni(NQ); q[::7, 0] = np.nan; q[3::11, 2] = np.inf; q[5::13, 1] = -np.inf
    t = uni(NT); t[::5, 1] = np.nan; t[1::9, 0] = np.inf; t[2::17, 2] = -np.inf
    S["nonfinite"] = (q, t)
    return S


SCENES = _scenes()
_BRUTE = {}


def brute(name):
    if name not in _BRUTE:
        _BRUTE[name] = rc.brute_nearest(*SCENES[name])
    return _BRUTE[name]


def check_nearest(ctx, name, label=""):
    q, t = SCENES[name]
    want_d, want_i = brute(name)
    d, i = ctx.cloud_nearest(cu(q), cu(t), want_index=True)
    assert d.shape == (len(q),) and i.shape == (len(q),) and i.dtype == torch.int32
    d, i = d.cpu().numpy(), i.cpu().numpy()
    nd, ni = int((bits(d) != bits(want_d)).sum()), int((i != want_i).sum())
    print("%s%s: %d x %d, %d distances and %d indices differ from the brute force, %d targets skipped" % (name, label, len(q), len(t), nd, ni, ctx.last_skipped))
    assert nd == 0 and ni == 0
    assert ctx.last_skipped == int((~np.isfinite(t).all(1)).sum())
    only_d = ctx.cloud_nearest(cu(q), cu(t)).cpu().numpy()
    assert (bits(only_d) == bits(d)).all()
    return d, i


@pytest.mark.parametrize("name", sorted(SCENES))
def test_nearest_equals_the_brute_force_bit_for_bit(ctx, name):
    d, i = check_nearest(ctx, name)
    q, t = SCENES[name]
    if name == "query_is_target":
        assert (d[:1000] == 0).all()
    if name == "nonfinite":
        bad = ~np.isfinite(q).all(1)
        assert bad.sum() > 1000 and np.isnan(d[bad]).all() and (i[bad] == -1).all() and np.isfinite(d[~bad]).all()
        assert np.isfinite(t[i[~bad]]).all()
    if name == "duplicates":
        first = {}
        for k, p in enumerate(map(bytes, t)):
            first.setdefault(p, k)
        assert all(first[bytes(t[k])] == k for k in i[:500])


@pytest.mark.parametrize("mode", [1, 2, 4, 5])
@pytest.mark.parametrize("name", ["sheets", "lattice", "far", "nonfinite"])
def test_every_query_form_gives_the_same_bits(ctx, name, mode):
    """cloud_query_mode: bit 0 a wave per query, + 2 queries in input order, + 4 queries in cell order (the default is a thread per query,
    in cell order from 2^19 queries on: at the sizes of these tests that is input order)"""
    ctx.set_tuning("cloud_query_mode", mode)
    try:
        check_nearest(ctx, name, " (mode %d)" % mode)
    finally:
        ctx.set_tuning("cloud_query_mode", 0)


@pytest.mark.parametrize("cells_x4", [1, 64])
def test_the_grid_density_does_not_change_the_bits(ctx, cells_x4):
    ctx.set_tuning("cloud_cells_x4", cells_x4)
    try:
        for name in ("sheets", "lattice", "ball"):
            check_nearest(ctx, name, " (cells_x4 %d)" % cells_x4)
    finally:
        ctx.set_tuning("cloud_cells_x4", 4)


def test_queries_in_cell_order_from_the_threshold_on(ctx):
    """2^19 queries: the first size at which the default form orders the queries by cell"""
    rng = np.random.default_rng(5)
    q = rng.uniform(-0.1, 1.1, (1 << 19, 3)).astype(np.float32); t = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    want_d, want_i = rc.brute_nearest(q, t, chunk=16384)
    d, i = ctx.cloud_nearest(cu(q), cu(t), want_index=True)
    assert (bits(d.cpu().numpy()) == bits(want_d)).all() and (i.cpu().numpy() == want_i).all()
    ctx.profile_begin(); ctx.cloud_nearest(cu(q), cu(t)); groups = ctx.profile_end()
    assert "cloud_order" in groups
    ctx.profile_begin(); ctx.cloud_nearest(cu(q[:-1]), cu(t)); groups = ctx.profile_end()
    assert "cloud_order" not in groups


def test_nearest_without_a_finite_target_and_errors(ctx):
    import nice_slam_cpp_amd as pkg
    q = SCENES["nonfinite"][0]
    t = np.full((40, 3), np.nan, np.float32); t[::2] = [np.inf, 0, 0]
    d, i = ctx.cloud_nearest(cu(q), cu(t), want_index=True)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    bad = ~np.isfinite(q).all(1)
    assert ctx.last_skipped == 40 and (i == -1).all() and np.isnan(d[bad]).all() and (d[~bad] == np.inf).all()
    with pytest.raises(pkg.NskError):
        ctx.cloud_nearest(cu(q), cu(np.zeros((0, 3), np.float32)))
    assert ctx.cloud_nearest(cu(np.zeros((0, 3), np.float32)), cu(SCENES["sheets"][1])).shape == (0,)


def test_larger_clouds_against_a_kd_tree(ctx):
    from scipy.spatial import cKDTree
    q, t = rc.sheet_clouds(50000, 50000, seed=4)
    d = ctx.cloud_nearest(cu(q), cu(t)).cpu().numpy().astype(np.float64)
    d64, _ = cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
    rel = np.abs(d - d64) / d64
    print("50000 x 50000 against cKDTree: max relative %.2e" % rel.max())
    # five fp32 roundings of 2^-24 on d2 bound d by about 2e-7; the factor on top covers the float64 tree choosing another near-tie
    assert rel.max() < 1e-6


# ---- 3. stats ---------------------------------------------------------------------------------------------------------------------
def test_stats_against_numpy_float64(ctx):
    q, t = SCENES["nonfinite"]
    dist = ctx.cloud_nearest(cu(q), cu(t))
    d = dist.cpu().numpy().copy()
    thr = float(np.sort(d[np.isfinite(d)])[len(d) // 3])      # a distance that occurs: it must not count as below itself
    d[1] = np.inf; d[2] = thr
    dist = cu(d)
    got = ctx.cloud_stats(dist, thr)
    want = rc.stats(d, thr)
    print("stats: device %r, numpy %r" % (got, want))
    assert got["count"] == want["count"] == int(np.isfinite(d).sum()) < len(d)
    assert got["below"] == want["below"] and got["below"] == int((d[np.isfinite(d)] < np.float32(thr)).sum())
    assert got["max"] == want["max"]
    assert abs(got["sum"] - want["sum"]) <= 1e-12 * want["sum"]
    assert ctx.cloud_stats(dist, thr) == got
    assert ctx.cloud_stats(cu(np.array([np.nan, np.inf], np.float32)), 1.0) == dict(sum=0.0, count=0, below=0, max=0.0)
    one = ctx.cloud_stats(cu(np.array([0.05], np.float32)), float(np.float32(0.05)))
    assert one["count"] == 1 and one["below"] == 0
    # more entries than one pass of the grid covers
    big = np.abs(np.random.default_rng(2).normal(size=300001)).astype(np.float32)
    got, want = ctx.cloud_stats(cu(big), 0.5), rc.stats(big, 0.5)
    assert got["count"] == want["count"] and got["below"] == want["below"] and got["max"] == want["max"]
    assert abs(got["sum"] - want["sum"]) <= 1e-12 * want["sum"]


# ---- 4. metrics end to end -----------------------------------------------------------------------------------------------------------
def numpy_metrics(ctx, rec, gt, n, threshold, seed):
    """the three numbers formed by numpy from the device's own samples through the brute force"""
    a = ctx.sample_mesh(cu(rec[0]), cui(rec[1]), n, seed).cpu().numpy()
    b = ctx.sample_mesh(cu(gt[0]), cui(gt[1]), n, seed + 1).cpu().numpy()
    acc = rc.stats(rc.brute_nearest(a, b)[0], threshold); comp = rc.stats(rc.brute_nearest(b, a)[0], threshold)
    return 100 * acc["sum"] / acc["count"], 100 * comp["sum"] / comp["count"], 100 * comp["below"] / comp["count"]


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


N_E2E = 20000


def test_two_sheets_three_centimetres_apart(ctx):
    rec = rc.sheet(); gt = rc.sheet(nx=11, ny=13, origin=(0.0, 0.0, 0.03), seed=1)
    m = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n=N_E2E)
    print(m)
    hi = 100 * np.sqrt(0.03 ** 2 + 1.0 / N_E2E)
    assert 3.0 <= m["accuracy_cm"] <= hi and 3.0 <= m["completion_cm"] <= hi
    assert m["completion_ratio_pct"] == 100.0
    assert close(m["rec_area"], 1.0, 1e-6) and close(m["gt_area"], 1.0, 1e-6)
    assert m["rec_degenerate"] == m["gt_degenerate"] == m["rec_skipped"] == m["gt_skipped"] == 0
    assert m["accuracy_max_cm"] >= m["accuracy_cm"] and m["completion_max_cm"] >= m["completion_cm"]
    want = numpy_metrics(ctx, rec, gt, N_E2E, 0.05, 0)
    assert close(m["accuracy_cm"], want[0]) and close(m["completion_cm"], want[1]) and close(m["completion_ratio_pct"], want[2])


def test_a_far_patch_of_the_ground_truth_is_not_completed(ctx):
    rec = rc.sheet()
    # a quarter of the ground truth's area two metres away: (1 + 1/3) in all, 1/3 of it far
    gt = rc.merge(rc.sheet(nx=11, ny=13, origin=(0.0, 0.0, 0.01), seed=1), rc.sheet(nx=5, ny=7, size=(1.0, 1.0 / 3.0), origin=(0.0, 0.0, 2.0), seed=2))
    m = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n=N_E2E, seed=3)
    print(m)
    assert close(m["gt_area"], 4.0 / 3.0, 1e-6)
    assert abs(m["completion_ratio_pct"] - 75.0) <= 100 * 4 * np.sqrt(0.25 * 0.75 / N_E2E)
    want = numpy_metrics(ctx, rec, gt, N_E2E, 0.05, 3)
    assert close(m["accuracy_cm"], want[0]) and close(m["completion_cm"], want[1]) and close(m["completion_ratio_pct"], want[2])


def test_the_extracted_mesh_goes_in_as_it_is(ctx):
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    c = make_ctx(sc)
    b = sc["bound"]
    origin, step = b[:, 0] - np.float32(0.1), (b[:, 1] - b[:, 0] + np.float32(0.2)) / np.float32(11)
    verts, tris = c.extract_mesh(c.eval_lattice("fine", origin, step, 12, 12, 12), origin, step, 0.0)
    assert verts.shape[0] > 0 and tris.shape[0] > 0
    pv, pt = verts.data_ptr(), tris.data_ptr()
    m = c.recon_metrics(verts, tris, verts, tris, n=N_E2E)
    print(m)
    assert verts.data_ptr() == pv and tris.data_ptr() == pt
    # both directions draw from the same surface with different seeds: the means agree statistically, and a sample's nearest
    # neighbour on the same surface is closer than a lattice step
    assert 0 < m["accuracy_cm"] < 100 * float(step.min()) and 0 < m["completion_cm"] < 100 * float(step.min())
    assert abs(m["accuracy_cm"] - m["completion_cm"]) < 0.2 * m["accuracy_cm"]
    assert m["rec_area"] == m["gt_area"] > 0


# ---- 5. C++ ---------------------------------------------------------------------------------------------------------------------------
def write_own_ply(path, v, t):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t))).encode())
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        rec = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)]); rec["n"] = 3; rec["i"] = t
        f.write(rec.tobytes())


def write_ascii_quads(path, nx, ny, z):
    """an ascii PLY of a flat nx x ny sheet of quads with normals -> the (verts, tris) its fan triangulation gives"""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    v = np.stack([gx / nx, gy / ny, np.full(gx.shape, z)], -1).reshape(-1, 3)
    quads = [(k * (nx + 1) + i, k * (nx + 1) + i + 1, (k + 1) * (nx + 1) + i + 1, (k + 1) * (nx + 1) + i) for k in range(ny) for i in range(nx)]
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment quads\nelement vertex %d\nproperty float nx\nproperty float ny\nproperty float nz\n"
                "property double x\nproperty double y\nproperty double z\nelement face %d\nproperty list uchar uint vertex_indices\nend_header\n" % (len(v), len(quads)))
        for p in v:
            f.write("0 0 1 %r %r %r\n" % (float(p[0]), float(p[1]), float(p[2])))
        for q in quads:
            f.write("4 %d %d %d %d\n" % q)
    tris = np.array([(q[0], q[k], q[k + 1]) for q in quads for k in (1, 2)], np.int32)
    return v.astype(np.float32), tris


def test_eval_recon_of_the_host_class_equals_recon_metrics(ctx, tmp_path):
    exe = os.path.join(HOST, "eval_recon_test")
    assert os.path.exists(exe), "build() makes host/eval_recon_test"
    rec = rc.sheet()
    write_own_ply(str(tmp_path / "rec.ply"), *rec)
    gt = write_ascii_quads(str(tmp_path / "gt.ply"), 7, 5, 0.02)
    out = subprocess.run([exe, str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "20000", "0.05", "7"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n=20000, threshold=0.05, seed=7)
    print(got, want)
    for k in ("accuracy_cm", "completion_cm", "completion_ratio_pct", "accuracy_max_cm", "completion_max_cm", "rec_area", "gt_area"):
        assert close(got[k], want[k]), k
    for k in ("rec_degenerate", "gt_degenerate", "rec_skipped", "gt_skipped"):
        assert got[k] == want[k], k

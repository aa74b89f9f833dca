"""GPU tests of the alignment: nsk_cloud_pair_sums, nsk_cloud_transform, nsk_cloud_icp, Context.align_mesh, recon_metrics / recon_depth_l1
with align=True and the host class.  What they must give is computed by tests/icp_checks.py in numpy (tests/test_icp_cpu.py proves it)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import icp_checks as ic
import recon_checks as rc
from gpu_util import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    c = pkg.Context(0)
    yield c
    c.set_tuning("cloud_query_mode", 0); c.set_tuning("cloud_cells_x4", 4)


def cui(a):
    return cu(a, torch.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


OBLIQUE = ic.motion(30.0, (1.0, 2.0, -1.0), (0.3, -0.2, 0.5))


# ---- 1. pair sums ---------------------------------------------------------------------------------------------------------------------
def _clouds(ns, nt, seed):
    rng = np.random.default_rng(seed)
    S = rng.uniform(0, 1, (ns, 3)).astype(np.float32); T = rng.uniform(0, 1, (nt, 3)).astype(np.float32)
    if ns > 100:
        S[::7, 0] = np.nan; S[3::11, 2] = np.inf; S[5::13, 1] = -np.inf
        S[1] = [3e38, 3e38, 3e38]                                    # finite, but not under the oblique transform
    if nt > 100:
        T[::9, 1] = np.nan; T[4::17, 0] = -np.inf
        if ns > 100:
            S[2:40:2] = T[1:20]                                      # queries that are targets (finite ones among them)
        else:
            S[0] = T[1]
    return S, T


SIZES = [(6000, 5000), (257, 1023), (1, 5000), (5000, 1)]


@pytest.mark.parametrize("ns,nt", SIZES)
@pytest.mark.parametrize("which", ["identity", "oblique"])
def test_pair_sums_equal_the_restatement(ctx, ns, nt, which):
    S, T = _clouds(ns, nt, ns + nt)
    M = np.eye(4) if which == "identity" else OBLIQUE
    if which == "oblique":                                          # the targets live where the transform sends the sources
        T = np.where(np.isfinite(T), ic.transform(M, np.where(np.isfinite(T), T, 0).astype(np.float32)), T).astype(np.float32)
    sp, dist, idx, _ = ic.pairs(S, T, M, 0.0)
    fin = np.sort(dist[np.isfinite(dist)])
    dS, dT = cu(S), cu(T)
    # thresholds: a generous one, the median distance itself (it occurs, so it must count), 0 (only a query that is a target), none in reach
    ths = [0.1, float(fin[len(fin) // 2]), 0.0, -1.0]
    for th in ths:
        if th < 0:                                                  # every pair beyond the threshold: move the targets a metre away
            far = T + np.float32(50.0)
            got = ctx.cloud_pair_sums(dS, cu(far), M, 0.1)
            assert (got == 0).all()
            continue
        want, wd, wi = ic.pair_sums(S, T, M, th)
        got, gd, gi = ctx.cloud_pair_sums(dS, dT, M if which == "oblique" else None, th, want_pairs=True)
        gd, gi = gd.cpu().numpy(), gi.cpu().numpy()
        assert ctx.last_skipped == int((~np.isfinite(T).all(1)).sum())
        assert (bits(gd) == bits(wd))[~np.isnan(wd)].all() and (np.isnan(gd) == np.isnan(wd)).all() and (gi == wi).all()
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print("%d x %d %s threshold %.9g: count %d (numpy %d), worst relative difference %.3g" % (ns, nt, which, th, got[0], want[0], rel[want != 0].max(initial=0)))
        assert got[0] == want[0]
        assert (np.abs(got[1:] - want[1:]) <= 1e-12 * np.abs(want[1:])).all()
        if th == ths[1]:
            assert (wd == np.float32(th)).any() and 0 < want[0] < np.isfinite(wd).sum() or ns == 1     # the threshold is a distance that occurs
        if th == 0.0 and nt > 100 and which == "identity":
            assert want[0] > 0                                      # the queries that are targets count at threshold 0


def test_pair_sums_are_the_same_bytes_under_every_mode(ctx):
    S, T = _clouds(6000, 5000, 1)
    dS, dT = cu(S), cu(T)
    ref = None
    try:
        for mode in (0, 1, 2, 4, 5):
            for cells in (1, 4, 64):
                ctx.set_tuning("cloud_query_mode", mode); ctx.set_tuning("cloud_cells_x4", cells)
                for rep in range(2):
                    got = ctx.cloud_pair_sums(dS, dT, OBLIQUE, 0.7).tobytes()
                    ref = ref or got
                    assert got == ref, (mode, cells, rep)
    finally:
        ctx.set_tuning("cloud_query_mode", 0); ctx.set_tuning("cloud_cells_x4", 4)
    assert np.frombuffer(ref, np.float64)[0] > 1000


def test_cell_ordered_queries_give_the_same_bytes(ctx):
    n = 1 << 19                                                     # CLOUD_ORDER_MIN: from here on the sources run in cell order
    rng = np.random.default_rng(2)
    S = rng.uniform(0, 1, (n, 3)).astype(np.float32); T = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    S[::1001, 1] = np.nan
    dS, dT = cu(S), cu(T)
    try:
        a, ad, ai = ctx.cloud_pair_sums(dS, dT, OBLIQUE, 0.6, want_pairs=True)
        ctx.set_tuning("cloud_query_mode", 2)
        b, bd, bi = ctx.cloud_pair_sums(dS, dT, OBLIQUE, 0.6, want_pairs=True)
    finally:
        ctx.set_tuning("cloud_query_mode", 0)
    assert a.tobytes() == b.tobytes() and a[0] > 1000
    assert torch.equal(ai, bi) and torch.equal(ad.view(torch.int32), bd.view(torch.int32))
    # a sample of the correspondences against the brute force
    k = rng.integers(0, n, 2000)
    wd, wi = rc.brute_nearest(ic.transform(OBLIQUE, S[k]), T)
    gd = ad.cpu().numpy()[k]
    assert (ai.cpu().numpy()[k] == wi).all() and (bits(gd) == bits(wd))[np.isfinite(wd)].all()


# ---- 2. the transform -------------------------------------------------------------------------------------------------------------------
def test_transform_equals_numpy_bit_for_bit(ctx):
    rng = np.random.default_rng(4)
    p = (rng.uniform(-3, 3, (10001, 3)) * 10.0 ** rng.integers(-3, 3, (10001, 1))).astype(np.float32)
    p[5] = [np.nan, 1, 2]; p[9] = [0, np.inf, 1]; p[11] = [1, 2, -np.inf]; p[13] = [3e38, -3e38, 3e38]
    d = cu(p)
    for M in (OBLIQUE, np.eye(4), ic.MOVE):
        out = ctx.cloud_transform(M, d)
        assert out.data_ptr() != d.data_ptr()
        with np.errstate(over="ignore"):
            assert (bits(out.cpu().numpy()) == bits(ic.transform(M, p))).all()
    assert (bits(ctx.cloud_transform(None, d).cpu().numpy()) == bits(p)).all()
    for i in (5, 9, 11):                                            # non-finite points pass through with their bits
        assert (bits(ctx.cloud_transform(OBLIQUE, d).cpu().numpy()[i]) == bits(p[i])).all()
    same = d.clone()
    assert ctx.cloud_transform(OBLIQUE, same, out=same) is same     # in place
    assert (bits(same.cpu().numpy()) == bits(ic.transform(OBLIQUE, p))).all()
    assert ctx.cloud_transform(OBLIQUE, d[:0]).shape == (0, 3)


# ---- 3. ICP on the shared scene -----------------------------------------------------------------------------------------------------------
def entry_shift(tol=1e-9):
    """the corner displacement that a difference of tol in every entry of M can cause on the scene's box (|x|, |y| <= 1, |z| <= 0.25)"""
    return float(np.sqrt(3.0) * tol * (1.0 + 1.0 + 0.25 + 1.0))


def test_icp_equals_the_restatement_on_the_scene(ctx):
    S, T, truth = ic.scene()
    wantM, want = ic.scene_icp()
    e_ref = ic.corner_shift(wantM, truth)
    dS, dT = cu(S), cu(T)
    M, info = ctx.cloud_icp(dS, dT)
    R = M[:3, :3]
    e = ic.corner_shift(M, truth)
    print("updates %d (numpy %d), |M - numpy| %.3g, fitness %.9g, rmse %.6e (numpy %.6e), corner displacement %.3e (numpy e_ref %.3e)" % (
        info["iterations"], want["iterations"], np.abs(M - wantM).max(), info["fitness"], info["rmse"], want["rmse"], e, e_ref))
    assert info["iterations"] == want["iterations"] and info["converged"] and not info["degenerate"]
    assert np.abs(M - wantM).max() <= 1e-9
    assert abs(info["fitness"] - want["fitness"]) <= 1e-9 * want["fitness"] and abs(info["rmse"] - want["rmse"]) <= 1e-9 * want["rmse"]
    assert info["correspondences"] == want["correspondences"] and info["target_skipped"] == 0 and info["source_nonfinite"] == 0
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and (M[3] == [0, 0, 0, 1]).all()
    assert e <= e_ref + entry_shift()
    # two runs: the same bytes
    M2, info2 = ctx.cloud_icp(dS, dT)
    assert M2.tobytes() == M.tobytes() and info2 == info
    # the evaluation alone
    M0, i0 = ctx.cloud_icp(dS, dT, max_iter=0)
    assert (M0 == np.eye(4)).all() and i0["iterations"] == 0 and not i0["converged"]
    assert abs(i0["fitness"] - want["history"][0][0]) <= 1e-9 and abs(i0["rmse"] - want["history"][0][1]) <= 1e-9 * want["history"][0][1]
    Mi, ii = ctx.cloud_icp(dS, dT, max_iter=0, init=OBLIQUE)
    assert (Mi == OBLIQUE).all() and ii["iterations"] == 0
    # a start at the answer is honoured
    M1, i1 = ctx.cloud_icp(dS, dT, init=truth)
    assert i1["iterations"] <= 1 and i1["converged"] and ic.corner_shift(M1, truth) <= e_ref + entry_shift()
    # two updates are not enough
    M2, i2 = ctx.cloud_icp(dS, dT, max_iter=2)
    w2M, w2 = ic.icp(S, T, max_iter=2)
    assert i2["iterations"] == 2 and not i2["converged"] and not w2["converged"] and np.abs(M2 - w2M).max() <= 1e-9


def test_icp_without_correspondence_and_degenerate_clouds(ctx):
    import nice_slam_cpp_amd as pkg
    S, T, _ = ic.scene()
    dS = cu(S)
    # a metre apart: nothing within reach
    M, info = ctx.cloud_icp(dS, cu(T + np.float32([0, 0, 1.5])), threshold=0.1)
    assert (M == np.eye(4)).all() and info["fitness"] == 0 and info["iterations"] == 0 and info["correspondences"] == 0 and not info["converged"]
    M, info = ctx.cloud_icp(dS, cu(T + np.float32([0, 0, 1.5])), threshold=0.1, init=ic.MOVE)
    assert (M == ic.MOVE).all() and info["iterations"] == 0
    # collinear clouds (coordinates that are multiples of 2^-10, so the sums are exact): the solve has rank 1
    u = (np.arange(400) / 512.0).astype(np.float32)
    line = np.stack([u, 1 - 2 * u, 0.5 * u], 1).astype(np.float32)
    M, info = ctx.cloud_icp(cu(line + np.float32([2.0 ** -7, 0, 0])), cu(line), threshold=0.1, max_iter=3)
    R = M[:3, :3]
    assert info["degenerate"] and np.isfinite(M).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1) < 1e-13
    # no source: the init; non-finite points are counted
    M, info = ctx.cloud_icp(dS[:0], cu(T), init=ic.MOVE)
    assert (M == ic.MOVE).all() and info["iterations"] == 0
    S2, T2 = S.copy(), T.copy()
    S2[3, 0] = np.nan; S2[9, 2] = np.inf; T2[5, 1] = np.nan
    M, info = ctx.cloud_icp(cu(S2), cu(T2), max_iter=1)
    assert info["source_nonfinite"] == 2 and info["target_skipped"] == 1 and info["correspondences"] == len(S) - 2
    # errors leave the context usable
    for bad in (lambda: ctx.cloud_icp(dS, cu(T[:0])), lambda: ctx.cloud_icp(dS, cu(T), threshold=-0.1), lambda: ctx.cloud_icp(dS, cu(T), max_iter=-1),
                lambda: ctx.cloud_pair_sums(dS, cu(T[:0])), lambda: ctx.cloud_pair_sums(dS, cu(T), threshold=-1.0)):
        with pytest.raises(pkg.NskError):
            bad()
    M, info = ctx.cloud_icp(dS, cu(T))
    assert info["converged"] and np.abs(M - ic.scene_icp()[0]).max() <= 1e-9


def test_the_grid_is_built_once(ctx):
    S, T, _ = ic.scene()
    dS, dT = cu(S), cu(T)
    ctx.cloud_icp(dS, dT)                                           # (the buffers have grown)
    ctx.profile_begin()
    ctx.cloud_nearest(dS, dT)
    one = ctx.profile_end()
    ctx.profile_begin()
    M, info = ctx.cloud_icp(dS, dT)
    prof = ctx.profile_end()
    k = info["iterations"]
    print(prof)
    # one scope per evaluation: icp_query counts evaluations (each a single launch of k_icp_query), icp_sums likewise
    assert k >= 2 and prof["cloud_grid"][0] == one["cloud_grid"][0] == 1 and prof["cloud_box"][0] == 1
    assert prof["icp_query"][0] == k + 1 and prof["icp_sums"][0] == k + 1
    assert "cloud_query" not in prof and "cloud_order" not in prof and "icp_order" not in prof


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------
N_E2E = 20000
# what separates the aligned reconstruction from the unmoved one, as a displacement of its surface points (m): the restatement's own residual
# on these vertices and the 1e-9 per entry allowed between device and restatement; the two roundings of a vertex to float32 (moved, moved
# back: coordinates below 2, half an ulp each, three axes); and the five roundings of a surface sample on either side (values below 1)
def displacement_bound():
    e_mesh = ic.mesh_scene_icp()[2]
    return e_mesh + entry_shift() + 2 * np.sqrt(3.0) * 2.0 ** -24 + 2 * 5 * np.sqrt(3.0) * 2.0 ** -25


def test_recon_metrics_with_alignment(ctx):
    gt, rec0, rec, truth = ic.mesh_scene()
    wantM, want, e_mesh = ic.mesh_scene_icp()
    g = (cu(gt[0]), cui(gt[1]))
    base = ctx.recon_metrics(cu(rec0[0]), cui(rec0[1]), *g, n=N_E2E, seed=3)
    moved = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), *g, n=N_E2E, seed=3)
    again = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), *g, n=N_E2E, seed=3, align=False)
    got = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), *g, n=N_E2E, seed=3, align=True)
    assert again == moved and "transform" not in moved             # the default is what it was
    bound = 100.0 * displacement_bound()
    print("e_mesh %.3e m, bound %.3e cm" % (e_mesh, bound))
    for k in ("accuracy_cm", "completion_cm", "accuracy_max_cm", "completion_max_cm"):
        print("  %s: unmoved %.9f, moved %.9f, aligned %.9f (difference %.3e)" % (k, base[k], moved[k], got[k], abs(got[k] - base[k])))
    assert moved["accuracy_cm"] > base["accuracy_cm"] + 0.5         # without alignment the numbers measure the offset
    for k in ("accuracy_cm", "completion_cm", "accuracy_max_cm", "completion_max_cm"):
        assert abs(got[k] - base[k]) <= bound, k
    assert got["completion_ratio_pct"] == base["completion_ratio_pct"] == 100.0
    assert got["icp_iterations"] == want["iterations"] and np.abs(got["transform"] - wantM).max() <= 1e-9
    assert abs(got["icp_fitness"] - want["fitness"]) <= 1e-9 and abs(got["icp_rmse"] - want["rmse"]) <= 1e-9 * want["rmse"]
    assert ic.corner_shift(got["transform"], truth) <= e_mesh + entry_shift()
    # align_mesh on the vertices is that transform; on surface samples it lands within what two different samplings allow
    M, info = ctx.align_mesh(cu(rec[0]), cu(gt[0]))
    assert M.tobytes() == got["transform"].tobytes() and info["iterations"] == got["icp_iterations"]


def test_align_mesh_on_surface_samples(ctx):
    gt, rec0, rec, truth = ic.mesh_scene()
    # five updates: two samplings of a surface slide towards each other slowly, so where the loop would stop by itself is no fixed point
    # to hold the device to; after a given number of updates it must be where the restatement is
    M, info = ctx.align_mesh(cu(rec[0]), cu(gt[0]), max_iter=5, n_points=3000, rec_tris=cui(rec[1]), gt_tris=cui(gt[1]), seed=3)
    # the restatement on the very samples the device drew (sampling is bit-exact: tests/test_gpu_recon.py)
    s = rc.sample_mesh(rec[0], rec[1], 3000, 3)[0]; t = rc.sample_mesh(gt[0], gt[1], 3000, 4)[0]
    wantM, want = ic.icp(s, t, max_iter=5)
    e_ref = ic.corner_shift(wantM, truth)
    print("updates %d (numpy %d), corner displacement %.3e from %.3e (numpy %.3e), |M - numpy| %.3e" % (
        info["iterations"], want["iterations"], ic.corner_shift(M, truth), ic.corner_shift(np.eye(4), truth), e_ref, np.abs(M - wantM).max()))
    assert info["iterations"] == want["iterations"] == 5 and info["fitness"] == 1.0
    assert np.abs(M - wantM).max() <= 1e-9
    assert ic.corner_shift(M, truth) <= e_ref + entry_shift()
    assert e_ref < ic.corner_shift(np.eye(4), truth)                # and that is nearer than it started


def test_recon_depth_l1_with_alignment(ctx):
    gt, rec0, rec, truth = ic.mesh_scene()
    g = (cu(gt[0]), cui(gt[1]))
    kw = dict(n_views=8, HW=(64, 64), focal=40.0, seed=2)
    base = ctx.recon_depth_l1(cu(rec0[0]), cui(rec0[1]), *g, **kw)
    moved = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), *g, **kw)
    again = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), *g, align=False, **kw)
    got = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), *g, align=True, **kw)
    assert again["depth_l1_cm"] == moved["depth_l1_cm"] and (again["stats"] == moved["stats"]).all() and "transform" not in moved
    # a pixel's depth moves by the displacement over the cosine between its ray and the surface normal; rays that graze the sheet closer
    # than 5 degrees cover no share of a 64 x 64 view that matters, so 1 / cos(85 degrees) bounds the mean
    bound = 100.0 * displacement_bound() / np.cos(np.deg2rad(85.0))
    print("depth L1: unmoved %.9f cm, moved %.9f, aligned %.9f (difference %.3e, bound %.3e); pixels hit by both %s / %s" % (
        base["depth_l1_cm"], moved["depth_l1_cm"], got["depth_l1_cm"], abs(got["depth_l1_cm"] - base["depth_l1_cm"]), bound,
        got["stats"][:, 1], base["stats"][:, 1]))
    assert base["stats"][:, 3].sum() > 0.1 * 8 * 64 * 64            # the views see the sheet
    assert abs(moved["depth_l1_cm"] - base["depth_l1_cm"]) > 10 * bound
    assert abs(got["depth_l1_cm"] - base["depth_l1_cm"]) <= bound
    assert abs(got["restricted_l1_cm"] - base["restricted_l1_cm"]) <= bound
    assert got["icp_iterations"] == ic.mesh_scene_icp()[1]["iterations"] and np.abs(got["transform"] - ic.mesh_scene_icp()[0]).max() <= 1e-9


# ---- 5. the host class ------------------------------------------------------------------------------------------------------------------
def write_ply(path, v, t):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t))).encode())
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        rec = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)]); rec["n"] = 3; rec["i"] = t
        f.write(rec.tobytes())


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


def test_the_host_class_aligns_as_python_does(ctx, tmp_path):
    gt, rec0, rec, truth = ic.mesh_scene()
    write_ply(str(tmp_path / "rec.ply"), *rec); write_ply(str(tmp_path / "gt.ply"), *gt)
    g = (cu(gt[0]), cui(gt[1]))
    # eval_recon_test ... 1
    exe = os.path.join(HOST, "eval_recon_test")
    assert os.path.exists(exe), "build() makes host/eval_recon_test"
    out = subprocess.run([exe, str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), str(N_E2E), "0.05", "3", "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), *g, n=N_E2E, threshold=0.05, seed=3, align=True)
    print(got, want)
    for k in ("accuracy_cm", "completion_cm", "completion_ratio_pct", "accuracy_max_cm", "completion_max_cm", "rec_area", "gt_area", "icp_fitness", "icp_rmse"):
        assert close(got[k], want[k]), k
    for k in ("rec_degenerate", "gt_degenerate", "rec_skipped", "gt_skipped", "icp_iterations"):
        assert got[k] == want[k], k
    assert (np.array(got["transform"]).reshape(4, 4) == want["transform"]).all()
    # the old argument list still means no alignment
    out = subprocess.run([exe, str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), str(N_E2E), "0.05", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    plain = json.loads(out.stdout.strip().splitlines()[-1])
    assert "transform" not in plain and close(plain["accuracy_cm"], ctx.recon_metrics(cu(rec[0]), cui(rec[1]), *g, n=N_E2E, seed=3)["accuracy_cm"])
    # eval_depth_test ... 1
    exe = os.path.join(HOST, "eval_depth_test")
    assert os.path.exists(exe), "build() makes host/eval_depth_test"
    out = subprocess.run([exe, str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "8", "64", "64", "40", "2", "1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    want = ctx.recon_depth_l1(cu(rec[0]), cui(rec[1]), *g, n_views=8, HW=(64, 64), focal=40.0, seed=2, align=True)
    print(got)
    for k in ("depth_l1_cm", "restricted_l1_cm", "icp_fitness", "icp_rmse"):
        assert close(got[k], want[k]), k
    for k in ("n_views", "n_used", "icp_iterations"):
        assert got[k] == want[k], k
    assert got["rec_skipped"] == 0 and got["gt_skipped"] == 0
    assert (np.array(got["transform"]).reshape(4, 4) == want["transform"]).all()

"""GPU tests of the metrics against the surface: nsk_mesh_nearest, nsk_normal_stats, Context.recon_metrics(surface=True) and
Mesher::eval_recon's surface argument.  What they must give is computed by tests/surface_checks.py in numpy (tests/test_surface_cpu.py
proves those helpers and measures the float32 rule's accuracy); the device is held to brute_mesh_nearest(float32) bytes for bytes."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import recon_checks as rc
import surface_checks as sc
from gpu_util import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def cui(a):
    return cu(a, torch.int32)


bits = sc.bits32


# ---- 1. nearest: the brute force's bytes ------------------------------------------------------------------------------------------------
def _scenes():
    S = {}
    (v, t), (v1, t1) = sc.tilted_sheets(0.03)
    S["tilted"] = (rc.sample_mesh(v1, t1, 600, 2)[0], v, t)
    S["box7"] = (sc.box_queries(v, 600, 7.0, 3), v, t)
    fv, ft = rc.sheet(origin=(0.0, 0.0, 0.25))
    S["flat"] = (np.concatenate([rc.sample_mesh(*rc.sheet(nx=11, ny=13, origin=(0.0, 0.0, 0.28), seed=1), 300, 2)[0], sc.box_queries(fv, 300, 3.0, 4)]), fv, ft)
    lo, hi = v.min(0), v.max(0)
    big = np.array([lo, [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]], np.float32)
    wv, wt = rc.merge((v, t), (big, np.array([[0, 1, 2]], np.int32)))
    S["wide"] = (np.concatenate([sc.box_queries(wv, 400, 2.0, 5), rc.sample_mesh(v1, t1, 200, 6)[0]]), wv, wt)
    S["single"] = (sc.box_queries(big, 600, 3.0, 7), big, np.array([[0, 1, 2]], np.int32))
    # everything that does not take part at once: degenerate triangles, indices out of range, a NaN and an infinite vertex; queries that are not finite
    ev = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0]]]).astype(np.float32)
    nv = len(v)
    et = np.concatenate([[[0, 0, 1], [0, 1, nv]], t[:100], [[3, 3, 3], [0, 1, nv + 2], [-1, 0, 1], [2, 5, nv + 1]], t[100:], [[7, 8, 7]]]).astype(np.int32)
    eq = np.concatenate([rc.sample_mesh(v1, t1, 300, 8)[0], sc.box_queries(v, 300, 4.0, 9)])
    eq[::7, 0] = np.nan; eq[3::11, 2] = np.inf; eq[5::13, 1] = -np.inf
    S["left_out"] = (eq, ev, et)
    cv, ct = rc.merge((v, t), (v, t))
    S["coincident"] = (np.concatenate([rc.sample_mesh(v1, t1, 300, 10)[0], rc.sample_mesh(v, t, 300, 11)[0]]), cv, ct)
    return S


SCENES = _scenes()
_BRUTE = {}


def brute(name):
    if name not in _BRUTE:
        _BRUTE[name] = sc.brute_mesh_nearest(*SCENES[name])
    return _BRUTE[name]


def check_nearest(ctx, name, label=""):
    q, v, t = SCENES[name]
    want_d, want_t, want_p = brute(name)
    d, tri, p = ctx.mesh_nearest(cu(q), cu(v), cui(t), want_tri=True, want_point=True)
    skipped = ctx.last_skipped
    assert d.shape == (len(q),) and tri.shape == (len(q),) and tri.dtype == torch.int32 and p.shape == (len(q), 3)
    d, tri, p = d.cpu().numpy(), tri.cpu().numpy(), p.cpu().numpy()
    nd, nt, npt = int((bits(d) != bits(want_d)).sum()), int((tri != want_t).sum()), int((bits(p) != bits(want_p)).any(1).sum())
    print("%s%s: %d queries x %d triangles, %d distances, %d triangles and %d points differ from the brute force, %d triangles skipped" % (
        name, label, len(q), len(t), nd, nt, npt, skipped))
    assert nd == 0 and nt == 0 and npt == 0
    assert skipped == len(t) - len(sc.participating(v, t))
    return d, tri, p


@pytest.mark.parametrize("name", sorted(SCENES))
def test_mesh_nearest_equals_the_brute_force_bytes_for_bytes(ctx, name):
    d, tri, p = check_nearest(ctx, name)
    q, v, t = SCENES[name]
    only_d = ctx.mesh_nearest(cu(q), cu(v), cui(t))
    assert isinstance(only_d, torch.Tensor) and (bits(only_d.cpu().numpy()) == bits(d)).all()
    if name == "left_out":
        bad = ~np.isfinite(q).all(1)
        assert ctx.last_skipped == 7 and bad.sum() > 100
        assert np.isnan(d[bad]).all() and (tri[bad] == -1).all() and np.isnan(p[bad]).all() and np.isfinite(d[~bad]).all()
        assert set(tri[~bad]) <= set(sc.participating(v, t))
    if name == "coincident":
        assert tri.max() < len(t) // 2 and (d[300:] < 1e-6).all()
    if name == "wide":
        assert (tri == len(t) - 1).sum() > 10
    if name == "box7":
        assert d.max() > 1.0


def test_every_setting_gives_the_same_bytes(ctx):
    """surface_query_mode: + 2 queries in input order, + 4 in cell order (0: by size, which is input order here); surface_cells_x4: the
    grid's density, through which a triangle's references and the wide list change.  No setting may change a byte; nor may a second run"""
    try:
        for mode in (0, 2, 4):
            for cells_x4 in (1, 4, 64):
                ctx.set_tuning("surface_query_mode", mode); ctx.set_tuning("surface_cells_x4", cells_x4)
                for name in ("tilted", "box7", "wide", "left_out"):
                    check_nearest(ctx, name, " (mode %d, cells_x4 %d)" % (mode, cells_x4))
        check_nearest(ctx, "tilted", " (again)")
    finally:
        ctx.set_tuning("surface_query_mode", 0); ctx.set_tuning("surface_cells_x4", 16)
    import nice_slam_cpp_amd as pkg
    for key, value in (("surface_query_mode", 1), ("surface_query_mode", 6), ("surface_cells_x4", 0)):
        with pytest.raises(pkg.NskError):
            ctx.set_tuning(key, value)


def test_queries_in_cell_order_from_the_threshold_on(ctx):
    """2^19 queries: the first size at which the default form visits the queries in cell order"""
    v, t = sc.slivers(1e-2)
    q = sc.box_queries(v, 1 << 19, 2.0, 12)
    want = sc.brute_mesh_nearest(q, v, t, chunk=1 << 15)
    d, tri, p = ctx.mesh_nearest(cu(q), cu(v), cui(t), want_tri=True, want_point=True)
    assert (bits(d.cpu().numpy()) == bits(want[0])).all() and (tri.cpu().numpy() == want[1]).all() and (bits(p.cpu().numpy()) == bits(want[2])).all()
    ctx.profile_begin(); ctx.mesh_nearest(cu(q), cu(v), cui(t)); groups = ctx.profile_end()
    assert "surface_order" in groups and "surface_query" in groups
    ctx.profile_begin(); ctx.mesh_nearest(cu(q[:-1]), cu(v), cui(t)); groups = ctx.profile_end()
    assert "surface_order" not in groups


def test_no_participating_triangle_no_query_and_errors(ctx):
    import nice_slam_cpp_amd as pkg
    q, v, t = SCENES["left_out"]
    none = np.array([[0, 0, 1], [0, 1, len(v)], [-1, 0, 1], [0, 1, len(v) - 2]], np.int32)
    d, tri, p = ctx.mesh_nearest(cu(q), cu(v), cui(none), want_tri=True, want_point=True)
    d, tri, p = d.cpu().numpy(), tri.cpu().numpy(), p.cpu().numpy()
    bad = ~np.isfinite(q).all(1)
    assert ctx.last_skipped == 4 and (tri == -1).all() and np.isnan(p).all() and np.isnan(d[bad]).all() and (d[~bad] == np.inf).all()
    want = sc.brute_mesh_nearest(q, v, none)
    assert (bits(d) == bits(want[0])).all() and (bits(p) == bits(want[2])).all()
    with pytest.raises(pkg.NskError):
        ctx.mesh_nearest(cu(q), cu(v), cui(np.zeros((0, 3), np.int32)))
    assert ctx.mesh_nearest(cu(np.zeros((0, 3), np.float32)), cu(v), cui(t)).shape == (0,) and ctx.last_skipped == 7
    check_nearest(ctx, "single", " (after the error)")


# ---- 2. normals -------------------------------------------------------------------------------------------------------------------------
def test_normal_stats_equals_the_restatement(ctx):
    va, ta = SCENES["tilted"][1:]
    vb = sc.tilt(rc.sheet(nx=11, ny=13, seed=1)[0], (0.7, -0.7, 1.1)); tb = rc.sheet(nx=11, ny=13, seed=1)[1]
    tb = np.concatenate([tb, [[0, 0, 1], [0, 1, len(vb)]]]).astype(np.int32)          # a degenerate triangle and one with a vertex out of range
    rng = np.random.default_rng(0)
    ia = rng.integers(0, len(ta), 1000).astype(np.int32); ib = rng.integers(0, len(tb), 1000).astype(np.int32)
    ia[::50] = -1; ib[7::90] = len(tb); ia[3::200] = len(ta) + 5; ib[11::100] = -7
    want = sc.normal_stats(va, ta, ia, vb, tb, ib)
    got = ctx.normal_stats(cu(va), cui(ta), cui(ia), cu(vb), cui(tb), cui(ib))
    print("normal_stats: device %r, numpy %r, sums differ by %.3g relative" % (got, want, abs(got["sum"] - want["sum"]) / want["sum"]))
    assert got["count"] == want["count"] and got["skipped"] == want["skipped"] and got["count"] + got["skipped"] == 1000 and got["skipped"] > 40
    assert np.float64(got["sum"]).view(np.uint64) == np.float64(want["sum"]).view(np.uint64)
    assert ctx.normal_stats(cu(va), cui(ta), cui(ia), cu(vb), cui(tb), cui(ib)) == got
    assert ctx.normal_stats(cu(va), cui(ta), cui(ia[:0]), cu(vb), cui(tb), cui(ib[:0])) == dict(sum=0.0, count=0, skipped=0)
    # more pairs than one pass of the grid covers
    ia = rng.integers(-1, len(ta), 300001).astype(np.int32); ib = rng.integers(0, len(tb), 300001).astype(np.int32)
    want = sc.normal_stats(va, ta, ia, vb, tb, ib)
    got = ctx.normal_stats(cu(va), cui(ta), cui(ia), cu(vb), cui(tb), cui(ib))
    assert got["count"] == want["count"] and got["skipped"] == want["skipped"]
    assert np.float64(got["sum"]).view(np.uint64) == np.float64(want["sum"]).view(np.uint64)


# ---- 3. metrics end to end -----------------------------------------------------------------------------------------------------------
N_E2E = 2000
OLD_KEYS = ["accuracy_cm", "completion_cm", "completion_ratio_pct", "accuracy_max_cm", "completion_max_cm", "rec_area", "gt_area",
            "rec_degenerate", "gt_degenerate", "rec_skipped", "gt_skipped", "n", "threshold"]
NEW_KEYS = ["surface", "precision_pct", "recall_pct", "fscore_pct", "normal_accuracy", "normal_completion", "normal_consistency", "normal_skipped"]


def test_two_tilted_sheets_three_centimetres_apart(ctx):
    rec, gt = sc.tilted_sheets(0.03)
    S = max(np.abs(rec[0]).max(), np.abs(gt[0]).max())
    args = (cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]))
    m = ctx.recon_metrics(*args, n=N_E2E, threshold=0.05, surface=True)
    print(m)
    tol = 100 * 4 * ULP * S
    assert list(m) == OLD_KEYS + NEW_KEYS and m["surface"] is True
    assert abs(m["accuracy_cm"] - 3.0) <= tol and abs(m["completion_cm"] - 3.0) <= tol
    assert m["precision_pct"] == 100.0 and m["recall_pct"] == 100.0 and m["fscore_pct"] == 100.0 and m["completion_ratio_pct"] == 100.0
    assert 1 - 1e-5 <= m["normal_consistency"] <= 1 + 1e-12 and m["normal_skipped"] == 0
    assert m["rec_skipped"] == m["gt_skipped"] == m["rec_degenerate"] == m["gt_degenerate"] == 0
    sampled = ctx.recon_metrics(*args, n=N_E2E, threshold=0.05, surface=False)
    plain = ctx.recon_metrics(*args, n=N_E2E, threshold=0.05)
    print(sampled)
    assert sampled["accuracy_cm"] > m["accuracy_cm"] and sampled["completion_cm"] > m["completion_cm"]
    assert list(sampled) == list(plain) == OLD_KEYS and sampled == plain
    # the figures are those of the calls they are made of
    a, own = ctx.sample_mesh(args[0], args[1], N_E2E, 0, want_tri=True)
    d, hit = ctx.mesh_nearest(a, args[2], args[3], want_tri=True)
    st = ctx.cloud_stats(d, 0.05)
    ns = ctx.normal_stats(args[0], args[1], own, args[2], args[3], hit)
    assert m["accuracy_cm"] == 100.0 * st["sum"] / st["count"] and m["normal_accuracy"] == ns["sum"] / ns["count"]


def test_a_sheet_turned_by_0_4_rad_has_that_normal_consistency(ctx):
    rec = sc.tilted_sheets(0.03)[0]
    v1, t1 = rc.sheet(nx=11, ny=13, origin=(0.0, 0.0, 0.03), seed=1)
    gt = (sc.tilt(v1, (0.3 + 0.4, -0.7, 1.1)), t1)           # turned by 0.4 rad about the sheet's own x axis before the common tilt
    m = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n=N_E2E, threshold=0.05, surface=True)
    print(m)
    for k in ("normal_accuracy", "normal_completion", "normal_consistency"):
        assert abs(m[k] - np.cos(0.4)) <= 1e-5, k
    assert m["normal_skipped"] == 0 and 0 < m["precision_pct"] < 100 and 0 < m["fscore_pct"] < 100
    p, r = m["precision_pct"], m["recall_pct"]
    assert m["fscore_pct"] == 2.0 * p * r / (p + r) and r == m["completion_ratio_pct"]


def test_alignment_and_the_surface_together(ctx):
    rec, gt = sc.tilted_sheets(0.03)
    m = ctx.recon_metrics(cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]), n=N_E2E, threshold=0.05, align=True, surface=True)
    print({k: v for k, v in m.items() if k != "transform"})
    assert list(m) == OLD_KEYS + NEW_KEYS + ["transform", "icp_fitness", "icp_rmse", "icp_iterations"]
    assert m["transform"].shape == (4, 4) and m["surface"] is True and np.isfinite(m["accuracy_cm"]) and np.isfinite(m["normal_consistency"])
    assert m["accuracy_cm"] <= 3.0 + 1e-3


# ---- 4. C++ ---------------------------------------------------------------------------------------------------------------------------
def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


def test_eval_recon_of_the_host_class_with_the_surface_argument(ctx, tmp_path):
    exe = os.path.join(HOST, "eval_recon_test")
    assert os.path.exists(exe), "build() makes host/eval_recon_test"
    rec, gt = sc.tilted_sheets(0.03)
    sc.write_ply(str(tmp_path / "rec.ply"), *rec); sc.write_ply(str(tmp_path / "gt.ply"), *gt)
    base = [exe, str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), "2000", "0.05", "0", "0"]
    out = subprocess.run(base + ["1"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    args = (cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]))
    want = ctx.recon_metrics(*args, n=2000, threshold=0.05, seed=0, surface=True)
    print(got, want)
    assert list(got) == OLD_KEYS + NEW_KEYS and got["surface"] is True
    for k in ("accuracy_cm", "completion_cm", "completion_ratio_pct", "accuracy_max_cm", "completion_max_cm", "rec_area", "gt_area",
              "precision_pct", "recall_pct", "fscore_pct", "normal_accuracy", "normal_completion", "normal_consistency"):
        assert close(got[k], want[k]), k
    for k in ("rec_degenerate", "gt_degenerate", "rec_skipped", "gt_skipped", "normal_skipped"):
        assert got[k] == want[k], k
    # without the argument: the line the program has always printed
    out = subprocess.run(base[:-1], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    old = json.loads(out.stdout.strip().splitlines()[-1])
    want = ctx.recon_metrics(*args, n=2000, threshold=0.05, seed=0)
    assert list(old) == OLD_KEYS
    for k in OLD_KEYS[:7]:
        assert close(old[k], want[k]), k
    for k in OLD_KEYS[7:11]:
        assert old[k] == want[k], k
    # the argument given as 0: the sampled figures, with the new fields at their defaults
    out = subprocess.run(base + ["0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    zero = json.loads(out.stdout.strip().splitlines()[-1])
    assert zero["surface"] is False and all(zero[k] == old[k] for k in OLD_KEYS)

"""GPU tests of culling a mesh to what a trajectory saw and of the depth views clear of the unseen: nsk_points_seen, nsk_mesh_select,
nsk_points_view_counts, Context.cull_mesh / unseen_points / depth_views_clear / recon_depth_l1(unseen=...), Mesher::cull_mesh.  What they
must give is computed by tests/cull_checks.py in numpy (tests/test_cull_cpu.py proves those helpers); the device must agree byte for byte."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import cull_checks as cc
import mesh_checks as mc
import mesh_cull_checks as mcc
import raster_checks as rc
import scenes
from gpu_util import cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
F = np.float32
H, W, INTR = mcc.IMG_H, mcc.IMG_W, mcc.INTR              # 24 x 32, fx = fy = 40, cx = 15.5, cy = 11.5
EPS = 0.5                                                # exact in float32, so D + eps is one rounding of an exact sum


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def cui(a):
    return cu(a, torch.int32)


def cub(a):
    return cu(a, torch.uint8)


# ---- the inputs of the points_seen tests ----------------------------------------------------------------------------------------------
# Frame 0 is the identity camera: c = p exactly and d = -z, so a point can be put on a decision boundary exactly.  At d = 5 the projection
# is u = 15.5 + 8 x, v = 11.5 - 8 y with every operation exact for the x, y used below.
@functools.lru_cache(None)
def pool():
    """-> dict(pts [1000, 3], w2c [65, 4, 4], depths [65, 24, 32], named indices of the special points)"""
    rng = np.random.default_rng(11)
    w2c = np.concatenate([rc.look()[None], rc.orbit_views(64, radius=4.0, seed=2)]).astype(F)
    depths = np.stack([mcc.depth_image(H, W, 4.0 + 0.05 * k, 9.0 - 0.03 * k) for k in range(65)])
    D0 = depths[0]
    def step(x, k):                                              # k float32 steps up (k > 0) or down
        x = F(x)
        for _ in range(abs(k)):
            x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
        return x
    up, dn = (lambda x: step(x, 4)), (lambda x: step(x, -4))    # (four steps: one step of x is half a step of u = 15.5 + 8 x near the far edges)
    pix = lambda i, j, d=5.0: [(i - 15.5) * d / 40.0, (11.5 - j) * d / 40.0, -d]
    lim = F(D0[15, 20] + F(EPS))
    named = dict(
        nan=[np.nan, 0.0, -5.0], inf=[0.5, np.inf, -5.0], behind=[0.3, 0.2, 1.0], on_plane=[0.3, 0.2, 0.0],
        half_u=[0.125, 0.0, -5.0], half_v=[0.0, 0.125, -5.0],                  # u + 0.5 = 17, v + 0.5 = 11 exactly
        left_in0=[-2.0, 0.0, -5.0], left_out0=[dn(-2.0), 0.0, -5.0],           # u + 0.5 = 0: pixel 0, and just below
        right_out0=[2.0, 0.0, -5.0], right_in0=[dn(2.0), 0.0, -5.0],           # u + 0.5 = 32: pixel 32 is outside
        left_in3=[-1.625, 0.0, -5.0], left_out3=[dn(-1.625), 0.0, -5.0],       # pixel 3 / 2 (edge 3)
        right_out3=[1.625, 0.0, -5.0], right_in3=[dn(1.625), 0.0, -5.0],       # pixel 29 / 28 (edge 3)
        top_in0=[0.0, 1.5, -5.0], top_out0=[0.0, up(1.5), -5.0],               # v + 0.5 = 0
        bottom_out0=[0.0, -1.5, -5.0], bottom_in0=[0.0, up(-1.5), -5.0],       # v + 0.5 = 24
        top_in3=[0.0, 1.125, -5.0], top_out3=[0.0, up(1.125), -5.0], bottom_out3=[0.0, -1.125, -5.0], bottom_in3=[0.0, up(-1.125), -5.0],
        depth_zero=pix(2, 2), depth_nan=pix(W // 2 - 2, H // 2), depth_inf=pix(W // 2 + 1, H // 2 - 2),
        at_limit=pix(20, 15, float(lim)), past_limit=pix(20, 15, float(step(lim, 1))))              # one ulp past D + eps
    names = list(named)
    pts = rng.uniform((-6, -4, -10), (6, 4, 2), (1000, 3))
    pts[1:1 + len(names)] = [named[k] for k in names]           # (point 0 stays an ordinary one: n = 1)
    assert D0[2, 2] == 0 and np.isnan(D0[H // 2, W // 2 - 2]) and np.isinf(D0[H // 2 - 2, W // 2 + 1]) and np.isfinite(lim)
    return dict(pts=pts.astype(F), w2c=w2c, depths=depths, idx={k: 1 + q for q, k in enumerate(names)})


def test_the_special_points_stand_where_they_claim():
    """frame 0 alone, by the restatement: the inputs exercise the boundaries they are named after"""
    P = pool()
    one = lambda edge, **kw: cc.points_seen(P["pts"], P["w2c"][:1], INTR, (H, W), edge=edge, eps=EPS, **kw)
    at = lambda m, k: int(m[P["idx"][k]])
    f0, f3 = one(0), one(3)
    for k in ("nan", "inf", "behind", "on_plane", "left_out0", "right_out0", "top_out0", "bottom_out0"):
        assert at(f0, k) == 0, k
    for k in ("half_u", "half_v", "left_in0", "right_in0", "top_in0", "bottom_in0", "depth_zero", "depth_nan", "depth_inf", "at_limit", "past_limit"):
        assert at(f0, k) == 1, k
    for k in ("left_in3", "right_in3", "top_in3", "bottom_in3"):
        assert at(f3, k) == 1, k
    for k in ("left_out3", "right_out3", "top_out3", "bottom_out3", "left_in0"):
        assert at(f3, k) == 0, k
    d0, d1 = one(0, depths=P["depths"][:1]), one(0, depths=P["depths"][:1], zero_sees=True)
    assert [at(d0, k) for k in ("depth_zero", "depth_nan", "depth_inf", "at_limit", "past_limit")] == [0, 0, 0, 1, 0]
    assert [at(d1, k) for k in ("depth_zero", "depth_nan", "depth_inf", "at_limit", "past_limit")] == [1, 0, 0, 1, 0]


MODES = (("depth", False), ("depth", True), ("null", False))


def _seen_both(ctx, n, K, edge, mode, zero_sees):
    P = pool()
    pts, w, d = P["pts"][:n], P["w2c"][:K], (P["depths"][:K] if mode == "depth" else None)
    want = cc.points_seen(pts, w, INTR, (H, W), d, edge, EPS, zero_sees)
    dd = None if d is None else (cu(d) if K else torch.empty((0, H, W), device="cuda"))
    got, n_seen = ctx.points_seen(cu(pts).reshape(-1, 3), w, INTR, (H, W), dd, edge, EPS, zero_sees)
    return want, got.cpu().numpy(), n_seen


@pytest.mark.parametrize("K", [0, 1, 32, 33, 65])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 257, 1000])
def test_points_seen_equals_the_restatement(ctx, n, K):
    for edge in (0, 3):
        for mode, zero_sees in MODES:
            want, got, n_seen = _seen_both(ctx, n, K, edge, mode, zero_sees)
            assert got.dtype == np.uint8 and got.shape == (n,)
            assert (got == want).all(), "n %d K %d edge %d %s zero_sees %d: %d bytes differ" % (n, K, edge, mode, zero_sees, int((got != want).sum()))
            assert n_seen == int(want.sum())
    if n == 1000 and K >= 1:
        want = _seen_both(ctx, n, K, 0, "depth", False)[0]
        assert 0 < want.sum() < n


def test_points_seen_accumulates_and_clears(ctx):
    P = pool()
    pts, dev = P["pts"], cu(P["pts"])
    for mode, zero_sees in MODES:
        d = cu(P["depths"]) if mode == "depth" else None
        sl = lambda a, b: None if d is None else d[a:b].contiguous()
        one, n1 = ctx.points_seen(dev, P["w2c"], INTR, (H, W), d, 0, EPS, zero_sees)
        part, na = ctx.points_seen(dev, P["w2c"][:20], INTR, (H, W), sl(0, 20), 0, EPS, zero_sees)
        assert (part.cpu().numpy() == cc.points_seen(pts, P["w2c"][:20], INTR, (H, W), None if d is None else P["depths"][:20], 0, EPS, zero_sees)).all()
        both, nb = ctx.points_seen(dev, P["w2c"][20:], INTR, (H, W), sl(20, 65), 0, EPS, zero_sees, seen=part)
        assert both.data_ptr() == part.data_ptr() and torch.equal(both, one) and nb == n1 == int(one.sum()) and na <= nb
        kept, nk = ctx.points_seen(dev, P["w2c"][:0], INTR, (H, W), None, 0, EPS, zero_sees, seen=both)        # K = 0, accumulate: unchanged
        assert torch.equal(kept, one) and nk == n1
    cleared, nc = ctx.points_seen(dev, P["w2c"][:0], INTR, (H, W))                                              # K = 0: cleared
    assert nc == 0 and int(cleared.sum()) == 0


def test_points_seen_agrees_with_lattice_seen(ctx):
    """the new kernel on the lattice's node points gives the bytes of the kernel the map's own mesh is culled with"""
    sc = mcc.cull_scene(scenes.REF_BOUND)
    pts = mc.lattice_points(sc["origin"], sc["step"], sc["nx"], sc["ny"], sc["nz"])
    for edge, trunc in sc["params"]:
        valid, n_lat = ctx.lattice_seen(sc["origin"], sc["step"], sc["nx"], sc["ny"], sc["nz"], cu(sc["depths"]), sc["intr"], sc["w2c"], edge, trunc)
        got, n_pts = ctx.points_seen(cu(pts), sc["w2c"], sc["intr"], (mcc.IMG_H, mcc.IMG_W), cu(sc["depths"]), edge, trunc)
        assert torch.equal(got, valid.reshape(-1)) and n_pts == n_lat and 0 < n_pts < got.numel()


# ---- mesh_select ------------------------------------------------------------------------------------------------------------------------
def _select_input(nv, seed=3):
    """nv vertices, nv triangles; the last five vertices are named by no triangle; a repeated index, -1 and nv among the indices"""
    rng = np.random.default_rng(seed + nv)
    verts = rng.normal(size=(nv, 3)).astype(F)
    tris = rng.integers(0, nv - 5, (nv, 3)).astype(np.int32)
    tris[3] = (tris[3, 0], tris[3, 0], tris[3, 1])
    tris[7, 1] = -1
    tris[11, 2] = nv
    return verts, tris, (rng.random(nv) < 0.7).astype(np.uint8)


def _select_both(ctx, verts, tris, mask, part):
    want = cc.select(verts, tris, mask, part)
    got = ctx.mesh_select(cu(verts), cui(tris), cub(mask), part)
    again = ctx.mesh_select(cu(verts), cui(tris), cub(mask), part)
    for a, b in zip(got[:3], again[:3]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), "two runs differ"
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and tuple(got[0].shape) == want[0].shape
    assert got[1].cpu().numpy().tobytes() == want[1].tobytes() and tuple(got[1].shape) == want[1].shape
    assert got[2].cpu().numpy().tobytes() == want[2].tobytes()
    assert got[3] == want[3] == again[3]
    return got


@pytest.mark.parametrize("nv", [255, 256, 257, 65537])
def test_mesh_select_equals_the_restatement(ctx, nv):
    verts, tris, mask = _select_input(nv)
    kept = [_select_both(ctx, verts, tris, mask, part) for part in (0, 1)]
    assert kept[0][3] == 2 and kept[0][1].shape[0] + kept[1][1].shape[0] + kept[0][3] == nv
    assert kept[0][1].shape[0] > 0 and kept[1][1].shape[0] > 0
    ones, zeros = np.ones(nv, np.uint8), np.zeros(nv, np.uint8)
    ident = _select_both(ctx, verts, tris, ones, 0)                       # the identity up to dropped vertices
    assert ident[1].shape[0] == nv - 2 and ident[0].shape[0] <= nv - 5
    for mask2, part in ((zeros, 0), (ones, 1)):                           # the empty result
        e = _select_both(ctx, verts, tris, mask2, part)
        assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0,) and e[3] == 2
    assert _select_both(ctx, verts, tris, zeros, 1)[1].shape[0] == nv - 2


def test_mesh_select_without_triangles_or_vertices(ctx):
    verts, tris, mask = _select_input(256)
    e = _select_both(ctx, verts, tris[:0], mask, 0)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[3] == 0
    e = _select_both(ctx, verts[:0], tris[:4], mask[:0], 1)               # every index is out of range
    assert e[1].shape == (0, 3) and e[3] == 4


# ---- points_view_counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [0, 1, 33])
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_view_counts_equal_the_restatement(ctx, n, V):
    P = pool()
    pts, w = P["pts"][:n], P["w2c"][:V]
    for edge in (0, 3):
        want = cc.view_counts(pts, w, (H, W), INTR, edge)
        got = ctx.points_view_counts(cu(pts).reshape(-1, 3), w, (H, W), INTR, edge)
        assert got.dtype == np.int64 and got.shape == (V,) and (got == want).all(), (n, V, edge, got, want)
    if n == 1000 and V == 33:
        assert want.max() > 1 and (want > 0).sum() > 8                      # waves add to shared counters
        nans = np.full((130, 3), np.nan, F)
        both = ctx.points_view_counts(cu(np.concatenate([nans, pts, nans])), w, (H, W), INTR, 3)
        assert (both == want).all(), "a NaN point was counted"


# ---- cull_mesh ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def cull_scene(name):
    """(verts, tris, w2c, intr, HW, sensor depths, eps) of the CPU file's scenes; the room's sensor depth is its own rendering"""
    if name == "room":
        verts, tris, _ = cc.room()
        w = cc.room_trajectory()
        return verts, tris, w, cc.ROOM_INTR, cc.ROOM_HW, rc.render(verts, tris, w, *cc.ROOM_HW, *cc.ROOM_INTR)[0], 0.03
    verts, tris, _, w = cc.sheets()
    return verts, tris, w, cc.SHEETS_INTR, cc.SHEETS_HW, rc.render(verts, tris, w, *cc.SHEETS_HW, *cc.SHEETS_INTR)[0], cc.SHEETS_EPS


@pytest.mark.parametrize("occlusion", ["none", "depth", "self"])
@pytest.mark.parametrize("name", ["room", "sheets"])
def test_cull_mesh_equals_the_restatement(ctx, name, occlusion):
    verts, tris, w, intr, HW, depths, eps = cull_scene(name)
    want = cc.cull_mesh(verts, tris, w, intr, HW, depths, occlusion, 0, eps)
    for fpb in (1, 2, 32):
        got = ctx.cull_mesh(cu(verts), cui(tris), w, intr, HW, depths if fpb == 2 else cu(depths), occlusion, 0, eps, frames_per_batch=fpb)
        assert sorted(got) == ["n_seen", "seen", "skipped", "tris", "vertex_src", "verts"]
        for k in ("verts", "tris", "seen", "vertex_src"):
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), (name, occlusion, fpb, k)
        assert got["n_seen"] == want["n_seen"] and got["skipped"] == want["skipped"] == 0
    assert 0 < want["n_seen"] < len(verts) or (name == "sheets" and occlusion == "none")
    # the unseen complement's samples lie on triangles that were not kept
    seen = cub(want["seen"])
    assert ctx.unseen_points(cu(verts), cui(tris), seen, 0).shape == (0, 3)
    assert ctx.unseen_points(cu(verts), cui(tris), torch.ones_like(seen), 50).shape == (0, 3)
    if want["n_seen"] < len(verts):
        cv, ct, _, _ = cc.select(verts, tris, want["seen"], 1)
        u = ctx.unseen_points(cu(verts), cui(tris), seen, 200, seed=4)
        assert u.shape == (200, 3) and torch.equal(u, ctx.sample_mesh(cu(cv), cui(ct), 200, 4))


# ---- depth views clear of the unseen ----------------------------------------------------------------------------------------------------
def test_depth_views_clear_equals_the_restatement(ctx):
    gt = rc.cube_room(cc.ROOM_LO, cc.ROOM_HI)
    patch = cc.wall_patch()
    want = cc.clear_views(cc.room_box(), patch, cc.CLEAR_VIEWS, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0)
    w, idx, tried = ctx.depth_views_clear(cu(gt[0]), cu(patch), cc.CLEAR_VIEWS, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0)
    assert w.dtype == np.float32 and w.tobytes() == want[0].tobytes() and (idx == want[1]).all() and tried == want[2]
    assert len(idx) == cc.CLEAR_VIEWS and tried > cc.CLEAR_VIEWS
    Hc, Wc = cc.CLEAR_HW
    cam = (cc.CLEAR_FOCAL, cc.CLEAR_FOCAL, Wc / 2.0 - 0.5, Hc / 2.0 - 0.5)
    assert (ctx.points_view_counts(cu(patch), w, cc.CLEAR_HW, cam) == 0).all()
    # no unseen point: the stream's first views
    w0, idx0, tried0 = ctx.depth_views_clear(cu(gt[0]), cu(patch[:0]).reshape(0, 3), 5, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0)
    assert (idx0 == np.arange(5)).all() and tried0 == 5 and w0.tobytes() == rc.draw_views(cc.room_box(), 5, 0, 0.7).tobytes()


def test_depth_views_clear_returns_short(ctx):
    gt = rc.cube_room(cc.ROOM_LO, cc.ROOM_HI)
    w, idx, tried = ctx.depth_views_clear(cu(gt[0]), cu(cc.box_scatter()), 4, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0, max_factor=4)
    want = cc.clear_views(cc.room_box(), cc.box_scatter(), 4, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0, max_factor=4)
    assert w.shape == (0, 4, 4) and len(idx) == 0 and tried == 16 == want[2] and len(want[1]) == 0


def _room_pair():
    gt = rc.cube_room(cc.ROOM_LO, cc.ROOM_HI)
    rng = np.random.default_rng(8)
    return ((gt[0] + rng.uniform(-0.05, 0.05, gt[0].shape)).astype(F), gt[1]), gt


def test_recon_depth_l1_with_unseen_points(ctx):
    rec, gt = _room_pair()
    patch = cc.wall_patch()
    Hc, Wc = cc.CLEAR_HW
    cam = (cc.CLEAR_FOCAL, cc.CLEAR_FOCAL, Wc / 2.0 - 0.5, Hc / 2.0 - 0.5)
    args = (cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]))
    r = ctx.recon_depth_l1(*args, n_views=cc.CLEAR_VIEWS, HW=cc.CLEAR_HW, focal=cc.CLEAR_FOCAL, seed=0, unseen=cu(patch))
    want = cc.clear_views(cc.room_box(), patch, cc.CLEAR_VIEWS, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0)
    assert r["w2c"].tobytes() == want[0].tobytes() and (r["view_index"] == want[1]).all() and r["candidates_tried"] == want[2]
    assert (ctx.points_view_counts(cu(patch), r["w2c"], cc.CLEAR_HW, cam) == 0).all(), "a used view has an unseen point in its image"
    assert r["n_used"] == cc.CLEAR_VIEWS == len(r["view_l1"])
    dg = ctx.mesh_depth(args[2], args[3], r["w2c"], Hc, Wc, *cam)
    dr = ctx.mesh_depth(args[0], args[1], r["w2c"], Hc, Wc, *cam)
    st = ctx.depth_pair_stats(dg, dr)
    l1 = 0.0
    for k in range(len(st)):
        l1 += st[k, 0] / (Hc * Wc)
    assert r["depth_l1_cm"] == 100.0 * l1 / len(st) and r["depth_l1_cm"] > 0
    plain = ctx.recon_depth_l1(*args, n_views=cc.CLEAR_VIEWS, HW=cc.CLEAR_HW, focal=cc.CLEAR_FOCAL, seed=0)
    assert plain["w2c"].tobytes() != r["w2c"].tobytes()


def test_recon_depth_l1_without_unseen_is_unchanged(ctx):
    rec, gt = _room_pair()
    args = (cu(rec[0]), cui(rec[1]), cu(gt[0]), cui(gt[1]))
    a = ctx.recon_depth_l1(*args, n_views=7, HW=cc.CLEAR_HW, focal=cc.CLEAR_FOCAL, seed=3)
    b = ctx.recon_depth_l1(*args, n_views=7, HW=cc.CLEAR_HW, focal=cc.CLEAR_FOCAL, seed=3, unseen=None, max_factor=16)
    assert list(a) == list(b) and "candidates_tried" not in a and "view_index" not in a
    assert list(a) == ["depth_l1_cm", "n_used", "restricted_l1_cm", "view_l1", "view_cover", "stats", "w2c", "n_views", "H", "W", "focal", "seed",
                       "shrink", "min_cover"]
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and type(a[k]) is type(b[k]), k
    want = rc.depth_l1(rec, gt, 7, *cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=3)
    assert abs(a["depth_l1_cm"] - want[0]) <= 1e-9 * want[0] and a["n_used"] == want[1]


# ---- end to end: the host program ------------------------------------------------------------------------------------------------------
def _write_ply(path, v, t):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t))).encode())
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        rec = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)])
        rec["n"], rec["i"] = 3, t
        f.write(rec.tobytes())


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw[:raw.index(b"end_header\n") + 11], raw[raw.index(b"end_header\n") + 11:]
    nv = int(head.split(b"element vertex ")[1].split()[0]); nt = int(head.split(b"element face ")[1].split()[0])
    assert b"red" not in head
    v = np.frombuffer(body[:12 * nv], "<f4").reshape(nv, 3)
    t = np.frombuffer(body[12 * nv:], dtype=[("n", "u1"), ("i", "<i4", 3)])
    assert len(t) == nt and (t["n"] == 3).all()
    return v, t["i"].astype(np.int32)


def test_host_program_culls_the_room_as_python_does(ctx, tmp_path):
    exe = os.path.join(HOST, "cull_mesh_test")
    assert os.path.exists(exe), "build() makes host/cull_mesh_test"
    verts, tris, wall, twall = cc.room_with_panel()
    c2w = cc.panel_trajectory()
    w2c = np.stack([mcc.w2c_of(m) for m in c2w])                            # (the program inverts the float32 c2w in double, as this does)
    Hh, Wh = cc.E2E_HW
    five = twall != 1
    sensor = ctx.mesh_depth(cu(verts), cui(tris[five]), w2c, Hh, Wh, *cc.E2E_INTR)          # the sensor never measured the wall x = hi
    d = str(tmp_path)
    np.save(os.path.join(d, "c2ws.npy"), c2w.astype(F)); np.save(os.path.join(d, "intr.npy"), np.array(cc.E2E_INTR, F))
    np.save(os.path.join(d, "depths.npy"), sensor.cpu().numpy())
    _write_ply(os.path.join(d, "in.ply"), verts, tris)
    out = subprocess.run([exe, d, os.path.join(d, "in.ply"), os.path.join(d, "out.ply"), "depth", "0", repr(cc.E2E_EPS), "300", os.path.join(d, "unseen.npy")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    js = json.loads(out.stdout.strip().splitlines()[-1])
    py = ctx.cull_mesh(cu(verts), cui(tris), w2c, cc.E2E_INTR, cc.E2E_HW, sensor, "depth", 0, cc.E2E_EPS)
    pv, pt = _read_ply(os.path.join(d, "out.ply"))
    assert pv.tobytes() == py["verts"].cpu().numpy().tobytes() and pt.tobytes() == py["tris"].cpu().numpy().tobytes()
    assert js["vertices"] == len(pv) and js["triangles"] == len(pt) and js["n_seen"] == py["n_seen"] and js["skipped"] == 0
    assert js["in_vertices"] == len(verts) and js["in_triangles"] == len(tris) and js["frames"] == 3 and js["unseen_points"] == 300
    # that wall is entirely in the complement, and it is the whole complement
    seen = py["seen"].cpu().numpy().astype(bool)
    assert not seen[wall == 1].any() and seen[wall != 1].all()
    assert (twall[np.isin(tris, np.nonzero(seen)[0]).all(1)] != 1).all() and len(pt) == int(five.sum())
    u = np.load(os.path.join(d, "unseen.npy"))
    assert u.shape == (300, 3) and u.dtype == np.float32
    # (a sample is (w_a a + w_b b) + w_c c with weights that sum to 1 up to their own rounding: a few ulps of 2 off the plane at most)
    tol = 2e-6
    assert (np.abs(u[:, 0] - cc.ROOM_HI[0]) <= tol).all() and (np.abs(u[:, 1]) <= 1.0 + tol).all() and (np.abs(u[:, 2]) <= 2.0 + tol).all(), "an unseen point off the wall x = hi"
    assert u.tobytes() == ctx.unseen_points(cu(verts), cui(tris), py["seen"], 300, 0).cpu().numpy().tobytes()


def test_host_program_streams_more_frames_than_a_batch(ctx, tmp_path):
    """33 frames of 24 x 32 pixels cross the 32-frame batch of Mesher::cull_mesh with the sensor's depth images: the room's first two poses
    32 times, each moved along y by its own multiple of 1 / 64 (exact, like the inversion of these poses), and, alone in the second batch,
    the third pose.  Each batch sees vertices the other does not (a condition of the input); the PLY and the counts are those of the
    Python path, whose result does not depend on its own batch (test_cull_mesh_equals_the_restatement)."""
    exe = os.path.join(HOST, "cull_mesh_test")
    assert os.path.exists(exe), "build() makes host/cull_mesh_test"
    verts, tris, wall, twall = cc.room_with_panel()
    c2w = cc.panel_trajectory()[[0, 1] * 16 + [2]].astype(np.float64)
    c2w[:, 1, 3] += (np.arange(33) - 16) / 64.0
    c2w = c2w.astype(F)
    w2c = np.stack([mcc.w2c_of(m) for m in c2w])
    sensor = ctx.mesh_depth(cu(verts), cui(tris[twall != 1]), w2c, H, W, *INTR)
    cull = lambda sl: ctx.cull_mesh(cu(verts), cui(tris), w2c[sl], INTR, (H, W), sensor[sl], "depth", 0, cc.E2E_EPS)
    py = cull(slice(None))
    n_first, n_last = cull(slice(0, 32))["n_seen"], cull(slice(32, 33))["n_seen"]
    print("33 frames: %d vertices seen, %d by the first batch alone, %d by the second alone" % (py["n_seen"], n_first, n_last))
    assert len(w2c) == 33 and 0 < n_first < py["n_seen"] and 0 < n_last < py["n_seen"]
    d = str(tmp_path)
    np.save(os.path.join(d, "c2ws.npy"), c2w); np.save(os.path.join(d, "intr.npy"), np.array(INTR, F))
    np.save(os.path.join(d, "depths.npy"), sensor.cpu().numpy())
    _write_ply(os.path.join(d, "in.ply"), verts, tris)
    out = subprocess.run([exe, d, os.path.join(d, "in.ply"), os.path.join(d, "out.ply"), "depth", "0", repr(cc.E2E_EPS)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    js = json.loads(out.stdout.strip().splitlines()[-1])
    pv, pt = _read_ply(os.path.join(d, "out.ply"))
    assert len(pt) > 0 and pv.tobytes() == py["verts"].cpu().numpy().tobytes() and pt.tobytes() == py["tris"].cpu().numpy().tobytes()
    assert js["frames"] == 33 and js["vertices"] == len(pv) and js["triangles"] == len(pt) and js["n_seen"] == py["n_seen"] and js["skipped"] == 0

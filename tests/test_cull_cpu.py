"""CPU tests (-m "not gpu") of the culling restatement (tests/cull_checks.py) on scenes whose answer is known by construction, and of
nsk_depth_views_range, which needs no device.  tests/test_gpu_cull.py holds the device to the helpers proved here."""
import ctypes as C

import numpy as np

import cull_checks as cc
import raster_checks as rc

F = np.float32


# ---- cube room, one camera inside looking at one wall ---------------------------------------------------------------------------------
def _analytic_frustum(verts, w, intr, HW):
    """float64: in front of the camera and the projection inside [-0.5, W - 0.5) x [-0.5, H - 0.5) (the nearest pixel is in the image);
    -> (inside, the smallest distance of any vertex to a boundary: depth in metres, image bounds in pixels)"""
    P = verts.astype(np.float64) @ w[:3, :3].astype(np.float64).T + w[:3, 3].astype(np.float64)
    fx, fy, cx, cy = intr
    H, W = HW
    d = -P[:, 2]
    with np.errstate(all="ignore"):
        u, v = cx + fx * P[:, 0] / d, cy - fy * P[:, 1] / d
    front = d > 0
    inside = front & (u >= -0.5) & (u < W - 0.5) & (v >= -0.5) & (v < H - 0.5)
    edge = np.minimum(np.minimum(np.abs(u + 0.5), np.abs(u - (W - 0.5))), np.minimum(np.abs(v + 0.5), np.abs(v - (H - 0.5))))
    margin = np.minimum(np.abs(d), np.where(front, edge, np.inf))
    return inside, float(margin.min())


def test_room_frustum_is_the_analytic_one():
    verts, tris, wall = cc.room()
    w = cc.room_camera()
    inside, margin = _analytic_frustum(verts, w[0], cc.ROOM_INTR, cc.ROOM_HW)
    assert margin > 1e-3, "a vertex stands within float32's reach of a frustum boundary: move the camera (margin %g)" % margin
    seen = cc.points_seen(verts, w, cc.ROOM_INTR, cc.ROOM_HW)
    assert (seen.astype(bool) == inside).all()
    assert seen[wall == 4].all(), "the wall the camera looks at"
    assert not seen[wall == 5].any(), "the wall behind the camera"
    assert 0 < seen[wall == 0].sum() < (wall == 0).sum(), "a side wall is cut by the frustum"
    # the depth of the room itself changes nothing here: every wall vertex is a nearest surface (eps covers the rasteriser's rounding)
    r = cc.cull_mesh(verts, tris, w, cc.ROOM_INTR, cc.ROOM_HW, occlusion="none")
    assert (r["seen"] == seen).all() and r["n_seen"] == int(inside.sum())


def test_select_parts_partition_the_valid_triangles():
    verts, tris, _ = cc.room()
    seen = cc.points_seen(verts, cc.room_camera(), cc.ROOM_INTR, cc.ROOM_HW)
    nv = len(verts)
    bad = np.array([[0, 1, nv], [-1, 2, 3]], np.int32)
    tt = np.concatenate([tris[:40], bad[:1], tris[40:], bad[1:]])
    parts = [cc.select(verts, tt, seen, p) for p in (0, 1)]
    orig = [p[2][p[1]] for p in parts]                    # the kept triangles in input indices, in order
    valid = tt[((tt >= 0) & (tt < nv)).all(1)]
    assert parts[0][3] == parts[1][3] == 2
    assert len(orig[0]) + len(orig[1]) + 2 == len(tt) and len(orig[0]) > 0 and len(orig[1]) > 0
    face = seen[valid].all(1)
    assert (orig[0] == valid[face]).all() and (orig[1] == valid[~face]).all()          # disjoint, complete, order kept
    for (v, t, src, _), o in zip(parts, orig):
        assert (v == verts[src]).all() and (np.diff(src) > 0).all()
        assert len(src) == len(np.unique(o)), "unreferenced vertices are dropped, referenced ones kept"


# ---- two fronto-parallel sheets, the front one smaller --------------------------------------------------------------------------------
def _sheets_expectation():
    verts, tris, which, w = cc.sheets()
    fx, fy, cx, cy = cc.SHEETS_INTR
    zb, hxb, hyb, m = cc.SHEET_BACK
    zf, hxf, hyf, _ = cc.SHEET_FRONT
    u = cx + fx * verts[:, 0].astype(np.float64) / -verts[:, 2].astype(np.float64)
    v = cy - fy * verts[:, 1].astype(np.float64) / -verts[:, 2].astype(np.float64)
    lo_u, hi_u, lo_v, hi_v = cx - fx * hxf / zf, cx + fx * hxf / zf, cy - fy * hyf / zf, cy + fy * hyf / zf        # the front sheet's silhouette
    back = which == 0
    # the construction: the silhouette runs between pixel centres, and no back vertex projects within a pixel of it
    for e in (lo_u, hi_u, lo_v, hi_v):
        assert abs(e - np.floor(e) - 0.5) < 1e-9
    du = np.minimum(np.abs(u[back] - lo_u), np.abs(u[back] - hi_u))
    dv = np.minimum(np.abs(v[back] - lo_v), np.abs(v[back] - hi_v))
    assert du.min() > 1.0 and dv.min() > 1.0
    hidden = back & (u > lo_u) & (u < hi_u) & (v > lo_v) & (v < hi_v)
    border = back & ((np.abs(np.abs(verts[:, 0]) - F(hxb)) < 1e-6) | (np.abs(np.abs(verts[:, 1]) - F(hyb)) < 1e-6))
    assert hidden.sum() > 0 and border.sum() == 4 * (m - 1) and not (hidden & border).any()
    return verts, tris, which, w, hidden, border


def test_sheets_self_occlusion_and_zero_sees():
    verts, tris, which, w, hidden, border = _sheets_expectation()
    H, W = cc.SHEETS_HW
    depth, skipped = rc.render(verts, tris, w, H, W, *cc.SHEETS_INTR)
    assert skipped == 0
    # a border vertex's nearest pixel hits nothing; every other vertex's hits its own sheet or the one in front
    seen1 = cc.points_seen(verts, w, cc.SHEETS_INTR, cc.SHEETS_HW, depth, 0, cc.SHEETS_EPS, zero_sees=True)
    seen0 = cc.points_seen(verts, w, cc.SHEETS_INTR, cc.SHEETS_HW, depth, 0, cc.SHEETS_EPS, zero_sees=False)
    assert (seen1.astype(bool) == ~hidden).all(), "self depth: exactly the back vertices behind the front sheet's silhouette are unseen"
    assert (seen0.astype(bool) == ~(hidden | border)).all(), "zero_sees = 0: the back sheet's border sees a pixel without a hit"
    assert seen1[which == 1].all() and seen0[which == 1].all()
    r = cc.cull_mesh(verts, tris, w, cc.SHEETS_INTR, cc.SHEETS_HW, occlusion="self", eps=cc.SHEETS_EPS)
    assert (r["seen"] == seen1).all()
    assert (cc.points_seen(verts, w, cc.SHEETS_INTR, cc.SHEETS_HW).astype(bool)).all(), "the frustum alone sees both sheets whole"
    # a non-finite point is never seen, whatever the depth says
    bad = np.array([[np.nan, 0, -3], [np.inf, 0, -3], [0, 0, -np.inf], [0, 0, -3]], F)
    assert cc.points_seen(bad, w, cc.SHEETS_INTR, cc.SHEETS_HW).tolist() == [0, 0, 0, 1]


# ---- nsk_depth_views_range and the view stream -------------------------------------------------------------------------------------------
def _range(box, seed, shrink, first, V):
    import nice_slam_cpp_amd as pkg
    L = pkg.nsk.lib()
    b = np.ascontiguousarray(np.asarray(box, F))
    w = np.full((V, 4, 4), np.nan, F)
    rcode = L.nsk_depth_views_range(b.ctypes.data_as(C.c_void_p), C.c_ulonglong(seed), C.c_double(shrink), C.c_longlong(first), C.c_int(V),
                                    w.ctypes.data_as(C.c_void_p))
    assert rcode == 0, L.nsk_last_error()
    return w


def test_depth_views_range_is_the_stream_of_depth_views():
    import nice_slam_cpp_amd as pkg
    box = cc.room_box()
    for seed, shrink in ((0, 0.7), (12345678901234567, 0.4)):
        whole = pkg.nsk.depth_views_from_box(box, 70, seed, shrink)
        assert whole.tobytes() == rc.draw_views(box, 70, seed, shrink).tobytes()
        assert _range(box, seed, shrink, 0, 70).tobytes() == whole.tobytes()
        for a, b in ((0, 1), (5, 0), (31, 33), (64, 6)):
            assert _range(box, seed, shrink, a, b).tobytes() == whole[a:a + b].tobytes()
        assert pkg.nsk.depth_views_range(box, 7, 9, seed, shrink).tobytes() == whole[7:16].tobytes()
    L = pkg.nsk.lib()
    b = np.ascontiguousarray(box)
    assert L.nsk_depth_views_range(b.ctypes.data_as(C.c_void_p), C.c_ulonglong(0), C.c_double(0.7), C.c_longlong(-1), C.c_int(1), None) != 0


# ---- the redraw ----------------------------------------------------------------------------------------------------------------------------
def test_redraw_cap_has_a_factor_of_four_in_hand():
    """the scene of the GPU tests must fill its 16 views within 4 x 16 candidates, so that the 16 x cap is a factor of 4 away"""
    w, idx, tried = cc.clear_views(cc.room_box(), cc.wall_patch(), cc.CLEAR_VIEWS, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0, max_factor=4)
    print("clear views: %d accepted of %d candidates tried (acceptance %.2f)" % (len(idx), tried, len(idx) / tried))
    assert len(idx) == cc.CLEAR_VIEWS and tried <= 4 * cc.CLEAR_VIEWS and tried == idx[-1] + 1
    assert (np.diff(idx) > 0).all() and 0 < tried - len(idx), "some candidate is rejected, or the test shows nothing"
    H, W = cc.CLEAR_HW
    intr = (cc.CLEAR_FOCAL, cc.CLEAR_FOCAL, W / 2.0 - 0.5, H / 2.0 - 0.5)
    assert (cc.view_counts(cc.wall_patch(), w, cc.CLEAR_HW, intr) == 0).all()
    stream = rc.draw_views(cc.room_box(), tried, 0, 0.7)
    assert w.tobytes() == stream[idx].tobytes()
    rejected = np.setdiff1d(np.arange(tried), idx)
    assert (cc.view_counts(cc.wall_patch(), stream[rejected], cc.CLEAR_HW, intr) > 0).all()
    # the full cap gives the same views: the accepted set does not depend on max_factor once it is reached
    w16, idx16, tried16 = cc.clear_views(cc.room_box(), cc.wall_patch(), cc.CLEAR_VIEWS, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0, max_factor=16)
    assert (idx16 == idx).all() and tried16 == tried


def test_redraw_returns_short_when_every_view_sees_an_unseen_point():
    n_views, max_factor = 4, 4
    w, idx, tried = cc.clear_views(cc.room_box(), cc.box_scatter(), n_views, cc.CLEAR_HW, cc.CLEAR_FOCAL, seed=0, max_factor=max_factor)
    assert len(idx) < n_views and len(w) == len(idx) and tried == max_factor * n_views
    assert len(idx) == 0, "points through the whole box: no view of this scene is clear"

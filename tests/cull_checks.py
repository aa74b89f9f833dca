"""What culling a mesh to a trajectory (include/nsk.h: nsk_points_seen, nsk_mesh_select, nsk_points_view_counts, nsk_depth_views_range) and
the pipelines built on it must give, in pure numpy: nothing here is imported from the product.  The per-(point, frame) rule is
mesh_cull_checks.seen_f32 itself, imported and called -- a second copy could drift; the variants of the new entry points (no depth, depth
rendered from the mesh itself) are realised by replacing depth values with FLT_MAX before that call.  tests/test_cull_cpu.py proves these
helpers on scenes whose answer is known by construction."""
import numpy as np

import mesh_cull_checks as mcc
import raster_checks as rc

F = np.float32
FLT_MAX = np.finfo(F).max


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def points_seen(pts, w2c, intr, HW, depths=None, edge=0, eps=0.03, zero_sees=False, seen=None):
    """nsk_points_seen -> uint8 [n].  depths None: every pixel reads FLT_MAX; zero_sees: a pixel with D == 0 reads FLT_MAX; a point with a
    component that is not finite is never seen; seen: the old mask, ORed in"""
    pts = np.asarray(pts, F).reshape(-1, 3)
    w = np.asarray(w2c, F).reshape(-1, 4, 4)
    K, H, W = len(w), int(HW[0]), int(HW[1])
    if depths is None:
        D = np.full((K, H, W), FLT_MAX, F)
    else:
        D = np.array(depths, F).reshape(K, H, W)
        if zero_sees:
            D[D == 0] = FLT_MAX
    out = mcc.seen_f32(pts, D, intr, w, edge, eps) if len(pts) else np.zeros(0, np.uint8)
    out = (out.astype(bool) & np.isfinite(pts).all(1))
    if seen is not None:
        out |= np.asarray(seen).astype(bool)
    return out.astype(np.uint8)


def select(verts, tris, seen, part):
    """nsk_mesh_select: mask[tris].all(1) (part 0) or its complement among the valid triangles (part 1), unreferenced vertices removed,
    order kept, re-indexed -> (verts float32 [m, 3], tris int32 [k, 3], vertex_src int32 [m], skipped)"""
    verts = np.asarray(verts, F).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    mask = np.asarray(seen).reshape(-1) != 0
    nv = len(verts)
    valid = ((tris >= 0) & (tris < nv)).all(1) if len(tris) else np.zeros(0, bool)
    face = np.zeros(len(tris), bool)
    face[valid] = mask[tris[valid]].all(1)
    keep = valid & (face if part == 0 else ~face)
    used = np.zeros(nv, bool)
    used[tris[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    return verts[used], new[tris[keep]].astype(np.int32).reshape(-1, 3), np.nonzero(used)[0].astype(np.int32), int((~valid).sum())


def view_counts(pts, w2c, HW, intr, edge=0):
    """nsk_points_view_counts: per view, the number of points the frustum rule has in the image -> int64 [V]"""
    w = np.asarray(w2c, F).reshape(-1, 4, 4)
    return np.array([int(points_seen(pts, w[k:k + 1], intr, HW, None, edge, 0.0).sum()) for k in range(len(w))], np.int64)


def cull_mesh(verts, tris, w2c, intr, HW, depths=None, occlusion="none", edge=0, eps=0.03):
    """the whole cull: "none" the frusta, "depth" the given images, "self" images rendered from the mesh itself (raster_checks.render)
    -> dict(verts, tris, seen, vertex_src, n_seen, skipped)"""
    H, W = HW
    if occlusion == "none":
        d = None
    elif occlusion == "depth":
        d = depths
    else:
        d = rc.render(verts, tris, w2c, H, W, *intr)[0]
    seen = points_seen(verts, w2c, intr, HW, d, edge, eps, occlusion == "self")
    v, t, src, skipped = select(verts, tris, seen, 0)
    return dict(verts=v, tris=t, seen=seen, vertex_src=src, n_seen=int(seen.sum()), skipped=skipped)


def clear_views(box, unseen, n_views, HW, focal, seed=0, shrink=0.7, edge=0, max_factor=16):
    """the redraw as a plain loop over the candidate stream: candidate k is view k of raster_checks.draw_views; it is accepted when none of
    the unseen points is in its image; stop at n_views accepted or after max_factor * n_views candidates
    -> (w2c [m, 4, 4], index int64 [m], tried)"""
    H, W = HW
    intr = (focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5)
    cap = max_factor * n_views
    stream = rc.draw_views(box, cap, seed, shrink)
    ws, idx, tried = [], [], 0
    for k in range(cap):
        if len(idx) == n_views:
            break
        tried = k + 1
        if view_counts(unseen, stream[k:k + 1], HW, intr, edge)[0] == 0:
            ws.append(stream[k]); idx.append(k)
    return (np.stack(ws) if ws else np.zeros((0, 4, 4), F)), np.array(idx, np.int64), tried


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
ROOM_LO, ROOM_HI = (-2.0, -1.5, -2.5), (2.0, 1.5, 2.5)
ROOM_HW, ROOM_INTR = (48, 64), (40.0, 40.0, 31.5, 23.5)


def wall(axis, value, lo, hi, m):
    """one tessellated wall of a box: the plane coordinate[axis] = value over the other two axes' [lo, hi], m x m vertices"""
    o = [a for a in range(3) if a != axis]
    g0, g1 = np.linspace(lo[o[0]], hi[o[0]], m), np.linspace(lo[o[1]], hi[o[1]], m)
    A, B = np.meshgrid(g0, g1, indexing="ij")
    v = np.zeros((m, m, 3))
    v[..., axis], v[..., o[0]], v[..., o[1]] = value, A, B
    return v.reshape(-1, 3).astype(F), rc.grid_tris(m, m)


def room(m=9):
    """raster_checks.cube_room's box with every wall tessellated into m x m vertices of its own (walls do not share vertices)
    -> (verts, tris, wall [nv]: 0 / 1 the x walls (lo, hi), 2 / 3 the y walls, 4 / 5 the z walls)"""
    vs, ts, ws = [], [], []
    for axis in range(3):
        for side, value in enumerate((ROOM_LO[axis], ROOM_HI[axis])):
            v, t = wall(axis, value, ROOM_LO, ROOM_HI, m)
            ts.append(t + sum(len(x) for x in vs)); vs.append(v); ws.append(np.full(len(v), 2 * axis + side))
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32), np.concatenate(ws)


def room_camera():
    """one camera inside the room, a little off the centre, looking along -z at the wall z = lo (wall 4); the identity rotation, so camera
    space is world space shifted"""
    return rc.look(None, (-0.13, 0.07, -0.4))[None]


def room_trajectory():
    """three frames inside the room that never face the wall x = hi (wall 1): looking along -z, along -x and along +z"""
    return np.stack([rc.look(None, (-0.13, 0.07, -0.4)), rc.look(rc.rot_y(-np.pi / 2), (0.1, 0.05, -0.2)), rc.look(rc.rot_y(np.pi), (0.2, -0.1, 0.3))]).astype(F)


# Two fronto-parallel sheets in front of the identity camera (which looks along -z), 64 x 48 image, focal 40, cx = 31.5, cy = 23.5.
#   back sheet: z = -4, |x| <= 2.025, |y| <= 1.525, 10 x 10 vertices.  Its border projects to u = 31.5 -+ 20.25, v = 23.5 -+ 15.25, a quarter
#     of a pixel inside the pixel centres 11, 52, 8 and 39: a border vertex's nearest pixel lies outside the sheet and hits nothing.
#   front sheet: z = -2, |x| <= 0.5, |y| <= 0.35, 4 x 4 vertices.  Its silhouette is u in [21.5, 41.5], v in [16.5, 30.5]: between pixel
#     centres, and more than a pixel from every back-sheet vertex's projection (test_cull_cpu.py asserts both).
SHEETS_HW, SHEETS_INTR = (48, 64), (40.0, 40.0, 31.5, 23.5)
SHEET_BACK, SHEET_FRONT = (4.0, 2.025, 1.525, 10), (2.0, 0.5, 0.35, 4)
# d = 4 is exact (the identity camera); the rendered D = (a_z n_z) / -n_z is one rounded product and one rounded quotient of exact inputs:
# |D - 4| <= 4 (2 * 2^-24 + 2^-48) < 2^-21.  The sheets are 2 m apart, so any eps in [2^-21, 2) separates them; 2^-20 is used.
SHEETS_EPS = 2.0 ** -20


def sheets():
    """-> (verts, tris, which [nv]: 0 back, 1 front, w2c [1, 4, 4])"""
    vs, ts, ws = [], [], []
    for q, (z, hx, hy, m) in enumerate((SHEET_BACK, SHEET_FRONT)):
        X, Y = np.meshgrid(np.linspace(-hx, hx, m), np.linspace(-hy, hy, m), indexing="ij")
        v = np.stack([X, Y, np.full_like(X, -z)], -1).reshape(-1, 3).astype(F)
        ts.append(rc.grid_tris(m, m) + sum(len(x) for x in vs)); vs.append(v); ws.append(np.full(len(v), q))
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32), np.concatenate(ws), rc.look()[None]


# The scene of the clear-view tests: the room's box, unseen points on a patch of the wall x = hi, 64 x 48 views, focal 40.
CLEAR_HW, CLEAR_FOCAL, CLEAR_VIEWS = (48, 64), 40.0, 16


def room_box():
    return np.array(ROOM_LO + ROOM_HI, F)


def wall_patch(m=12):
    """m x m points on the wall x = hi over y in [-0.6, 0.6], z in [-0.8, 0.8]"""
    Y, Z = np.meshgrid(np.linspace(-0.6, 0.6, m), np.linspace(-0.8, 0.8, m), indexing="ij")
    return np.stack([np.full_like(Y, ROOM_HI[0]), Y, Z], -1).reshape(-1, 3).astype(F)


def box_scatter(n=3000, seed=5):
    """points scattered through the whole box: every view inside it has some in its image"""
    rng = np.random.default_rng(seed)
    return rng.uniform(ROOM_LO, ROOM_HI, (n, 3)).astype(F)


# The scene of the end-to-end test: the room with the wall x = hi (wall 1) as a panel of its own, 0.5 m short of its neighbours on every
# side, so that none of its vertices shares a position with a vertex the trajectory sees.  The sensor never measured that wall (its depth
# images are rendered from the five other walls: the pixels that look through the opening carry 0), and three wide frames from inside,
# looking along -z, -x and +z, cover every other wall.
E2E_HW, E2E_INTR, E2E_EPS = (192, 256), (32.0, 32.0, 127.5, 95.5), 0.5


def room_with_panel(m=9, inset=0.5):
    """-> (verts, tris, wall [nv], wall_of_triangle [nt])"""
    vs, ts, ws, tw = [], [], [], []
    for axis in range(3):
        for side, value in enumerate((ROOM_LO[axis], ROOM_HI[axis])):
            lo, hi = np.array(ROOM_LO), np.array(ROOM_HI)
            if 2 * axis + side == 1:
                lo, hi = lo + inset, hi - inset
            v, t = wall(axis, value, lo, hi, m)
            ts.append(t + sum(len(x) for x in vs)); vs.append(v); ws.append(np.full(len(v), 2 * axis + side)); tw.append(np.full(len(t), 2 * axis + side))
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32), np.concatenate(ws), np.concatenate(tw)


def panel_trajectory():
    """camera-to-world [3, 4, 4] float32 (as a pose file holds them) of three frames at x = 0.5 that never face the wall x = hi"""
    quarter = lambda th: np.round(rc.rot_y(th))                            # entries 0 and +-1: every inversion of these poses is exact
    w = np.stack([rc.look(None, (-0.5, 0.0, -2.0)),                        # at (0.5, 0, 2) looking along -z
                  rc.look(quarter(-np.pi / 2), (0.0, 0.0, -0.5)),          # at (0.5, 0, 0) looking along -x
                  rc.look(quarter(np.pi), (0.5, 0.0, -2.0))])              # at (0.5, 0, -2) looking along +z
    return np.linalg.inv(w.astype(np.float64)).astype(F)

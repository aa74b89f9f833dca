"""No GPU: the numpy restatement of the mesh depth views (tests/raster_checks.py) on scenes whose images are known analytically, and the
view draw against upstream's viewmatrix in plain float64 and against the library's own host code."""
import numpy as np

import raster_checks as rk

H, W, F = 48, 64, 40.0
CX, CY = W / 2.0 - 0.5, H / 2.0 - 0.5


def pixel_rays():
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (ii - CX) / F, -(jj - CY) / F


def test_sheet_has_no_hole_and_lies_on_its_plane():
    """bound 1e-5 relative: the rule's own error on this scene is 2.6e-7 (fp32 rounding of the vertices and of a dozen operations); a depth
    taken from the wrong formula is off by the triangle's size over its distance, 0.1 here"""
    v, t, w0 = rk.sheet()
    assert len(t) == 3042
    views = rk.sheet_views()[:2]
    dep, skipped = rk.render(v, t, views, H, W, F, F, CX, CY)
    assert skipped == 0 and dep.dtype == np.float32
    x, y = pixel_rays()
    m = np.array(rk.SHEET_PLANE[1:] + (-1.0,))                  # the plane m . p = 3 in the first view's camera space
    worst, covered = 0.0, 0
    for k in range(2):
        T = views[k].astype(np.float64) @ np.linalg.inv(w0.astype(np.float64))       # camera 0 -> camera k
        Rt, tt = T[:3, :3], T[:3, 3]
        mk = Rt @ m
        ray = np.stack([x, y, -np.ones_like(x)], -1)
        ta = (-rk.SHEET_PLANE[0] + mk @ tt) / (ray @ mk)
        p0 = (ta[..., None] * ray - tt) @ Rt                    # the hit point back in camera 0
        inside = (ta > 0) & np.isfinite(ta) & (np.abs(p0[..., 0]) < 5.8) & (np.abs(p0[..., 1]) < 5.8)
        hit = dep[k] > 0
        rel = np.abs(dep[k][inside & hit] / ta[inside & hit] - 1).max()
        print("view %d: %d pixels inside the outline, %d of them not hit, worst relative depth error %.2e" % (
            k, int(inside.sum()), int((inside & ~hit).sum()), rel))
        assert inside.sum() > 500 and not (inside & ~hit).any()
        assert rel <= 1e-5
        worst = max(worst, rel); covered += int(inside.sum())
    assert (dep[0] > 0).sum() == H * W                           # the first view sees nothing but the sheet


def test_floor_across_the_camera_plane():
    v, t = rk.floor()
    dep, _ = rk.render(v, t, rk.look()[None], H, W, F, F, CX, CY)
    x, y = pixel_rays()
    below = y < 0
    ta = np.where(below, -1.0 / np.where(below, y, 1.0), np.inf)
    inside = below & (ta * np.maximum(np.abs(x), 1.0) < 49.0)   # the hit point lies on the 100 m floor
    outside = ~below | (ta * np.maximum(np.abs(x), 1.0) > 51.0)  # above the horizon, or beyond the floor's far edge (the row next to the horizon)
    assert inside.sum() == below.sum() - W and outside.sum() == H * W - inside.sum()
    assert (dep[0][inside] > 0).all() and (dep[0][outside] == 0).all()
    rel = np.abs(dep[0][inside] / ta[inside] - 1).max()
    print("floor: worst relative depth error %.2e" % rel)
    assert rel <= 1e-5


def test_closed_room_from_inside_is_hit_everywhere():
    v, t = rk.cube_room()
    dep, _ = rk.render(v, t, rk.room_views_inside(), H, W, F, F, CX, CY)
    assert (dep > 0).all() and dep.max() < 8.0                  # the room's diagonal is 7.1
    # the identity view looks at the wall z = -2.5 wherever the ray does not meet a side wall first
    x, y = pixel_rays()
    wall = (np.abs(2.5 * x) < 1.99) & (np.abs(2.5 * y) < 1.49)
    assert wall.sum() > 1000 and np.abs(dep[0][wall] / 2.5 - 1).max() <= 1e-5
    out, _ = rk.render(v, t, rk.room_views_outside(), H, W, F, F, CX, CY)
    assert (out[0] > 0).any() and (out[0] == 0).any() and abs(out[0][H // 2, W // 2] - 6.5) < 1e-4        # 9 m away, the near wall at z = 2.5


def test_left_out_triangles_and_empty_inputs():
    v, t = rk.cube_room()
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    t2 = np.concatenate([t, [[0, 0, 1], [0, 1, 8], [0, 1, 9], [-1, 2, 3]]]).astype(np.int32)
    a, sa = rk.render(v, t, rk.room_views_inside()[:1], 12, 16, 10, 10, 7.5, 5.5)
    b, sb = rk.render(v2, t2, rk.room_views_inside()[:1], 12, 16, 10, 10, 7.5, 5.5)
    assert sa == 0 and sb == 2 and (a.view(np.uint32) == b.view(np.uint32)).all()
    e, _ = rk.render(v, t[:0], rk.room_views_inside()[:1], 12, 16, 10, 10, 7.5, 5.5)
    assert e.shape == (1, 12, 16) and (e == 0).all()
    assert rk.render(v, t, np.zeros((0, 16)), 12, 16, 10, 10, 7.5, 5.5)[0].shape == (0, 12, 16)
    # behind the camera: nothing
    behind, _ = rk.render(v + np.float32([0, 0, 10]), t, rk.look()[None], 12, 16, 10, 10, 7.5, 5.5)
    assert (behind == 0).all()


def test_pair_stats_by_hand():
    a = np.array([[0, 1, 2, np.nan, np.inf, 3]], np.float32)
    b = np.array([[1, 0, 2.5, 1, 1, np.inf]], np.float32)
    s = rk.pair_stats(a, b)[0]
    assert s[0] == 1 + 1 + 0.5 and s[1] == 3 and s[2] == 0.5 and s[3] == 4


def test_view_draw_against_viewmatrix():
    box = np.array([-1.5, -2.0, 0.25, 3.0, 1.0, 2.75], np.float32)
    n = 200
    w = rk.draw_views(box, n, seed=5, shrink=0.7)
    o, target = rk.view_parts(box, n, seed=5, shrink=0.7)
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    assert (np.abs(o - ctr) <= 0.7 * half + 1e-12).all() and (target >= lo).all() and (target <= hi).all()
    assert np.abs(o - ctr).max(0).min() > 0.6 * 0.7 * half.min() and o.std(0).min() > 0.1          # spread over the box, not a point
    worst = 0.0
    for k in range(n):
        want = rk.viewmatrix_w2c(o[k], target[k])
        worst = max(worst, float(np.abs(w[k].astype(np.float64) - want).max()))
        # the camera looks at its target along -z
        p = want @ np.append(target[k], 1.0)
        assert abs(p[0]) < 1e-9 and abs(p[1]) < 1e-9 and p[2] < 0
    print("largest difference to float64 viewmatrix + numpy inverse: %.2e" % worst)
    assert worst <= 4e-7                     # float32 rounding of entries up to 4 in magnitude: half an ulp is 2.4e-7
    assert (rk.draw_views(box, n, seed=6).view(np.uint32) != w.view(np.uint32)).any()


def test_view_draw_of_the_library_has_the_same_bits():
    import nice_slam_cpp_amd as pkg
    for box, seed, shrink in (([-1.5, -2.0, 0.25, 3.0, 1.0, 2.75], 5, 0.7), ([0.1, 0.2, 0.3, 7.7, 5.1, 2.9], 2 ** 40 + 3, 0.5),
                              ([-2, -1.5, -2.5, 2, 1.5, 2.5], 0, 1.0)):
        got = pkg.nsk.depth_views_from_box(box, 300, seed, shrink)
        want = rk.draw_views(np.asarray(box, np.float32), 300, seed, shrink)
        assert got.shape == (300, 4, 4) and (got.view(np.uint32) == want.view(np.uint32)).all()

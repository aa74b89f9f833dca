"""CPU tests (-m "not gpu") of the helpers the mesh-culling GPU tests rest on (tests/mesh_cull_checks.py): the float32 restatement of the
seen rule against a float64 one with a derived error margin, on every scene the GPU tests use; the numpy union-find against a breadth-first
search and against known answers."""
import numpy as np
import pytest

import mesh_checks as mc
import mesh_cull_checks as cc
import scenes


def _table():
    import nice_slam_cpp_amd as pkg
    pkg.build()
    return [pkg.nsk.mesh_table(c) for c in range(256)]


SEEN_SCENES = {"lattice test": lambda: cc.cull_scene(scenes.REF_BOUND),
               "mesher": lambda: cc.mesher_scene(scenes.REF_BOUND)}


@pytest.mark.parametrize("name", sorted(SEEN_SCENES))
def test_seen_f32_agrees_with_f64_outside_the_margin(name):
    """per scene and (edge, trunc): equal wherever the margin exceeds 1; at most 1 % of the lattice at or below 1; every class of node
    present (seen, behind the camera, outside each image edge, behind depth + trunc, on a zero / NaN / inf pixel); the keyframe that looks
    away sees nothing"""
    sc = SEEN_SCENES[name]()
    for edge, trunc in sc["params"]:
        a = cc.check_scene(sc, edge, trunc)
        _, margin, classes = cc.seen_f64(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], edge, trunc)
        print("%s edge %d trunc %.1f: %d of %d nodes seen, %d within the bound, classes %s" % (
            name, edge, trunc, int(a.sum()), a.size, int((margin <= 1).sum()), np.bincount(classes.reshape(-1), minlength=10).tolist()))
    if sc["away"] is not None:
        k = sc["away"]
        assert cc.seen_f32(sc["pts"], sc["depths"][k:k + 1], sc["intr"], sc["w2c"][k:k + 1], 0, 0.5).sum() == 0


def test_seen_margin_is_zero_on_a_boundary_and_large_far_from_it():
    """a camera at the origin looking down -z: a point on the axis projects to (cx, cy) = (15.5, 11.5), the rounding point of both pixel
    indices (margin 0); a point well inside a pixel, well in front of the surface has a margin in the thousands"""
    depths = np.full((1, cc.IMG_H, cc.IMG_W), 5.0, np.float32)
    w2c = np.eye(4, dtype=np.float32)[None]
    pts = np.array([[0.0, 0.0, -2.0], [0.005, 0.005, -2.0], [0.0, 0.0, 2.0]], np.float32)
    seen, margin, classes = cc.seen_f64(pts, depths, cc.INTR, w2c, 0, 0.0)
    assert margin[0] == 0.0 and margin[1] > 1000 and margin[2] > 1000
    assert classes[0].tolist() == [cc.SEEN, cc.SEEN, cc.BEHIND] and seen.tolist() == [1, 1, 0]
    assert cc.seen_f32(pts, depths, cc.INTR, w2c, 0, 0.0).tolist() == [1, 1, 0]
    # d = D + trunc exactly: on the boundary (seen: the rule is <=), margin 0
    seen, margin, _ = cc.seen_f64(np.array([[0.005, 0.005, -5.5]], np.float32), depths, cc.INTR, w2c, 0, 0.5)
    assert seen[0] == 1 and margin[0] == 0.0


def test_components_against_bfs_and_known_answers():
    table = _table()
    # a few hundred triangles of noise: many components of every size
    vol = np.random.default_rng(21).standard_normal((7, 6, 8)).astype(np.float32)
    v, t = cc.numpy_mesh(table, vol, (0.0, 0.0, 0.0), (0.1, 0.2, 0.15), 0.9)
    mc.check_topology(t, mc.check_vertices(v, vol, (0.0, 0.0, 0.0), (0.1, 0.2, 0.15), 0.9), vol)
    r = cc.components(v, t)
    assert 200 < len(t) < 1000 and r["n_components"] > 5
    assert (r["label"] == cc.components_bfs(len(v), t)).all()
    assert np.isclose(r["area"].sum(), cc.triangle_areas(v, t).astype(np.float64).sum(), rtol=1e-12)
    # filtered mesh: order kept, re-indexed, positions untouched
    th = float(np.sort(r["area"])[len(r["area"]) // 2]) * 1.01
    f = cc.components(v, t, min_area=th)
    assert 0 < f["n_kept"] < f["n_components"] and f["n_kept"] == int((r["area"] > np.float32(th)).sum())
    keep_t = np.isin(r["label"][t[:, 0]], r["comp"][r["area"] > np.float32(th)])
    assert (f["verts"][f["tris"]] == v[t[keep_t]]).all() and len(np.unique(f["tris"])) == len(f["verts"])
    big = cc.components(v, t, largest_only=True)
    assert big["n_kept"] == 1 and np.isclose(cc.triangle_areas(big["verts"], big["tris"]).astype(np.float64).sum(), r["area"].max())
    none = cc.components(v, t, min_area=1e9)
    assert none["verts"].shape == (0, 3) and none["tris"].shape == (0, 3) and none["n_kept"] == 0
    # three spheres and a blob
    v, t = cc.numpy_mesh(table, cc.spheres_volume(), cc.SPHERES_ORIGIN, cc.SPHERES_STEP)
    r = cc.components(v, t)
    assert r["n_components"] == 4
    got = np.sort(r["area"])[::-1]
    for a, (_, rad) in zip(got, cc.SPHERES):
        assert abs(a - 4 * np.pi * rad ** 2) < 0.05 * 4 * np.pi * rad ** 2, (a, rad)
    assert got[3] < 0.1
    # the serpentine tube is one component
    v, t = cc.numpy_mesh(table, cc.serpentine_volume(), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    r = cc.components(v, t)
    assert r["n_components"] == 1 and (r["label"] == 0).all() and len(t) > 5000
    assert mc.euler_characteristic(t, len(v)) == 2

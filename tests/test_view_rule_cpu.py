"""CPU tests (-m "not gpu") of the one projection the seen mask and the depth fusion are restated with (tests/mesh_cull_checks.py
project_f32): what the device asserts as an identity, weight > 0 == seen mask, holds between the two restatements, and a point that is
not a number reaches no pixel."""
import numpy as np
import pytest

import mesh_cull_checks as cc
import scenes
import tsdf_checks as tc


@pytest.mark.parametrize("edge,trunc", [(0, 0.5), (3, 0.15)])
def test_fused_weight_is_positive_exactly_where_the_node_is_seen(edge, trunc):
    sc = cc.cull_scene(scenes.REF_BOUND)
    seen = cc.seen_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], edge, trunc)
    weight = tc.fuse_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], edge, trunc)[1]
    assert 0 < seen.sum() < seen.size
    assert ((weight > 0) == (seen != 0)).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_point_with_a_nan_component_fails_the_pixel_test(axis):
    """the point stands in front of the camera, on pixel (16, 11) next to the middle of the image; with one component NaN every comparison of the pixel test is
    false, under a generic pose and under the identity (whose zeros multiply the NaN)"""
    depths = np.full((1, cc.IMG_H, cc.IMG_W), 5.0, np.float32)
    for c2w in (np.eye(4), cc.look_at((0.3, -0.2, 2.0), (0.1, 0.1, -1.0), 0.1)):
        w2c = cc.w2c_of(c2w)
        p = (np.asarray(c2w)[:3, :3] @ [0.005, 0.005, -2.0] + np.asarray(c2w)[:3, 3]).astype(np.float32)[None]
        d, fi, fj = cc.project_f32(p, w2c, cc.INTR)
        assert cc.pixel_of(d, fi, fj, depths[0], 0)[0].tolist() == [True] and (fi[0], fj[0]) == (16.0, 11.0)
        p[0, axis] = np.nan
        d, fi, fj = cc.project_f32(p, w2c, cc.INTR)
        assert np.isnan(fi[0]) or np.isnan(fj[0]) or np.isnan(d[0])
        assert cc.pixel_of(d, fi, fj, depths[0], 0)[0].tolist() == [False]
        assert cc.seen_f32(p, depths, cc.INTR, w2c[None], 0, 0.5).tolist() == [0]
        assert tc.fuse_f32(p, depths, cc.INTR, w2c[None], 0, 0.5)[1].tolist() == [0.0]

"""GPU test of the frame-batch driver that nsk_lattice_seen, nsk_points_seen, nsk_points_view_counts and nsk_tsdf_integrate share: frames
go to the device in launches of 32, so the frame counts below are its joints (no launch's worth, one frame, one full launch, one frame
more, two launches and one frame).  All four decide "frame k sees point p" by one rule (csrc/nsk_view.h), so on the same nodes and frames
they give the same bytes, those of tests/mesh_cull_checks.py seen_f32."""
import numpy as np
import pytest
import torch

import cull_checks as ck
import mesh_cull_checks as cc
import tsdf_checks as tc
from gpu_util import cu

pytestmark = pytest.mark.gpu

EDGE, TRUNC = 1, 0.25


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def u8(t):
    return t.cpu().numpy().reshape(-1).astype(np.uint8).tobytes()


@pytest.mark.parametrize("K", [0, 1, 32, 33, 65])
def test_the_four_entry_points_agree_at_the_joints_of_the_frame_batches(ctx, K):
    sc = cc.view_scene(K)
    lat = (sc["origin"], sc["step"], sc["nx"], sc["ny"], sc["nz"])
    HW = (cc.IMG_H, cc.IMG_W)
    pts, depths = cu(sc["pts"]), cu(sc["depths"]).reshape(K, *HW)
    want = cc.seen_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], EDGE, TRUNC)
    wT, wW = tc.fuse_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], EDGE, TRUNC)
    wcounts = ck.view_counts(sc["pts"], sc["w2c"], HW, sc["intr"], EDGE)
    n_want = int(want.sum())
    assert len(want) == 385 and (n_want == 0 if K == 0 else 0 < n_want < 385)

    valid, n_lat = ctx.lattice_seen(*lat, depths, sc["intr"], sc["w2c"], EDGE, TRUNC)
    seen, n_pts = ctx.points_seen(pts, sc["w2c"], sc["intr"], HW, depths, EDGE, TRUNC, False)
    tsdf, weight, n_obs = ctx.tsdf_integrate(*lat, depths, sc["intr"], sc["w2c"], EDGE, TRUNC)
    counts = ctx.points_view_counts(pts, sc["w2c"], HW, sc["intr"], EDGE)
    print("K = %d: %d of 385 nodes seen (lattice_seen %d, points_seen %d, tsdf_integrate %d), largest weight %g, view counts %s"
          % (K, n_want, n_lat, n_pts, n_obs, float(wW.max()) if K else 0.0, counts.tolist()))
    assert u8(valid) == want.tobytes() and u8(seen) == want.tobytes() and u8(weight > 0) == want.tobytes()
    assert (n_lat, n_pts, n_obs) == (n_want,) * 3
    assert tsdf.cpu().numpy().tobytes() == wT.tobytes() and weight.cpu().numpy().tobytes() == wW.tobytes()
    assert counts.dtype == np.int64 and counts.tolist() == wcounts.tolist()

    # the first 32 frames, then the rest on top of them: the bytes and counts of the one call
    a, b = slice(0, min(K, 32)), slice(min(K, 32), K)
    v2, _ = ctx.lattice_seen(*lat, depths[a], sc["intr"], sc["w2c"][a], EDGE, TRUNC)
    v2, n2 = ctx.lattice_seen(*lat, depths[b], sc["intr"], sc["w2c"][b], EDGE, TRUNC, v2)
    s2, _ = ctx.points_seen(pts, sc["w2c"][a], sc["intr"], HW, depths[a], EDGE, TRUNC, False)
    s2, m2 = ctx.points_seen(pts, sc["w2c"][b], sc["intr"], HW, depths[b], EDGE, TRUNC, False, s2)
    T2, W2, _ = ctx.tsdf_integrate(*lat, depths[a], sc["intr"], sc["w2c"][a], EDGE, TRUNC)
    T2, W2, o2 = ctx.tsdf_integrate(*lat, depths[b], sc["intr"], sc["w2c"][b], EDGE, TRUNC, 64, (T2, W2))
    c2 = np.concatenate([ctx.points_view_counts(pts, sc["w2c"][q], HW, sc["intr"], EDGE) for q in (a, b)])
    assert u8(v2) == want.tobytes() and u8(s2) == want.tobytes() and (n2, m2, o2) == (n_want,) * 3
    assert torch.equal(T2.view(torch.int32), tsdf.view(torch.int32)) and torch.equal(W2, weight)
    assert c2.tolist() == wcounts.tolist()

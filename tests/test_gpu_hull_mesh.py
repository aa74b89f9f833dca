"""GPU tests of the hull-bounded scene mesh: Context.hull_mesh and Mesher::get_hull_mesh (host/test/hull_mesh_test) on a small synthetic
room at resolution 32.  The hull and the mask themselves are tests/test_gpu_hull.py's business; here the pieces are put together."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hull_checks as hc
import mesh_checks as mc
import mesh_cull_checks as cc
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
F = np.float32
N = 32
SCALE = 1.02


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    """the small scene, four cameras inside its analytic room (the bound shrunk by 0.3 m) and what they measure, the scene's files in
    the drivers' layout, and the Python path's result, computed once"""
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    b = sc["bound"].astype(F)
    # four cameras near the middle of the room, one towards each wall round the height axis: narrow frusta that leave most of the room unseen
    ctr, ext = b.astype(np.float64).mean(axis=1), (b[:, 1] - b[:, 0]).astype(np.float64)
    c2w = np.tile(np.eye(4), (4, 1, 1))
    for k, (yaw, pitch, roll, off) in enumerate(((0.1, 0.05, 0.02, (0.05, 0.02, -0.04)), (1.6, -0.08, -0.03, (-0.06, -0.03, 0.03)),
                                                 (3.2, 0.04, 0.05, (0.02, 0.04, 0.06)), (4.7, -0.02, 0.01, (-0.03, 0.01, -0.05)))):
        c2w[k, :3, :3] = scenes.look_rotation(yaw, pitch, roll)
        c2w[k, :3, 3] = ctr + np.array(off) * ext
    c2w = c2w.astype(F).astype(np.float64)              # poses as a float32 file holds them
    H, W, intr = cc.IMG_H, cc.IMG_W, cc.INTR
    depths = np.stack([scenes.frame_depth_image(b, m, H, W, *intr) for m in c2w]).astype(F)
    origin, step = b[:, 0].copy(), ((b[:, 1] - b[:, 0]) / F(N - 1)).astype(F)          # the Mesher's own expressions, padding 0
    w2c = np.stack([cc.w2c_of(m) for m in c2w])
    centres = c2w[:, :3, 3].astype(F)
    d = str(tmp_path_factory.mktemp("hull_mesh"))
    np.save(os.path.join(d, "bound.npy"), b)
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(F))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(F))
    np.save(os.path.join(d, "depths.npy"), depths)
    np.save(os.path.join(d, "c2ws.npy"), c2w.astype(F))
    np.save(os.path.join(d, "intr.npy"), np.array(intr, F))
    verts, tris, info = ctx.hull_mesh("fine", origin, step, N, cu(depths), w2c, intr, (H, W), centres=centres, scale=SCALE)
    return dict(sc=sc, ctx=ctx, dir=d, origin=origin, step=step, depths=depths, w2c=w2c, c2w=c2w, intr=intr, HW=(H, W), centres=centres,
                verts=verts, tris=tris, info=info)


def run(exe, *args):
    path = os.path.join(HOST, exe)
    if not os.path.exists(path):
        pytest.fail("%s is not built (run __graft_entry__.build())" % exe)
    r = subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_python_and_cpp_give_the_same_mesh(room):
    info = room["info"]
    hi = info["hull_info"]
    print("fusion %d vertices; hull %d vertices, %d faces, %d insertions; %d of %d nodes inside; mesh %d vertices, %d triangles"
          % (info["fused"]["n_vertices"], hi[3], hi[4], hi[5], info["n_inside"], N ** 3, len(room["verts"]), len(room["tris"])))
    assert hi[2] == 3 and len(room["verts"]) > 0 and len(room["tris"]) > 0
    # the hull is the rule's, on the fused vertices and the camera centres
    want = hc.hull(info["fused_vertices"].cpu().numpy(), room["centres"])
    assert info["hull_vertices"].tobytes() == want["vertices"].tobytes() and info["hull_faces"].tobytes() == np.ascontiguousarray(want["faces"]).tobytes()
    out = os.path.join(room["dir"], "hull.ply")
    js = json.loads(run("hull_mesh_test", room["dir"], out, N, SCALE).strip().splitlines()[-1])
    assert F(js["scale"]) == F(SCALE) and js["uploaded"] == 0 and js["resolution"] == N and js["frames"] == 4
    assert (js["hull_vertices"], js["hull_faces"], js["inside"], js["evaluated"]) == (hi[3], hi[4], info["n_inside"], info["n_inside"])
    assert (js["vertices"], js["triangles"], js["n_observed"]) == (len(room["verts"]), len(room["tris"]), info["fused"]["n_observed"])
    pv, pc, pf = mc.read_ply(out)
    assert pc is None and pv.tobytes() == room["verts"].cpu().numpy().tobytes() and pf.tobytes() == room["tris"].cpu().numpy().tobytes()


def test_every_vertex_lies_inside_the_scaled_hull(room):
    info = room["info"]
    pts = np.concatenate([info["fused_vertices"].cpu().numpy(), room["centres"]])
    hv, hf = info["hull_vertices"], info["hull_faces"]
    n, A, lo, hi = hc.mask_planes(pts[hv], hc.local_faces(hv, hf), SCALE)
    v = room["verts"].cpu().numpy().astype(np.float64)
    dist = ((v[:, None, :] - A[None]) * n[None]).sum(-1) / np.linalg.norm(n, axis=1)[None]
    print("largest signed distance of a mesh vertex to a hull plane: %.3g m (one lattice step: %.3g m)" % (dist.max(), room["step"].max()))
    assert dist.max() <= float(room["step"].max())


def test_mesh_equals_the_dense_volume_under_the_same_mask(room):
    ctx, info = room["ctx"], room["info"]
    valid = info["valid"]
    want = hc.lattice_in_hull(room["origin"], room["step"], N, N, N, np.concatenate([info["fused_vertices"].cpu().numpy(), room["centres"]])[info["hull_vertices"]],
                              hc.local_faces(info["hull_vertices"], info["hull_faces"]), SCALE)
    assert valid.cpu().numpy().tobytes() == want.tobytes() and info["n_inside"] == int(want.sum())
    dense = ctx.eval_lattice("fine", room["origin"], room["step"], N, N, N)
    v, t = ctx.extract_mesh(dense, room["origin"], room["step"], 0.0, valid)
    assert v.cpu().numpy().tobytes() == room["verts"].cpu().numpy().tobytes() and t.cpu().numpy().tobytes() == room["tris"].cpu().numpy().tobytes()


def test_a_hull_round_the_whole_lattice_gives_get_mesh(room):
    b = room["sc"]["bound"].astype(F)
    lo, hi = b[:, 0] - F(1), b[:, 1] + F(1)
    xyz = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F) * (hi - lo) + lo
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    faces = np.array([t for a, b_, c, d in quads for t in ((a, b_, c), (a, c, d))], F)
    d = room["dir"]
    np.save(os.path.join(d, "hull_xyz.npy"), xyz.astype(F))
    np.save(os.path.join(d, "hull_faces.npy"), faces)
    try:
        out = os.path.join(d, "all.ply")
        js = json.loads(run("hull_mesh_test", d, out, N).strip().splitlines()[-1])
    finally:
        os.remove(os.path.join(d, "hull_xyz.npy")); os.remove(os.path.join(d, "hull_faces.npy"))
    assert js["uploaded"] == 1 and js["inside"] == N ** 3
    run("mesh_test", "scene", d, N, 0, 0)
    assert open(out, "rb").read() == open(os.path.join(d, "mesh.ply"), "rb").read() and js["vertices"] > 0


def test_the_hull_adds_the_unobserved_interior(room):
    out = run("clean_mesh_test", room["dir"], N, 0, 0, 0, 0)
    n_seen = int(re.search(r"(\d+) seen", out).group(1))
    n_inside = room["info"]["n_inside"]
    print("nodes: %d seen by the frames, %d inside the hull, %d in all" % (n_seen, n_inside, N ** 3))
    assert n_seen < n_inside < N ** 3


def test_clean_mesh_bound_scale_is_read_from_the_configuration(room):
    out = os.path.join(room["dir"], "scale.ply")
    absent = json.loads(run("hull_mesh_test", room["dir"], out, N).strip().splitlines()[-1])
    given = json.loads(run("hull_mesh_test", room["dir"], out, N, "1.25").strip().splitlines()[-1])
    assert F(absent["scale"]) == F(1.02) and given["scale"] == 1.25
    assert absent["inside"] == room["info"]["n_inside"] and given["inside"] > absent["inside"]

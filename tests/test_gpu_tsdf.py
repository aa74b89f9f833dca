"""GPU tests of the depth fusion: nsk_tsdf_integrate, nsk_tsdf_volume, Context.fuse_depth_mesh / fuse_rendered_mesh, Mesher::get_fused_mesh.
What they must give is computed by tests/tsdf_checks.py, tests/mesh_cull_checks.py and tests/mesh_checks.py in numpy (tests/test_tsdf_cpu.py
proves the first)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_checks as mc
import mesh_cull_checks as cc
import scenes
import tsdf_checks as tc
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


@pytest.fixture(scope="module")
def scene():
    return cc.cull_scene(scenes.REF_BOUND)


@pytest.fixture(scope="module")
def sphere():
    """the sphere scene and what fuse_depth_mesh must give on it: numpy_mesh on fuse_f32's volume"""
    import nice_slam_cpp_amd as pkg
    sc = tc.sphere_scene()
    T, W = tc.fuse_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], 0, sc["trunc"])
    vol, valid = tc.volume_of(T, W, 1, (sc["nz"], sc["ny"], sc["nx"]))
    table = [pkg.nsk.mesh_table(c) for c in range(256)]
    sc["verts"], sc["tris"] = cc.numpy_mesh(table, vol, sc["origin"], sc["step"])
    sc["n_observed"], sc["n_valid"] = int((W > 0).sum()), int(valid.sum())
    return sc


def integrate(ctx, sc, ks, edge, trunc, max_weight=64, state=None):
    d = cu(sc["depths"][ks]) if len(ks) else torch.empty((0,) + sc["depths"].shape[1:], device="cuda")
    return ctx.tsdf_integrate(sc["origin"], sc["step"], sc["nx"], sc["ny"], sc["nz"], d, sc["intr"], sc["w2c"][ks], edge, trunc, max_weight, state)


def rule(sc, ks, edge, trunc, max_weight=64, state=None):
    return tc.fuse_f32(sc["pts"], sc["depths"][ks], sc["intr"], sc["w2c"][ks], edge, trunc, max_weight, state)


def same(t, a):
    return t.cpu().numpy().reshape(-1).tobytes() == np.ascontiguousarray(a).tobytes()


def check_byte_for_byte(ctx, sc, edge, trunc, max_weight):
    ks = [0, 1, 0, 1, 0]
    T, W = rule(sc, ks, edge, trunc, max_weight)
    tsdf, weight, n_obs = integrate(ctx, sc, ks, edge, trunc, max_weight)
    gT, gW = tsdf.cpu().numpy().reshape(-1), weight.cpu().numpy().reshape(-1)
    print("edge %d trunc %g max_weight %g: %d observed (rule %d), largest weight %g, %d tsdf / %d weight values differ"
          % (edge, trunc, max_weight, n_obs, int((W > 0).sum()), W.max(), int((gT.view(np.uint32) != T.view(np.uint32)).sum()), int((gW != W).sum())))
    assert tsdf.shape == (sc["nz"], sc["ny"], sc["nx"]) and tsdf.dtype == torch.float32 and weight.shape == tsdf.shape
    assert gT.tobytes() == T.tobytes() and gW.tobytes() == W.tobytes()
    assert n_obs == int((W > 0).sum()) and 0 < n_obs < W.size
    assert min(3, max_weight) <= W.max() <= min(5, max_weight)      # (weights pass 2 unless the cap holds them)
    d = cu(sc["depths"][ks])
    seen, n_seen = ctx.lattice_seen(sc["origin"], sc["step"], sc["nx"], sc["ny"], sc["nz"], d, sc["intr"], sc["w2c"][ks], edge, trunc)
    assert (weight > 0).to(torch.uint8).cpu().numpy().tobytes() == seen.cpu().numpy().tobytes() and n_seen == n_obs


# ---- 1. byte for byte -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_weight", [64, 2])
@pytest.mark.parametrize("edge,trunc", [(0, 0.5), (3, 0.5), (0, 0.15)])
def test_tsdf_equals_the_float32_rule_at_every_node(ctx, scene, edge, trunc, max_weight):
    check_byte_for_byte(ctx, scene, edge, trunc, max_weight)


# ---- 2. streaming and state -------------------------------------------------------------------------------------
def test_streaming_and_state(ctx, scene):
    sc = scene
    ks = [0, 1, 0, 1, 0]
    one_T, one_W, n1 = integrate(ctx, sc, ks, 0, 0.5)
    state, n5 = None, None
    for k in ks:
        a, b, n5 = integrate(ctx, sc, [k], 0, 0.5, 64, state)
        state = (a, b)
    assert torch.equal(state[0].view(torch.int32), one_T.view(torch.int32)) and torch.equal(state[1], one_W) and n5 == n1
    # K = 0 with state keeps the bytes
    keep_T, keep_W = one_T.clone(), one_W.clone()
    _, _, nk = integrate(ctx, sc, [], 0, 0.5, 64, (keep_T, keep_W))
    assert torch.equal(keep_T.view(torch.int32), one_T.view(torch.int32)) and torch.equal(keep_W, one_W) and nk == n1
    # K = 0 without state clears whatever the buffers held
    L = __import__("nice_slam_cpp_amd").nsk.lib()
    junk_T, junk_W = torch.full_like(one_T, float("nan")), torch.full_like(one_W, 7.0)
    o = np.ascontiguousarray(sc["origin"], F); s = np.ascontiguousarray(sc["step"], F)
    n = C.c_longlong(-1)
    torch.cuda.synchronize()                                 # (the direct calls below are not ordered against torch's stream)
    rc = L.nsk_tsdf_integrate(ctx.h, o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), sc["nx"], sc["ny"], sc["nz"], 0, None, 24, 32, 40.0, 40.0,
                              15.5, 11.5, None, 0, 0.5, 64.0, 0, C.c_void_p(junk_T.data_ptr()), C.c_void_p(junk_W.data_ptr()), C.byref(n))
    ctx.sync()
    assert rc == 0 and n.value == 0
    assert not bool(junk_T.view(torch.int32).any()) and not bool(junk_W.view(torch.int32).any())
    # frames onto NaN buffers without state: the old values are never read
    junk_T.fill_(float("nan")); junk_W.fill_(7.0)
    d = cu(sc["depths"][ks]); w = np.ascontiguousarray(sc["w2c"][ks].reshape(-1, 16), F)
    torch.cuda.synchronize()
    rc = L.nsk_tsdf_integrate(ctx.h, o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), sc["nx"], sc["ny"], sc["nz"], len(ks),
                              C.c_void_p(d.data_ptr()), 24, 32, 40.0, 40.0, 15.5, 11.5, w.ctypes.data_as(C.c_void_p), 0, 0.5, 64.0, 0,
                              C.c_void_p(junk_T.data_ptr()), C.c_void_p(junk_W.data_ptr()), C.byref(n))
    ctx.sync()
    assert rc == 0 and n.value == n1 and torch.equal(junk_T.view(torch.int32), one_T.view(torch.int32)) and torch.equal(junk_W, one_W)


def test_more_frames_than_a_launch_holds_in_order(ctx, scene):
    """35 frames cross the 32-frame launch boundary; among them the look-away frame and a frame whose matrix is all NaN (it sees nothing);
    the running mean depends on the order, so the reversed list has to equal the reversed rule"""
    sc = dict(scene)
    sc["depths"] = np.concatenate([scene["depths"], scene["depths"][:1]])
    sc["w2c"] = np.concatenate([scene["w2c"], np.full((1, 4, 4), np.nan, F)])
    ks = ([0, 1, 1, 0, 2, 3, 1] * 5)
    assert len(ks) == 35 and ks[31] != ks[32] and sc["away"] == 2
    res = {}
    for name, order in (("forward", ks), ("reversed", ks[::-1])):
        T, W = rule(sc, order, 0, 0.5)
        tsdf, weight, n_obs = integrate(ctx, sc, order, 0, 0.5)
        print("%s: %d observed, largest weight %g" % (name, n_obs, W.max()))
        assert same(tsdf, T) and same(weight, W) and n_obs == int((W > 0).sum())
        assert W.max() >= 10                                # (frames 0 and 1 come ten times each)
        res[name] = T
        alone, _ = rule(sc, [k for k in order if k in (0, 1)], 0, 0.5)
        assert alone.tobytes() == T.tobytes()               # (the two frames that see nothing change nothing)
    print("forward and reversed differ at %d nodes" % int((res["forward"].view(np.uint32) != res["reversed"].view(np.uint32)).sum()))


# ---- 3. volume --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_weight", [1, 2])
def test_volume_flips_the_sign_bit_and_masks(ctx, scene, min_weight):
    sc = scene
    T, W = rule(sc, [0, 1, 0], 0, 0.5)
    T = T.copy()
    zero = np.flatnonzero(W >= 2)[:3]
    T[zero[0]] = F(0.0); T[zero[1]] = -F(0.0)               # a node with T == +0.0 gives -0.0, one with -0.0 gives +0.0
    shape = (sc["nz"], sc["ny"], sc["nx"])
    vol, valid, n_valid = ctx.tsdf_volume(cu(T.reshape(shape)), cu(W.reshape(shape)), min_weight)
    gv, gm = vol.cpu().numpy().reshape(-1), valid.cpu().numpy().reshape(-1)
    ok = W >= min_weight
    assert vol.shape == shape and valid.shape == shape and valid.dtype == torch.uint8
    assert gm.tobytes() == ok.astype(np.uint8).tobytes() and n_valid == int(ok.sum()) and 0 < n_valid < ok.size
    assert (gv.view(np.uint32)[ok] == (T.view(np.uint32)[ok] ^ np.uint32(0x80000000))).all()
    assert (gv.view(np.uint32)[~ok] == np.uint32(0x7fc00000)).all()
    assert gv.view(np.uint32)[zero[0]] == 0x80000000 and gv.view(np.uint32)[zero[1]] == 0
    want, wmask = tc.volume_of(T, W, min_weight, shape)
    assert (np.isnan(want) == np.isnan(gv.reshape(shape))).all() and (want[wmask != 0] == gv.reshape(shape)[wmask != 0]).all()
    if min_weight == 2:
        assert n_valid < int((W >= 1).sum())
    # without the mask and the count the volume is the same
    L = __import__("nice_slam_cpp_amd").nsk.lib()
    v2, dT, dW = torch.empty_like(vol), cu(T), cu(W)
    torch.cuda.synchronize()
    assert L.nsk_tsdf_volume(ctx.h, T.size, C.c_void_p(dT.data_ptr()), C.c_void_p(dW.data_ptr()), float(min_weight), C.c_void_p(v2.data_ptr()), None, None) == 0
    ctx.sync()
    assert torch.equal(v2.view(torch.int32), vol.view(torch.int32))


# ---- 4. mesh ----------------------------------------------------------------------------------------------------
def fuse_sphere(ctx, sc, batch=32):
    return ctx.fuse_depth_mesh(sc["origin"], sc["step"], sc["nx"], sc["depths"], sc["w2c"], sc["intr"], (sc["H"], sc["W"]), frames_per_batch=batch)


def test_fused_sphere_mesh(ctx, sphere):
    sc = sphere
    v, t, info = fuse_sphere(ctx, sc)
    gv, gt = v.cpu().numpy(), t.cpu().numpy()
    print("sphere: %s; the rule gives %d vertices, %d triangles" % (info, len(sc["verts"]), len(sc["tris"])))
    assert info["trunc"] == float(sc["trunc"])               # (the default: three times the largest step)
    assert info["n_observed"] == sc["n_observed"] and info["n_valid"] == sc["n_valid"]
    assert gv.tobytes() == sc["verts"].tobytes() and gt.tobytes() == sc["tris"].tobytes()
    tc.check_sphere_mesh(gv, sc, "device mesh")
    assert mc.signed_volume(gv, gt) > 0                      # wound towards free space: the sphere's outside
    for batch in (32, 3):
        v2, t2, info2 = fuse_sphere(ctx, sc, batch)
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(t2, t) and info2 == info
    # the filter, when asked for: the sphere is one component
    v3, t3, info3 = ctx.fuse_depth_mesh(sc["origin"], sc["step"], sc["nx"], cu(sc["depths"]), sc["w2c"], sc["intr"], (sc["H"], sc["W"]), largest_only=True)
    assert info3["n_kept"] == 1 and 0 < len(t3) <= len(t)


# ---- 5. errors --------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ctx, scene):
    import nice_slam_cpp_amd as pkg
    sc = scene
    L = pkg.nsk.lib()
    err = lambda: L.nsk_last_error().decode()
    nodes = sc["nx"] * sc["ny"] * sc["nz"]
    tsdf = torch.full((nodes,), 9.0, device="cuda"); weight = torch.full((nodes,), 9.0, device="cuda")
    d = cu(sc["depths"]); w = np.ascontiguousarray(sc["w2c"].reshape(-1, 16), F)
    o = np.ascontiguousarray(sc["origin"], F); s = np.ascontiguousarray(sc["step"], F)
    torch.cuda.synchronize()

    def call(trunc=0.5, max_weight=64.0, H=24, W=32, nx=sc["nx"], ny=sc["ny"], nz=sc["nz"], edge=0):
        return L.nsk_tsdf_integrate(ctx.h, o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), nx, ny, nz, 3, C.c_void_p(d.data_ptr()), H, W,
                                    40.0, 40.0, 15.5, 11.5, w.ctypes.data_as(C.c_void_p), edge, trunc, max_weight, 0, C.c_void_p(tsdf.data_ptr()),
                                    C.c_void_p(weight.data_ptr()), None)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert call(trunc=bad) < 0 and "trunc" in err(), bad
    assert call(max_weight=0.0) < 0 and "max_weight" in err()
    assert call(max_weight=float(2 ** 24 + 2)) < 0 and "max_weight" in err()
    assert call(max_weight=float("nan")) < 0
    assert call(H=0) < 0 and "image" in err()
    assert call(nx=1 << 10, ny=1 << 10, nz=(1 << 8) + 1) < 0 and "at most" in err()
    assert call(edge=-1) < 0 and "edge" in err()
    # inside a capture (which records one small launch, so that the graph is not empty) both calls are refused
    p, g, m, v = (torch.zeros(8, device="cuda") for _ in range(4))
    torch.cuda.synchronize()
    with torch.cuda.stream(ctx.tstream):
        ctx.graph_begin()
        try:
            ctx.adam_vector(p, g, m, v, 1e-3, 1)
            rc = call()
            msg = err()
            rc2 = L.nsk_tsdf_volume(ctx.h, nodes, C.c_void_p(tsdf.data_ptr()), C.c_void_p(weight.data_ptr()), 1.0, C.c_void_p(tsdf.data_ptr()), None, None)
            msg2 = err()
        finally:
            ctx.graph_end()
    assert rc < 0 and "captured" in msg and rc2 < 0 and "captured" in msg2
    ctx.sync()
    assert int((tsdf != 9).sum()) == 0 and int((weight != 9).sum()) == 0, "a refused call wrote to the buffers"
    with pytest.raises(pkg.NskError):
        integrate(ctx, sc, [0], 0, 0.0)
    check_byte_for_byte(ctx, sc, 0, 0.5, 64)                 # and a good call follows, on the same context


# ---- 6. rendered ------------------------------------------------------------------------------------------------
def test_fused_rendered_mesh_equals_integrating_the_rendered_frames(tmp_path):
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    ctx = make_ctx(sc)
    ks = cc.cull_scene(sc["bound"], (24, 24, 24), 0.0, keyframes=(0, 1))          # (no padding: the lattice of a Mesher with padding 0)
    n, HW = 24, (cc.IMG_H, cc.IMG_W)
    trunc = F(3.0) * ks["step"].max()
    v, t, info = ctx.fuse_rendered_mesh("color", ks["origin"], ks["step"], n, ks["c2w"], ks["depths"], ks["intr"], HW)
    frames = []
    for k in range(2):
        pose = cu(ks["c2w"][k][:3, :4].astype(F))
        frames.append(ctx.render_image("color", HW, ks["intr"], pose, cu(ks["depths"][k]))[1])
    frames = torch.stack(frames).contiguous()
    tsdf, weight, n_obs = ctx.tsdf_integrate(ks["origin"], ks["step"], n, n, n, frames, ks["intr"], ks["w2c"], 0, trunc)
    vol, valid, n_valid = ctx.tsdf_volume(tsdf, weight, 1)
    v2, t2 = ctx.extract_mesh(vol, ks["origin"], ks["step"], 0.0, valid)
    print("rendered: %s" % info)
    assert info["n_observed"] == n_obs > 0 and info["n_valid"] == n_valid and info["trunc"] == float(trunc)
    assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(t, t2)
    # and the rule on the frames as they came back
    T, W = tc.fuse_f32(ks["pts"], frames.cpu().numpy(), ks["intr"], ks["w2c"], 0, trunc)
    assert same(tsdf, T) and same(weight, W)
    # Mesher::get_rendered_mesh: the same mesh from the C++ host (its colours are not compared here)
    exe = os.path.join(HOST, "fuse_mesh_test")
    if not os.path.exists(exe):
        pytest.fail("fuse_mesh_test is not built (run __graft_entry__.build())")
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(F))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(F))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(F))
    save_frames(d, ks)
    r = subprocess.run([exe, d, os.path.join(d, "r.ply"), str(n), "3", "1", "render"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    pv, pc, pf = mc.read_ply(os.path.join(d, "r.ply"))
    assert out["n_observed"] == n_obs and out["n_valid"] == n_valid and out["vertices"] == len(v) and out["triangles"] == len(t)
    assert pv.tobytes() == v.cpu().numpy().tobytes() and pf.tobytes() == t.cpu().numpy().tobytes()
    assert pc is not None and len(pc) == len(v)


def save_frames(d, sc):
    np.save(os.path.join(d, "depths.npy"), sc["depths"].astype(F))
    np.save(os.path.join(d, "c2ws.npy"), sc["c2w"].astype(F))
    np.save(os.path.join(d, "intr.npy"), np.array(sc["intr"], F))


# ---- 7. host ----------------------------------------------------------------------------------------------------
def test_fuse_mesh_cpp_equals_the_python_path(ctx, sphere, tmp_path):
    exe = os.path.join(HOST, "fuse_mesh_test")
    if not os.path.exists(exe):
        pytest.fail("fuse_mesh_test is not built (run __graft_entry__.build())")
    sc = sphere
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), np.array([[-1.0, 1.0]] * 3, F))
    save_frames(d, sc)
    v, t, info = fuse_sphere(ctx, sc)
    r = subprocess.run([exe, d, os.path.join(d, "fused.ply"), str(sc["nx"]), "3", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    pv, pc, pf = mc.read_ply(os.path.join(d, "fused.ply"))
    assert pc is None
    assert pv.tobytes() == v.cpu().numpy().tobytes() == sc["verts"].tobytes() and pf.tobytes() == t.cpu().numpy().tobytes() == sc["tris"].tobytes()
    assert out["mode"] == "depth" and out["frames"] == 8 and out["resolution"] == sc["nx"]
    assert out["n_observed"] == info["n_observed"] and out["n_valid"] == info["n_valid"]
    assert out["vertices"] == len(v) and out["triangles"] == len(t)


def test_fuse_mesh_cpp_streams_more_frames_than_a_batch(ctx, tmp_path):
    """33 frames cross the 32-frame batch of Mesher::get_fused_mesh on a 24^3 lattice: 32 views from outside, no two alike (the running mean
    depends on their order), and, alone in the second batch, the view from inside.  Each batch observes nodes the other does not (a
    condition of the input); the PLY and the counts are those of the Python path, whose result does not depend on its own batch
    (test_fused_sphere_mesh)."""
    exe = os.path.join(HOST, "fuse_mesh_test")
    if not os.path.exists(exe):
        pytest.fail("fuse_mesh_test is not built (run __graft_entry__.build())")
    n, HW = 24, (cc.IMG_H, cc.IMG_W)
    sc = cc.cull_scene(scenes.REF_BOUND, (n,) * 3, 0.0, keyframes=(0, 1))         # (no padding: the lattice of a Mesher with padding 0)
    tr = cc.long_trajectory(sc, [0] * 32 + [1])
    fuse = lambda sl: ctx.fuse_depth_mesh(sc["origin"], sc["step"], n, tr["depths"][sl], tr["w2c"][sl], sc["intr"], HW)
    v, t, info = fuse(slice(None))
    n_first, n_last = fuse(slice(0, 32))[2]["n_observed"], fuse(slice(32, 33))[2]["n_observed"]
    print("33 frames: %s; %d nodes observed by the first batch alone, %d by the second alone" % (info, n_first, n_last))
    assert len(tr["w2c"]) == 33 and 0 < n_first < info["n_observed"] and 0 < n_last < info["n_observed"]
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), np.asarray(scenes.REF_BOUND, F))
    save_frames(d, tr | {"intr": sc["intr"]})
    r = subprocess.run([exe, d, os.path.join(d, "fused.ply"), str(n), "3", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    pv, pc, pf = mc.read_ply(os.path.join(d, "fused.ply"))
    assert pc is None and len(v) > 0
    assert pv.tobytes() == v.cpu().numpy().tobytes() and pf.tobytes() == t.cpu().numpy().tobytes()
    assert out["mode"] == "depth" and out["frames"] == 33 and out["resolution"] == n
    assert out["n_observed"] == info["n_observed"] and out["n_valid"] == info["n_valid"]
    assert out["vertices"] == len(v) and out["triangles"] == len(t)

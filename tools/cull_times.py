"""times of culling a mesh to a trajectory: python tools/cull_times.py [--quick]
Meshes: the 256^3-lattice mesh of a `scenes` scene and the 12-triangle box room.  Frames: K = 32 and 2000 views drawn inside the mesh's box
(nsk_depth_views, seed 0) standing in for a trajectory, 500 x 500 images, focal 300.
HIP-event medians of 20 repeats after 5 warm-ups, all in one process, per group of nsk_profile:
  points_seen         ms per frame, with depth images rendered from the mesh (zero_sees = 1) and with none (the frustum alone);
  points_view_counts  ms per view, 200 000 surface samples of the mesh as the unseen points;
  select_*            the sub-mesh selection, ms per call;
then cull_mesh(occlusion="self") as a whole on the host clock (rendering included), and the early wave exit's share: the same frames
with every vertex already seen.  --quick: 5 repeats, 2 warm-ups, 128 frames instead of 2000.  No pass/fail time is set."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes
import raster_checks as rk

QUICK = "--quick" in sys.argv
WARM, REPS = (2, 5) if QUICK else (5, 20)
MANY = 128 if QUICK else 2000
H = W = 500
FOCAL = 300.0
CAM = (FOCAL, FOCAL, W / 2.0 - 0.5, H / 2.0 - 0.5)
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
b = sc["bound"]
RES = 256
origin = b[:, 0].astype(np.float32)
step = ((b[:, 1] - b[:, 0]) / np.float32(RES - 1)).astype(np.float32)
verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, RES, RES, RES), origin, step, 0.0)
verts, tris = verts.clone(), tris.clone()                 # (the context's mesh buffers belong to the next extract)
rv, rt = rk.cube_room()
room = (torch.tensor(rv, device="cuda"), torch.tensor(rt, device="cuda"))
print("scene mesh: %d vertices, %d triangles; room: %d triangles; %d x %d, focal %g" % (verts.shape[0], tris.shape[0], rt.shape[0], H, W, FOCAL))


def events(fn):
    rows, whole = [], []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            fn()
        for _ in range(REPS):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.profile_begin(); a.record(); fn(); e.record(); rows.append(ctx.profile_end()); e.synchronize()
            whole.append(a.elapsed_time(e))
    return float(np.median(whole)), {k: float(np.median([r[k][1] for r in rows])) for k in rows[0]}


def run(name, mesh, K):
    v, t = mesh
    w2c = ctx.depth_views(v, K, 0, 0.7)
    w32 = w2c[:32]
    depth = ctx.mesh_depth(v, t, w32, H, W, *CAM)
    for label, d, zs in (("self depth", depth, True), ("frustum   ", None, False)):
        _, g = events(lambda: ctx.points_seen(v, w32, CAM, (H, W), d, 0, 0.03, zs))
        print("%-6s points_seen, 32 frames, %s: %9.4f ms/frame" % (name, label, g["points_seen"] / 32))
    ones = torch.ones(v.shape[0], dtype=torch.uint8, device="cuda")
    _, g = events(lambda: ctx.points_seen(v, w32, CAM, (H, W), depth, 0, 0.03, True, seen=ones))
    print("%-6s points_seen, 32 frames, every vertex seen before (the wave exit): %9.4f ms/frame" % (name, g["points_seen"] / 32))
    del depth
    pts = ctx.sample_mesh(v, t, 200000, 0)
    _, g = events(lambda: ctx.points_view_counts(pts, w32, (H, W), CAM))
    print("%-6s points_view_counts, 200 000 points, 32 views: %9.4f ms/view" % (name, g["points_view_counts"] / 32))
    seen, _ = ctx.points_seen(v, w32[:4], CAM, (H, W))
    _, g = events(lambda: ctx.mesh_select(v, t, seen, 0))
    print("%-6s mesh_select: flags %.4f, scans %.4f, compact %.4f ms" % (name, g["select_flags"], g["select_scan"], g["select_compact"]))
    host = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = ctx.cull_mesh(v, t, w2c, CAM, (H, W), occlusion="self")
        torch.cuda.synchronize(); host.append(1e3 * (time.perf_counter() - t0))
    print("%-6s cull_mesh(self, %d frames) %.1f ms on the host clock (median of 3), %.3f ms/frame: %d of %d vertices seen, %d triangles kept" % (
        name, K, float(np.median(host)), float(np.median(host)) / K, r["n_seen"], v.shape[0], r["tris"].shape[0]))


for name, mesh in (("scene", (verts, tris)), ("room", room)):
    for K in (32, MANY):
        run(name, mesh, K)

"""times of the mesh depth views: python tools/raster_times.py [--quick]
Meshes: the 256^3-lattice mesh of a `scenes` scene and its copy displaced by 1 cm (what Depth L1 compares), and the 12-triangle box room,
where every triangle goes through the queue.  Views: 32 and 1000 (nsk_depth_views, seed 0) at 500 x 500, focal 300.
HIP-event medians of 20 repeats after 5 warm-ups, all in one process: per group of nsk_profile (raster_tris: the triangle kernel,
raster_queue: the queue kernel, raster_finish, depth_stats) in ms per view, and the whole recon_depth_l1 on the host clock.
Then the open choices on 32 views: raster_inline_max 16 .. 1024, and the bare atomic against the load in front of it; every setting must
give the same bytes.  --quick: 5 repeats, 2 warm-ups, 128 views instead of 1000.  No CPU yardstick: no mesh renderer is installed beside it."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes
import raster_checks as rk

QUICK = "--quick" in sys.argv
WARM, REPS = (2, 5) if QUICK else (5, 20)
MANY = 128 if QUICK else 1000
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
verts2 = (verts + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
rv, rt = rk.cube_room()
room = (torch.tensor(rv, device="cuda"), torch.tensor(rt, device="cuda"))
room2 = ((room[0] * 0.99).contiguous(), room[1])
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


def run(name, gt, rec, n_views):
    w2c = ctx.depth_views(gt[0], n_views, 0, 0.7)
    out = {}
    w, g = events(lambda: out.__setitem__("a", ctx.mesh_depth(gt[0], gt[1], w2c[:min(n_views, 512)], H, W, *CAM)))
    V = min(n_views, 512)
    a = out["a"]; c = ctx.mesh_depth(rec[0], rec[1], w2c[:V], H, W, *CAM)
    ws, gs = events(lambda: ctx.depth_pair_stats(a, c))
    print("%-6s %4d views: mesh_depth %9.3f ms/view  (tris %.4f, queue %.4f, finish %.4f)   stats %.4f ms/view" % (
        name, V, w / V, g.get("raster_tris", 0) / V, g.get("raster_queue", 0) / V, g.get("raster_finish", 0) / V, gs["depth_stats"] / V))
    del a, c, out
    host = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m = ctx.recon_depth_l1(rec[0], rec[1], gt[0], gt[1], n_views=n_views, HW=(H, W), focal=FOCAL)
        torch.cuda.synchronize(); host.append(1e3 * (time.perf_counter() - t0))
    print("       recon_depth_l1(%d views) %.1f ms on the host clock (median of 3): depth L1 %.4f cm, both-hit %.4f cm, %d views used" % (
        n_views, float(np.median(host)), m["depth_l1_cm"], m["restricted_l1_cm"], m["n_used"]))
    return w2c


for name, gt, rec in (("scene", (verts, tris), (verts2, tris)), ("room", room, room2)):
    for nviews in (32, MANY):
        w2c = run(name, gt, rec, nviews)
    w32 = w2c[:32]
    base = ctx.mesh_depth(gt[0], gt[1], w32, H, W, *CAM)
    for key, values in (("raster_inline_max", (16, 32, 64, 128, 256, 512, 1024)), ("raster_load_first", (0, 1))):
        for val in values:
            ctx.set_tuning(key, val)
            out = {}
            w, g = events(lambda: out.__setitem__("d", ctx.mesh_depth(gt[0], gt[1], w32, H, W, *CAM)))
            same = bool((out["d"].view(torch.int32) == base.view(torch.int32)).all())
            print("  %-6s %s = %-5d  %9.4f ms/view  (tris %.4f, queue %.4f)  same bytes %s" % (
                name, key, val, w / 32, g.get("raster_tris", 0) / 32, g.get("raster_queue", 0) / 32, same))
        ctx.set_tuning(key, {"raster_inline_max": 64, "raster_load_first": 1}[key])

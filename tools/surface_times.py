"""times of the metrics against the surface: python tools/surface_times.py [N ...] (default 200000 500000 1000000)
N queries -- samples of the 256^3-lattice mesh of a `scenes` scene displaced by 1 cm -- against that mesh.  HIP-event medians of 7 repeats
after 2 warm-ups, all in one process: nsk_mesh_nearest as a whole and by nsk_profile group (the records and the box, the grid build, the
queries' ordering, the query), the query in both visiting orders and at other grid densities (nsk_set_tuning surface_query_mode /
surface_cells_x4: the open choices of DESIGN 7i), nsk_normal_stats, recon_metrics(surface=True) as a whole (host clock), and
nsk_cloud_nearest at the same N for comparison.
Before the times: the bias figure of DESIGN 7i -- accuracy_cm of the displaced copy against the mesh, sampled at n = 50000 / 200000 /
800000 and against the surface at 200000."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

WARM, REPS = 2, 7
sizes = [int(a) for a in sys.argv[1:]] or [200000, 500000, 1000000]
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
b = sc["bound"]
RES = 256
origin = b[:, 0].astype(np.float32)
step = ((b[:, 1] - b[:, 0]) / np.float32(RES - 1)).astype(np.float32)
verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, RES, RES, RES), origin, step, 0.0)
verts2 = (verts + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
print("mesh: %d vertices, %d triangles, lattice step %s" % (verts.shape[0], tris.shape[0], step))


def events(fn):
    """median ms of the whole of fn by HIP events on the context's stream, and the per-group medians of nsk_profile"""
    rows, whole = [], []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            fn()
        for _ in range(REPS):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.profile_begin(); a.record(); fn(); e.record(); rows.append(ctx.profile_end()); e.synchronize()
            whole.append(a.elapsed_time(e))
    return float(np.median(whole)), {k: float(np.median([r[k][1] for r in rows])) for k in rows[0]}


# ---- the bias of measuring against samples -------------------------------------------------------------------------------------------
print("== accuracy_cm of the mesh displaced by 1 cm (rec) against the mesh (gt)")
for n in (50000, 200000, 800000):
    m = ctx.recon_metrics(verts2, tris, verts, tris, n=n)
    print("sampled, n = %7d: accuracy_cm %.4f  completion_cm %.4f" % (n, m["accuracy_cm"], m["completion_cm"]))
m = ctx.recon_metrics(verts2, tris, verts, tris, n=200000, surface=True)
print("surface, n = %7d: accuracy_cm %.4f  completion_cm %.4f  precision %.2f recall %.2f fscore %.2f  normal_consistency %.5f  (skipped: %d / %d triangles, %d normals)" % (
    200000, m["accuracy_cm"], m["completion_cm"], m["precision_pct"], m["recall_pct"], m["fscore_pct"], m["normal_consistency"],
    m["rec_skipped"], m["gt_skipped"], m["normal_skipped"]))

for N in sizes:
    out = {}
    q, own = ctx.sample_mesh(verts2, tris, N, 0, want_tri=True)
    print("== N = %d queries against %d triangles" % (N, tris.shape[0]))
    w, g = events(lambda: out.__setitem__("r", ctx.mesh_nearest(q, verts, tris, want_tri=True)))
    d, hit = out["r"]
    build = sum(v for k, v in g.items() if k not in ("surface_query", "surface_order"))
    print("mesh_nearest (call) %8.3f ms  grid build %.3f ms, ordering %.3f ms, query %.3f ms  %s" % (
        w, build, g.get("surface_order", 0.0), g["surface_query"], {k: round(v, 3) for k, v in g.items()}))
    for mode, name in ((2, "input order"), (4, "cell order")):
        ctx.set_tuning("surface_query_mode", mode)
        _, g2 = events(lambda: out.__setitem__("d2", ctx.mesh_nearest(q, verts, tris)))
        same = bool((out["d2"].view(torch.int32) == d.view(torch.int32)).all())
        print("  query, %-12s %8.3f ms  (ordering %.3f ms)  same bits %s" % (name, g2["surface_query"], g2.get("surface_order", 0.0), same))
    ctx.set_tuning("surface_query_mode", 0)
    for x4 in (4, 16, 64):
        ctx.set_tuning("surface_cells_x4", x4)
        _, g2 = events(lambda: out.__setitem__("d2", ctx.mesh_nearest(q, verts, tris)))
        same = bool((out["d2"].view(torch.int32) == d.view(torch.int32)).all())
        print("  cells per triangle %5.2f: query %8.3f ms, grid build %8.3f ms  same bits %s" % (
            x4 / 4.0, g2["surface_query"], sum(v for k, v in g2.items() if k not in ("surface_query", "surface_order")), same))
    ctx.set_tuning("surface_cells_x4", 16)
    w_n, _ = events(lambda: ctx.normal_stats(verts2, tris, own, verts, tris, hit))
    print("normal_stats        %8.3f ms" % w_n)
    host = []
    for k in range(WARM + 3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m = ctx.recon_metrics(verts2, tris, verts, tris, n=N, surface=True)
        torch.cuda.synchronize(); host.append(1e3 * (time.perf_counter() - t0))
    print("recon_metrics(surface=True) %8.3f ms  (host clock, median of 3)" % float(np.median(host[WARM:])))
    c = ctx.sample_mesh(verts, tris, N, 1)
    w_c, g_c = events(lambda: ctx.cloud_nearest(q, c))
    print("cloud_nearest, N targets    %8.3f ms  (query %.3f ms)" % (w_c, g_c["cloud_query"]))

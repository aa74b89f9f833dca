"""times of the reconstruction metrics: python tools/recon_times.py [N ...] (default 200000 1000000)
Two clouds of N points each: samples of the 256^3-lattice mesh of a `scenes` scene (seed) and of the same mesh displaced by 1 cm (seed + 1).
HIP-event medians of 20 repeats after 5 warm-ups, all in one process: the sampling (areas + scan, the draw), the grid build (box, cells +
scan + placement, the queries' ordering), the query, the stats and the whole recon_metrics call (host clock around the synchronising call);
the query again as a wave per query, in input order, and at other grid densities (nsk_set_tuning cloud_query_mode / cloud_cells_x4).
Beside them the yardstick a user had before: torch.cdist + min over chunks on the same GPU and points (and its largest relative
difference to the exact distances), and scipy's cKDTree.query(workers=16) on the host for orientation."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

WARM, REPS = 5, 20
sizes = [int(a) for a in sys.argv[1:]] or [200000, 1000000]
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
b = sc["bound"]
RES = 256
origin = b[:, 0].astype(np.float32)
step = ((b[:, 1] - b[:, 0]) / np.float32(RES - 1)).astype(np.float32)
verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, RES, RES, RES), origin, step, 0.0)
verts2 = (verts + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
print("mesh: %d vertices, %d triangles" % (verts.shape[0], tris.shape[0]))


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


def cdist_min(q, t, chunk, mode):
    out = torch.empty(q.shape[0], device=q.device)
    for s in range(0, q.shape[0], chunk):
        out[s:s + chunk] = torch.cdist(q[s:s + chunk], t, compute_mode=mode).min(1).values
    return out


failed = False
for N in sizes:
    out = {}
    w_s, g_s = events(lambda: out.__setitem__("a", ctx.sample_mesh(verts, tris, N, 0)))
    a = out["a"]; c = ctx.sample_mesh(verts2, tris, N, 1)
    print("== N = %d per cloud" % N)
    print("sampling           %8.3f ms  %s" % (w_s, {k: round(v, 3) for k, v in g_s.items()}))
    w_q, g_q = events(lambda: out.__setitem__("d", ctx.cloud_nearest(a, c)))
    d = out["d"]
    build = sum(v for k, v in g_q.items() if k != "cloud_query")
    print("nearest (call)     %8.3f ms  grid build %.3f ms, query %.3f ms  %s" % (w_q, build, g_q["cloud_query"], {k: round(v, 3) for k, v in g_q.items()}))
    w_t, g_t = events(lambda: ctx.cloud_stats(d, 0.05))
    print("stats              %8.3f ms  %s" % (w_t, {k: round(v, 3) for k, v in g_t.items()}))
    host = []
    for k in range(WARM + 5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m = ctx.recon_metrics(verts, tris, verts2, tris, n=N)
        torch.cuda.synchronize(); host.append(1e3 * (time.perf_counter() - t0))
    print("recon_metrics      %8.3f ms  (host clock, median of 5)  %s" % (float(np.median(host[WARM:])), {k: round(v, 4) for k, v in m.items() if k.endswith("cm") or k.endswith("pct")}))
    # the open choices
    for mode, name in ((4, "a thread per query, cell order"), (2, "a thread per query, input order"), (5, "a wave per query, cell order"), (3, "a wave per query, input order")):
        ctx.set_tuning("cloud_query_mode", mode)
        _, g = events(lambda: out.__setitem__("d2", ctx.cloud_nearest(a, c)))
        same = bool((out["d2"].view(torch.int32) == d.view(torch.int32)).all())
        print("  query, %-32s %8.3f ms  (ordering %.3f ms)  same bits %s" % (name, g["cloud_query"], g.get("cloud_order", 0.0), same))
    ctx.set_tuning("cloud_query_mode", 0)
    for x4 in (1, 2, 4, 8, 16, 32, 64):
        ctx.set_tuning("cloud_cells_x4", x4)
        _, g = events(lambda: out.__setitem__("d2", ctx.cloud_nearest(a, c)))
        same = bool((out["d2"].view(torch.int32) == d.view(torch.int32)).all())
        print("  cells per target %5.2f: query %8.3f ms, grid build %8.3f ms  same bits %s" % (x4 / 4.0, g["cloud_query"], sum(v for k, v in g.items() if k != "cloud_query"), same))
    ctx.set_tuning("cloud_cells_x4", 4)
    # the yardstick: cdist + min over chunks of the queries.  A chunk's distance matrix is kept at 2^23 entries: the direct form launches
    # one 256-thread workgroup per entry, and a launch of 2^32 threads or more does not run.  The default form goes through a
    # matrix product (|q|^2 + |t|^2 - 2 q.t) and cancels at these distances; the direct form computes the differences first and is the
    # one whose distances must agree with the exact ones
    chunk = max(1, min(N, (1 << 23) // N))
    for mode, name in (("donot_use_mm_for_euclid_dist", "direct"), ("use_mm_for_euclid_dist_if_necessary", "default (matrix product)")):
        with torch.cuda.stream(ctx.tstream):
            for _ in range(2):
                y = cdist_min(a, c, chunk, mode)
            ts = []
            for _ in range(5 if N <= 200000 else 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); y = cdist_min(a, c, chunk, mode); e1.record(); e1.synchronize(); ts.append(e0.elapsed_time(e1))
        rel = float(((y - d).abs() / d.clamp_min(1e-30)).max())
        t_c = float(np.median(ts))
        print("torch.cdist %-26s + min  %9.3f ms  (chunks of %d queries; largest relative difference to the exact distances %.2e); query / cdist = %.5f" % (
            name, t_c, chunk, rel, g_q["cloud_query"] / t_c))
        if mode.startswith("donot") and not (g_q["cloud_query"] < t_c and rel < 1e-5):
            print("  FAILED: the query must take less time than the direct cdist form and agree with it to 1e-5 relative"); failed = True
    try:
        from scipy.spatial import cKDTree
        ah, ch = a.cpu().numpy().astype(np.float64), c.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter(); tree = cKDTree(ch); t1 = time.perf_counter(); dk, _ = tree.query(ah, workers=16); t2 = time.perf_counter()
        print("cKDTree on the host: build %.1f ms, query(workers=16) %.1f ms; largest relative difference %.2e" % (
            1e3 * (t1 - t0), 1e3 * (t2 - t1), float(np.max(np.abs(dk - d.cpu().numpy()) / np.maximum(dk, 1e-30)))))
    except ImportError:
        print("cKDTree: scipy is not installed")
sys.exit(1 if failed else 0)

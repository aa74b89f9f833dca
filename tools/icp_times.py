"""times of the alignment: python tools/icp_times.py [N ...] (default 200000 1000000 0; 0 = the mesh's own vertices)
Source and target: N surface samples each of the 256^3-lattice mesh of a `scenes` scene and of the same mesh displaced by 1 cm (seeds 0, 1),
or that mesh's vertices against the displaced copy's.  HIP-event medians of 20 repeats after 5 warm-ups, all in one process: per evaluation
the query that transforms on load (icp_query, and icp_order where the sources run in cell order) and the pair sums (icp_sums), the grid
build once (cloud_box + cloud_grid), and the host-clock total of a 30-update nsk_cloud_icp.
The yardstick, same run: what a caller did per iteration before nsk_cloud_icp existed -- torch transform of the source, cloud_nearest,
cloud_stats -- on the host clock.  cloud_icp's time per evaluation must be below it at every size, or the tool exits 1."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

WARM, REPS = 5, 20
sizes = [int(a) for a in sys.argv[1:]] or [200000, 1000000, 0]
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
b = sc["bound"]
RES = 256
origin = b[:, 0].astype(np.float32)
step = ((b[:, 1] - b[:, 0]) / np.float32(RES - 1)).astype(np.float32)
verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, RES, RES, RES), origin, step, 0.0)
verts, tris = verts.clone(), tris.clone()
verts2 = (verts + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
print("mesh: %d vertices, %d triangles" % (verts.shape[0], tris.shape[0]))
M1 = np.eye(4); M1[:3, 3] = [-0.004, 0.003, 0.002]


def events(fn):
    """the per-group medians of nsk_profile (ms) and launch counts over REPS runs of fn"""
    rows = []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            fn()
        for _ in range(REPS):
            ctx.profile_begin(); fn(); rows.append(ctx.profile_end())
    return {k: (rows[0][k][0], float(np.median([r[k][1] for r in rows]))) for k in rows[0]}


def host_clock(fn, reps=REPS):
    ts = []
    for k in range(WARM + reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[WARM:])), out


failed = False
for N in sizes:
    if N:
        src, tgt = ctx.sample_mesh(verts, tris, N, 0), ctx.sample_mesh(verts2, tris, N, 1)
        print("== %d x %d surface samples" % (N, N))
    else:
        src, tgt = verts, verts2
        print("== the mesh's %d vertices against its displaced copy's" % verts.shape[0])
    g = events(lambda: ctx.cloud_pair_sums(src, tgt, M1, 0.1))
    build = sum(v[1] for k, v in g.items() if k in ("cloud_box", "cloud_grid"))
    order = g.get("icp_order", (0, 0.0))[1]
    print("one evaluation     icp_query %8.3f ms, icp_order %8.3f ms, icp_sums %8.3f ms;  the grid, once: %8.3f ms  %s" % (
        g["icp_query"][1], order, g["icp_sums"][1], build, {k: round(v[1], 3) for k, v in g.items()}))
    gn = events(lambda: ctx.cloud_nearest(src, tgt))
    print("cloud_nearest      cloud_query %8.3f ms (the same sources untransformed; the query's share of an evaluation is measured against this)" % gn["cloud_query"][1])
    t_icp, (M, info) = host_clock(lambda: ctx.cloud_icp(src, tgt, 0.1, 30, 0.0, 0.0), reps=5)      # (tolerances 0: all 30 updates)
    evals = info["iterations"] + 1
    per_eval = t_icp / evals
    print("cloud_icp          %8.3f ms on the host clock for %d updates (%d evaluations + the grid): %8.3f ms per evaluation; fitness %.4f, rmse %.5f m" % (
        t_icp, info["iterations"], evals, per_eval, info["fitness"], info["rmse"]))
    # the yardstick: one iteration of a caller's own loop on the parent's API
    R = torch.tensor(M1[:3, :3].T.copy(), dtype=torch.float32, device="cuda"); tr = torch.tensor(M1[:3, 3], dtype=torch.float32, device="cuda")

    def yard():
        moved = (src @ R + tr).contiguous()
        d = ctx.cloud_nearest(moved, tgt)
        return ctx.cloud_stats(d, 0.1)
    t_y, _ = host_clock(yard)
    print("yardstick          %8.3f ms per iteration on the host clock (torch transform + cloud_nearest + cloud_stats); cloud_icp per evaluation / yardstick = %.3f" % (
        t_y, per_eval / t_y))
    if not per_eval < t_y:
        print("  FAILED: cloud_icp's time per evaluation must be below the yardstick's time per iteration"); failed = True
sys.exit(1 if failed else 0)

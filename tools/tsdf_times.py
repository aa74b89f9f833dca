"""times of the depth fusion: python tools/tsdf_times.py [--quick]
HIP events around every launch (nsk_profile_begin / _end), 3 warm-ups, 10 repeats, medians.  nsk_tsdf_integrate in ms per frame on
128^3 and 256^3 lattices over the reference bound, 680 x 1200 and 24 x 32 frames of the analytic room, K = 32 and 320 (the depth stack of a
call is resident: 104 MB per 32 full-size frames, so K = 320 goes in ten calls of 32 with state, as fuse_depth_mesh streams it), with the
bytes a 32-frame launch must move (8 B per node read with state, 8 B written, K H W 4 B of depth at most) and the time those take at
8 TB/s; nsk_tsdf_volume at the same lattices (8 B read, 5 B written per node); fuse_depth_mesh as a whole on the host clock (synchronised
work: upload of the frames, fusion, volume, extraction; 3 repeats).  --quick: 128^3 only, K = 32, 3 repeats.  Needs an MI355X: there is
no fallback, and a run elsewhere says nothing."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes, mesh_cull_checks as cc

QUICK = "--quick" in sys.argv[1:]
WARM, REPS, HBM = 3, (3 if QUICK else 10), 8.0e12
LATTICES = (128,) if QUICK else (128, 256)
FRAMES = ((680, 1200, 600.0), (24, 32, 16.0))           # H, W, focal
COUNTS = (32,) if QUICK else (32, 320)
b = scenes.REF_BOUND.astype(np.float32)
ctx = pkg.Context(0)
ctr = b.astype(np.float64).mean(axis=1)


def trajectory(K, H, W, f):
    """K poses on a circle inside the room looking outwards, and the analytic room's depth from each (32 distinct frames, repeated)"""
    m = min(K, 32)
    c2ws = [cc.look_at(ctr + 0.5 * np.array([np.cos(a), 0.1, np.sin(a)]), ctr + 3.0 * np.array([np.cos(a + 0.4), 0.05, np.sin(a + 0.4)]), 0.02)
            for a in np.arange(m) * (2 * np.pi / m)]
    depth = np.stack([scenes.frame_depth_image(b, c, H, W, f, f, W / 2 - 0.5, H / 2 - 0.5) for c in c2ws]).astype(np.float32)
    return torch.tensor(depth, device="cuda"), np.stack([cc.w2c_of(c) for c in c2ws])


def medians(fn):
    rows = []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            fn()
        for _ in range(REPS):
            ctx.profile_begin(); fn(); rows.append(ctx.profile_end())
    return {k: float(np.median([r[k][1] for r in rows])) for k in rows[0]}


print("| lattice | frames | K | tsdf_integrate ms / frame | ms / 32-frame launch | must move per launch | at 8 TB/s |")
print("|---|---|---|---|---|---|---|")
for n in LATTICES:
    origin = b[:, 0].copy()
    step = ((b[:, 1] - b[:, 0]) / np.float32(n - 1)).astype(np.float32)
    trunc = np.float32(3.0) * step.max()
    nodes = n ** 3
    for H, W, f in FRAMES:
        depth, w2c = trajectory(32, H, W, f)
        intr = (f, f, W / 2 - 0.5, H / 2 - 0.5)
        for K in COUNTS:
            out = {}

            def fuse():
                state = None
                for _ in range(K // 32):
                    t, w, n_obs = ctx.tsdf_integrate(origin, step, n, n, n, depth, intr, w2c, 0, trunc, 64, state)
                    state = (t, w)
                out["state"], out["n"] = state, n_obs
            t = medians(fuse)["tsdf_integrate"]
            must = nodes * 16 + 32 * H * W * 4
            print("| %d^3 | %d x %d | %d | %.4f | %.3f | %.1f MB | %.3f ms |" % (n, H, W, K, t / K, t / (K // 32), must / 1e6, 1e3 * must / HBM))
        tsdf, weight = out["state"]
        tv = medians(lambda: ctx.tsdf_volume(tsdf, weight, 1))["tsdf_volume"]
        print("tsdf_volume %d^3 (%d of %d nodes observed): %.3f ms   %.1f MB   %.3f ms at 8 TB/s" % (n, out["n"], nodes, tv, nodes * 13 / 1e6, 1e3 * nodes * 13 / HBM))
        host = depth.cpu().numpy()
        ts = []
        for _ in range(1 + 3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            v, tr, info = ctx.fuse_depth_mesh(origin, step, n, host, w2c, intr, (H, W))
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        print("fuse_depth_mesh %d^3, 32 frames of %d x %d from the host: %.1f ms (median of 3 after one warm-up, host clock), %d vertices, %d triangles"
              % (n, H, W, 1e3 * float(np.median(ts[1:])), info["n_vertices"], info["n_triangles"]))
        del depth, tsdf, weight, out

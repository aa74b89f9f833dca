"""times of the convex hull, the inside mask and the hull-bounded mesh: python tools/hull_times.py [--quick]
Cloud: the vertices of the 256^3-lattice mesh of tools/normals_times.py's scene (reference bound, grids of std 0.3), extracted on the
device (--quick: the 128^3 lattice).  Wall-clock medians of 3 repeats after one warm-up, the stream synchronised around each (--quick: one
repeat, no warm-up): the hull synchronises once per insertion, so HIP events around it would measure the same thing.
  points_hull       the whole call (bounds, quantisation, first simplex, every insertion), and the insertions / re-compactions it made;
  lattice_in_hull   the mask of the same lattice at scale 1.02;
  hull_mesh         fusion of 8 synthetic 120 x 160 depth frames of the analytic room -> hull -> mask -> masked evaluation -> extraction;
  scipy             scipy.spatial.ConvexHull on the same points on the host, download included: what a caller would otherwise do.
No pass/fail time is set."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

QUICK = "--quick" in sys.argv
WARM, REPS = (0, 1) if QUICK else (1, 3)
RES = 128 if QUICK else 256
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
print("box: %s, torch %s; %d warm-ups, %d repeats, medians" % (torch.cuda.get_device_name(0), torch.__version__, WARM, REPS))


def wall(fn):
    out, ts = None, []
    for k in range(WARM + REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        if k >= WARM:
            ts.append(1e3 * (t1 - t0))
    return float(np.median(ts)), out


b = sc["bound"]
origin = b[:, 0].astype(np.float32)
step = ((b[:, 1] - b[:, 0]) / np.float32(RES - 1)).astype(np.float32)
verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, RES, RES, RES), origin, step, 0.0)
verts = verts.clone()
print("%d^3 lattice: %d vertices" % (RES, verts.shape[0]))
ms, (hv, hf, info) = wall(lambda: ctx.points_hull(verts))
print("  %-18s %10.2f ms   %d hull vertices, %d faces, %d insertions, %d re-compactions" % ("points_hull", ms, info[3], info[4], info[5], info[7]))
ms, (valid, n_in) = wall(lambda: ctx.lattice_in_hull(origin, step, RES, RES, RES, 1.02))
print("  %-18s %10.2f ms   %d of %d nodes inside, %d faces" % ("lattice_in_hull", ms, n_in, RES ** 3, info[4]))
try:
    from scipy.spatial import ConvexHull
    t0 = time.perf_counter()
    ref = ConvexHull(verts.cpu().numpy().astype(np.float64))
    print("  %-18s %10.2f ms   %d hull vertices (one run, download included)" % ("scipy on the host", 1e3 * (time.perf_counter() - t0), len(ref.vertices)))
except ImportError:
    print("  scipy is not installed: no host time")

rng = np.random.default_rng(7)
H, W, intr = 120, 160, (150.0, 150.0, 79.5, 59.5)
c2w = np.stack([scenes.make_camera(rng, b) for _ in range(8)]).astype(np.float64)
for k in range(8):                                           # look round the height axis, so that the frames see every wall
    c2w[k, :3, :3] = scenes.look_rotation(k * np.pi / 4, 0.05 * (k % 3 - 1), 0.0)
c2w = c2w.astype(np.float32).astype(np.float64)
depths = torch.tensor(np.stack([scenes.frame_depth_image(b, m, H, W, *intr) for m in c2w]), device="cuda")
w2c = np.stack([np.linalg.inv(m).astype(np.float32) for m in c2w])
ms, (mv, mt, minfo) = wall(lambda: ctx.hull_mesh("fine", origin, step, RES, depths, w2c, intr, (H, W), centres=c2w[:, :3, 3].astype(np.float32)))
print("  %-18s %10.2f ms   fusion %d vertices, hull %d vertices / %d insertions, %d of %d nodes inside, mesh %d vertices"
      % ("hull_mesh", ms, minfo["fused"]["n_vertices"], minfo["hull_info"][3], minfo["hull_info"][5], minfo["n_inside"], RES ** 3, mv.shape[0]))

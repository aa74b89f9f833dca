"""times of mesh simplification (nsk_mesh_simplify) on the scene mesh of tools/mesh_times.py: python tools/simplify_times.py [--quick]
The reference-bound scene of tests/scenes.py is evaluated on a 256^3 lattice (--quick: 96^3) and meshed; the mesh is clustered at cell = 2
and 4 lattice steps (the largest step of the three axes).  Per cell: HIP events around every pass (nsk_profile_begin / _end), 3 warm-ups,
10 repeats (--quick: 1 and 3), medians in ms; the call as a whole on the host clock around synchronised work (it synchronises three times);
vertices and triangles before and after, collapsed and duplicate triangles, cells and occupied cells; and
recon_metrics(surface=True) accuracy_cm / completion_cm of the simplified mesh against the original (200 000 samples each way)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

quick = "--quick" in sys.argv[1:]
WARM, REPS, n = (1, 3, 96) if quick else (3, 10, 256)
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
b = sc["bound"]
origin = b[:, 0].astype(np.float32)
step = ((b[:, 1] - b[:, 0]) / np.float32(n - 1)).astype(np.float32)
verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, n, n, n), origin, step, 0.0)
nv, nt = verts.shape[0], tris.shape[0]
print("== %d^3 nodes, %d vertices, %d triangles (%.1f MB as a PLY without colours), lattice steps %s m" % (n, nv, nt, (nv * 12 + nt * 13) / 1e6, step.tolist()))
PASSES = ("simp_bounds", "simp_cells", "simp_scan", "simp_accumulate", "simp_tris", "simp_lists", "simp_dups", "simp_compact", "simp_out")
for steps in (2, 4):
    cell = float(np.float32(steps) * step.max())
    out = {}
    rows, wall = [], []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            ctx.simplify_mesh(verts, tris, cell)
        for _ in range(REPS):
            ctx.profile_begin(); out["mesh"] = ctx.simplify_mesh(verts, tris, cell, want_info=True); rows.append(ctx.profile_end())
        for _ in range(REPS):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ctx.simplify_mesh(verts, tris, cell)
            torch.cuda.synchronize(); wall.append(time.perf_counter() - t0)
    med = {k: float(np.median([r[k][1] for r in rows])) for k in rows[0]}
    sv, st, info = out["mesh"]
    print("-- cell = %d steps = %.5f m: %d -> %d vertices (%.1f %%), %d -> %d triangles (%.1f %%), %d collapsed, %d duplicates, %d of %d cells occupied, PLY %.1f MB"
          % (steps, cell, nv, sv.shape[0], 100.0 * sv.shape[0] / max(nv, 1), nt, st.shape[0], 100.0 * st.shape[0] / max(nt, 1), info[3], info[4], info[5],
             info[6], (sv.shape[0] * 12 + st.shape[0] * 13) / 1e6))
    for k in PASSES:
        if k in med:
            print("  %-16s %8.3f ms" % (k, med[k]))
    print("  kernels %.3f ms; the call %.3f ms (host clock, median of %d; output tensors allocated and cloned by the binding included)"
          % (sum(med.values()), 1e3 * float(np.median(wall)), REPS))
    m = ctx.recon_metrics(sv, st, verts, tris, surface=True)
    print("  simplified against original, surface distances: accuracy %.4f cm, completion %.4f cm (cell %.3f cm)" % (m["accuracy_cm"], m["completion_cm"], 100.0 * cell))

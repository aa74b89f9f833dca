"""times of the vertex normals and of colouring a mesh along them: python tools/normals_times.py [--quick]
Meshes: the 128^3- and 256^3-lattice meshes of a `scenes` scene (reference bound, grids of std 0.3), extracted on the device.
HIP-event medians of 20 repeats after 5 warm-ups, all in one process (--quick: 5 repeats after 2), per group of nsk_profile:
  mesh_vertex_normals   the whole call, its adjacency (vn_face + vn_scan + vn_place + vn_sort) and its sum (vn_accumulate);
  normal_rays           one launch;
  mesh_vertex_colors    along the normals (48 samples per vertex, and one point query per vertex for the select) and as the point query.
Beside every time: the bytes the launches must move when no cache helps -- counted from the shapes below -- and that amount at 8 TB/s.
  face        per triangle 12 (indices) + 36 (three vertices) + 12 (the normal) + 12 (three counts)
  scan        per vertex 16 (two passes, read and write)
  place       per triangle 12 (indices) + 12 (the normal) + 12 (three cursors) + 12 (three corners)
  sort        per vertex 8 (its segment), per triangle 24 (three corners read and written)
  accumulate  per vertex 8 (its segment) + 12 (the normal), per triangle 12 (three corners) + 36 (three face normals)
  rays        per vertex 24 read, 29 written
  colours     per sample the 3 077 B of the colour stage in nsk_last_call_stats' accounting (feature rows of three levels, the sample itself)
The ratio of the two colourings is a finding, not a target.  No pass/fail time is set."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

QUICK = "--quick" in sys.argv
WARM, REPS = (2, 5) if QUICK else (5, 20)
TBS = 8e12
LENGTH = 0.1
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
S = ctx.n_samples + ctx.n_surface
print("box: %s, torch %s; %d warm-ups, %d repeats, medians; %d samples per ray" % (torch.cuda.get_device_name(0), torch.__version__, WARM, REPS, S))


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


def line(name, ms, nbytes):
    print("  %-34s %9.4f ms   %9.1f MB   %8.4f ms at 8 TB/s   x %.1f" % (name, ms, nbytes / 1e6, 1e3 * nbytes / TBS, ms / (1e3 * nbytes / TBS)))


for res in (128, 256):
    b = sc["bound"]
    origin = b[:, 0].astype(np.float32)
    step = ((b[:, 1] - b[:, 0]) / np.float32(res - 1)).astype(np.float32)
    verts, tris = ctx.extract_mesh(ctx.eval_lattice("fine", origin, step, res, res, res), origin, step, 0.0)
    verts, tris = verts.clone(), tris.clone()             # (the context's mesh buffers belong to the next extract)
    nv, nt = int(verts.shape[0]), int(tris.shape[0])
    normals, info = ctx.mesh_vertex_normals(verts, tris, want_info=True)
    print("%d^3 lattice: %d vertices, %d triangles; %d without a normal, most namings %d" % (res, nv, nt, info["zero"], info["max_valence"]))
    whole, g = events(lambda: ctx.mesh_vertex_normals(verts, tris))
    by = dict(vn_face=72 * nt, vn_scan=16 * nv, vn_place=48 * nt, vn_sort=8 * nv + 24 * nt, vn_accumulate=20 * nv + 48 * nt)
    adj = ("vn_face", "vn_scan", "vn_place", "vn_sort")
    line("mesh_vertex_normals (whole call)", whole, sum(by.values()))
    line("  adjacency", sum(g[k] for k in adj), sum(by[k] for k in adj))
    for k in adj:
        line("    " + k, g[k], by[k])
    line("  vn_accumulate", g["vn_accumulate"], by["vn_accumulate"])
    _, g = events(lambda: ctx.normal_rays(verts, normals, LENGTH))
    line("normal_rays", g["normal_rays"], 53 * nv)
    along, _ = events(lambda: ctx.mesh_vertex_colors(verts, normals, LENGTH))
    line("mesh_vertex_colors along normals", along, 3077.0 * nv * (S + 1) + 53 * nv + 28 * nv)
    point, _ = events(lambda: ctx.mesh_vertex_colors(verts, None, LENGTH))
    line("mesh_vertex_colors point query", point, 3077.0 * nv + 28 * nv)
    print("  along normals / point query: %.1f (samples per vertex: %d against 1)" % (along / point, S + 1))

"""times of the scene-mesh path on the reference bound: python tools/mesh_times.py [resolutions ...] (default 128 256 384)
HIP events around every launch group (nsk_profile_begin / _end), 5 warm-ups, 20 repeats, medians in ms.  Per resolution: lattice evaluation
(fine stage), each extraction pass with the bytes it must move and the time those bytes take at 8 TB/s, the seen mask over K = 16 synthetic
keyframes (1 B per node + K H W 4 B), the lattice evaluation at the set nodes of that mask and of an all-ones mask (nsk_eval_lattice_masked,
same process and context as the dense row, with their ratios to it and the seen fraction), the component filter (12 B per vertex + 24 B per triangle read and written), the colour query on the vertices.
For 256 also what the same volume costs without nsk_eval_lattice: points built on the host, uploaded, nsk_eval_points in chunks, raw
downloaded (host clock around synchronised work, 5 repeats)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes, mesh_cull_checks as cc

WARM, REPS, HBM = 5, 20, 8.0e12
res = [int(a) for a in sys.argv[1:]] or [128, 256, 384]
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
b = sc["bound"]
CHUNK = 1 << 21
# 16 keyframes on a circle inside the room, looking outwards at the walls of the analytic room scenes.frame_depth_image renders
KF, KH, KW, KFX = 16, 240, 320, 200.0
ctr = b.astype(np.float64).mean(axis=1)
c2ws = [cc.look_at(ctr + 0.5 * np.array([np.cos(a), 0.1, np.sin(a)]), ctr + 3.0 * np.array([np.cos(a + 0.4), 0.05, np.sin(a + 0.4)]), 0.02) for a in np.arange(KF) * (2 * np.pi / KF)]
kdepth = torch.tensor(np.stack([scenes.frame_depth_image(b, m, KH, KW, KFX, KFX, KW / 2 - 0.5, KH / 2 - 0.5) for m in c2ws]).astype(np.float32), device="cuda")
kw2c = np.stack([cc.w2c_of(m) for m in c2ws])


def medians(fn):
    rows = []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            fn()
        for _ in range(REPS):
            ctx.profile_begin(); fn(); rows.append(ctx.profile_end())
    return {k: float(np.median([r[k][1] for r in rows])) for k in rows[0]}, rows[0]


for n in res:
    origin = b[:, 0].astype(np.float32)
    step = ((b[:, 1] - b[:, 0]) / np.float32(n - 1)).astype(np.float32)
    nodes = n ** 3
    out = {}
    lat, cnt = medians(lambda: out.__setitem__("vol", ctx.eval_lattice("fine", origin, step, n, n, n)))
    vol = out["vol"]
    ext, _ = medians(lambda: out.__setitem__("mesh", ctx.extract_mesh(vol, origin, step, 0.0)))
    verts, tris = out["mesh"]
    nv, nt = verts.shape[0], tris.shape[0]
    sn, _ = medians(lambda: out.__setitem__("seen", ctx.lattice_seen(origin, step, n, n, n, kdepth, (KFX, KFX, KW / 2 - 0.5, KH / 2 - 0.5), kw2c, 0, 0.5)))
    valid, n_seen = out["seen"]
    # the masked evaluation against the dense one above: under the seen mask (what get_clean_mesh pays) and under all ones (the pure overhead
    # of counting, compacting and scattering); the dense call once more afterwards, so that a drift of the box over the run shows
    ones = torch.ones_like(valid)
    msk, _ = medians(lambda: out.__setitem__("mvol", ctx.eval_lattice("fine", origin, step, n, n, n, valid=valid)))
    same_seen = bool((out["mvol"].view(torch.int32)[valid != 0] == vol.view(torch.int32)[valid != 0]).all()) and bool((out["mvol"][valid == 0] == 100.0).all())
    one, _ = medians(lambda: out.__setitem__("mvol", ctx.eval_lattice("fine", origin, step, n, n, n, valid=ones)))
    same_ones = bool((out["mvol"].view(torch.int32) == vol.view(torch.int32)).all())
    lat2, _ = medians(lambda: ctx.eval_lattice("fine", origin, step, n, n, n))
    del ones

    def culled():
        ctx.extract_mesh(vol, origin, step, 0.0, valid)
        out["clean"] = ctx.filter_mesh(0.2, False)
    flt, _ = medians(culled)
    cv, ct, ncomp, nkept = out["clean"]
    mv, mt = ctx.extract_mesh(vol, origin, step, 0.0, valid)

    def colour():
        for v0 in range(0, nv, CHUNK):
            ctx.eval_points("color", verts[v0:v0 + CHUNK])
    col, _ = medians(colour)
    print("== %d^3 nodes (%.1f M), %d vertices, %d triangles, %d slabs" % (n, nodes / 1e6, nv, nt, cnt["lattice_points"][0]))
    print("lattice evaluation %.3f ms  %s" % (sum(lat.values()), {k: round(v, 3) for k, v in lat.items()}))
    # bytes each pass must move: volume 4 B / node read, cell case 1 B / node, edge map 12 B / node, vertices / triangles 12 B each
    must = {"mc_cells": nodes * 5, "mc_edge_count": nodes * 5, "mc_scan": 0, "mc_vertices": nodes * 17 + nv * 12, "mc_triangles": nodes * 1 + nt * 24}
    for k in ("mc_cells", "mc_edge_count", "mc_scan", "mc_vertices", "mc_triangles"):
        if k in ext:
            print("  %-14s %8.3f ms   %7.1f MB   %.3f ms at 8 TB/s" % (k, ext[k], must[k] / 1e6, 1e3 * must[k] / HBM))
    print("extraction kernels %.3f ms (the call also synchronises twice and reads 8 bytes back)" % sum(ext.values()))
    must_seen = nodes * 1 + KF * KH * KW * 4
    print("seen mask (K = %d, %d x %d): %d of %d nodes seen, %.3f ms   %7.1f MB   %.3f ms at 8 TB/s" % (KF, KH, KW, n_seen, nodes, sn["lattice_seen"], must_seen / 1e6, 1e3 * must_seen / HBM))
    t_lat, t_lat2 = sum(lat.values()), sum(lat2.values())
    for name, t, same in (("seen mask (fraction %.3f)" % (n_seen / nodes), msk, same_seen), ("all-ones mask", one, same_ones)):
        print("lattice evaluation, %s: %.3f ms = %.3f of dense (lattice_compact %.3f ms, same bits: %s)  %s" % (
            name, sum(t.values()), sum(t.values()) / t_lat, t["lattice_compact"], same, {k: round(v, 3) for k, v in t.items()}))
    print("lattice evaluation, dense again after them: %.3f ms (%.3f of the first)" % (t_lat2, t_lat2 / t_lat))
    must_flt = mv.shape[0] * 12 + mt.shape[0] * 24
    fk = {k: v for k, v in flt.items() if k.startswith("cc_")}
    print("filter of the culled mesh (%d vertices, %d triangles, %d components -> %d kept, %d vertices, %d triangles): %.3f ms   %7.1f MB   %.3f ms at 8 TB/s  %s" % (
        mv.shape[0], mt.shape[0], ncomp, nkept, cv.shape[0], ct.shape[0], sum(fk.values()), must_flt / 1e6, 1e3 * must_flt / HBM, {k: round(v, 3) for k, v in fk.items()}))
    print("extraction with the mask %.3f ms" % sum(v for k, v in flt.items() if k.startswith("mc_")))
    print("colour query %.3f ms  %s" % (sum(col.values()), {k: round(v, 3) for k, v in col.items()}))
    if n == 256:
        ts = []
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            c = [(origin[a] + np.arange(n, dtype=np.float32) * step[a]).astype(np.float32) for a in range(3)]
            P = np.empty((n, n, n, 3), np.float32)
            P[..., 0] = c[0][None, None, :]; P[..., 1] = c[1][None, :, None]; P[..., 2] = c[2][:, None, None]
            P = P.reshape(-1, 3)
            raw = np.empty((nodes, 4), np.float32)
            for m0 in range(0, nodes, 1 << 22):
                d = torch.from_numpy(P[m0:m0 + (1 << 22)]).cuda()
                raw[m0:m0 + (1 << 22)] = ctx.eval_points("fine", d).cpu().numpy()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        same = bool((raw[:, 3].view(np.int32) == vol.cpu().numpy().reshape(-1).view(np.int32)).all())
        print("host-built points + chunked nsk_eval_points + download of raw: %.1f ms (median of 5, host clock; same bits: %s)" % (1e3 * float(np.median(ts)), same))
    del vol, verts, tris, out, valid, cv, ct, mv, mt

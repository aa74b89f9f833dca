"""times of importance sampling (nsk_set_importance): python tools/importance_times.py [--quick]
  the forward (nsk_render_forward, colour stage) at 5000 x 48 and 1000 x 48 with n_importance = 0 and 16,
  the colour-stage step (nsk_map_step + nsk_adam_step, colour decoder trainable) at the same sizes,
  the resample launch alone (nsk_importance_resample, 48 -> 64 depths).
Wall time per call over a synchronised batch of calls on the context's stream, the median of several batches, and the HIP-event times of the
launches inside one forward.  On a tree without nsk_set_importance only the n_importance = 0 rows are printed (for A/B runs against it)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes
QUICK = "--quick" in sys.argv
CALLS, BATCHES = (20, 3) if QUICK else (100, 7)
cu = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
sc = scenes.make_scene(42)
HAS = hasattr(pkg.Context, "set_importance")


def wall(fn):
    """microseconds per call: the median over BATCHES synchronised batches of CALLS calls"""
    for _ in range(5): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(BATCHES):
        t0 = time.perf_counter()
        for _ in range(CALLS): fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / CALLS * 1e6)
    return float(np.median(out)), float(min(out)), float(max(out))


def events(ctx, fn, n=20):
    ctx.profile_begin()
    for _ in range(n): fn()
    return {k: round(1e3 * ms / c, 1) for k, (c, ms) in ctx.profile_end().items()}


for N in (5000, 1000):
    r = scenes.make_rays(7, N, sc["bound"], n_frames=5)
    ro, rd, gd, gc = cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), cu(r["gt_color"])
    base = {}
    for Ni in ((0, 16) if HAS else (0,)):
        ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
        ctx.decoder_set_trainable("color", True)
        if Ni: ctx.set_importance(Ni)
        loss = torch.zeros(1, device="cuda")
        out = (torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda"))
        lr = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]
        with torch.cuda.stream(ctx.tstream):
            fwd = lambda: ctx.render_forward("color", ro, rd, gd, want_weights=False)
            def step():
                ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.2, True, flags=3, loss=loss, outputs=out)
                ctx.adam_step(lr)
            tf, ts = wall(fwd), wall(step)
            ev = events(ctx, fwd)
        for name, t in (("forward", tf), ("step", ts)):
            ratio = "" if not Ni else "  (%.2f x n_importance = 0)" % (t[0] / base[name])
            base.setdefault(name, t[0])
            print("%-8s %5d x 48  n_importance %2d: %8.1f us  [%.1f .. %.1f]%s" % (name, N, Ni, t[0], t[1], t[2], ratio))
        print("         launches of one forward (HIP events, us): %s" % ev)
        if Ni:
            z = torch.sort(torch.rand(N, 48, device="cuda") * 5 + 0.1, 1)[0].contiguous(); w = (torch.rand(N, 48, device="cuda") / 48).contiguous()
            with torch.cuda.stream(ctx.tstream):
                res = lambda: ctx.importance_resample(z, w, Ni)
                tr, er = wall(res), events(ctx, res)
            print("resample %5d x 48 -> 64 alone: %8.1f us wall per call, HIP events %s" % (N, tr[0], er))
        ctx.close()

"""Bit-level A/B of two builds of libnsk.so on the steps tools/ab_outputs.py does not run (NSK_LIB selects the library; run once per build, compare
the printed lines): a K2 colour step (forward k_decode_fwd_multi_bf16<8,2>, backward k_decode_bwd_multi<false>), a K3 fine-stage step (backward
k_decode_bwd_frozen) and one Tracker step (k_decode_bwd_track), each at its BASELINE size and in the product mode, with the launch forms the host
recorded.

What a step computes in a fixed order is printed as a SHA digest and must be equal between the builds: the loss, the rendered colour / depth /
variance, the ReLU bits the forward saved, the per-sample raw gradient.  What the merged backward kernels ADD WITH FLOAT ATOMICS (grid gradients,
ray gradients) or sum over slabs whose split moves with the tile dealing (decoder gradient) has no fixed order: the step runs twice per build, a
digest is printed where the two runs agree, and otherwise "order-dependent" with the largest difference between the two runs relative to the
array's largest magnitude.  With --save DIR the first run's arrays are written to DIR/<step>.npz; with --against DIR the largest difference to the
arrays saved there (the other build's) is printed beside it: it must be of the size of the run-to-run figure.  The deterministic mode of
ab_outputs.py fixes the order, but runs the one-decoder kernels and not these.
usage: NSK_LIB=<lib> python tools/ab_outputs_steps.py [--save DIR] [--against DIR]"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import scenes
from gpu_util import cu, make_ctx
import test_gpu_configs as tc

opt = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
SAVE, AGAINST = opt("--save"), opt("--against")
dg = lambda a: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]
rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def map_run(sc, rays, stage, trainable, flags):
    """one mapping step on a fresh context: (arrays in a fixed order, accumulated arrays, launch forms)"""
    N = rays["rays_o"].shape[0]; M = N * 48
    gmax = float(rays["gt_depth"].max())
    ro, rd, gd, gc = cu(rays["rays_o"]), cu(rays["rays_d"]), cu(rays["gt_depth"]), cu(rays["gt_color"])
    ctx = make_ctx(sc, trainable=trainable)
    loss = torch.zeros(1, device="cuda")
    out = (torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda"))
    ctx.map_step(stage, ro, rd, gd, gc, gmax, 0.5, stage == "color", flags=flags, loss=loss, outputs=out)
    ctx.sync()
    levels = ("middle", "fine", "color") if stage == "color" else ("middle", "fine")
    fixed = dict(loss=np.float32(float(loss)), rgb=out[0].cpu().numpy(), depth=out[1].cpu().numpy(), var=out[2].cpu().numpy(), g_raw=ctx.debug_fetch("g_raw", M))
    for k in levels:
        fixed["relu_" + k] = ctx.debug_relu_bits(k, M)
    summed = {"g_" + k: ctx.grid_download(k, grad=True) for k in levels}
    for k in trainable:
        summed["g_dec_" + k] = ctx.decoder_download(k, grad=True)
    forms = "forward %s, backward %s" % (ctx.debug_last_split()["form"], ctx.debug_last_split(backward=True)["form"])
    ctx.close()
    return fixed, summed, forms


def track_run():
    """one Tracker step at 200 rays (tools/track_times.py)"""
    N = 200
    sc = scenes.make_scene(42)
    r = scenes.make_rays(7, N, sc["bound"], H=680, W=1200, n_frames=1, edge=20)
    ctx = make_ctx(sc)
    ro, rd, gd, gc = cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), cu(r["gt_color"])
    loss = torch.zeros(1, device="cuda")
    g_ro, g_rd = torch.empty(N, 3, device="cuda"), torch.empty(N, 3, device="cuda")
    ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, True, True, True, flags=4, loss=loss, g_rays=(g_ro, g_rd))
    ctx.sync()
    fixed = dict(loss=np.float32(float(loss)), median_thr=ctx.debug_fetch("median_thr", N * 48))
    for k in ("middle", "fine", "color"):
        fixed["relu_" + k] = ctx.debug_relu_bits(k, N * 48)
    summed = dict(g_rays_o=g_ro.cpu().numpy(), g_rays_d=g_rd.cpu().numpy())
    forms = "forward %s, backward %s" % (ctx.debug_last_split()["form"], ctx.debug_last_split(backward=True)["form"])
    ctx.close()
    return fixed, summed, forms


def report(name, run):
    (fixed, summed, forms), (fixed2, summed2, _) = run(), run()
    words = ["%s (%s):" % (name, forms)]
    for k, a in fixed.items():
        words += [k, dg(a) if dg(a) == dg(fixed2[k]) else "NOT-REPRODUCIBLE"]
    other = np.load(os.path.join(AGAINST, name + ".npz")) if AGAINST else None
    for k, a in summed.items():
        same = dg(a) == dg(summed2[k])
        words += [k, dg(a) if same else "order-dependent(run-to-run %.1e)" % rel(summed2[k], a)]
        if other is not None:
            words.append("[other build %.1e]" % rel(other[k], a))
    if SAVE:
        os.makedirs(SAVE, exist_ok=True)
        np.savez(os.path.join(SAVE, name + ".npz"), **summed)
    print(" ".join(words))


sc, rays, _, _ = tc._strict_case("K2-color")
report("K2-color", lambda: map_run(sc, rays, "color", ["color"], 3))
sc, rays, _, _ = tc._strict_case("K3-fine")
report("K3-fine", lambda: map_run(sc, rays, "fine", [], 1))
report("Tracker", track_run)

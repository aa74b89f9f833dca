"""times of the whole-frame render on the reference bound: python tools/render_times.py H W [chunk ...] (default 680 1200, chunks 25600 ... the frame)
HIP events on the context's stream around each call, 5 warm-ups, 20 repeats, medians in ms.  Per chunk size (a context of its own, so that the
workspace is the one that chunk size needs): Context.render_image; the same chunks rendered by Context.render_forward from rays built beforehand
(what a user could do before nsk_render_image: the yardstick) and the ratio of the two; device memory the render allocated (workspace + the
chunk's rays).  Once: the rays kernel alone over the whole frame and the metrics call (its one synchronisation included)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg, scenes

WARM, REPS = 5, 20
H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (680, 1200)
total = H * W
chunks = [int(a) for a in sys.argv[3:]] or sorted({min(c, total) for c in (25600, 51200, 102400, 204800, 409600, total)})
STAGE = "color"
sc = scenes.make_scene(3, grid_std=0.3, bias_std=0.1)
b = sc["bound"]
c2w = scenes.make_camera(np.random.default_rng(0), b)
intr = (600.0 * W / 1200.0, 600.0 * W / 1200.0, (W - 1) / 2.0, (H - 1) / 2.0)          # config/nice_slam.yaml's camera, scaled to the image
depth_np = scenes.frame_depth_image(b, c2w, H, W, *intr)
color_np = scenes.frame_color_image(b, c2w, H, W, *intr)
depth = torch.tensor(depth_np, device="cuda"); color = torch.tensor(color_np, device="cuda")
pose = torch.tensor(np.ascontiguousarray(c2w[:3, :4], np.float32), device="cuda")


def median_ms(ctx, fn):
    ts = []
    with torch.cuda.stream(ctx.tstream):
        for k in range(WARM + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            if k >= WARM:
                ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def new_ctx():
    ctx = pkg.Context(0); ctx.set_render_opts(); ctx.load_scene(b, sc["grids"], sc["decoders"])
    return ctx


print("== %d x %d = %d rays, stage %s, 48 samples per ray" % (H, W, total, STAGE))
print("%10s %7s %14s %16s %7s %14s" % ("chunk", "chunks", "render_image", "render_forward", "ratio", "device memory"))
rows, img = [], None
for chunk in chunks:
    ctx = new_ctx()
    ro, rd, gd = ctx.image_rays((H, W), intr, pose, depth)
    warm = [torch.empty(H, W, 3, device="cuda"), torch.empty(H, W, device="cuda"), torch.empty(H, W, device="cuda")]; del warm      # the images' blocks stay with torch's allocator
    torch.cuda.synchronize(); free0 = torch.cuda.mem_get_info()[0]
    img = ctx.render_image(STAGE, (H, W), intr, pose, depth, chunk_rays=chunk)
    torch.cuda.synchronize(); mem = free0 - torch.cuda.mem_get_info()[0]
    t_img = median_ms(ctx, lambda: ctx.render_image(STAGE, (H, W), intr, pose, depth, chunk_rays=chunk))

    def by_hand():
        for a in range(0, total, chunk):
            ctx.render_forward(STAGE, ro[a:a + chunk], rd[a:a + chunk], gd[a:a + chunk], want_weights=False)
    t_fwd = median_ms(ctx, by_hand)
    rows.append((chunk, t_img, t_fwd, mem))
    print("%10d %7d %11.3f ms %13.3f ms %7.3f %11.1f MB" % (chunk, -(-total // chunk), t_img, t_fwd, t_img / t_fwd, mem / 1e6), flush=True)
    if chunk != chunks[-1]:
        del ctx, ro, rd, gd
best = min(r[1] for r in rows)
pick = min(r[0] for r in rows if r[1] <= 1.03 * best)
print("best render_image %.3f ms; smallest chunk within 3 %% of it: %d (%.2f M rays/s)" % (best, pick, total / best / 1e3))
t_rays = median_ms(ctx, lambda: ctx.image_rays((H, W), intr, pose, depth))
print("rays kernel alone (whole frame, one launch, 28 B written + 4 B read per ray): %.4f ms" % t_rays)
t_met = median_ms(ctx, lambda: ctx.image_metrics(img[0], img[1], depth, color))
t_met_r = median_ms(ctx, lambda: ctx.image_metrics(img[0], img[1], depth, color, want_residuals=True))
m = ctx.image_metrics(img[0], img[1], depth, color)
print("metrics call (two launches + the read-back of 64 B): %.4f ms; with both residual images: %.4f ms" % (t_met, t_met_r))
print("frame against the analytic room: depth L1 %.4f over %d pixels, PSNR %.2f dB, %d non-finite pixels" % (m["depth_l1"], m["depth_pixels"], m["psnr"], m["nonfinite"]))

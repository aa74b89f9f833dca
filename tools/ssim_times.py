"""times of the structural similarity of two frames: python tools/ssim_times.py [--quick]
Images: 680 x 1200 x 3 (a keyframe of config/nice_slam.yaml's camera) and 161 x 176 x 3 (the smallest frame five levels hold), uniform
noise against noise + 0.1 N(0, 1), clipped, as device tensors.  Per size: SSIM (one level) and five-level MS-SSIM, with and without the
level-0 map, ms per call (the call's one synchronisation included), and per group of nsk_profile (ssim_tile, ssim_pool, ssim_sums) the
sum over the call's launches; beside them nsk_image_metrics on a frame of the same size.
HIP-event medians of 20 repeats after 5 warm-ups, all in one process; the per-group times come from a second pass with the profile on.  --quick: 5 repeats, 2 warm-ups.  No pass/fail time is set."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import nice_slam_cpp_amd as pkg

QUICK = "--quick" in sys.argv
WARM, REPS = (2, 5) if QUICK else (5, 20)
ctx = pkg.Context(0)


def events(fn):
    """(ms per call with the profile off, {group: ms} from a second pass with it on): the profile's events are not in the call's time"""
    rows, whole = [], []
    with torch.cuda.stream(ctx.tstream):
        for k in range(WARM + REPS):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); e.record(); e.synchronize()
            if k >= WARM:
                whole.append(a.elapsed_time(e))
        for _ in range(REPS):
            ctx.profile_begin(); fn(); rows.append(ctx.profile_end())
    return float(np.median(whole)), {k: float(np.median([r[k][1] for r in rows])) for k in rows[0]}


print("%-16s %-28s %10s   %s" % ("frame", "call", "ms / call", "per group, ms (sum over the call's launches)"))
for H, W in ((680, 1200), (161, 176)):
    rng = np.random.default_rng(H)
    a_np = rng.random((H, W, 3)).astype(np.float32)
    b_np = np.clip(a_np + 0.1 * rng.standard_normal((H, W, 3)), 0.0, 1.0).astype(np.float32)
    a, b = torch.tensor(a_np, device="cuda"), torch.tensor(b_np, device="cuda")
    depth, gt = a[:, :, 0].contiguous(), b[:, :, 0].contiguous()
    frame = "%d x %d x 3" % (H, W)
    for levels in (1, 5):
        for want_map in (False, True):
            t, groups = events(lambda: ctx.image_ssim(a, b, levels=levels, want_map=want_map))
            name = "%s%s" % ("SSIM" if levels == 1 else "MS-SSIM, 5 levels", ", with the map" if want_map else "")
            print("%-16s %-28s %10.4f   %s" % (frame, name, t, ", ".join("%s %.4f" % (k, v) for k, v in sorted(groups.items()))), flush=True)
    t, groups = events(lambda: ctx.image_metrics(a, depth, gt, b))
    print("%-16s %-28s %10.4f   %s" % (frame, "nsk_image_metrics", t, ", ".join("%s %.4f" % (k, v) for k, v in sorted(groups.items()))), flush=True)
    m = ctx.image_ssim(a, b, levels=5)
    print("%-16s SSIM %.6f, MS-SSIM %.6f, %d windows left out" % (frame, m["ssim"], m["ms_ssim"], m["left_out"]))

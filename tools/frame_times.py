"""times of the frame preparation: python tools/frame_times.py [--quick]
ms per frame of Context.prepare_frames (nsk_frame_prepare) for three shapes, in batches of 1 and 32 raw frames that already lie on the device:
  TUM      480 x 640 uint8 / uint16, five coefficients, crop_size 384 x 512, crop_edge 8       (S0 S1 S3 S4)
  ScanNet  968 x 1296 colour over 480 x 640 depth, crop_edge 10                                (S0 S2 S4)
  Replica  680 x 1200, nothing on                                                              (S0)
HIP-event medians of 20 repeats after 5 warm-ups, all in one process (--quick: 5 after 2): the kernel alone (nsk_profile's frame_prepare
group) and the whole call (with undistortion it reads the border count back, which synchronises).  Beside each: the bytes the launch must
move when no cache helps (every raw byte once, every output float once) and that amount at 8 TB/s; and what the frame costs today, the
upload of the same frame as float32 images from pageable host memory (colour + depth at the raw sizes), next to the upload of its raw bytes.
No pass/fail time is set."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import nice_slam_cpp_amd as pkg

QUICK = "--quick" in sys.argv
WARM, REPS = (2, 5) if QUICK else (5, 20)
TBS = 8e12
SHAPES = [
    ("TUM", (480, 640), (480, 640), dict(intr=(517.3, 516.5, 318.6, 255.3), distortion=[0.2624, -0.9531, -0.0054, 0.0026, 1.1633], crop_size=(384, 512),
                                         crop_edge=8, png_depth_scale=5000.0)),
    ("ScanNet", (968, 1296), (480, 640), dict(intr=(577.590698, 578.729797, 318.905426, 242.683609), crop_edge=10, png_depth_scale=1000.0)),
    ("Replica", (680, 1200), (680, 1200), dict(intr=(600.0, 600.0, 599.5, 339.5), png_depth_scale=6553.5)),
]
ctx = pkg.Context(0)
print("box: %s, torch %s; %d warm-ups, %d repeats, medians" % (torch.cuda.get_device_name(0), torch.__version__, WARM, REPS))


def events(fn):
    rows, whole = [], []
    with torch.cuda.stream(ctx.tstream):
        for _ in range(WARM):
            fn()
        for _ in range(REPS):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.profile_begin(); a.record(); fn(); e.record(); rows.append(ctx.profile_end()); e.synchronize()
            whole.append(a.elapsed_time(e))
    return float(np.median(whole)), float(np.median([r["frame_prepare"][1] for r in rows]))


def upload_ms(arrays):
    """wall ms of copying the host arrays to the device, synchronised; the median of the repeats"""
    ts = []
    for _ in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = [torch.from_numpy(a).cuda() for a in arrays]
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
        del keep
    return float(np.median(ts[WARM:]))


rng = np.random.default_rng(0)
for name, (Hc, Wc), (Hd, Wd), kw in SHAPES:
    H, W, intr_out = pkg.nsk.frame_plan((Hc, Wc), (Hd, Wd), **kw)
    print("%s: colour %d x %d, depth %d x %d -> %d x %d, fx %.3f fy %.3f cx %.3f cy %.3f" % ((name, Hc, Wc, Hd, Wd, H, W) + tuple(float(v) for v in intr_out)))
    for n in (1, 32):
        c8 = rng.integers(0, 256, size=(n, Hc, Wc, 3), dtype=np.uint8)
        d16 = rng.integers(0, 65536, size=(n, Hd, Wd), dtype=np.uint16).view(np.int16)
        tc, td = torch.from_numpy(c8).cuda(), torch.from_numpy(d16).cuda()
        out = ctx.prepare_frames(tc, td, **kw)
        whole, kern = events(lambda: ctx.prepare_frames(tc, td, **kw))
        nbytes = n * (Hc * Wc * 3 + Hd * Wd * 2 + H * W * 16)
        up_raw = upload_ms([c8[:1], d16[:1]])
        up_f32 = upload_ms([c8[:1].astype(np.float32), d16[:1].astype(np.float32)])
        print("  n = %2d   kernel %8.4f ms / frame   call %8.4f ms / frame   %7.2f MB / frame   %7.4f ms at 8 TB/s   x %5.1f   n_border %d / frame"
              % (n, kern / n, whole / n, nbytes / n / 1e6, 1e3 * nbytes / n / TBS, kern / (1e3 * nbytes / TBS), out[3] // n))
        print("           upload of one frame: raw bytes %.3f ms (%.2f MB), as float32 images %.3f ms (%.2f MB)"
              % (up_raw, (Hc * Wc * 3 + Hd * Wd * 2) / 1e6, up_f32, (Hc * Wc * 12 + Hd * Wd * 4) / 1e6))

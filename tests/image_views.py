"""numpy restatements for the whole-frame tests (tests/test_render_image_cpu.py, tests/test_gpu_render_image.py): the pixel lists of a view,
the residual metrics of nsk_image_metrics, the small frame both test files render, and the oracle's chunk-by-chunk render."""
import numpy as np

import scenes

H, W = 24, 32
INTR = (30.0, 29.0, 15.5, 11.5)          # fx, fy, cx, cy
CHUNKS = (768, 200, 32, 5000)            # the whole view; a ragged last chunk of 168; one row; larger than the view


def view_shape(H, W, window=None, stride=1):
    H0, H1, W0, W1 = window if window is not None else (0, H, 0, W)
    return (H1 - H0 + stride - 1) // stride, (W1 - W0 + stride - 1) // stride


def view_pixels(H, W, window=None, stride=1):
    """(pix_i columns, pix_j rows) int32 of the view's pixels, row-major: n = row * Wv + col -> i = W0 + stride col, j = H0 + stride row"""
    H0, H1, W0, W1 = window if window is not None else (0, H, 0, W)
    assert 0 <= H0 < H1 <= H and 0 <= W0 < W1 <= W and stride >= 1
    jj, ii = np.meshgrid(np.arange(H0, H1, stride), np.arange(W0, W1, stride), indexing="ij")
    return ii.reshape(-1).astype(np.int32), jj.reshape(-1).astype(np.int32)


def metrics_ref(rgb, depth, gt_depth=None, gt_color=None):
    """nsk_image_metrics restated: every difference one float32 operation, widened to float64 (squared, for the colour), summed in float64;
    a pixel whose rendered depth or colour is not finite is left out of every sum and counted in h[5].
    -> (h [8] float64, res_depth or None, res_color or None)"""
    rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
    depth = np.asarray(depth, np.float32).reshape(-1)
    good = np.isfinite(depth) & np.isfinite(rgb).all(axis=1)
    h = np.zeros(8, np.float64)
    h[0] = depth.size
    h[5] = int((~good).sum())
    res_d = res_c = None
    with np.errstate(invalid="ignore"):
        if gt_depth is not None:
            g = np.asarray(gt_depth, np.float32).reshape(-1)
            res_d = np.where(g > 0, np.abs((g - depth).astype(np.float32)), np.float32(0)).astype(np.float32)
            m = good & (g > 0) & np.isfinite(res_d)
            h[1] = int(m.sum())
            h[2] = res_d[m].astype(np.float64).sum()
        if gt_color is not None:
            gc = np.asarray(gt_color, np.float32).reshape(-1, 3)
            res_c = np.abs((gc - rgb).astype(np.float32)).astype(np.float32)
            m = good[:, None] & np.isfinite(res_c)
            h[3] = int(m.sum())
            h[4] = (res_c[m].astype(np.float64) ** 2).sum()
    return h, res_d, res_c


def psnr(h):
    return -10.0 * np.log10(h[4] / h[3])


def make_frame(seed=5):
    """the 24 x 32 frame of the tests: the small scene, a camera inside its room, the room's depth and colour images; a 5 x 7 block and
    about 5 % scattered pixels of the depth image carry no measurement (0), so that every chunk holds some (src/Renderer.cpp:94-98)"""
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    rng = np.random.default_rng(seed)
    c2w = scenes.make_camera(rng, sc["bound"])
    fx, fy, cx, cy = INTR
    depth = scenes.frame_depth_image(sc["bound"], c2w, H, W, fx, fy, cx, cy)
    color = scenes.frame_color_image(sc["bound"], c2w, H, W, fx, fy, cx, cy)
    depth[9:14, 11:18] = 0.0
    depth[rng.random((H, W)) < 0.05] = 0.0
    return dict(scene=sc, c2w=np.ascontiguousarray(c2w[:3, :4], np.float32), depth=np.ascontiguousarray(depth, np.float32),
                color=np.ascontiguousarray(color, np.float32), intr=INTR, HW=(H, W))


def frame_rays(oracle, fr, window=None, stride=1):
    """rays and gathered depth of the frame's view through the oracle's explicit-index functions"""
    pi, pj = view_pixels(H, W, window, stride)
    fx, fy, cx, cy = fr["intr"]
    ro, rd = oracle.rays_from_pixels(pi, pj, fx, fy, cx, cy, fr["c2w"])
    gd, _ = oracle.gather_pixels(pi, pj, fr["depth"], fr["color"])
    return ro, rd, gd


def chunk_ranges(n, chunk):
    return [(a, min(chunk, n - a)) for a in range(0, n, chunk)]


def oracle_render(oracle, sc, stage, ro, rd, gd, chunk, gt_depth_max=-1.0, n_samples=32, n_surface=16):
    """the oracle's render of the rays chunk by chunk (each chunk a batch of its own: gt_depth_max < 0 takes the chunk's maximum)"""
    opts = oracle.opts(sc["bound"], n_samples=n_samples, n_surface=n_surface)
    parts = []
    for a, n in chunk_ranges(ro.shape[0], chunk):
        parts.append(oracle.render_forward(opts, sc["grids"], sc["decoders"], stage, ro[a:a + n], rd[a:a + n], None if gd is None else gd[a:a + n], gt_depth_max))
    return {k: np.concatenate([p[k] for p in parts]) for k in ("rgb", "depth", "var")}

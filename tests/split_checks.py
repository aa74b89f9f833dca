"""helpers shared by tests/test_gpu_split.py and tests/test_gpu_parity.py: the gradient assertion of the parity tests, and the scene, batches and
oracle references of the workgroup-split sweep (computed once per (stage, size, filtered) and reused by every knob setting: the sweep itself
costs GPU launches only)"""
import numpy as np

import scenes
from gpu_util import cu, make_ctx, stage_levels
from scenes import rel_l2

TOL = 1e-4
# tiles of 16 samples -> (rays, n_samples, n_surface): 999 tiles is the smallest batch at which one role can sit at its cap of 125 workgroups
# while another has one; 17 x 13 samples = 14 tiles, fewer than the waves of one workgroup per role; one ray
SIZES = {999: (333, 32, 16), 14: (17, 8, 5), 3: (1, 32, 16)}
SPLIT_KEYS = ("frozen_cost", "frozen_cost_rays", "frozen_mid_pct", "dead_tile_pct", "fwd_fine_cost", "fwd_occ_cost", "fwd_color_cost",
              "no_frozen_kernel", "no_piggyback", "no_occ_role")
SPLIT_DEFAULTS = dict(frozen_mid_pct=100, dead_tile_pct=12)
_cache = {}


def assert_gradients(out, what):
    """filtered rays (no ReLU input within 2e-5 of zero): strictly within 1e-4 of the fp32 oracle, no escape.  All rays: within 1e-2,
    and within 1e-4 or within 2x of the fp32 oracle's own distance to the fp64 oracle.  A ReLU input within rounding of zero falls
    on either side of the kink and switches one unit of one sample; the fp32 oracle differs from the fp64 one by such flips
    (2e-4 .. 1e-3 of a gradient in these scenes), and the HIP path has proportionally more of them: its sin/cos is accurate to
    1.4e-7 absolute (library sinf: 0.5 ulp), which puts its pre-activations ~1e-6 from the fp64 ones instead of ~3e-7."""
    kept = out.pop("_kept")
    for k, (got, ref, ref64) in out.items():
        e, e64, eo = rel_l2(got, ref), rel_l2(got, ref64), rel_l2(ref, ref64)
        msg = "%s %s (%.0f %% of the rays): hip-vs-f32 %.2e hip-vs-f64 %.2e f32-vs-f64 %.2e" % (what, k, 100 * kept, e, e64, eo)
        if what == "filtered":
            assert e < TOL, msg
        else:
            assert e < 100 * TOL and (e < TOL or e64 < 2 * eo + TOL), msg


def scene():
    """the parity tests' scene (tests/test_gpu_parity.py::_scene: seed 3, grid_std 0.3, bias_std 0.1)"""
    if "sc" not in _cache:
        _cache["sc"] = scenes.make_scene(3, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    return _cache["sc"]


def batch(tiles):
    key = ("rays", tiles)
    if key not in _cache:
        n, S = SIZES[tiles][0], SIZES[tiles][1] + SIZES[tiles][2]
        # make_rays gives n // n_frames rays per camera: 333 = 3 x 111, 17 and 1 from one camera
        _cache[key] = scenes.make_rays(4, n, scene()["bound"], n_frames=3 if n % 3 == 0 else 1, zero_frac=0.1 if n > 1 else 0.0)
        assert _cache[key]["rays_o"].shape[0] == n and (n * S + 15) // 16 == tiles, (n, S, tiles)
    return _cache[key]


def opts_of(tiles):
    return dict(n_samples=SIZES[tiles][1], n_surface=SIZES[tiles][2])


def tune(ctx, knobs):
    """every split key back to its default, then `knobs`"""
    for k in SPLIT_KEYS:
        ctx.set_tuning(k, dict(knobs).get(k, SPLIT_DEFAULTS.get(k, 0)))


def signature(split):
    """what two launches must differ in to count as differently split"""
    return (split["form"], split["which"], split["wgs"])


def forward_reference(oracle32, stage, tiles):
    key = ("fwd", stage, tiles)
    if key not in _cache:
        sc, r = scene(), batch(tiles)
        _cache[key] = oracle32.render_forward(oracle32.opts(sc["bound"], **opts_of(tiles)), sc["grids"], sc["decoders"], stage, r["rays_o"], r["rays_d"], r["gt_depth"])
    return _cache[key]


def backward_reference(oracle32, oracle64, stage, tiles, filtered):
    """upstream gradients (zero on the rays the fragility filter drops when `filtered`) and the fp32 / fp64 oracle's gradients of everything"""
    key = ("bwd", stage, tiles, filtered)
    if key not in _cache:
        sc, r = scene(), batch(tiles)
        N = r["rays_o"].shape[0]
        rng = np.random.default_rng(5)
        g_rgb, g_d, g_v = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
        keep = np.ones(N, bool)
        if filtered:
            frag = oracle64.ray_fragility(oracle64.opts(sc["bound"], **opts_of(tiles)), sc["grids"], sc["decoders"], stage, r["rays_o"], r["rays_d"], r["gt_depth"])
            keep = frag > 2e-5
            assert keep.mean() > 0.5
        g_rgb[~keep] = 0; g_d[~keep] = 0; g_v[~keep] = 0
        refs = [o.render_backward(o.opts(sc["bound"], **opts_of(tiles)), sc["grids"], sc["decoders"], stage, r["rays_o"], r["rays_d"], r["gt_depth"], -1.0, g_rgb, g_d, g_v)
                for o in (oracle32, oracle64)]
        _cache[key] = dict(up=(g_rgb, g_d, g_v), ref=refs[0], ref64=refs[1], kept=float(keep.mean()))
    return _cache[key]


def run_backward(R, stage, tiles, trainable, flags, knobs, backward_mode=2):
    """nsk_render_backward under `knobs` -> (the dict assert_gradients takes, the launch's split)"""
    sc, r = scene(), batch(tiles)
    ctx = make_ctx(sc, trainable=trainable, **opts_of(tiles))
    tune(ctx, knobs)
    ctx.set_backward_mode(backward_mode)
    g_rgb, g_d, g_v = R["up"]
    g_ro, g_rd = ctx.render_backward(stage, cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), -1.0, cu(g_rgb), cu(g_d), cu(g_v), flags=flags)
    ctx.sync()
    out = {}
    if flags & 1:
        for k in stage_levels(stage):
            out["grid_" + k] = (ctx.grid_download(k, grad=True), R["ref"]["g_grids"][k], R["ref64"]["g_grids"][k])
    if flags & 2:
        for k in trainable:
            out["dec_" + k] = (ctx.decoder_download(k, grad=True), R["ref"]["g_decoders"][k], R["ref64"]["g_decoders"][k])
    if flags & 4:
        out["rays_o"] = (g_ro.cpu().numpy(), R["ref"]["g_rays_o"], R["ref64"]["g_rays_o"])
        out["rays_d"] = (g_rd.cpu().numpy(), R["ref"]["g_rays_d"], R["ref64"]["g_rays_d"])
    out["_kept"] = R["kept"]
    split = ctx.debug_last_split(backward=True)
    ctx.close()
    return out, split


def worst(out):
    """the largest hip-vs-f32 error of a run_backward result (for the report printed beside the split)"""
    return max(rel_l2(v[0], v[1]) for k, v in out.items() if k != "_kept")

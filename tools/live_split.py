"""What the dead-tile skip does to a workload's backward, on the GPU: the tiles the frozen roles ran (nsk_debug_live_tiles, to be compared with
tools/live_tiles.py), the workgroup split the launch chose and the launch's time, with the skip, without it (no_dead_skip), and -- `cost` --
with every tile dead against every tile live, which is what a skipped tile costs in the split (nsk_set_tuning "dead_tile_pct"; the split
itself is csrc/nsk_split.h, and tests/test_split_cpu.py shows what it gives for a tile count without a GPU).
usage: [NSK_LIB=<lib>] python tools/live_split.py [K3 K3:fine K2 K4 cost]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bench                      # noqa: E402
import nice_slam_cpp_amd as pkg   # noqa: E402
import scenes                     # noqa: E402


def run(name, stage, tune, masks="frustum", steps=40):
    wl = bench.workloads()[name]
    cam, N = wl["cam"], wl["rays"]
    sc = scenes.make_scene(42, scenes.grid_shapes_for(wl["bound"]), bound=wl["bound"])
    pool = [scenes.make_rays(1234 + 17 * i, N, sc["bound"], n_frames=5, cam_seed=4242, up=wl["up"], **cam) for i in range(4)]
    ctx = pkg.Context(0)
    for k, v in tune.items():
        ctx.set_tuning(k, v)
    ctx.set_render_opts()
    ctx.load_scene(sc["bound"], sc["grids"], sc["decoders"])
    cu = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda").contiguous()
    if masks == "frustum":
        c2w = pool[0]["c2w"][-1]
        depth = cu(scenes.frame_depth_image(sc["bound"], c2w, **cam))
        for k in ("coarse", "middle", "fine", "color"):
            ctx.frustum_mask(k, depth, (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), c2w)
    else:
        for k in ("middle", "fine", "color"):
            ctx.set_mask(k, np.full(sc["grids"][k].shape[1:], masks == "ones"))
    ctx.decoder_set_trainable("color", stage == "color")
    flags = 3 if stage == "color" else 1
    b = [(cu(r["rays_o"]), cu(r["rays_d"]), cu(r["gt_depth"]), cu(r["gt_color"]), float(r["gt_depth"].max())) for r in pool]
    loss = torch.zeros(1, device="cuda")
    with torch.cuda.stream(ctx.tstream):
        for i in range(steps):
            if i == steps // 2:
                ctx.profile_begin()
            n = b[(i + 1) % 4]
            ctx.map_prepare(stage, n[0], n[1], n[2], n[4], flags=flags)
            c = b[i % 4]
            ctx.map_step(stage, c[0], c[1], c[2], c[3], c[4], 0.5, stage == "color", flags=flags, loss=loss)
            ctx.adam_step(bench.STAGE_LR[stage])
        prof = ctx.profile_end()
    counts, _, _ = ctx.debug_live_tiles(N * 48)
    ctx.close()
    launches, ms = prof["decode_bwd_multi"]
    return counts, 1e3 * ms / launches


if __name__ == "__main__":
    for w in (sys.argv[1:] or ["K3", "K3:fine", "K2", "K4", "cost"]):
        if w == "cost":
            (c0, t0), (c1, t1) = run("K3", "fine", {}, "zeros"), run("K3", "fine", {}, "ones")
            print("K3 fine stage, every tile dead %.2f us (ran %s), every tile live %.2f us (ran %s): a dead tile costs %.1f %% of a live one, the launch's fixed part included"
                  % (t0, c0[:2].tolist(), t1, c1[:2].tolist(), 100 * t0 / t1))
            continue
        name, stage = (w.split(":") + ["color"])[:2]
        for label, tune in (("skip", {}), ("no_dead_skip", {"no_dead_skip": 1})):
            c, t = run(name, stage, tune)
            print("%s %s %-12s backward %.2f us; tiles %d, ran middle/fine/colour %s (share %s); workgroups middle/fine/colour %s"
                  % (name, stage, label, t, c[7], c[:3].tolist(), ["%.3f" % (x / c[7]) if x >= 0 else "-" for x in c[:3]], c[4:7].tolist()))

"""How much of the frozen roles' backward the optimiser mask makes dead, on the CPU: for the bench's K2 / K3 / K4-shard batches, the fraction of
marked voxels, of samples with a marked corner, and of 16-sample tiles (cell order) with such a sample, per level.  The GPU's tile counters
(nsk_debug_live_tiles) are to be compared against the last column.  Needs no GPU:  python tools/live_tiles.py [K2 K3 K4]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bench            # noqa: E402  (the workloads' bounds, cameras and ray counts)
import live_tiles as lt  # noqa: E402
import scenes            # noqa: E402
from oracle.nso import Oracle  # noqa: E402


def table(name, n_rays=None):
    wl = bench.workloads()[name]
    cam = wl["cam"]
    N = n_rays or (1250 if name == "K4" else wl["rays"])
    sc = scenes.make_scene(42, scenes.grid_shapes_for(wl["bound"]), bound=wl["bound"])
    r = scenes.make_rays(1234, N, sc["bound"], n_frames=5, cam_seed=4242, up=wl["up"], **cam)
    o = Oracle("f32")
    depth = scenes.frame_depth_image(sc["bound"], r["c2w"][-1], **cam)
    intr = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    shapes = {k: sc["grids"][k].shape[1:] for k in ("middle", "fine", "color")}
    masks = {k: np.asarray(o.frustum_mask(sc["bound"], shapes[k], depth, intr, r["c2w"][-1])).astype(bool) for k in shapes}
    z = o.render_forward(o.opts(sc["bound"]), sc["grids"], sc["decoders"], "color", r["rays_o"], r["rays_d"], r["gt_depth"], want_aux=True)["z"]
    pts = lt.sample_points(r["rays_o"], r["rays_d"], z)
    b = lt.sample_bytes(sc["bound"], shapes, masks, pts)
    order = lt.cell_order(sc["bound"], shapes["color"], shapes["middle"], pts)
    ntiles = (len(b) + 15) // 16
    print("%s: %d rays x %d samples, %d tiles" % (name, N, z.shape[1], ntiles))
    for k in ("middle", "fine"):
        bit = lt.LEVEL_BIT[k]
        print("  %-6s mask fraction %.3f   live samples %.3f   live 16-tiles %.3f (%d)" %
              (k, masks[k].mean(), ((b & bit) != 0).mean(), lt.live_tiles(b[order], bit) / ntiles, lt.live_tiles(b[order], bit)))


if __name__ == "__main__":
    for w in (sys.argv[1:] or ["K2", "K3", "K4"]):
        table(w)

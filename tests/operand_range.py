"""Helpers of the operand-range tests (tests/test_operand_range_cpu.py, tests/test_gpu_operand_range.py): function-preserving power-of-two
transforms that move the MAGNITUDE of a decoder's hidden values, weights or grid features without changing what the network computes, and
scenes with non-finite values in the map.  No GPU needed here.

  rebalance       a factor 2^a across one block of a packed decoder: the block's own layers times 2^a, its consumer's columns times 2^-a
  scale_features  a level's grid times 2^a, the fc columns (coarse: input columns) that read it times 2^-a
Both are exact in floating point as long as nothing under- or overflows: ReLU is positively homogeneous and the factors are powers of two,
so every sum the decoder forms is the unscaled sum times a power of two, rounding included (tests/test_operand_range_cpu.py proves it
against the fp32 and fp64 oracles, which also proves the packing offsets used here)."""
import numpy as np
import torch

import scenes
from oracle import torch_ref as T

DECODERS_OF = {"coarse": ["coarse"], "middle": ["middle"], "fine": ["middle", "fine"], "color": ["middle", "fine", "color"]}
F16_MAX = 65504.0
W_LIMIT = 15                        # every weight of a transformed decoder stays below 2^15 in magnitude
TARGETS = (-14, -8, 0, 8, 14)       # log2 of the peak hidden values the in-range tests aim for
POISON_BITS = {"+inf": 0x7f800000, "-inf": 0xff800000, "nan+": 0x7fc00000, "nan-": 0xffc00000}


def _view(P, ent):
    o, shp = ent
    return P[o:o + int(np.prod(shp))].reshape(shp)


def rebalance(packed, which, i, a):
    """packed decoder `which` with a factor 2^a moved across block i (0..4): pts_linear[i].{weight,bias} and fc[i].{weight,bias} (the coarse
    decoder has no fc) times 2^a; the consumer's columns that read the block's output times 2^-a -- pts_linear[i+1].weight, for the skip
    layer (i = 2) only its last 32 columns (the input is cat(embedded | c, h)), for i = 4 output_linear.weight.  The block's hidden values
    (ReLU inputs and block output) become exactly 2^a times the original, everything behind the consumer is unchanged."""
    lay = T.decoder_layout(which)
    P = np.array(packed, dtype=np.float32, copy=True)
    up, dn = np.float32(2.0) ** np.float32(a), np.float32(2.0) ** np.float32(-a)
    for key in ("W", "b") + (("Fw", "Fb") if lay["has_xyz"] else ()):
        _view(P, lay[key][i])[...] *= up
    if i == 4:
        _view(P, lay["Wo"])[...] *= dn
    elif i == 2:
        _view(P, lay["W"][3])[:, lay["in_dims"][3] - T.H_DIM:] *= dn
    else:
        _view(P, lay["W"][i + 1])[...] *= dn
    return P


def rebalance_all(packed, which, exps):
    """rebalance with exps[i] on every block i"""
    P = packed
    for i, a in enumerate(exps):
        P = rebalance(P, which, i, int(a))
    return P


def scale_features(grids, decoders, level, a):
    """(grids, decoders) with the grid of `level` times 2^a and every weight column that reads it times 2^-a: fc[*].weight of the level's
    own decoder (middle also: columns 32..63 of the fine decoder's fc, which reads fine || middle features); for the coarse decoder the
    input columns of pts_linear[0] and the first 32 columns of the skip layer pts_linear[3]."""
    up, dn = np.float32(2.0) ** np.float32(a), np.float32(2.0) ** np.float32(-a)
    g = dict(grids)
    g[level] = (np.asarray(grids[level], np.float32) * up).astype(np.float32)
    d = {k: np.array(v, dtype=np.float32, copy=True) for k, v in decoders.items()}
    if level == "coarse":
        lay = T.decoder_layout("coarse")
        _view(d["coarse"], lay["W"][0])[...] *= dn
        _view(d["coarse"], lay["W"][3])[:, :32] *= dn
        return g, d
    readers = {"middle": [("middle", slice(0, 32)), ("fine", slice(32, 64))], "fine": [("fine", slice(0, 32))], "color": [("color", slice(0, 32))]}[level]
    for which, cols in readers:
        lay = T.decoder_layout(which)
        for i in range(5):
            _view(d[which], lay["Fw"][i])[:, cols] *= dn
    return g, d


def max_weight(packed, which):
    """largest magnitude among the decoder's layer parameters (everything but the embedding matrix B, which no transform touches)"""
    lay = T.decoder_layout(which)
    return float(np.abs(packed[lay["W"][0][0]:]).max())


def exponent_window(packed, which, i):
    """(lo, hi): the exponents a for which rebalance(packed, which, i, a) keeps every weight below 2^W_LIMIT in magnitude.  Two-sided: the
    block's own layers grow with a, the consumer's columns grow as a falls."""
    lay = T.decoder_layout(which)
    own = max(float(np.abs(_view(packed, lay[key][i])).max()) for key in ("W", "b") + (("Fw", "Fb") if lay["has_xyz"] else ()))
    if i == 4:
        cons = float(np.abs(_view(packed, lay["Wo"])).max())
    elif i == 2:
        cons = float(np.abs(_view(packed, lay["W"][3])[:, lay["in_dims"][3] - T.H_DIM:]).max())
    else:
        cons = float(np.abs(_view(packed, lay["W"][i + 1])).max())
    hi = int(np.ceil(W_LIMIT - np.log2(own))) - 1            # own * 2^hi < 2^W_LIMIT
    lo = -(int(np.ceil(W_LIMIT - np.log2(cons))) - 1)
    return lo, hi


def exponent_for(peak, target_log2, window=None):
    """the exponent that takes a value of magnitude `peak` nearest to 2^target_log2, clipped to window = (lo, hi)"""
    a = int(np.rint(target_log2 - np.log2(peak)))
    if window is not None:
        a = max(window[0], min(window[1], a))
    return a


def op_scene(seed=61):
    return scenes.make_scene(seed, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)


def op_points(sc, n=300, seed=62):
    """n points over the bound and a margin of 5 % around it (outside: clamped lookup, occupancy 100)"""
    b = sc["bound"]
    rng = np.random.default_rng(seed)
    return (b[:, 0] + (b[:, 1] - b[:, 0]) * rng.uniform(-0.05, 1.05, (n, 3))).astype(np.float32)


def op_rays(sc, n=48, seed=63, zero_frac=0.1):
    return scenes.make_rays(seed, n, sc["bound"], n_frames=2, zero_frac=zero_frac)


def in_range_cases(sc, stage, peaks):
    """The in-range transforms of `stage`: [(label, grids, decoders)] -- every block of every decoder the stage runs, one at a time, with its
    peak hidden value (peaks[which][i], read from the oracle at scale 1) taken near 2^t for t in TARGETS inside the block's weight window;
    all five blocks at once with alternating signs; every level the stage reads with its peak feature taken near 2^t (the fc columns grow as
    the features shrink: the same window)."""
    cases = []
    for which in DECODERS_OF[stage]:
        P = sc["decoders"][which]
        for i in range(5):
            for t in TARGETS:
                a = exponent_for(peaks[which][i], t, exponent_window(P, which, i))
                cases.append(("%s block %d x 2^%d (peak 2^%.1f)" % (which, i, a, np.log2(peaks[which][i]) + a), sc["grids"], dict(sc["decoders"], **{which: rebalance(P, which, i, a)})))
        for m in (4, 7, -4, -7):
            # all five blocks at once, alternating signs: block i + 1's own layer is also block i's consumer and moves by 2^(a[i+1] - a[i]),
            # so |a| stays at 7 (weights of ~0.5 x 2^14)
            exps = [m if i % 2 == 0 else -m for i in range(5)]
            Q = rebalance_all(P, which, exps)
            assert max_weight(Q, which) < 2.0 ** W_LIMIT
            cases.append(("%s all blocks x 2^%s" % (which, exps), sc["grids"], dict(sc["decoders"], **{which: Q})))
    for level in DECODERS_OF[stage]:
        peak = float(np.abs(sc["grids"][level]).max())
        for t in TARGETS:
            a = exponent_for(peak, t)
            g, d = scale_features(sc["grids"], sc["decoders"], level, a)
            while max(max_weight(d[w], w) for w in DECODERS_OF[stage]) >= 2.0 ** W_LIMIT:      # the fc columns grow as the features shrink
                a += 1
                g, d = scale_features(sc["grids"], sc["decoders"], level, a)
            cases.append(("%s features x 2^%d (peak 2^%.1f)" % (level, a, np.log2(peak) + a), g, d))
    return cases


# ---- non-finites in the map ---------------------------------------------------------------------------------------------------------
def poison_value(name):
    """the float32 with exactly the bits POISON_BITS[name] (the two NaNs differ in the sign bit only)"""
    return np.array([POISON_BITS[name]], np.uint32).view(np.float32)[0]


def poison_voxel(grids, level, zyx, name, channels=None):
    """grids with voxel zyx of `level` set to the poison value in all 32 channels (channels=None) or in the listed ones"""
    g = dict(grids)
    v = np.array(grids[level], dtype=np.float32, copy=True)
    bits = v.view(np.uint32)
    z, y, x = zyx
    if channels is None:
        bits[:, z, y, x] = POISON_BITS[name]
    else:
        bits[list(channels), z, y, x] = POISON_BITS[name]
    g[level] = v
    return g


def central_voxel(sc, level):
    _, Z, Y, X = sc["grids"][level].shape
    return (Z // 2, Y // 2, X // 2)


def torch_scene(sc, grids=None, decoders=None):
    return (torch.tensor(np.asarray(sc["bound"], np.float32)), {k: torch.tensor(np.array(v, np.float32)[None].copy()) for k, v in (grids or sc["grids"]).items()},
            {k: torch.tensor(np.array(v, np.float32).copy()) for k, v in (decoders or sc["decoders"]).items()})


def aten_eval_points(sc, stage, pts, grids=None, decoders=None):
    """Renderer::eval_points on ATen-CPU (oracle/torch_ref.py: F.grid_sample, F.linear, torch.relu -- the ops the reference calls): raw [M, 4]"""
    bound, g, d = torch_scene(sc, grids, decoders)
    with torch.no_grad():
        return T.eval_points(torch.tensor(np.asarray(pts, np.float32)), stage, d, g, bound).numpy()


def aten_map_step(sc, stage, rays, trainable, w_color, use_color, gt_depth_max, grids=None):
    """one Mapper iteration (render_batch_ray, loss_map, autograd) on ATen-CPU: loss, d loss / d grids of the stage's levels ([C,Z,Y,X]) and
    d loss / d packed parameters of the trainable decoders"""
    bound, g, d = torch_scene(sc, grids)
    levels = DECODERS_OF[stage]
    for k in levels:
        g[k].requires_grad_(True)
    for k in trainable:
        d[k].requires_grad_(True)
    ro, rd, gd, gc = (torch.tensor(rays[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color"))
    rgb, depth, var, _ = T.render_batch_ray(g, d, rd, ro, stage, gd, bound, gt_depth_max=gt_depth_max)
    loss = T.loss_map(depth, rgb, gd, gc, w_color, use_color)
    loss.backward()
    return dict(loss=float(loss.detach()), depth=depth.detach().numpy(), rgb=rgb.detach().numpy(),
                g_grids={k: g[k].grad[0].numpy().copy() for k in levels}, g_decoders={k: d[k].grad.numpy().copy() for k in trainable})


def voxel_rows_finite(g):
    """[Z,Y,X] bool: every channel of the voxel's gradient row is finite (g [C,Z,Y,X])"""
    return np.isfinite(g).all(axis=0)

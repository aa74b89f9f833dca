"""Scenes built at the geometric edges of the render (pure numpy, like scenes.py): rays with exact zero direction components, samples on
voxel planes, origins on / outside the bound, rays that miss it, levels one or two voxels thick, every sample in one cell, samples spread over
as many cells as possible.  scenes.make_rays produces none of these: its camera sits well inside a generic room and looks in a generic direction.

Every scene is a dict: name, sc (bound, grids, decoders as scenes.make_scene), rays (rays_o, rays_d, gt_depth, gt_color), stages (the
stages it is meant for), made_nonfinite (bool [N]: the rays CONSTRUCTED to come out non-finite: an origin on the upper x face with a zero x
direction gives 0/0 in the box exit, see include/nsk.h), n_samples / n_surface.
"""
import numpy as np

import scenes

LATTICE_BOUND = np.array([[0.0, 8.0], [0.0, 4.0], [0.0, 8.0]], np.float32)
LATTICE_SHAPE = (32, 9, 5, 9)                          # [C, Z, Y, X]: pitch exactly 1 along every axis


def _pack(name, sc, ro, rd, gt, stages, made_nonfinite=None, n_samples=32, n_surface=16):
    ro, rd, gt = np.asarray(ro, np.float64), np.asarray(rd, np.float64), np.asarray(gt, np.float64)
    hit = ro + rd * gt[:, None]
    color = 0.5 + 0.5 * np.sin(hit * np.array([1.3, 2.1, 0.7]) + np.array([0.0, 1.0, 2.0]))
    c32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    rays = dict(rays_o=c32(ro), rays_d=c32(rd), gt_depth=c32(gt), gt_color=c32(color))
    mn = np.zeros(len(gt), bool) if made_nonfinite is None else np.asarray(made_nonfinite, bool)
    return dict(name=name, sc=sc, rays=rays, stages=stages, made_nonfinite=mn, n_samples=n_samples, n_surface=n_surface)


def _scene(seed, shapes, bound, grid_std=0.3, bias_std=0.1, occ_bias=0.1, occ_scale=0.1):
    """seeded grids and decoders.  The occupancy decoders' output layer is scaled down and its bias raised: sigma stays small and mostly positive,
    so that relu(sigma) is on along most of a ray, every sample that touches a voxel also sends a gradient there (the coverage assertions need
    it), and no ray saturates: behind a transmittance of 1e-20 the compositing's 1 - alpha + 1e-10 cancels and the fp32 REFERENCE itself loses
    ten percent of a gradient that only such samples feed (measured: kappa_ref 0.1 at one corner voxel), which would hand the GPU a limit
    that judges nothing"""
    sc = scenes.make_scene(seed, shapes, bound=bound, grid_std=grid_std, bias_std=bias_std)
    for k in ("coarse", "middle", "fine"):
        sc["decoders"][k][-33:] *= np.float32(occ_scale)         # output_linear: 32 weights + 1 bias
        sc["decoders"][k][-1] += np.float32(occ_bias)
    return sc


def _exit(bound, ro, rd):
    return scenes._ray_box_far(np.asarray(bound, np.float64), np.asarray(ro, np.float64), np.asarray(rd, np.float64))


def position_in_grid(idx_zyx, shape_zyx):
    """interior / face / edge / corner of a voxel index"""
    n = sum(int(i == 0 or i == s - 1) for i, s in zip(idx_zyx, shape_zyx) if s > 1)
    return ("interior", "face", "edge", "corner")[min(n, 3)]


def border_voxels(shape_zyx):
    """bool [Z,Y,X]: voxels on a face, an edge or a corner"""
    m = np.zeros(shape_zyx, bool)
    for ax, s in enumerate(shape_zyx):
        sl = [slice(None)] * 3
        sl[ax] = 0; m[tuple(sl)] = True
        sl[ax] = s - 1; m[tuple(sl)] = True
    return m


def lattice_coordinates_fp32(bound, dims_xyz, p):
    """tri_setup's normalise -> unnormalise chain in numpy fp32 (utils.h:135-137, GridSampler.h:31), unclipped: [M,3] grid coordinates"""
    b = np.asarray(bound, np.float32)
    p = np.asarray(p, np.float32)
    out = np.zeros_like(p)
    for k in range(3):
        lo, hi = b[k, 0], b[k, 1]
        u = ((p[:, k] - lo) / (hi - lo)) * np.float32(2) - np.float32(1)
        out[:, k] = ((u + np.float32(1)) / np.float32(2)) * np.float32(dims_xyz[k] - 1)
    return out


def lattice(seed=301):
    """Bound [0,8] x [0,4] x [0,8], 9 x 5 x 9 voxels on every level: the grid coordinate of a world point is the point itself, so a sample
    at an integer world coordinate sits exactly on a voxel plane.  Rays:
      axis     along +-x, +-y, +-z (two zero components) and the twelve in-plane diagonals (one zero component) from origins on lattice
               points, on lattice lines and at half pitch; gt depth puts the surface samples (0.95 gt .. 1.05 gt) across a voxel plane
      face     running INSIDE the faces x = 0, x = 8 and y = 4 (origin on the face, zero component across it) and along the twelve edges
      cover    one ray towards every border voxel (aimed a quarter pitch inside it, gt depth at the aim point), so that every face, edge and
               corner voxel of every level receives gradient"""
    shapes = {k: LATTICE_SHAPE for k in scenes.LEVELS}
    sc = _scene(seed, shapes, LATTICE_BOUND)
    ro, rd, gt, made = [], [], [], []
    axis = [np.eye(3)[k] * s for k in range(3) for s in (1.0, -1.0)]
    diag = []
    for a in range(3):
        for b in range(a + 1, 3):
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    d = np.zeros(3); d[a] = sa; d[b] = sb
                    diag.append(d)
    origins = [(2.0, 1.0, 3.0), (5.0, 2.0, 6.0),            # lattice points
               (2.5, 1.0, 3.0), (4.0, 2.5, 5.0),            # lattice lines
               (2.5, 1.5, 3.5), (5.5, 2.5, 4.5)]            # half pitch
    def add(o, d, nonfinite=False):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        with np.errstate(all="ignore"):
            ex = _exit(LATTICE_BOUND, o[None], d[None])[0]
        if not np.isfinite(ex):
            ex = 3.0
        k = int(np.flatnonzero(d != 0)[0])                   # first moving axis: the surface samples must straddle one of ITS planes
        g = max(1.0, np.floor(0.6 * ex))
        if (o[k] * 2) % 2 == 1:                              # half-integer start: half-integer distance reaches a plane
            g -= 0.5
        ro.append(o); rd.append(d); gt.append(g); made.append(nonfinite)
    for o in origins:
        for d in axis + diag:
            add(o, d)
    # inside the faces x = 0, x = 8, y = 4: axis-aligned and diagonal; (o_x = 8 with d_x = 0: (0 - 8) / 0 = -inf against 0 / 0 = NaN, see nsk.h)
    for (o, ds, bad) in (((0.0, 1.5, 2.5), [(0, 1, 0), (0, 0, -1), (0, 1, 1)], False),
                         ((8.0, 2.0, 5.5), [(0, -1, 0), (0, 0, 1)], True),
                         ((3.5, 4.0, 2.0), [(1, 0, 0), (0, 0, 1), (-1, 0, 1)], False)):
        for d in ds:
            add(o, d, bad)
    for a in range(3):                                       # the twelve edges: along axis a, the other two coordinates on faces
        b, c = [k for k in range(3) if k != a]
        for fb in (0, 1):
            for fc in (0, 1):
                o = np.zeros(3); o[a] = 1.5; o[b] = LATTICE_BOUND[b, fb]; o[c] = LATTICE_BOUND[c, fc]
                d = np.zeros(3); d[a] = 1.0
                add(o, d, nonfinite=bool(a != 0 and o[0] == 8.0))
    # coverage rays: from one half-pitch origin to a quarter pitch inside every border voxel
    Z, Y, X = LATTICE_SHAPE[1:]
    o = np.array([4.5, 2.5, 3.5])
    for iz, iy, ix in np.argwhere(border_voxels((Z, Y, X))):
        tgt = np.array([np.clip(ix, 0.25, X - 1.25), np.clip(iy, 0.25, Y - 1.25), np.clip(iz, 0.25, Z - 1.25)])
        ro.append(o); rd.append(tgt - o); gt.append(1.0); made.append(False)
    return _pack("lattice", sc, ro, rd, gt, ("middle", "fine", "color"), made)


def outside_and_on_bound(seed=302):
    """Small grids in the reference's bound.  Rays:
      outside  origins 0.5 m outside each of the six faces looking in (axis-aligned and oblique): the samples before entry are clamped and
               masked (occ = 100, Renderer.cpp:36)
      on-face  origins exactly on each face: looking in obliquely, and axis-aligned INSIDE the face (0/0 in the box exit)
      miss     origins outside, looking away or past the bound: far < 0, clamped to 0 with ground truth
      beyond   ground truth 1.3 x the box exit (what the inside filter drops)"""
    b = scenes.REF_BOUND.astype(np.float64)
    sc = _scene(seed, scenes.SMALL_GRID_SHAPES, scenes.REF_BOUND)
    ctr = b.mean(axis=1)
    ext = b[:, 1] - b[:, 0]
    rng = np.random.default_rng(seed)
    ro, rd, gt, made = [], [], [], []
    for k in range(3):
        for side in (0, 1):
            inward = np.zeros(3); inward[k] = 1.0 if side == 0 else -1.0
            for rep in range(12):
                o = ctr + rng.uniform(-0.3, 0.3, 3) * ext
                o[k] = b[k, side] - 0.5 * inward[k]                              # 0.5 m outside
                d = inward.copy() if rep < 3 else inward + rng.uniform(-0.4, 0.4, 3) * (np.arange(3) != k)
                ex = _exit(b, o[None], d[None])[0]
                ro.append(o); rd.append(d); gt.append(0.0 if rep == 3 else (0.5 + 0.5 * rng.uniform(0.2, 0.9) * (ex - 0.5))); made.append(False)
            for rep in range(8):
                o = ctr + rng.uniform(-0.3, 0.3, 3) * ext
                o[k] = b[k, side]                                                # exactly on the face (the bound's own fp32 value)
                if rep < 6:
                    d = inward + rng.uniform(-0.4, 0.4, 3) * (np.arange(3) != k)
                    bad = False
                else:                                                            # axis-aligned inside the face
                    d = np.zeros(3); d[(k + 1 + rep % 2) % 3] = 1.0 if rep % 2 else -1.0
                    bad = bool(k == 0 and side == 1)
                with np.errstate(all="ignore"):
                    ex = _exit(b, o[None], d[None])[0]
                ro.append(o); rd.append(d); gt.append(0.6 * ex if np.isfinite(ex) and ex > 0 else 1.0); made.append(bad)
            for rep in range(4):                                                 # misses: outside, looking away / sideways past the bound
                o = ctr + rng.uniform(-0.3, 0.3, 3) * ext
                o[k] = b[k, side] - 0.5 * inward[k]
                d = -inward + rng.uniform(-0.3, 0.3, 3) * (np.arange(3) != k) if rep < 2 else np.roll(inward, 1) + 0.05 * -inward
                ro.append(o); rd.append(d); gt.append(1.0 + rep); made.append(False)
    for rep in range(24):                                                        # inside, ground truth beyond the exit
        o = ctr + rng.uniform(-0.3, 0.3, 3) * ext
        d = rng.standard_normal(3)
        ex = _exit(b, o[None], d[None])[0]
        ro.append(o); rd.append(d); gt.append(1.3 * ex); made.append(False)
    # the on-face coordinates must be the fp32 bound's own values: go through float32 once
    ro = np.asarray(ro)
    for k in range(3):
        for side in (0, 1):
            on = ro[:, k] == b[k, side]
            ro[on, k] = np.float64(scenes.REF_BOUND[k, side])
    return _pack("outside-on-bound", sc, ro, rd, gt, ("middle", "fine", "color"), made)


def misses_without_gt(seed=306):
    """rays that miss the bound, rendered WITHOUT ground truth depth (Renderer.cpp:54-57: no surface samples, far not clamped): origins 0.5 m
    outside each face looking away or sideways past the bound, so far < 0 and z descends from 0.01 to far; plus eight ordinary rays from inside.
    Returns (sc, rays_o, rays_d) float32"""
    b = scenes.REF_BOUND.astype(np.float64)
    sc = _scene(seed, scenes.SMALL_GRID_SHAPES, scenes.REF_BOUND)
    ctr, ext = b.mean(axis=1), b[:, 1] - b[:, 0]
    rng = np.random.default_rng(seed)
    ro, rd = [], []
    for k in range(3):
        for side in (0, 1):
            inward = np.zeros(3); inward[k] = 1.0 if side == 0 else -1.0
            for rep in range(4):
                o = ctr + rng.uniform(-0.3, 0.3, 3) * ext
                o[k] = b[k, side] - 0.5 * inward[k]
                d = -inward + rng.uniform(-0.3, 0.3, 3) * (np.arange(3) != k) if rep < 2 else np.roll(inward, 1) + 0.05 * -inward
                ro.append(o); rd.append(d)
    for rep in range(8):
        ro.append(ctr + rng.uniform(-0.3, 0.3, 3) * ext); rd.append(rng.standard_normal(3))
    return sc, np.asarray(ro, np.float32), np.asarray(rd, np.float32)


THIN_SHAPES = {"coarse": (32, 1, 2, 3), "middle": (32, 1, 5, 7), "fine": (32, 2, 2, 2), "color": (32, 2, 1, 4)}


def thin_grids(seed=303):
    """Levels with a dimension of 2 and of 1 (scenes.grid_shapes_for of a flat bound gives such a coarse level): align_corners scales a
    1-voxel axis by dim - 1 = 0, every sample reads voxel 0 there with weight 1 and no spatial gradient"""
    bound = np.array([[-1.0, 3.0], [0.0, 2.5], [-0.4, 0.4]], np.float32)
    sc = _scene(seed, THIN_SHAPES, bound)
    r = scenes.make_rays(seed, 192, bound, n_frames=2, shrink=0.05, up="z", zero_frac=0.05)
    s = _pack("thin-grids", sc, r["rays_o"], r["rays_d"], r["gt_depth"], ("coarse", "middle", "fine", "color"))
    s["rays"]["gt_color"] = r["gt_color"]
    return s


ONE_CELL_SHAPES = {"coarse": (32, 2, 2, 2), "middle": (32, 2, 2, 2), "fine": (32, 2, 2, 2), "color": (32, 2, 2, 2)}


def one_cell(n=4096, seed=304):
    """every level 2 x 2 x 2: every sample of every tile lies in the one cell there is (one run per tile, one key in k_sample's table)"""
    bound = np.array([[-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0]], np.float32)
    sc = _scene(seed, ONE_CELL_SHAPES, bound)
    r = scenes.make_rays(seed, n, bound, n_frames=4, shrink=0.1, zero_frac=0.02)
    s = _pack("one-cell", sc, r["rays_o"], r["rays_d"], r["gt_depth"], ("fine", "color"))
    s["rays"]["gt_color"] = r["gt_color"]
    return s


SPREAD_SHAPES = {"coarse": (32, 3, 2, 4), "middle": (32, 16, 16, 16), "fine": (32, 64, 64, 64), "color": (32, 64, 64, 64)}


def max_spread(n=256, seed=305):
    """a 64^3 fine level and rays fanned from a corner over the whole bound: the 8 rays x 48 samples of a k_sample workgroup fall into
    well over 300 distinct cells (distinct_cells_per_group counts them), so its cell table probes and every thread makes its one add"""
    bound = np.array([[-2.0, 2.0], [-2.0, 2.0], [-2.0, 2.0]], np.float32)
    rng = np.random.default_rng(seed)
    sc = scenes.make_scene(seed, {k: SPREAD_SHAPES[k] if k != "color" else (32, 2, 2, 2) for k in scenes.LEVELS}, bound=bound, grid_std=0.3, bias_std=0.1)
    for k in ("middle", "fine"):
        sc["decoders"][k][-33:] *= np.float32(0.1)
        sc["decoders"][k][-1] += np.float32(0.1)
    d = np.abs(rng.standard_normal((n, 3))) + 0.3                               # fanned over the octant the bound lies in, seen from its corner:
    d /= np.linalg.norm(d, axis=1, keepdims=True)                               # every ray is 4 .. 6.9 m long, its samples further apart than a cell
    o = -1.9 + rng.uniform(-0.05, 0.05, (n, 3))
    ex = _exit(bound, o, d)
    # seven rays of eight without ground truth depth: their 16 "surface" samples are spread from 0.001 to max(gt) (Renderer.cpp:94-98) instead of
    # bunched in the three cells around a surface, so a ray's 48 samples fall into ~42 cells
    return _pack("max-spread", sc, o, d, np.where(np.arange(n) % 8 == 0, 0.9 * ex, 0.0), ("fine",))


def distinct_cells_per_group(bound, dims_xyz, z, rays_o, rays_d, group=8):
    """number of distinct cells of a level that the samples z [N,S] of each block of `group` consecutive rays fall into"""
    p = rays_o[:, None, :].astype(np.float64) + rays_d[:, None, :] * z[:, :, None]
    b = np.asarray(bound, np.float64)
    idx = []
    for k in range(3):
        x = (p[..., k] - b[k, 0]) / (b[k, 1] - b[k, 0]) * (dims_xyz[k] - 1)
        idx.append(np.clip(np.floor(np.clip(x, 0, dims_xyz[k] - 1)), 0, dims_xyz[k] - 1).astype(np.int64))
    cell = (idx[2] * dims_xyz[1] + idx[1]) * dims_xyz[0] + idx[0]
    return [len(np.unique(cell[i:i + group])) for i in range(0, cell.shape[0], group)]


def principal_point(H=480, W=640, fx=517.0, fy=516.0, cx=320.0, cy=240.0):
    """pixels on the principal-point row j = cy and column i = cx of an identity-pose camera with integer cx, cy (TUM-like intrinsics
    rounded): the camera-frame directions ((i - cx) / fx, -(j - cy) / fy, -1) hold exact zeros there.  Returns (pix_i, pix_j, intr, c2w [4,4])"""
    col = np.arange(40, H - 40, 4)
    row = np.arange(40, W - 40, 4)
    pix_i = np.concatenate([np.full(len(col), int(cx)), row]).astype(np.int32)
    pix_j = np.concatenate([col, np.full(len(row), int(cy))]).astype(np.int32)
    return pix_i, pix_j, (fx, fy, cx, cy), np.eye(4, dtype=np.float32)

"""What the depth fusion (nsk_tsdf_integrate, nsk_tsdf_volume) must give, in pure numpy: nothing here is imported from the product.
Conventions restated from include/nsk.h: the lattice, the camera and the "frame k sees node p" rule are those of nsk_lattice_seen
(mesh_cull_checks.seen_f32); a frame that sees the node updates it, frames in ascending order, every operation one float32 rounding:
  sdf = D - d;   t = min(1, sdf / trunc);   T <- ((W T) + t) / (W + 1);   W <- min(W + 1, max_weight)."""
import numpy as np

import mesh_checks as mc
import mesh_cull_checks as cc

F = np.float32
EPS = cc.EPS


def fuse_f32(pts, depths, intr, w2c, edge, trunc, max_weight=64, state=None):
    """the rule in float32, one numpy operation per fp32 operation.  pts [n, 3] float32, depths [K, H, W] float32, intr = (fx, fy, cx, cy),
    w2c [K, 4, 4] float32; state: (T, W) float32 [n] to continue from (not changed) -> (T, W) float32 [n]"""
    K = depths.shape[0]
    w = np.asarray(w2c, F).reshape(K, 16)
    trunc, max_weight = F(trunc), F(max_weight)
    if state is None:
        T, Wt = np.zeros(len(pts), F), np.zeros(len(pts), F)
    else:
        T, Wt = np.array(state[0], F).reshape(-1), np.array(state[1], F).reshape(-1)
    with np.errstate(all="ignore"):
        for k in range(K):
            d, fi, fj = cc.project_f32(pts, w[k], intr)
            ok, D = cc.pixel_of(d, fi, fj, depths[k], edge)
            ok &= np.isfinite(D) & (D > 0)
            ok &= d <= (D + trunc).astype(F)
            sdf = (D - d).astype(F)
            t = np.minimum(F(1), (sdf / trunc).astype(F))
            Tn = (((Wt * T).astype(F) + t).astype(F) / (Wt + F(1)).astype(F)).astype(F)
            Wn = np.minimum((Wt + F(1)).astype(F), max_weight)
            T = np.where(ok, Tn, T).astype(F)
            Wt = np.where(ok, Wn, Wt).astype(F)
    return T, Wt


def fuse_f64(pts, depths, intr, w2c, edge, trunc, max_weight=64, state=None):
    """The same on the same float32 inputs in float64 -> (T float64 [n], W float64 [n], bound float64 [n]).

    bound: what float32 can have moved T by at a node where every frame took the same decision and the same pixel in both precisions
    (mesh_cull_checks.seen_f64's margin > 1 says where that is); fuse_f32 must stay within it there.  It follows the node's own operations,
    eps = 2^-24 per rounding, E_x the bound carried for x:
      d = -c_2: as in seen_f64, six roundings below eps S, S = |w8 p0| + |w9 p1| + |w10 p2| + |w11|          ->  E_d = 6 eps S
      sdf = D - d: D is a float32 input, one rounding                                                         ->  E_s = E_d + eps (|sdf| + E_d)
      q = sdf / trunc: trunc is a float32 input, one rounding                                                 ->  E_q = E_s / trunc + eps (|q| + E_s / trunc)
      t = min(1, q): min moves its result no farther than its argument moved                                  ->  E_t = E_q
      a = W T: W is a whole number below 2^24, the same in both; one rounding                                ->  E_a = W E_T + eps W (|T| + E_T)
      b = a + t: one rounding                                                                                 ->  E_b = E_a + E_t + eps (|b| + E_a + E_t)
      T' = b / (W + 1): W + 1 is exact; one rounding                                                          ->  E_T' = E_b / (W + 1) + eps (|T'| + E_b / (W + 1))
    A frame that does not see the node leaves E_T as it is.  state: (T, W) float32 values, taken as exact (E_T = 0)."""
    K = depths.shape[0]
    w = np.asarray(w2c, F).reshape(K, 16)
    trunc, max_weight = float(F(trunc)), float(F(max_weight))
    n = len(pts)
    if state is None:
        T, Wt = np.zeros(n), np.zeros(n)
    else:
        T, Wt = np.array(state[0], np.float64).reshape(-1), np.array(state[1], np.float64).reshape(-1)
    ET = np.zeros(n)
    with np.errstate(all="ignore"):
        for k in range(K):
            d, fi, fj, Ed, _ = cc.project_f64(pts, w[k], intr)
            ok, D = cc.pixel_of(d, fi, fj, depths[k], edge)
            ok &= np.isfinite(D) & (D > 0)
            ok &= d <= D + trunc
            sdf = D - d
            Es = Ed + EPS * (np.abs(sdf) + Ed)
            q = sdf / trunc
            Et = Es / trunc + EPS * (np.abs(q) + Es / trunc)
            t = np.minimum(1.0, q)
            Ea = Wt * ET + EPS * Wt * (np.abs(T) + ET)
            b = Wt * T + t
            Eb = Ea + Et + EPS * (np.abs(b) + Ea + Et)
            Tn = b / (Wt + 1.0)
            En = Eb / (Wt + 1.0) + EPS * (np.abs(Tn) + Eb / (Wt + 1.0))
            T = np.where(ok, Tn, T)
            ET = np.where(ok, En, ET)
            Wt = np.where(ok, np.minimum(Wt + 1.0, max_weight), Wt)
    return T, Wt, ET


def volume_of(T, Wt, min_weight, shape):
    """nsk_tsdf_volume: (-T where W >= min_weight, NaN elsewhere; valid uint8), shaped [nz, ny, nx], in T's own precision"""
    ok = np.asarray(Wt) >= min_weight
    vol = np.where(ok, -np.asarray(T), np.nan).astype(np.asarray(T).dtype)
    return vol.reshape(shape), ok.astype(np.uint8).reshape(shape)


# ---- the sphere scene ------------------------------------------------------------------------------------------------------------
SPHERE_N = 40
SPHERE_CENTRE, SPHERE_RADIUS = (0.03, -0.02, 0.05), 0.6
SPHERE_H, SPHERE_W = 96, 128
SPHERE_INTR = (150.0, 150.0, 63.5, 47.5)
SPHERE_EYES = (((3.0, 0.21, 0.13), 0.03), ((-3.0, -0.17, 0.22), -0.05), ((0.25, 3.0, 0.31), 0.04), ((-0.19, -3.0, 0.27), -0.02),
               ((0.16, -0.23, 3.0), 0.06), ((0.28, 0.14, -3.0), -0.04), ((1.8, 1.7, 1.75), 0.05), ((-1.75, 1.65, -1.8), -0.03))      # eye, roll


def sphere_depth(c2w, H, W, intr, centre, radius):
    """z-depth [H, W] float32 of a sphere seen by the camera c2w (looking along -z, x right, y up) by analytic ray-sphere intersection at
    the pixel centres, in float64; 0 where the ray misses"""
    fx, fy, cx, cy = [float(x) for x in intr]
    j, i = np.mgrid[0:H, 0:W].astype(np.float64)
    dc = np.stack([(i - cx) / fx, -(j - cy) / fy, -np.ones_like(i)], -1)      # per unit of z-depth: the ray parameter IS the z-depth
    R, o = np.asarray(c2w, np.float64)[:3, :3], np.asarray(c2w, np.float64)[:3, 3]
    dw = dc @ R.T
    oc = o - np.asarray(centre, np.float64)
    A = (dw * dw).sum(-1)
    B = 2.0 * (dw @ oc)
    Cc = oc @ oc - radius * radius
    disc = B * B - 4.0 * A * Cc
    with np.errstate(all="ignore"):
        t = (-B - np.sqrt(disc)) / (2.0 * A)
    return np.where((disc > 0) & (t > 0), t, 0.0).astype(F)


def sphere_scene():
    """a 40^3 lattice over [-1, 1]^3, a sphere of radius 0.6 a little off its centre, eight cameras about 3 m out (six near the axes, two on
    diagonals, small rolls), 96 x 128 depth images, trunc = 3 steps"""
    n = SPHERE_N
    origin = np.full(3, -1.0, F)
    step = np.full(3, F(2.0) / F(n - 1), F)
    c2w = np.stack([cc.look_at(e, SPHERE_CENTRE, r) for e, r in SPHERE_EYES]).astype(F).astype(np.float64)      # poses as a float32 file holds them
    depths = np.stack([sphere_depth(m, SPHERE_H, SPHERE_W, SPHERE_INTR, SPHERE_CENTRE, SPHERE_RADIUS) for m in c2w])
    return dict(origin=origin, step=step, nx=n, ny=n, nz=n, depths=depths, intr=SPHERE_INTR, c2w=c2w, w2c=np.stack([cc.w2c_of(m) for m in c2w]),
                pts=mc.lattice_points(origin, step, n, n, n), trunc=F(3.0) * step.max(), centre=np.array(SPHERE_CENTRE), radius=SPHERE_RADIUS,
                H=SPHERE_H, W=SPHERE_W)


def sphere_distances(verts, sc):
    """| |v - centre| - radius | of every vertex, in steps of the lattice"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    return np.abs(np.linalg.norm(v - sc["centre"], axis=1) - sc["radius"]) / float(sc["step"].max())


def check_sphere_mesh(verts, sc, what):
    """the two caps on a mesh of the sphere scene: mean distance at most half a step, largest at most one cell diagonal"""
    dist = sphere_distances(verts, sc)
    print("%s: %d vertices, distance to the sphere mean %.3f steps, max %.3f steps" % (what, len(dist), dist.mean(), dist.max()))
    assert len(dist) > 1000
    assert dist.mean() <= 0.5 and dist.max() <= np.sqrt(3.0), (dist.mean(), dist.max())
    return dist

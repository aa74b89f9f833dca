"""What the seen mask of a lattice (nsk_lattice_seen) and the component filter of a mesh (nsk_mesh_filter) must give, in pure numpy: nothing here
is imported from the product.  Conventions restated from include/nsk.h:
  node (i, j, k) at origin + (i, j, k) * step in float32 (mesh_checks.lattice_points), mask[k, j, i];
  a camera looks along -z, x to the right, y up; w2c is row-major world-to-camera; pixel (i, j) = (column, row), depth[k][j][i];
  vertices joined by a triangle are connected; a component's label is its smallest vertex index."""
import numpy as np

import mesh_checks as mc

F = np.float32
EPS = 2.0 ** -24            # unit roundoff of float32 (round to nearest)

# classes of one (keyframe, node) pair, decided in float64 in the order the rule decides them
SEEN, BEHIND, LEFT, RIGHT, TOP, BOTTOM, ZERO, NAN, INF, FAR = range(10)
CLASS_NAMES = ("seen", "behind the camera", "left of the image", "right of the image", "above the image", "below the image",
               "zero depth", "NaN depth", "inf depth", "behind depth + trunc")


def project_f32(pts, w_k, intr):
    """camera depth and nearest pixel of the points under one frame, by the rule of include/nsk.h in float32, one numpy operation per fp32
    operation.  pts [n, 3] float32, w_k: the frame's row-major world-to-camera matrix (16 float32), intr = (fx, fy, cx, cy)
    -> (d, fi, fj) float32 [n]: fi, fj are floats, and a NaN among them fails every comparison of the pixel test"""
    pts, w = np.asarray(pts, F), np.asarray(w_k, F).reshape(16)
    fx, fy, cx, cy = [F(x) for x in intr]
    with np.errstate(all="ignore"):
        c = []
        for a in range(3):
            s = (w[4 * a] * pts[:, 0]).astype(F) + (w[4 * a + 1] * pts[:, 1]).astype(F)
            s = s.astype(F) + (w[4 * a + 2] * pts[:, 2]).astype(F)
            c.append((s.astype(F) + w[4 * a + 3]).astype(F))
        d = -c[2]
        u = (cx + ((fx * c[0]).astype(F) / d).astype(F)).astype(F)
        v = (cy - ((fy * c[1]).astype(F) / d).astype(F)).astype(F)
        return d, np.floor((u + F(0.5)).astype(F)), np.floor((v + F(0.5)).astype(F))


def project_f64(pts, w_k, intr):
    """project_f32's geometry in float64 on the same float32 inputs -> (d, fi, fj, E_d, m_pix), float64 [n].  E_d = 6 eps S bounds what
    float32 can have moved d by; m_pix is the margin of the pixel tests, the smaller of u's and v's (0 where d - E_d <= 0).  seen_f64's
    docstring derives both."""
    P, w = np.asarray(pts, F).astype(np.float64), np.asarray(w_k, F).astype(np.float64).reshape(16)
    fx, fy, cx, cy = [float(F(x)) for x in intr]
    with np.errstate(all="ignore"):
        c, Ec = [], []
        for a in range(3):
            terms = [w[4 * a + q] * P[:, q] for q in range(3)]
            c.append(terms[0] + terms[1] + terms[2] + w[4 * a + 3])
            Ec.append(6 * EPS * (np.abs(terms[0]) + np.abs(terms[1]) + np.abs(terms[2]) + abs(w[4 * a + 3])))
        d, Ed = -c[2], Ec[2]
        dlo = d - Ed
        t, m_t = [], []
        for f, ca, Eca, c0, sign in ((fx, c[0], Ec[0], cx, 1.0), (fy, c[1], Ec[1], cy, -1.0)):
            q = f * ca
            r = q / d
            uu = c0 + sign * r
            tt = uu + 0.5
            Er = EPS * np.abs(r) + (EPS * np.abs(q) + f * Eca + np.abs(r) * Ed) / np.where(dlo > 0, dlo, np.nan)
            Et = Er + EPS * (np.abs(uu) + np.abs(tt))
            t.append(tt)
            m_t.append(np.where(dlo > 0, np.abs(tt - np.round(tt)) / Et, 0.0))
        return d, np.floor(t[0]), np.floor(t[1]), Ed, np.minimum(m_t[0], m_t[1])


def pixel_of(d, fi, fj, depth_k, edge):
    """the pixel test on a projection, in its own precision: in front of the camera and at least `edge` pixels inside the image, decided on
    the floats (a NaN fails) -> (ok, D): the frame's depth at the nearest pixel (pixel (0, 0)'s where ok is False)"""
    H, W = depth_k.shape
    lo, ihi, jhi = d.dtype.type(edge), d.dtype.type(W - edge), d.dtype.type(H - edge)
    ok = (d > 0) & (fi >= lo) & (fi < ihi) & (fj >= lo) & (fj < jhi)
    return ok, depth_k[np.where(ok, fj, 0).astype(np.int64), np.where(ok, fi, 0).astype(np.int64)].astype(d.dtype)


def seen_f32(pts, depths, intr, w2c, edge, trunc):
    """the rule of include/nsk.h in float32, one numpy operation per fp32 operation (project_f32).  pts [n, 3] float32, depths [K, H, W]
    float32, intr = (fx, fy, cx, cy), w2c [K, 4, 4] float32 -> uint8 [n]"""
    K = depths.shape[0]
    w = np.asarray(w2c, F).reshape(K, 16)
    trunc = F(trunc)
    seen = np.zeros(len(pts), bool)
    with np.errstate(all="ignore"):
        for k in range(K):
            d, fi, fj = project_f32(pts, w[k], intr)
            ok, D = pixel_of(d, fi, fj, depths[k], edge)
            ok &= np.isfinite(D) & (D > 0)
            ok &= d <= (D + trunc).astype(F)
            seen |= ok
    return seen.astype(np.uint8)


def seen_f64(pts, depths, intr, w2c, edge, trunc):
    """The same geometry in float64 on the same float32 inputs -> (seen uint8 [n], margin float64 [n], classes int [K, n]).

    margin: how far the node stands from its nearest decision boundary, in units of a bound on what float32 can have moved the compared
    quantity; seen_f32 must agree wherever margin > 1.  The bound follows the node's own operations, eps = 2^-24 per rounding:
      c_a = ((w0 p0 + w1 p1) + w2 p2) + w3: three products and three sums, every one of the six roundings at most eps * S_a with
            S_a = |w0 p0| + |w1 p1| + |w2 p2| + |w3| (every partial sum is below S_a)             ->  E_c[a] = 6 eps S_a
      d = -c_2 is exact                                                                         ->  E_d = E_c[2];  boundary d = 0
      q = fx * c_0: one rounding, and c_0's error times fx                                      ->  E_q = eps |q| + fx E_c[0]
      r = q / d: one rounding, q's error over d, d's error times |r| / d; d is taken at its low end d - E_d (the quotient's amplification)
                                                                                                ->  E_r = eps |r| + (E_q + |r| E_d) / (d - E_d)
      u = cx + r, t = u + 0.5: one rounding each                                                ->  E_t = E_r + eps (|u| + |t|)
      i = floor(t), compared with edge and W - edge: all of these switch where t crosses an integer (the rounding point of the pixel and
      the image edges alike), so the boundary is t's nearest integer; the same for v, j with fy, c_1, cy
      d <= D + trunc: D and trunc are float32 inputs, their sum is one rounding                 ->  E = E_d + eps |D + trunc|
    A pair decided by d <= 0 has the margin of that test alone; a pair that reaches a pixel with a measurement takes the minimum over all
    four tests, one that does not (outside the image, no measurement) over the first three.  A node's margin is the minimum over the keyframes."""
    K, H, W = depths.shape
    w = np.asarray(w2c, F).reshape(K, 16)
    trunc = float(F(trunc))
    n = len(pts)
    seen = np.zeros(n, bool)
    margin = np.full(n, np.inf)
    classes = np.zeros((K, n), np.int64)
    with np.errstate(all="ignore"):
        for k in range(K):
            d, fi, fj, Ed, m_pix = project_f64(pts, w[k], intr)
            m_d = np.abs(d) / Ed
            front = d > 0
            inimg, D = pixel_of(d, fi, fj, depths[k], edge)
            meas = inimg & np.isfinite(D) & (D > 0)
            lim = D + trunc
            m_z = np.abs(d - lim) / (Ed + EPS * np.abs(lim))
            ok = meas & (d <= lim)
            seen |= ok
            m = np.where(~front, m_d, np.minimum(m_d, m_pix))
            m = np.where(meas, np.minimum(m, m_z), m)
            margin = np.minimum(margin, np.nan_to_num(m, nan=0.0))
            cl = np.full(n, FAR)
            cl[ok] = SEEN
            cl[inimg & np.isinf(D)] = INF
            cl[inimg & np.isnan(D)] = NAN
            cl[inimg & (D <= 0)] = ZERO
            cl[front & (fj >= H - edge)] = BOTTOM
            cl[front & (fj < edge)] = TOP
            cl[front & (fi >= W - edge)] = RIGHT
            cl[front & (fi < edge)] = LEFT
            cl[~front] = BEHIND
            classes[k] = cl
    return seen.astype(np.uint8), margin, classes


# ---- the scenes of the seen-mask tests --------------------------------------------------------------------------------
def look_at(eye, target, roll=0.0):
    """camera-to-world [4, 4] float64 of a camera at `eye` looking along its -z towards `target` (x right, y up; world up = +y)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross([0.0, 1.0, 0.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    cr, sr = np.cos(roll), np.sin(roll)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = cr * right + sr * up, cr * up - sr * right, back, eye
    return M


def w2c_of(c2w):
    """world-to-camera in float32 from camera-to-world, inverted in float64"""
    return np.linalg.inv(np.asarray(c2w, np.float64)).astype(F)


def depth_image(H, W, near, far):
    """a ramp from `near` to `far` over the columns (tilted a little over the rows), a step down to `near` on the right fifth, a block of
    zeros in the top-left corner, one NaN and one inf near the middle"""
    j, i = np.mgrid[0:H, 0:W].astype(np.float64)
    D = near + (far - near) * (i / (W - 1)) + 0.02 * (far - near) * (j / (H - 1))
    D[:, W - W // 5:] = near
    D[:H // 4, :W // 4] = 0.0
    D = D.astype(F)
    D[H // 2, W // 2 - 2] = np.nan
    D[H // 2 - 2, W // 2 + 1] = np.inf
    return D


INTR = (40.0, 40.0, 15.5, 11.5)         # fx, fy, cx, cy of the 24 x 32 images
IMG_H, IMG_W = 24, 32


def cull_scene(bound, shape=(37, 23, 29), pad=0.3, keyframes=(0, 1, 2), params=((0, 0.0), (0, 0.5), (3, 0.0), (3, 0.5))):
    """lattice of shape (nx, ny, nz) over the bound enlarged by `pad` (as tests/test_gpu_mesh.py's lattice test) and up to three keyframes:
    0 outside the lattice looking in, 1 inside it, 2 outside looking away (it sees nothing).  params: the (edge, trunc) pairs it is used with"""
    b = np.asarray(bound, F)
    nx, ny, nz = shape
    origin = (b[:, 0] - F(pad)).astype(F)
    step = ((b[:, 1] - b[:, 0] + F(2 * pad)) / np.array([nx - 1, ny - 1, nz - 1], F)).astype(F)
    ctr = b.astype(np.float64).mean(axis=1)
    ext = (b[:, 1] - b[:, 0]).astype(np.float64)
    out_eye = ctr + np.array([-0.5 * ext[0] - 2.6, 0.13 * ext[1], 0.07 * ext[2]])
    in_eye = ctr + np.array([0.11 * ext[0], -0.06 * ext[1], 0.09 * ext[2]])
    c2w = np.stack([look_at(out_eye, ctr + [0.3, -0.11, 0.17], 0.05),
                    look_at(in_eye, ctr + [0.9 * ext[0], 0.21 * ext[1], -0.33 * ext[2]], -0.08),
                    look_at(out_eye, out_eye + (out_eye - ctr) + [0.0, 0.2, 0.1], 0.02)])[list(keyframes)]
    c2w = c2w.astype(F).astype(np.float64)               # poses as a float32 file holds them: a caller that inverts them in double gets w2c below
    depths = np.stack([depth_image(IMG_H, IMG_W, 4.0, 9.0), depth_image(IMG_H, IMG_W, 1.0, 3.5), depth_image(IMG_H, IMG_W, 4.0, 9.0)])[list(keyframes)]
    return dict(origin=origin, step=step, nx=nx, ny=ny, nz=nz, depths=depths, intr=INTR, c2w=c2w, params=tuple(params),
                away=list(keyframes).index(2) if 2 in keyframes else None,
                w2c=np.stack([w2c_of(m) for m in c2w]), pts=mc.lattice_points(origin, step, nx, ny, nz))


def view_scene(K, shape=(11, 7, 5)):
    """a small lattice (385 nodes by default: two workgroups, a partial last wave) round the origin and K frames: seven look_at poses
    (five round the lattice looking in, one inside it, the last looking away) cycled, five depth_image ramps cycled, so frame k's pose and image
    both differ from those of frames k - 32 and k - 1"""
    nx, ny, nz = shape
    step = np.full(3, 0.2, F)
    origin = (-0.5 * step * (np.array(shape, F) - F(1))).astype(F)
    eyes = [((3.0, 0.3, 0.2), (0.1, 0.0, 0.0), 0.04), ((-2.6, -0.4, 0.5), (0.0, 0.1, 0.0), -0.06), ((0.4, 2.8, 0.9), (0.0, 0.0, 0.1), 0.03),
            ((0.2, 0.1, 0.15), (0.9, 0.3, -0.2), 0.05), ((1.9, -1.8, -1.7), (0.0, 0.0, 0.0), 0.07), ((-0.5, -0.3, 3.1), (0.1, -0.1, 0.0), -0.02),
            ((3.0, 0.3, 0.2), (6.0, 0.8, 0.5), 0.02)]
    c2w = np.stack([look_at(e, t, r) for e, t, r in eyes]).astype(F).astype(np.float64)
    w2c = np.stack([w2c_of(m) for m in c2w])
    images = np.stack([depth_image(IMG_H, IMG_W, near, far) for near, far in ((2.2, 3.6), (0.3, 1.4), (2.6, 3.1), (1.8, 4.0), (2.9, 3.3))])
    ks = np.arange(K)
    return dict(origin=origin, step=step, nx=nx, ny=ny, nz=nz, intr=INTR, w2c=w2c[ks % len(w2c)].reshape(K, 4, 4),
                depths=images[ks % len(images)].reshape(K, IMG_H, IMG_W), pts=mc.lattice_points(origin, step, nx, ny, nz))


def long_trajectory(sc, order, shift=(0.01, -0.005, 0.0075)):
    """a trajectory longer than a scene's own: frame k is keyframe order[k] of `sc` (cull_scene) with its camera moved by k * shift (m, world)
    and its depth image scaled by 1 + k / 256 (zeros, NaN and inf stay what they are), so that no two frames are alike.
    -> dict(c2w [K, 4, 4] float64 holding float32 values, w2c [K, 4, 4] float32, depths [K, H, W] float32)"""
    order = list(order)
    k = np.arange(len(order))
    c2w = sc["c2w"][order].copy()
    c2w[:, :3, 3] += k[:, None] * np.asarray(shift, np.float64)
    c2w = c2w.astype(F).astype(np.float64)
    depths = (sc["depths"][order] * (F(1) + k.astype(F) / F(256))[:, None, None]).astype(F)
    return dict(c2w=c2w, w2c=np.stack([w2c_of(m) for m in c2w]), depths=depths)


MESHER_N, MESHER_PAD = 40, 0.1


def mesher_scene(bound):
    """what the C++ Mesher's get_clean_mesh is run on: resolution 40, padding 0.1, the first two keyframes, its default seen_edge / seen_trunc"""
    return cull_scene(bound, (MESHER_N,) * 3, MESHER_PAD, keyframes=(0, 1), params=((0, 0.5),))


def check_scene(sc, edge, trunc, max_unsure=0.01):
    """the CPU conditions of a scene: seen_f32 = seen_f64 wherever the margin exceeds 1, at most 1 % of the nodes at or below 1, every class
    present.  Returns seen_f32's mask (flat)."""
    a = seen_f32(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], edge, trunc)
    b, margin, classes = seen_f64(sc["pts"], sc["depths"], sc["intr"], sc["w2c"], edge, trunc)
    sure = margin > 1.0
    assert (a[sure] == b[sure]).all(), "%d nodes with margin > 1 differ between float32 and float64" % int((a[sure] != b[sure]).sum())
    assert (~sure).mean() <= max_unsure, "%.3f %% of the nodes within the float32 bound of a boundary" % (100 * (~sure).mean())
    have = set(np.unique(classes).tolist())
    missing = [CLASS_NAMES[q] for q in range(10) if q not in have]
    assert not missing, "edge %d trunc %g: no node is %s" % (edge, trunc, missing)
    assert 0 < a.sum() < a.size
    return a


# ---- connected components ----------------------------------------------------------------------------------------------
def triangle_areas(verts, tris):
    """0.5 |(v1 - v0) x (v2 - v0)| in float32, every operation rounded on its own"""
    v = np.asarray(verts, F)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e, f = (v[t[:, 1]] - v[t[:, 0]]).astype(F), (v[t[:, 2]] - v[t[:, 0]]).astype(F)
    x = ((e[:, 1] * f[:, 2]).astype(F) - (e[:, 2] * f[:, 1]).astype(F)).astype(F)
    y = ((e[:, 2] * f[:, 0]).astype(F) - (e[:, 0] * f[:, 2]).astype(F)).astype(F)
    z = ((e[:, 0] * f[:, 1]).astype(F) - (e[:, 1] * f[:, 0]).astype(F)).astype(F)
    s = (((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)
    return (F(0.5) * np.sqrt(s).astype(F)).astype(F)


def components(verts, tris, min_area=0.0, largest_only=False):
    """union-find over the triangle list: roots are hooked below smaller roots, paths compressed until every vertex points at its root
    (= the component's smallest vertex index).  -> dict: label [nv], comp (labels of the components with a triangle, ascending), area
    (float64 per component), kept (bool per component), verts / tris (the filtered mesh, order kept, re-indexed, vertices without a
    triangle dropped), n_components, n_kept"""
    verts = np.asarray(verts, F).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    nv = len(verts)
    parent = np.arange(nv)
    ea = np.concatenate([tris[:, 0], tris[:, 0]])
    eb = np.concatenate([tris[:, 1], tris[:, 2]])
    while True:
        while True:
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
        ra, rb = parent[ea], parent[eb]
        m = ra != rb
        if not m.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[m], np.minimum(ra, rb)[m])
    used = np.zeros(nv, bool)
    used[tris.reshape(-1)] = True
    comp = np.unique(parent[used])
    tl = parent[tris[:, 0]] if len(tris) else np.zeros(0, np.int64)
    area_v = np.bincount(tl, weights=triangle_areas(verts, tris).astype(np.float64), minlength=nv) if nv else np.zeros(0)
    area = area_v[comp]
    if largest_only:
        kept = np.zeros(len(comp), bool)
        if len(comp):
            kept[int(np.argmax(area))] = True                # (argmax returns the first, i.e. the smallest label, among equals)
    else:
        kept = area > float(F(min_area))
    keep_v = np.zeros(nv, bool)
    keep_v[comp[kept]] = True
    vk = used & keep_v[parent]
    tk = keep_v[tl]
    new = np.cumsum(vk) - 1
    return dict(label=parent, comp=comp, area=area, kept=kept, verts=verts[vk], tris=new[tris[tk]].astype(np.int32).reshape(-1, 3),
                n_components=len(comp), n_kept=int(kept.sum()))


def components_bfs(nv, tris):
    """labels by a plain breadth-first search (the check of `components`)"""
    adj = [[] for _ in range(nv)]
    for a, b, c in np.asarray(tris, np.int64).reshape(-1, 3):
        adj[a] += [b, c]; adj[b] += [a, c]; adj[c] += [a, b]
    label = np.full(nv, -1, np.int64)
    for s in range(nv):
        if label[s] >= 0:
            continue
        label[s] = s
        queue = [s]
        while queue:
            nxt = []
            for x in queue:
                for y in adj[x]:
                    if label[y] < 0:
                        label[y] = s
                        nxt.append(y)
            queue = nxt
    return label


def areas_clear_of(area, thresholds, largest_only, rel=1e-4):
    """the conditions a filter test puts on its INPUT: no component area within a relative `rel` of a threshold, and (largest_only) the two
    largest areas more than a relative `rel` apart"""
    area = np.sort(np.asarray(area, np.float64))
    for th in thresholds:
        if th > 0 and len(area) and (np.abs(area - th) <= rel * th).any():
            return False
    if largest_only and len(area) > 1 and area[-1] - area[-2] <= rel * area[-1]:
        return False
    return True


# ---- volumes of the filter tests -----------------------------------------------------------------------------------------
SPHERES = (((0.55, 0.60, 0.55), 0.40), ((1.45, 0.50, 1.40), 0.30), ((0.60, 1.50, 1.45), 0.20))       # centre, radius
BLOB = ((1.55, 1.60, 0.40), 0.07)
SPHERES_ORIGIN, SPHERES_STEP, SPHERES_N = (0.0, 0.0, 0.0), (0.05, 0.05, 0.05), 40


def spheres_volume():
    """three spheres and one small blob in a 40^3 volume: value = max over the balls of radius - distance (inside positive)"""
    cx, cy, cz = [c.astype(np.float64) for c in mc.lattice_coords(SPHERES_ORIGIN, SPHERES_STEP, (SPHERES_N,) * 3)]
    x, y, z = cx[None, None, :], cy[None, :, None], cz[:, None, None]
    vol = np.full((SPHERES_N,) * 3, -np.inf)
    for c, r in SPHERES + (BLOB,):
        vol = np.maximum(vol, r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2))
    return vol.astype(F)


def serpentine_volume(nx=64, ny=12, nz=12, radius=1.3):
    """one tube wound through the volume: runs along x, alternating direction, at (y, z) = (3, 3), (8, 3), (8, 8), (3, 8), joined at the ends;
    value = radius - distance to the polyline (node units): one long component whose vertex indices run back and forth"""
    rows = [(3.0, 3.0), (8.0, 3.0), (8.0, 8.0), (3.0, 8.0)]
    path = []
    for q, (y, z) in enumerate(rows):
        xs = (3.0, nx - 4.0) if q % 2 == 0 else (nx - 4.0, 3.0)
        path += [(xs[0], y, z), (xs[1], y, z)]
    path = np.array(path)
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    P = np.stack([i, j, k], -1)
    dist = np.full((nz, ny, nx), np.inf)
    for a, b in zip(path[:-1], path[1:]):
        ab = b - a
        t = np.clip(((P - a) @ ab) / (ab @ ab), 0.0, 1.0)
        dist = np.minimum(dist, np.linalg.norm(P - (a + t[..., None] * ab), axis=-1))
    return (radius - dist).astype(F)


def numpy_mesh(table, vol, origin, step, level=0.0):
    """marching cubes by hand with a 256-case table (list of edge-triple lists) -> (vertices float32 [nv, 3], triangles int32 [nt, 3]) in the
    order include/nsk.h fixes (tests/test_mesh_cpu.py checks this construction against the volume-only checks)"""
    nz, ny, nx = vol.shape
    keys, pos = mc.reference_vertices(vol, origin, step, level)
    ins = vol > F(level)
    code = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for c, (dx, dy, dz) in enumerate(mc.CORNER):
        code |= ins[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int32) << c
    code[~mc.processed_cells(vol)] = 0
    tris = []
    for k, j, i in zip(*np.nonzero((code != 0) & (code != 255))):
        for t in table[code[k, j, i]]:
            for e in t:
                dx, dy, dz = mc.CORNER[mc.edge_ends(e)[0]]
                tris.append((((k + dz) * ny + j + dy) * nx + i + dx) * 3 + (e >> 2))
    tris = np.searchsorted(keys, np.array(tris, np.int64)).astype(np.int32).reshape(-1, 3)
    return pos, tris

"""numpy restatement of the mesh depth views (include/nsk.h: nsk_mesh_depth, nsk_depth_pair_stats, nsk_depth_views) and the scenes their tests
share.  Every fp32 operation of the rule is one numpy float32 operation here, in the same order, so the device's images must equal these
bit for bit; the view draw is restated in float64 the same way.  tests/test_raster_cpu.py proves the helpers on analytic scenes."""
import numpy as np

f32 = np.float32
M64 = (1 << 64) - 1


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def camera(w, p):
    """camera space of the points p [n, 3] under the row-major world-to-camera matrix w (16 float32): three arrays [n]"""
    w = np.asarray(w, f32).reshape(-1)
    p = np.asarray(p, f32)
    return [((w[4 * a] * p[:, 0] + w[4 * a + 1] * p[:, 1]) + w[4 * a + 2] * p[:, 2]) + w[4 * a + 3] for a in range(3)]


def cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def pixel_box(a, b, c, H, W, fx, fy, cx, cy):
    """the pixel box (x0, x1, y0, y1) of a triangle with the camera-space vertices a, b, c (float32 triples), or None: no pixel"""
    d = [-a[2], -b[2], -c[2]]
    if all(x <= 0 for x in d):
        return None
    box = (0, W - 1, 0, H - 1)
    if all(x > 0 for x in d):
        u = [cx + (fx * p[0]) / x for p, x in zip((a, b, c), d)]
        v = [cy - (fy * p[1]) / x for p, x in zip((a, b, c), d)]
        if all(abs(x) < f32(1048576.0) for x in u + v):             # (a NaN fails)
            x0 = max(int(np.floor(min(u))) - 1, 0); x1 = min(int(np.floor(max(u))) + 2, W - 1)
            y0 = max(int(np.floor(min(v))) - 1, 0); y1 = min(int(np.floor(max(v))) + 2, H - 1)
            if x0 > x1 or y0 > y1:
                return None
            box = (x0, x1, y0, y1)
    return box


def render(verts, tris, w2c, H, W, fx, fy, cx, cy):
    """nsk_mesh_depth -> (depth [V, H, W] float32, the number of triangles with an index out of range)"""
    verts = np.asarray(verts, f32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, f32).reshape(-1, 16)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    nv = len(verts)
    good = ((tris >= 0) & (tris < nv)).all(1) if len(tris) else np.zeros(0, bool)
    out = np.zeros((len(w2c), H, W), f32)
    xs = (np.arange(W, dtype=f32) - cx) / fx
    ys = -((np.arange(H, dtype=f32) - cy) / fy)
    with np.errstate(all="ignore"):
        for k, w in enumerate(w2c):
            cam = camera(w, verts) if nv else [np.zeros(0, f32)] * 3
            dep = np.full((H, W), np.inf, f32)
            for t in np.nonzero(good)[0]:
                a, b, c = [tuple(cam[q][i] for q in range(3)) for i in tris[t]]
                if not np.isfinite(a + b + c).all():
                    continue
                box = pixel_box(a, b, c, H, W, fx, fy, cx, cy)
                if box is None:
                    continue
                x0, x1, y0, y1 = box
                x = xs[None, x0:x1 + 1]
                y = ys[y0:y1 + 1, None]
                E = []
                for p, q in ((b, c), (c, a), (a, b)):
                    n = cross(p, q)
                    E.append((x * n[0] + y * n[1]) - n[2])
                inside = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
                e1 = tuple(b[q] - a[q] for q in range(3)); e2 = tuple(c[q] - a[q] for q in range(3))
                n = cross(e1, e2)
                num = (a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]
                t_ = num / ((x * n[0] + y * n[1]) - n[2])
                assert t_.dtype == f32
                hit = inside & np.isfinite(t_) & (t_ > 0)
                sub = dep[y0:y1 + 1, x0:x1 + 1]
                sub[...] = np.where(hit & (t_ < sub), t_, sub)
            out[k] = np.where(np.isinf(dep), f32(0), dep)
    return out, int((~good).sum())


def pair_stats(a, b):
    """nsk_depth_pair_stats -> [V, 4] float64 (sums in numpy's own association: compare within 1e-12 relative; the counts are exact)"""
    a = np.asarray(a, f32).reshape(len(a), -1); b = np.asarray(b, f32).reshape(len(b), -1)
    out = np.zeros((len(a), 4))
    with np.errstate(all="ignore"):
        d = np.abs(a - b)
    assert d.dtype == f32
    fin = np.isfinite(d)
    both = (a > 0) & (b > 0)
    d64 = d.astype(np.float64)
    out[:, 0] = np.where(fin, d64, 0.0).sum(1)
    out[:, 1] = both.sum(1)
    out[:, 2] = np.where(fin & both, d64, 0.0).sum(1)
    out[:, 3] = (a > 0).sum(1)
    return out


# ---- the view draw ----------------------------------------------------------------------------------------------------------------
def hash_u32(seed, a, b):
    """the counter hash of nsk_sample_pixels"""
    x = (seed ^ (0x9E3779B97F4A7C15 * (a + 1)) ^ (0xC2B2AE3D27D4EB4F * (b + 1))) & M64
    x ^= x >> 33; x = (x * 0xFF51AFD7ED558CCD) & M64; x ^= x >> 33; x = (x * 0xC4CEB9FE1A85EC53) & M64; x ^= x >> 33
    return x >> 32


def finite_box(verts):
    v = np.asarray(verts, f32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return np.concatenate([v.min(0), v.max(0)]).astype(f32)


def view_parts(box, n_views, seed=0, shrink=0.7):
    """origin, target (float64 [V, 3]) of the draw"""
    box = np.asarray(box, f32).astype(np.float64)
    lo, hi = box[:3], box[3:]
    ext, ctr = hi - lo, 0.5 * (lo + hi)
    u = np.array([[(hash_u32(seed & M64, k, m) >> 8) * 2.0 ** -24 for m in range(6)] for k in range(n_views)]).reshape(n_views, 6)
    origin = ctr + (u[:, :3] - 0.5) * (np.float64(shrink) * ext)
    target = lo + u[:, 3:] * ext
    return origin, target


def draw_views(box, n_views, seed=0, shrink=0.7):
    """nsk_depth_views -> w2c [V, 4, 4] float32, every float64 operation in the order the header states"""
    o, target = view_parts(box, n_views, seed, shrink)
    w = np.zeros((n_views, 4, 4), f32)
    with np.errstate(all="ignore"):
        f = target - o
        f = f / np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])[:, None]
        sl = np.sqrt(f[:, 1] * f[:, 1] + f[:, 0] * f[:, 0])
        s = np.stack([f[:, 1] / sl, -f[:, 0] / sl, np.zeros(n_views)], 1)
        v = np.stack(cross((f[:, 0], f[:, 1], f[:, 2]), (s[:, 0], s[:, 1], s[:, 2])), 1)
        v = v / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[:, None]
        for a, r in enumerate((s, -v, -f)):
            w[:, a, :3] = r.astype(f32)
            w[:, a, 3] = (-((r[:, 0] * o[:, 0] + r[:, 1] * o[:, 1]) + r[:, 2] * o[:, 2])).astype(f32)
    w[:, 3, 3] = 1
    return w


def viewmatrix_w2c(origin, target):
    """upstream's viewmatrix (eval_recon.py) in plain float64 numpy, up = (0, 0, -1), turned to this project's camera (-z forward, y up) and
    inverted with numpy: what draw_views is checked against"""
    def normalize(x):
        return x / np.linalg.norm(x)
    z = normalize(np.asarray(target, np.float64) - np.asarray(origin, np.float64))
    x = normalize(np.cross(np.array([0.0, 0.0, -1.0]), z))
    y = normalize(np.cross(z, x))
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, -y, -z, origin
    return np.linalg.inv(c2w)


def depth_l1(rec, gt, n_views, H, W, focal, seed=0, shrink=0.7, min_cover=0.0):
    """the whole metric restated: (depth_l1_cm, n_used, restricted_l1_cm, stats)"""
    w = draw_views(finite_box(gt[0]), n_views, seed, shrink)
    cx, cy = W / 2.0 - 0.5, H / 2.0 - 0.5
    dg, _ = render(gt[0], gt[1], w, H, W, focal, focal, cx, cy)
    dr, _ = render(rec[0], rec[1], w, H, W, focal, focal, cx, cy)
    st = pair_stats(dg, dr)
    used = st[:, 3] / (H * W) >= min_cover
    n_used = int(used.sum())
    l1 = 100.0 * float((st[used, 0] / (H * W)).sum()) / n_used if n_used else float("nan")
    both = float(st[used, 1].sum())
    return l1, n_used, (100.0 * float(st[used, 2].sum()) / both if both else float("nan")), st


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def look(R=None, t=(0.0, 0.0, 0.0)):
    """a world-to-camera matrix [4, 4] float32 from a rotation and a translation (p_cam = R p + t)"""
    w = np.eye(4)
    if R is not None:
        w[:3, :3] = R
    w[:3, 3] = t
    return w.astype(f32)


def rot_y(th):
    return np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])


def rot_x(th):
    return np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])


def grid_tris(n, m):
    idx = np.arange(n * m).reshape(n, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return np.stack([np.stack([a, b, c], 1), np.stack([c, b, d], 1)], 1).reshape(-1, 3).astype(np.int32)


SHEET_PLANE = (-3.0, 0.3, 0.2)             # z = -3 + 0.3 x + 0.2 y in the camera space of sheet()'s first view


def sheet(n=40, seed=0):
    """a jittered n x n-vertex tilted sheet (2 (n - 1)^2 triangles; n = 40: 3 042), given in world space, and the view whose camera space
    holds it on SHEET_PLANE over |x|, |y| <= 6 -> (verts float32, tris int32, w2c [4, 4] float32)"""
    rng = np.random.default_rng(seed)
    g = np.linspace(-6, 6, n)
    X, Y = np.meshgrid(g, g)
    X = X + rng.uniform(-0.1, 0.1, X.shape); Y = Y + rng.uniform(-0.1, 0.1, X.shape)
    Z = SHEET_PLANE[0] + SHEET_PLANE[1] * X + SHEET_PLANE[2] * Y
    vc = np.stack([X, Y, Z], -1).reshape(-1, 3)
    R, tr = rot_y(0.7), np.array([0.3, -0.2, 0.5])
    return ((vc - tr) @ R).astype(f32), grid_tris(n, n), look(R, tr)


def sheet_views():
    """the sheet's own view, one turned and pulled back, one from the side that looks along the sheet"""
    w0 = sheet()[2].astype(np.float64)
    w1 = look(rot_y(0.4) @ rot_x(-0.3), (0.5, 0.2, -1.5)).astype(np.float64) @ w0
    w2 = look(rot_y(1.3), (0.0, 0.4, 0.0)).astype(np.float64) @ w0
    return np.stack([w0, w1, w2]).astype(f32)


def floor():
    """two 100 m triangles at y = -1 around the origin: they cross the camera plane of the identity view"""
    v = np.array([[-50, -1, -50], [50, -1, -50], [50, -1, 50], [-50, -1, 50]], f32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def cube_room(lo=(-2.0, -1.5, -2.5), hi=(2.0, 1.5, 2.5)):
    """the 12 triangles of a closed box, 8 shared vertices"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], f32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([[a, b, c] for a, b, c, d in q] + [[a, c, d] for a, b, c, d in q], np.int32)
    return v, t


def room_views_inside():
    return np.stack([look(), look(rot_y(2.1) @ rot_x(0.4), (0.3, -0.2, 0.5)), look(rot_x(-1.2), (-0.5, 0.4, 0.1))]).astype(f32)


def room_views_outside():
    return np.stack([look(None, (0.0, 0.0, -9.0)), look(rot_y(0.6) @ rot_x(0.5), (0.5, 0.0, -12.0))]).astype(f32)


def blob(n=11, seed=3):
    """a 200-triangle open surface with some relief around the origin (2 x 10 x 10 triangles)"""
    rng = np.random.default_rng(seed)
    g = np.linspace(-1.5, 1.5, n)
    X, Y = np.meshgrid(g, g)
    Z = 0.4 * np.sin(1.7 * X) * np.cos(1.3 * Y) + rng.uniform(-0.05, 0.05, X.shape)
    return np.stack([X, Y, Z], -1).reshape(-1, 3).astype(f32), grid_tris(n, n)


def orbit_views(n, radius=4.0, seed=1):
    """n views looking at the origin from a sphere: some from behind, some grazing"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        R = rot_y(rng.uniform(0, 2 * np.pi)) @ rot_x(rng.uniform(-1.2, 1.2))
        out.append(look(R, (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -radius * rng.uniform(0.3, 1.2))))
    return np.stack(out).astype(f32)

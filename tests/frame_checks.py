"""The rule of nsk_frame_prepare (include/nsk.h), restated in vectorised numpy: one numpy operation per fp32 operation of
the kernel, in the kernel's order, every stage's result a stored float32 array.  A stage that is off is skipped.

  S0  conversion     colour uint8: float(v) / 255 (a division); float32 passes.  depth: (float(v) / png_depth_scale) * scale.
  S1  undistort      colour only, n_dist > 0, needs colour size == depth size.  OpenCV's undistort with newCameraMatrix = K, bilinear taps
                     against a zero border.
  S2  to depth size  colour only, when the sizes differ: bilinear with half-pixel centres (cv2.resize INTER_LINEAR).
  S3  crop_size      colour: bilinear with aligned corners; depth: nearest.
  S4  crop_edge      e pixels off every side.
  swap_rb exchanges channels 0 and 2 of the output.

opts is a dict: fx fy cx cy (for the depth size), dist (a list of 0, 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]), crop_size ((H, W) or
None), crop_edge, png_depth_scale, scale, swap_rb.  Missing keys take the defaults of `options`.

Also here: the fp64 form of S1 with a per-pixel bound on what the fp32 form may differ by (undistort_f64), and the intrinsics in Python
doubles as upstream writes them (intrinsics_upstream)."""
import numpy as np

F = np.float32
U = 2.0 ** -24                      # the unit roundoff of fp32

TUM_DIST = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
TUM_CAM = dict(H=480, W=640, fx=517.3, fy=516.5, cx=318.6, cy=255.3, crop_size=(384, 512), crop_edge=8, png_depth_scale=5000.0)


def options(**kw):
    o = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, dist=[], crop_size=None, crop_edge=0, png_depth_scale=1.0, scale=1.0, swap_rb=False)
    for k in kw:
        assert k in o, k
    o.update(kw)
    o["dist"] = [] if o["dist"] is None else list(o["dist"])
    return o


def tum_options(H=480, W=640, **kw):
    """TUM's cam block with the intrinsics scaled to an H x W image (480 x 640: the block itself)"""
    sy, sx = H / 480.0, W / 640.0
    o = dict(fx=517.3 * sx, fy=516.5 * sy, cx=318.6 * sx, cy=255.3 * sy, dist=TUM_DIST, crop_size=(384, 512), crop_edge=8, png_depth_scale=5000.0)
    o.update(kw)
    return options(**o)


# ---- the plan: which stages run, the output size, the intrinsics ------------------------------------------------------------------------
def plan(opts, Hc, Wc, Hd, Wd):
    """-> dict(H, W, intr [fx fy cx cy] float32, s1, s2, s3); ValueError names the option that is wrong"""
    o = options(**opts)
    nd = len(o["dist"])
    if min(Hc, Wc, Hd, Wd) < 1:
        raise ValueError("image size")
    if nd not in (0, 4, 5, 8):
        raise ValueError("n_dist = %d" % nd)
    cs = o["crop_size"]
    if cs is not None and (int(cs[0]) <= 0) != (int(cs[1]) <= 0):
        raise ValueError("crop_size")
    if cs is not None and int(cs[0]) <= 0:
        cs = None
    e = int(o["crop_edge"])
    if e < 0:
        raise ValueError("crop_edge")
    same = Hc == Hd and Wc == Wd
    if nd > 0 and not same:
        raise ValueError("undistort needs equal sizes")
    H, W = (int(cs[0]), int(cs[1])) if cs is not None else (Hd, Wd)
    if 2 * e >= H or 2 * e >= W:
        raise ValueError("crop_edge")
    fx, fy, cx, cy = F(o["fx"]), F(o["fy"]), F(o["cx"]), F(o["cy"])
    if cs is not None:
        sx, sy = F(W) / F(Wd), F(H) / F(Hd)
        fx, cx, fy, cy = fx * sx, cx * sx, fy * sy, cy * sy
    if e > 0:
        cx, cy = cx - F(e), cy - F(e)
    return dict(H=H - 2 * e, W=W - 2 * e, intr=np.array([fx, fy, cx, cy], F), s1=nd > 0, s2=not same, s3=cs is not None, Hs=H, Ws=W, e=e)


def intrinsics_upstream(H, W, fx, fy, cx, cy, crop_size=None, crop_edge=0):
    """upstream's dataset layer (src/utils/datasets.py update_cam) in Python doubles -> (H, W, fx, fy, cx, cy)"""
    if crop_size is not None:
        sx, sy = crop_size[1] / W, crop_size[0] / H
        fx, cx, fy, cy = sx * fx, sx * cx, sy * fy, sy * cy
        H, W = crop_size
    if crop_edge > 0:
        H, W, cx, cy = H - 2 * crop_edge, W - 2 * crop_edge, cx - crop_edge, cy - crop_edge
    return H, W, fx, fy, cx, cy


# ---- S0 ---------------------------------------------------------------------------------------------------------------------------------
def convert_color(c):
    if c.dtype == np.uint8:
        return c.astype(F) / F(255.0)
    assert c.dtype == np.float32
    return c.copy()


def convert_depth(d, png_depth_scale, scale):
    assert d.dtype in (np.uint16, np.float32)
    with np.errstate(all="ignore"):
        return (d.astype(F) / F(png_depth_scale)) * F(scale)


# ---- the bilinear value: top = lx0 v00 + lx1 v01, bot = lx0 v10 + lx1 v11, out = ly0 top + ly1 bot, every product and sum rounded --------
def _bilinear(v00, v01, v10, v11, lx1, ly1):
    lx0, ly0 = F(1) - lx1, F(1) - ly1
    with np.errstate(all="ignore"):
        top = lx0 * v00 + lx1 * v01
        bot = lx0 * v10 + lx1 * v11
        return ly0 * top + ly1 * bot


def _axis_half(n_in, n_out):
    """S2 along one axis: taps i0, i1 and the weight l1 of i1"""
    s = F(n_in) / F(n_out)
    r = np.maximum((np.arange(n_out, dtype=F) + F(0.5)) * s - F(0.5), F(0))
    i0 = np.minimum(r.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, r - i0.astype(F)


def _axis_aligned(n_in, n_out):
    """S3 (colour) along one axis"""
    s = F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)
    r = np.arange(n_out, dtype=F) * s
    i0 = np.minimum(r.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, r - i0.astype(F)


def nearest_index(n_in, n_out):
    """S3 (depth) along one axis"""
    s = F(n_in) / F(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F) * s).astype(np.int32), n_in - 1)


def _resample(img, ay, ax):
    """img [..., H, W, C] through the per-axis taps ay, ax"""
    (y0, y1, ly), (x0, x1, lx) = ay, ax
    g = lambda yy, xx: img[..., yy[:, None], xx[None, :], :]
    return _bilinear(g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1), lx[None, :, None], ly[:, None, None])


def _any4(flag, ay, ax):
    (y0, y1, _), (x0, x1, _) = ay, ax
    g = lambda yy, xx: flag[..., yy[:, None], xx[None, :]]
    return g(y0, x0) | g(y0, x1) | g(y1, x0) | g(y1, x1)


def resize_half(img, H_out, W_out):
    """S2: [..., H, W, C] float32 -> [..., H_out, W_out, C]"""
    return _resample(img, _axis_half(img.shape[-3], H_out), _axis_half(img.shape[-2], W_out))


def resize_aligned(img, H_out, W_out):
    """S3 for colour"""
    return _resample(img, _axis_aligned(img.shape[-3], H_out), _axis_aligned(img.shape[-2], W_out))


def resize_nearest(d, H_out, W_out):
    """S3 for depth: [..., H, W]"""
    return d[..., nearest_index(d.shape[-2], H_out)[:, None], nearest_index(d.shape[-1], W_out)[None, :]]


# ---- S1 ---------------------------------------------------------------------------------------------------------------------------------
def _coeffs(dist):
    k = list(dist) + [0.0] * (8 - len(dist))
    return dict(k1=k[0], k2=k[1], p1=k[2], p2=k[3], k3=k[4], k4=k[5], k5=k[6], k6=k[7])


def source_coords(H, W, fx, fy, cx, cy, dist):
    """(us, vs) [H, W] float32: where the destination pixel (u, v) reads the distorted image"""
    k = {n: F(v) for n, v in _coeffs(dist).items()}
    fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
    u = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        x = (u - cx) / fx
        y = (v - cy) / fy
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r4 * r2
        num = ((F(1) + k["k1"] * r2) + k["k2"] * r4) + k["k3"] * r6
        den = ((F(1) + k["k4"] * r2) + k["k5"] * r4) + k["k6"] * r6
        rad = num / den
        xd = (x * rad + (F(2) * k["p1"]) * xy) + k["p2"] * (r2 + F(2) * xx)
        yd = (y * rad + k["p1"] * (r2 + F(2) * yy)) + (F(2) * k["p2"]) * xy
        us = fx * xd + cx
        vs = fy * yd + cy
    return us, vs


def undistort_f32(img, fx, fy, cx, cy, dist):
    """S1: img [..., H, W, C] float32 -> (the undistorted image, border [H, W] bool: the pixel read a tap outside the image)"""
    H, W = img.shape[-3], img.shape[-2]
    us, vs = source_coords(H, W, fx, fy, cx, cy, dist)
    with np.errstate(all="ignore"):
        inside = (us > F(-1)) & (us < F(W)) & (vs > F(-1)) & (vs < F(H))
    i0 = np.floor(np.where(inside, us, F(0))).astype(np.int32)
    j0 = np.floor(np.where(inside, vs, F(0))).astype(np.int32)
    lx1 = np.where(inside, us, F(0)) - i0.astype(F)
    ly1 = np.where(inside, vs, F(0)) - j0.astype(F)

    def tap(j, i):
        ok = (j >= 0) & (j < H) & (i >= 0) & (i < W)
        val = img[..., np.clip(j, 0, H - 1), np.clip(i, 0, W - 1), :]
        return np.where(ok[..., None], val, F(0)), ok
    (v00, o00), (v01, o01), (v10, o10), (v11, o11) = tap(j0, i0), tap(j0, i0 + 1), tap(j0 + 1, i0), tap(j0 + 1, i0 + 1)
    out = _bilinear(v00, v01, v10, v11, lx1[..., None], ly1[..., None])
    out = np.where(inside[..., None], out, F(0)).astype(F)
    border = ~(inside & o00 & o01 & o10 & o11)
    return out, border


class _E:
    """a double with a bound on how far the fp32 evaluation of the same expression may lie from it (running error analysis; every
    fp32 operation adds U |result|, widened by 1e-6 for taking the magnitudes from the doubles)"""
    S = U * (1.0 + 1e-6)

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    def _r(self, v, e):
        return _E(v, e * (1.0 + 1e-9) + _E.S * (np.abs(v) + e))

    def __add__(self, o):
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        q = self.v / o.v
        lo = np.maximum(np.abs(o.v) - o.e, 1e-300)
        return self._r(q, (self.e + np.abs(q) * o.e) / lo)


def source_coords_f64(H, W, fx, fy, cx, cy, dist):
    """the same expression in doubles on the fp32 parameters -> (us, vs, eu, ev): the coordinates and the fp32 rounding bounds of them"""
    k = {n: _E(float(F(v))) for n, v in _coeffs(dist).items()}
    fx, fy, cx, cy = (_E(float(F(a))) for a in (fx, fy, cx, cy))
    u = _E(np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W)))
    v = _E(np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W)))
    one, two = _E(1.0), _E(2.0)
    x = (u - cx) / fx
    y = (v - cy) / fy
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    r4 = r2 * r2
    r6 = r4 * r2
    num = ((one + k["k1"] * r2) + k["k2"] * r4) + k["k3"] * r6
    den = ((one + k["k4"] * r2) + k["k5"] * r4) + k["k6"] * r6
    rad = num / den
    xd = (x * rad + (two * k["p1"]) * xy) + k["p2"] * (r2 + two * xx)
    yd = (y * rad + k["p1"] * (r2 + two * yy)) + (two * k["p2"]) * xy
    us = fx * xd + cx
    vs = fy * yd + cy
    return us.v, vs.v, us.e, vs.e


def bilinear_zero_f64(img, us, vs):
    """img [H, W, C] double sampled bilinearly at (us, vs) [H, W] against a zero border (the interpolant itself, in doubles)"""
    H, W = img.shape[0], img.shape[1]
    pad = np.zeros((H + 2, W + 2) + img.shape[2:], np.float64)
    pad[1:-1, 1:-1] = img
    inside = (us > -1) & (us < W) & (vs > -1) & (vs < H)
    a, b = np.where(inside, us, 0.0), np.where(inside, vs, 0.0)
    i0, j0 = np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)
    lx, ly = (a - i0)[..., None], (b - j0)[..., None]
    g = lambda j, i: pad[j + 1, i + 1]
    top = (1 - lx) * g(j0, i0) + lx * g(j0, i0 + 1)
    bot = (1 - lx) * g(j0 + 1, i0) + lx * g(j0 + 1, i0 + 1)
    return np.where(inside[..., None], (1 - ly) * top + ly * bot, 0.0)


def undistort_f64(img, fx, fy, cx, cy, dist):
    """S1 in doubles on the fp32 image [H, W, C] -> (value, bound), both [H, W, C] doubles.  |undistort_f32 - value| <= bound:
         the interpolant is continuous and piecewise bilinear, its slope along an axis at most the largest difference D among the taps
         of the cells it passes, so moving the coordinates by (eu, ev) moves it by at most D (eu + ev); the taps touched are those of
         every cell between floor(us - eu) and floor(us + eu) + 1, likewise in v (zeros outside the image);
         the fp32 bilinear value is a convex combination of taps of magnitude <= M; l1 = us - float(i0) is exact, and a row carries
         the roundings of 1 - l1, of its products and of its sum (3 U M on the convex path), the combination of the two rows the same
         three again plus the rows' own (4 U M with the row's passed through): 7 U M, taken as 8 U M."""
    H, W = img.shape[0], img.shape[1]
    img = np.asarray(img, np.float64)
    us, vs, eu, ev = source_coords_f64(H, W, fx, fy, cx, cy, dist)
    val = bilinear_zero_f64(img, us, vs)
    pad = np.zeros((H + 2, W + 2) + img.shape[2:], np.float64)
    pad[1:-1, 1:-1] = img
    # the window of taps [i_lo, i_hi] x [j_lo, j_hi] in padded indices, clipped to the padded image (everything further out is zero, as the
    # rim is); at most 3 x 3 as long as eu, ev < 1, which the caller's coordinates satisfy by orders of magnitude
    assert float(np.max(eu)) < 0.5 and float(np.max(ev)) < 0.5
    cl = lambda a, n: np.clip(a, -1, n).astype(np.int64) + 1
    i_lo, j_lo = cl(np.floor(us - eu), W), cl(np.floor(vs - ev), H)
    i_hi, j_hi = cl(np.floor(us + eu) + 1, W), cl(np.floor(vs + ev) + 1, H)
    mx = np.full(val.shape, -np.inf)
    mn = np.full(val.shape, np.inf)
    for dj in range(3):
        for di in range(3):
            j, i = np.minimum(j_lo + dj, j_hi), np.minimum(i_lo + di, i_hi)
            t = pad[j, i]
            mx, mn = np.maximum(mx, t), np.minimum(mn, t)
    D, M = mx - mn, np.maximum(np.abs(mx), np.abs(mn))
    bound = D * (eu + ev)[..., None] * (1.0 + 1e-9) + 8.0 * U * (1.0 + 1e-3) * M
    return val, bound


# ---- the whole rule ---------------------------------------------------------------------------------------------------------------------
def prepare(color, depth, opts, depth_size=None):
    """color [n, Hc, Wc, 3] uint8 / float32 or None, depth [n, Hd, Wd] uint16 / float32 or None
    -> (color_out [n, H', W', 3] float32 or None, depth_out [n, H', W'] float32 or None, intr_out [4] float32, n_border)"""
    o = options(**opts)
    assert color is not None or depth is not None
    if depth is not None:
        Hd, Wd = depth.shape[1:3]
    elif depth_size is not None:
        Hd, Wd = depth_size
    else:
        Hd, Wd = color.shape[1:3]
    Hc, Wc = color.shape[1:3] if color is not None else (Hd, Wd)
    p = plan(o, Hc, Wc, Hd, Wd)
    e = p["e"]
    cut = (lambda a: a[:, e:a.shape[1] - e, e:a.shape[2] - e]) if e > 0 else (lambda a: a)
    c_out = d_out = None
    n_border = 0
    if color is not None:
        c = convert_color(color)
        border = None
        if p["s1"]:
            c, border = undistort_f32(c, o["fx"], o["fy"], o["cx"], o["cy"], o["dist"])
        elif p["s2"]:
            c = resize_half(c, Hd, Wd)
        if p["s3"]:
            if border is not None:
                border = _any4(border, _axis_aligned(Hd, p["Hs"]), _axis_aligned(Wd, p["Ws"]))
            c = resize_aligned(c, p["Hs"], p["Ws"])
        c = cut(c)
        if border is not None:
            n_border = int(cut(border[None]).sum()) * color.shape[0]
        if o["swap_rb"]:
            c = c[..., ::-1]
        c_out = np.ascontiguousarray(c, F)
    if depth is not None:
        d = convert_depth(depth, o["png_depth_scale"], o["scale"])
        if p["s3"]:
            d = resize_nearest(d, p["Hs"], p["Ws"])
        d_out = np.ascontiguousarray(cut(d), F)
    return c_out, d_out, p["intr"], n_border

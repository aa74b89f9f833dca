"""numpy float64 restatement of nsk_image_ssim (include/nsk.h states the rule; csrc/nsk_ssim.h is the device's form) and two independent
forms of the published definition (Wang et al. 2004, with the conventions of pytorch_msssim): torch.nn.functional.conv2d in float64
with the 2-D outer-product window plus avg_pool2d, and scipy.ndimage.correlate1d cropped to the valid region.
tests/test_ssim_cpu.py holds the restatement to both; tests/test_gpu_ssim.py holds the device to the restatement bytes for bytes.

The restatement: every pixel widened to float64 once; the five images x, y, x x, y y, x y filtered along W, then along H, the taps in
increasing index order (acc = g_0 v_0, then acc = acc + g_k v_k); numpy forms every product and sum as an operation of its own."""
import functools
import math

import numpy as np

import rows_checks as rw

STANDARD_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

# (H, W, C, win, sigma, levels): one window; a ragged strip two map rows high; a smaller window with another sigma; several tiles; the
# five-level pyramid whose last level is one window high
SHAPES = [(11, 11, 1, 11, 1.5, 1), (12, 43, 3, 11, 1.5, 1), (40, 33, 2, 7, 1.0, 1), (75, 70, 3, 11, 1.5, 1), (161, 176, 3, 11, 1.5, 5)]
KINDS = ("noise", "smooth", "flat")


def make_pair(kind, H, W, C, seed=0):
    """float32 [H, W, C] images: uniform noise against noise + 0.1 N(0, 1), clipped; a smooth sinusoid against itself + 0.05 N; the flat
    bright pair 0.999 against 0.999 - 1e-3 u (where E[x^2] - mu^2 cancels against C2)"""
    rng = np.random.default_rng(1000 * seed + 7 * H + W + C)
    if kind == "noise":
        a = rng.random((H, W, C))
        b = np.clip(a + 0.1 * rng.standard_normal((H, W, C)), 0.0, 1.0)
    elif kind == "smooth":
        i, j, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        a = 0.5 + 0.4 * np.sin(0.23 * i + 0.5 * c) * np.cos(0.17 * j - 0.3 * c)
        b = a + 0.05 * rng.standard_normal((H, W, C))
    elif kind == "flat":
        a = np.full((H, W, C), 0.999)
        b = 0.999 - 1e-3 * rng.random((H, W, C))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def window(win, sigma):
    """g_k = exp(-(k - win // 2)^2 / (2 sigma^2)) / sum, the sum in index order; math.exp is the C library's, as the host's"""
    g = [math.exp(-(float(k - win // 2) * float(k - win // 2)) / (2.0 * (sigma * sigma))) for k in range(win)]
    s = 0.0
    for v in g:
        s = s + v
    return np.array([v / s for v in g], np.float64)


def filter_valid(v, g):
    """[H, W, C] float64 -> [H - win + 1, W - win + 1, C]: along W, then along H, taps in increasing index order"""
    win = len(g)
    Wm, Hm = v.shape[1] - win + 1, v.shape[0] - win + 1
    r = g[0] * v[:, 0:Wm]
    for k in range(1, win):
        r = r + g[k] * v[:, k:k + Wm]
    o = g[0] * r[0:Hm]
    for k in range(1, win):
        o = o + g[k] * r[k:k + Hm]
    return o


def constants(data_range, k1, k2):
    return (k1 * data_range) * (k1 * data_range), (k2 * data_range) * (k2 * data_range)


def level_maps(x, y, g, C1, C2):
    """(ssim, cs) [Hm, Wm, C] float64 of one level (x, y float64 [H, W, C])"""
    with np.errstate(invalid="ignore", over="ignore"):
        mx, my = filter_valid(x, g), filter_valid(y, g)
        fxx, fyy, fxy = filter_valid(x * x, g), filter_valid(y * y, g), filter_valid(x * y, g)
        mxx, myy, mxy = mx * mx, my * my, mx * my
        sx, sy, sxy = fxx - mxx, fyy - myy, fxy - mxy
        cs = (2.0 * sxy + C2) / ((sx + sy) + C2)
        ssim = ((2.0 * mxy + C1) / ((mxx + myy) + C1)) * cs
    return ssim, cs


def pool(v):
    """level l + 1 of [H, W, C] float64: the 2 x 2 average with p = size mod 2 of zero padding per axis"""
    H, W, C = v.shape
    ph, pw = H % 2, W % 2
    H2, W2 = (H + 2 * ph) // 2, (W + 2 * pw) // 2
    z = np.zeros((2 * H2, 2 * W2, C))
    z[ph:ph + H, pw:pw + W] = v
    with np.errstate(invalid="ignore", over="ignore"):
        return ((z[0::2, 0::2] + z[0::2, 1::2]) + (z[1::2, 0::2] + z[1::2, 1::2])) * 0.25


def terms(ssim, cs):
    """[Hm Wm, 3 C] for rows_checks.reduce: columns 3 c + {0 ssim, 1 cs, 2 count}; a window with a non-finite value is a term of +0.0"""
    Hm, Wm, C = ssim.shape
    take = np.isfinite(ssim) & np.isfinite(cs)
    t = np.zeros((Hm * Wm, C, 3))
    t[:, :, 0] = np.where(take, ssim, 0.0).reshape(-1, C)
    t[:, :, 1] = np.where(take, cs, 0.0).reshape(-1, C)
    t[:, :, 2] = take.reshape(-1, C)
    return t.reshape(Hm * Wm, 3 * C)


def combine(sums, weights):
    """sums [levels, C, 3] -> (result, level-0 SSIM, h_levels [levels, C, 4]); the host's combine: the mean over channels of
    prod_l max(value_l, 0)^w_l, value_l the mean cs of a level, the mean ssim of the last (NaN without a window)"""
    levels, C, _ = sums.shape
    h = np.zeros((levels, C, 4))
    h[:, :, :3] = sums
    ms = s0 = 0.0
    for c in range(C):
        prod = 1.0
        for l in range(levels):
            s = sums[l, c]
            value = float((s[0] if l == levels - 1 else s[1]) / s[2]) if s[2] > 0 else math.nan
            h[l, c, 3] = value
            if levels > 1:
                base = value if value > 0 else (value if math.isnan(value) else 0.0)
                prod = prod * math.pow(base, weights[l])
        s0 = s0 + (float(sums[0, c, 0] / sums[0, c, 2]) if sums[0, c, 2] > 0 else math.nan)
        ms = ms + prod
    s0 = s0 / C
    return (ms / C if levels > 1 else s0), s0, h


def restate(a, b, data_range=1.0, win=11, sigma=1.5, k1=0.01, k2=0.03, levels=1, weights=None):
    """nsk_image_ssim restated -> dict: maps [(ssim, cs)] per level (float64), map (the float32 rounding of the level-0 ssim), sums
    [levels, C, 3] through the row reductions' tree, result, ssim, h_levels, left_out, windows"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.ndim == 2:
        a, b = a[:, :, None], b[:, :, None]
    if weights is None and levels == 5:
        weights = STANDARD_WEIGHTS
    g = window(win, sigma)
    C1, C2 = constants(data_range, k1, k2)
    x, y = a.astype(np.float64), b.astype(np.float64)
    maps, sums, windows = [], [], 0
    for l in range(levels):
        if l > 0:
            x, y = pool(x), pool(y)
        s, cs = level_maps(x, y, g, C1, C2)
        maps.append((s, cs))
        sums.append(rw.reduce(terms(s, cs)).reshape(-1, 3))
        windows += s.size
    sums = np.stack(sums)
    result, s0, h = combine(sums, weights)
    with np.errstate(over="ignore", invalid="ignore"):
        m32 = maps[0][0].astype(np.float32)
    return dict(maps=maps, map=m32, sums=sums, result=result, ssim=s0, h_levels=h, windows=windows, left_out=windows - int(sums[:, :, 2].sum()))


# ---- two independent forms of the published definition -----------------------------------------------------------------------------------
def _plain_window(win, sigma):
    k = np.arange(win, dtype=np.float64) - win // 2
    g = np.exp(-(k ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def _combine_plain(values, weights):
    """values [levels, C]: mean cs per level, mean ssim for the last -> the mean over channels of prod max(v, 0)^w"""
    if len(values) == 1:
        return float(np.mean(values[0]))
    v = np.maximum(np.asarray(values), 0.0)
    return float(np.mean(np.prod(v ** np.asarray(weights, np.float64)[:, None], axis=0)))


def torch_form(a, b, data_range=1.0, win=11, sigma=1.5, k1=0.01, k2=0.03, levels=1, weights=None):
    """conv2d in float64 with the 2-D window g g^T, one group per channel; avg_pool2d(kernel_size=2, padding=size % 2) between levels
    -> (result, level-0 SSIM, level-0 ssim map [Hm, Wm, C])"""
    import torch
    import torch.nn.functional as F
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.ndim == 2:
        a, b = a[:, :, None], b[:, :, None]
    C = a.shape[2]
    if weights is None and levels == 5:
        weights = STANDARD_WEIGHTS
    g = torch.tensor(_plain_window(win, sigma))
    w2 = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1)
    x = torch.tensor(a, dtype=torch.float64).permute(2, 0, 1)[None]
    y = torch.tensor(b, dtype=torch.float64).permute(2, 0, 1)[None]
    C1, C2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    values, map0, ssim0 = [], None, None
    for l in range(levels):
        if l > 0:
            pad = (x.shape[2] % 2, x.shape[3] % 2)
            x, y = F.avg_pool2d(x, kernel_size=2, padding=pad), F.avg_pool2d(y, kernel_size=2, padding=pad)
        f = lambda t: F.conv2d(t, w2, groups=C)
        mx, my = f(x), f(y)
        sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
        cs = (2 * sxy + C2) / (sx + sy + C2)
        s = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
        if l == 0:
            map0, ssim0 = s[0].permute(1, 2, 0).numpy(), float(s.mean(dim=(0, 2, 3)).mean())
        values.append((s if l == levels - 1 else cs).mean(dim=(0, 2, 3)).numpy())
    return _combine_plain(values, weights), ssim0, map0


def scipy_form(a, b, data_range=1.0, win=11, sigma=1.5, k1=0.01, k2=0.03, levels=1, weights=None):
    """scipy.ndimage.correlate1d along both axes, cropped to the valid region; the pooling as a reshape-mean over a zero-padded copy
    -> (result, level-0 SSIM, level-0 ssim map [Hm, Wm, C])"""
    from scipy.ndimage import correlate1d
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.ndim == 2:
        a, b = a[:, :, None], b[:, :, None]
    if weights is None and levels == 5:
        weights = STANDARD_WEIGHTS
    g, h = _plain_window(win, sigma), win // 2
    C1, C2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2

    def f(v):
        o = correlate1d(correlate1d(v, g, axis=0, mode="constant"), g, axis=1, mode="constant")
        return o[h:v.shape[0] - h, h:v.shape[1] - h]

    def down(v):
        H, W, C = v.shape
        z = np.zeros(((H + 2 * (H % 2)) // 2 * 2, (W + 2 * (W % 2)) // 2 * 2, C))       # (of 2 p + size rows the pooling reads an even number)
        z[H % 2:H % 2 + H, W % 2:W % 2 + W] = v
        return z.reshape(z.shape[0] // 2, 2, z.shape[1] // 2, 2, C).mean(axis=(1, 3))
    x, y = a.astype(np.float64), b.astype(np.float64)
    values, map0, ssim0 = [], None, None
    for l in range(levels):
        if l > 0:
            x, y = down(x), down(y)
        mx, my = f(x), f(y)
        sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
        cs = (2 * sxy + C2) / (sx + sy + C2)
        s = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
        if l == 0:
            map0, ssim0 = s, float(s.mean(axis=(0, 1)).mean())
        values.append((s if l == levels - 1 else cs).mean(axis=(0, 1)))
    return _combine_plain(values, weights), ssim0, map0


# ---- computed once, shared by the tests that need them, never written to ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """(a, b, restatement) of one of SHAPES x KINDS"""
    H, W, C, win, sigma, levels = shape
    a, b = make_pair(kind, H, W, C)
    r = restate(a, b, win=win, sigma=sigma, levels=levels)
    for v in (a, b, r["map"], r["sums"], r["h_levels"]):
        v.setflags(write=False)
    return a, b, r

"""numpy restatement of the association of the device's row reductions (csrc/nsk_reduce.h states it) and of what each entry point feeds
into it.  tests/test_rows_cpu.py proves `reduce` against a plain loop over the same tree; tests/test_gpu_rows.py holds the device to it
bytes for bytes.

The tree, for n elements, workgroups of `block` threads (waves of 64 lanes) and at most `cap` rows:
  1. nrows = min(ceil(n / block), cap);
  2. lane t of row b folds the elements b * block + t + j * nrows * block in order of j, starting from +0.0 (an element may bring several
     terms: they are folded in their order before the next element);
  3. the 64 lanes of a wave combine as v = v o v[lane ^ s] for s = 32, 16, 8, 4, 2, 1;
  4. the waves combine as ((w0 o w1) o w2) o w3;
  5. the rows combine in index order (a sum from +0.0, a minimum / maximum from the first row).
A skipped element is a term of +0.0: the accumulator starts at +0.0 and never becomes -0.0, so adding +0.0 leaves its bits alone."""
import numpy as np

SUM, MIN, MAX = "sum", "min", "max"
_OPS = {SUM: np.add, MIN: np.fmin, MAX: np.fmax}          # (fmin / fmax: the device's, which drop a NaN)


def n_rows(n, block=256, cap=1024):
    return min(-(-n // block), cap)


def reduce(terms, ops=None, block=256, cap=1024):
    """terms: float64 [n, COLS] (or [n, K, COLS]: K terms per element, folded in order); ops: one of SUM / MIN / MAX per column (None:
    every column a sum) -> float64 [COLS]"""
    x = np.asarray(terms, np.float64)
    if x.ndim == 2:
        x = x[:, None, :]
    n, K, cols = x.shape
    ops = [SUM] * cols if ops is None else list(ops)
    assert n >= 1 and len(ops) == cols and block % 64 == 0
    nrows = n_rows(n, block, cap)
    per = nrows * block
    J = -(-n // per)
    pad = np.zeros((J * per, K, cols))
    pad[:n] = x
    pad = pad.reshape(J, nrows, block, K, cols)
    out = np.empty(cols)
    for c, name in enumerate(ops):
        op = _OPS[name]
        acc = np.zeros((nrows, block))                      # 2. the lanes
        for j in range(J):
            for k in range(K):
                acc = op(acc, pad[j, :, :, k, c])
        v = acc.reshape(nrows, block // 64, 64)             # 3. the butterfly
        lane = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            v = op(v, v[:, :, lane ^ s])
        w = v[:, 0, 0]                                      # 4. the waves
        for i in range(1, block // 64):
            w = op(w, v[:, i, 0])
        r = 0.0 if name == SUM else w[0]                    # 5. the rows
        for b in range(0 if name == SUM else 1, nrows):
            r = op(r, w[b])
        out[c] = r
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- what each entry point feeds in ---------------------------------------------------------------------------------------------------
def _finite32(x):
    return np.abs(x) < np.float32(np.inf)                   # false for NaN and +-inf


CLOUD_STATS_OPS = (SUM, SUM, SUM, MAX)


def cloud_stats_terms(dist, threshold):
    """[n, 4]: the finite distance, 1, 1 below the threshold, the distance again (for the maximum, which starts from +0.0)"""
    d = np.asarray(dist, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        fin = _finite32(d); below = fin & (d < np.float32(threshold))
    dd = np.where(fin, d, np.float32(0)).astype(np.float64)
    return np.stack([dd, fin.astype(np.float64), below.astype(np.float64), dd], 1)


def image_metrics_terms(rgb, depth, gt_depth, gt_color):
    """[n, 3, 5]: columns as the kernel's (depth pixels, sum |gt - d|, colour components, sum (gt_c - c)^2, non-finite pixels); the three
    colour components of a pixel are three terms"""
    f = np.float32
    c = np.asarray(rgb, f).reshape(-1, 3); d = np.asarray(depth, f).reshape(-1)
    g = np.asarray(gt_depth, f).reshape(-1); gc = np.asarray(gt_color, f).reshape(-1, 3)
    n = len(d)
    out = np.zeros((n, 3, 5))
    with np.errstate(invalid="ignore", over="ignore"):
        good = _finite32(d) & _finite32(c).all(1)
        out[:, 0, 4] = ~good
        has = g > 0
        r = np.where(has, np.abs(g - d), f(0)).astype(f)
        take = good & has & _finite32(r)
        out[:, 0, 0] = take
        out[:, 0, 1] = np.where(take, r, f(0)).astype(np.float64)
        rc = np.abs(gc - c).astype(f)
        takec = good[:, None] & _finite32(rc)
        out[:, :, 2] = takec
        r64 = np.where(takec, rc, f(0)).astype(np.float64)
        out[:, :, 3] = r64 * r64
    return out


def icp_terms(moved, dist, index, target, threshold):
    """[n, 18] from the transformed sources (float32 [n, 3]: icp_checks.transform) and the correspondences: the count, d d, s', t,
    s'_a t_b, and the sources whose s' is not finite"""
    s = np.asarray(moved, np.float32).reshape(-1, 3); d = np.asarray(dist, np.float32).reshape(-1)
    j = np.asarray(index).reshape(-1); t = np.asarray(target, np.float32).reshape(-1, 3)
    out = np.zeros((len(s), 18))
    with np.errstate(invalid="ignore"):
        fin = _finite32(s).all(1)
        take = fin & (j >= 0) & (d <= np.float32(threshold))
    out[:, 17] = ~fin
    sv = s[take].astype(np.float64); tv = t[j[take]].astype(np.float64); dd = d[take].astype(np.float64)
    out[take, 0] = 1.0
    out[take, 1] = dd * dd
    out[take, 2:5] = sv
    out[take, 5:8] = tv
    out[take, 8:17] = (sv[:, :, None] * tv[:, None, :]).reshape(-1, 9)
    return out


def depth_pair_terms(a, b):
    """[n_pix, 4] of one view: |a - b| where finite, 1 where both are hit, |a - b| over those, 1 where a is hit"""
    f = np.float32
    x = np.asarray(a, f).reshape(-1); y = np.asarray(b, f).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(x - y).astype(f)
        fin = _finite32(d); both = (x > 0) & (y > 0)
    d64 = np.where(fin, d, f(0)).astype(np.float64)
    return np.stack([d64, both.astype(np.float64), np.where(both, d64, 0.0), (x > 0).astype(np.float64)], 1)

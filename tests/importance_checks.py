"""Hierarchical importance sampling (include/nsk.h, nsk_set_importance) restated in numpy: the rule in fp32, operation by operation (every
numpy float32 operation rounds on its own, there is no contraction), and the same rule in fp64.  linspace01 and the counter hash are restated
here; nothing of the device path is imported."""
import numpy as np

F = np.float32
_M64 = (1 << 64) - 1


def linspace01(steps, dtype=np.float32):
    """the t of at::linspace(0, 1, steps) as the sampling forms it: step * i in the lower half, 1 - step * (steps - 1 - i) in the upper"""
    T = dtype
    if steps == 1:
        return np.zeros(1, T)
    step = T(1) / T(steps - 1)
    i = np.arange(steps)
    lo = (step * i.astype(T)).astype(T)
    hi = (T(1) - (step * (steps - 1 - i).astype(T)).astype(T)).astype(T)
    return np.where(i < steps // 2, lo, hi).astype(T)


def hash_u32(seed, a, b):
    """the counter hash of the perturbation: 64-bit mix of (seed, a, b), its upper 32 bits"""
    x = (seed ^ (0x9E3779B97F4A7C15 * (a + 1)) ^ (0xC2B2AE3D27D4EB4F * (b + 1))) & _M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _M64
    x ^= x >> 33
    return x >> 32


def u_values(N, Ni, det=True, seed=0, dtype=np.float32):
    """[N, Ni]: step 6"""
    if det:
        return np.broadcast_to(linspace01(Ni, dtype), (N, Ni)).copy()
    u = np.empty((N, Ni), dtype)
    for n in range(N):
        for j in range(Ni):
            u[n, j] = dtype(hash_u32(seed, n, 64 + j) >> 8) * dtype(1.0 / 16777216.0)
    return u


def cdf_of(w, dtype=np.float32):
    """steps 2 - 5 for weights w [N, S1] -> cdf [N, S1 - 1]"""
    T = dtype
    w = np.asarray(w, T)
    N, S1 = w.shape
    assert S1 >= 3
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = (w[:, 1:-1] + T(np.float32(1e-5))).astype(T)                                # 2: [N, S1-2] (the constant is the fp32 one in both forms)
        total = q[:, 0].copy()                                                          # 3
        for k in range(1, S1 - 2):
            total = (total + q[:, k]).astype(T)
        pdf = (q / total[:, None]).astype(T)                                            # 4
        cdf = np.zeros((N, S1 - 1), T)                                                  # 5
        for k in range(S1 - 2):
            cdf[:, k + 1] = (cdf[:, k] + pdf[:, k]).astype(T)
    return cdf


def sample_zs(z, w, u, dtype=np.float32):
    """steps 1 - 11 for rays z, w [N, S1] and u [N, Ni] -> zs [N, Ni]; dtype float32: the rule; float64: the same rule in double"""
    T = dtype
    z = np.asarray(z, T); u = np.asarray(u, T)
    N, S1 = z.shape
    cdf = cdf_of(w, T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bins = (T(0.5) * (z[:, 1:] + z[:, :-1]).astype(T)).astype(T)                    # 1: [N, S1-1]
        inds = (cdf[:, None, :] <= u[:, :, None]).sum(-1)                               # 7: [N, Ni]
        below = np.maximum(inds - 1, 0)                                                 # 8
        above = np.minimum(inds, S1 - 2)
        cb = np.take_along_axis(cdf, below, 1)
        denom = (np.take_along_axis(cdf, above, 1) - cb).astype(T)                      # 9
        denom = np.where(denom < T(np.float32(1e-5)), T(1), denom).astype(T)
        t = ((u - cb).astype(T) / denom).astype(T)                                      # 10
        bb = np.take_along_axis(bins, below, 1)
        ba = np.take_along_axis(bins, above, 1)
        return (bb + (t * (ba - bb).astype(T)).astype(T)).astype(T)                     # 11


def rank_sort(zc):
    """step 12: ascending, ties by position, a NaN as +inf (it keeps its NaN in the output)"""
    key = np.where(np.isnan(zc), np.inf, zc)
    order = np.argsort(key, axis=1, kind="stable")
    return np.take_along_axis(zc, order, 1)


def resample(z, w, Ni, det=True, seed=0):
    """the whole rule in fp32: z, w [N, S1] -> z2 [N, S1 + Ni]"""
    z = np.asarray(z, F); w = np.asarray(w, F)
    zs = sample_zs(z, w, u_values(z.shape[0], Ni, det, seed), np.float32)
    return rank_sort(np.concatenate([z, zs], 1).astype(F))

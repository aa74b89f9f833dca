"""numpy restatements of the reconstruction metrics' rules (include/nsk.h: nsk_mesh_sample, nsk_cloud_nearest, nsk_cloud_stats) and the
scenes their tests share.  tests/test_recon_cpu.py proves these helpers; tests/test_gpu_recon.py holds the device to them."""
import numpy as np


def hash_u32(seed, a, b):
    """hash_u32 of csrc/nsk_device.h on arrays: seed a python int, a / b integers (arrays) below 2^32"""
    with np.errstate(over="ignore"):
        a = np.asarray(a, np.uint64); b = np.asarray(b, np.uint64)
        x = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ (np.uint64(0x9E3779B97F4A7C15) * (a + np.uint64(1))) ^ (np.uint64(0xC2B2AE3D27D4EB4F) * (b + np.uint64(1)))
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xFF51AFD7ED558CCD)
        x = x ^ (x >> np.uint64(33)); x = x * np.uint64(0xC4CEB9FE1A85EC53)
        x = x ^ (x >> np.uint64(33))
    return (x >> np.uint64(32)).astype(np.uint32)


def sample_u(seed, n):
    """u_k = (hash_u32(seed, s, k) >> 8) 2^-24 -> float32 [n, 3]"""
    s = np.arange(n, dtype=np.uint64)
    return np.stack([(hash_u32(seed, s, k) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) for k in range(3)], 1)


def tri_areas(verts, tris):
    """(areas float64 [nt] with 0 for every degenerate triangle, degenerate bool [nt])"""
    verts = np.asarray(verts, np.float32); tris = np.asarray(tris, np.int64)
    ok = ((tris >= 0) & (tris < len(verts))).all(1)
    t = np.where(ok[:, None], tris, 0)
    a, b, c = (verts[t[:, k]].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        ar = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(1))
    good = ok & np.isfinite(ar) & (ar > 0)
    return np.where(good, ar, 0.0), ~good


def cum_sequential(areas):
    return np.cumsum(areas.astype(np.float64))


def cum_blocked(areas, block=64):
    """another association: inclusive sums inside blocks of `block`, plus the sequential sum of the blocks before"""
    n = len(areas)
    pad = np.zeros(-(-n // block) * block); pad[:n] = areas
    inner = np.cumsum(pad.reshape(-1, block), 1)
    base = np.concatenate([[0.0], np.cumsum(inner[:, -1])[:-1]])
    return (inner + base[:, None]).reshape(-1)[:n]


def choose_tris(cum, u0):
    """the first t with cum[t] > (double)u0 cum[last]; also the gap of u0 cum[last] to the nearest cumulative boundary"""
    x = u0.astype(np.float64) * cum[-1]
    t = np.searchsorted(cum, x, side="right")
    tc = np.minimum(t, len(cum) - 1)
    gap = np.minimum(np.abs(cum[tc] - x), np.where(t > 0, np.abs(x - cum[np.maximum(tc - 1, 0)]), np.inf))
    return t.astype(np.int64), gap


def sample_points(verts, tris, tri, u):
    """p = ((1 - r) a + r (1 - u2) b) + r u2 c in float32, one rounding per operation"""
    verts = np.asarray(verts, np.float32); tris = np.asarray(tris, np.int64)
    f = np.float32
    r = np.sqrt(u[:, 1].astype(f)).astype(f)
    wa = (f(1) - r).astype(f); wb = (r * (f(1) - u[:, 2]).astype(f)).astype(f); wc = (r * u[:, 2]).astype(f)
    a, b, c = (verts[tris[tri, k]] for k in range(3))
    return (((wa[:, None] * a).astype(f) + (wb[:, None] * b).astype(f)).astype(f) + (wc[:, None] * c).astype(f)).astype(f)


def sample_mesh(verts, tris, n, seed, cum=None):
    """the whole rule -> (points float32 [n, 3], triangles [n], total area, degenerate count)"""
    ar, deg = tri_areas(verts, tris)
    cum = cum_sequential(ar) if cum is None else cum
    u = sample_u(seed, n)
    tri, _ = choose_tris(cum, u[:, 0])
    return sample_points(verts, tris, tri, u), tri, float(cum[-1]), int(deg.sum())


def brute_nearest(query, target, chunk=256):
    """(dist float32 [nq], index int32 [nq]) by the contract: d2 = (dx dx + dy dy) + dz dz in float32, the lowest index among equal d2,
    non-finite targets left out, non-finite queries NaN / -1, no finite target +inf / -1"""
    f = np.float32
    q = np.asarray(query, f).reshape(-1, 3); t = np.asarray(target, f).reshape(-1, 3)
    keep = np.flatnonzero(np.isfinite(t).all(1))
    dist = np.full(len(q), np.inf, f); idx = np.full(len(q), -1, np.int32)
    qok = np.isfinite(q).all(1)
    if len(keep):
        tk = t[keep]
        with np.errstate(over="ignore", invalid="ignore"):
            # one axis at a time into two reused [chunk, targets] buffers: every operation still rounds to float32 on its own
            tx = [np.ascontiguousarray(tk[:, a]) for a in range(3)]
            acc = np.empty((chunk, len(tk)), f); tmp = np.empty((chunk, len(tk)), f)
            for s in range(0, len(q), chunk):
                qq = np.where(qok[s:s + chunk, None], q[s:s + chunk], f(0))
                m = len(qq)
                for a in range(3):
                    dst = acc if a == 0 else tmp
                    np.subtract(qq[:, a:a + 1], tx[a][None, :], out=dst[:m])
                    np.multiply(dst[:m], dst[:m], out=dst[:m])
                    if a:
                        np.add(acc[:m], tmp[:m], out=acc[:m])
                j = acc[:m].argmin(1)                               # (the first of equal minima: the lowest index)
                dist[s:s + chunk] = np.sqrt(acc[np.arange(m), j]).astype(f)
                idx[s:s + chunk] = keep[j]
    dist[~qok] = np.nan; idx[~qok] = -1
    return dist, idx


def stats(dist, threshold):
    d = np.asarray(dist, np.float32)
    fin = d[np.isfinite(d)]
    return dict(sum=float(fin.astype(np.float64).sum()), count=int(len(fin)), below=int((fin < np.float32(threshold)).sum()),
                max=float(fin.max()) if len(fin) else 0.0)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def sheet(nx=13, ny=11, size=(1.0, 1.0), origin=(0.0, 0.0, 0.0), jitter=0.3, seed=0):
    """a planar grid of nx x ny cells in the plane z = origin[2], two triangles per cell, the inner nodes jittered inside the plane
    -> (verts float32 [(nx + 1)(ny + 1), 3], tris int32 [2 nx ny, 3]).  The default has 286 triangles."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64))
    j = rng.uniform(-jitter, jitter, (2,) + gx.shape)
    inner = (gx > 0) & (gx < nx) & (gy > 0) & (gy < ny)
    x = origin[0] + (gx + j[0] * inner) * size[0] / nx; y = origin[1] + (gy + j[1] * inner) * size[1] / ny
    verts = np.stack([x, y, np.full_like(x, origin[2])], -1).reshape(-1, 3).astype(np.float32)
    i, k = np.meshgrid(np.arange(nx), np.arange(ny))
    v00 = (k * (nx + 1) + i).reshape(-1); v10 = v00 + 1; v01 = v00 + nx + 1; v11 = v01 + 1
    tris = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32)
    return verts, tris


def merge(*meshes):
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(v); ts.append(t + off); off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts).astype(np.int32)


def sheet_clouds(nq, nt, gap=0.03, seed=0):
    """samples of two unit sheets `gap` apart: (query [nq, 3], target [nt, 3])"""
    a = sheet(seed=seed); b = sheet(nx=11, ny=13, origin=(0.0, 0.0, gap), seed=seed + 1)
    return sample_mesh(*a, nq, seed)[0], sample_mesh(*b, nt, seed + 1)[0]

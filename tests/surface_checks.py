"""numpy restatements of the rules of the surface metrics (include/nsk.h: nsk_mesh_nearest, nsk_normal_stats) and the helpers their tests
share.  tests/test_surface_cpu.py proves these helpers; tests/test_gpu_surface.py holds the device to them bytes for bytes."""
import numpy as np

import recon_checks as rc
import rows_checks as rows


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def participating(verts, tris):
    """the indices of the triangles that take part: those to which the sampler gives a positive area"""
    return np.flatnonzero(~rc.tri_areas(verts, tris)[1])


# ---- the rule: every operation below is one numpy operation in `f`, so with f = float32 each is rounded on its own ------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _clamp(p, lo, hi):
    return np.where(p < lo, lo, np.where(p > hi, hi, p))


def _take(best_d2, best_p, q, p, lo, hi, counts=None):
    """one candidate: clamp to the box, d2 = (dx dx + dy dy) + dz dz, taken where strictly smaller"""
    p = _clamp(p, lo, hi)
    d = q - p
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    better = d2 < best_d2
    if counts is not None:
        better &= counts
    return np.where(better, d2, best_d2), np.where(better[..., None], p, best_p)


def tri_candidates(q, a, b, c):
    """q [m, 1, 3] against triangles a, b, c [1, T, 3], all of one dtype -> (d2 [m, T], point [m, T, 3]) of every triangle on its own"""
    f = q.dtype.type
    lo = np.minimum(np.minimum(a, b), c); hi = np.maximum(np.maximum(a, b), c)
    shape = np.broadcast_shapes(q.shape, a.shape)
    best_d2 = np.full(shape[:-1], np.inf, f); best_p = np.full(shape, np.nan, f)
    with np.errstate(all="ignore"):
        e0 = b - a; e1 = c - a
        n = _cross(e0, e1)
        nn = _dot(n, n)
        s = _dot(q - a, n) / nn
        p = q - s[..., None] * n
        inside = (nn > 0) & (_dot(_cross(e0, p - a), n) >= 0) & (_dot(_cross(c - b, p - b), n) >= 0) & (_dot(_cross(a - c, p - c), n) >= 0)
        best_d2, best_p = _take(best_d2, best_p, q, p, lo, hi, inside)
        for u, v in ((a, b), (b, c), (c, a)):
            e = v - u
            ee = _dot(e, e)
            t = _dot(q - u, e) / ee
            t = np.where(ee > 0, np.where(t < 0, f(0), np.where(t > 1, f(1), t)), f(0)).astype(f)
            best_d2, best_p = _take(best_d2, best_p, q, u + t[..., None] * e, lo, hi)
    assert best_d2.dtype == f and best_p.dtype == f
    return best_d2, best_p


def brute_mesh_nearest(query, verts, tris, dtype=np.float32, chunk=256):
    """(dist dtype [nq], tri int32 [nq], point dtype [nq, 3]) by the contract, over all participating triangles: the lowest triangle among
    equal d2; a non-finite query NaN / -1 / NaN; no participating triangle (or no comparable d2) +inf / -1 / NaN.  With dtype float64
    the float32 inputs are widened and the same rule is evaluated in double."""
    f = dtype
    q = np.asarray(query, np.float32).reshape(-1, 3).astype(f)
    V = np.asarray(verts, np.float32).reshape(-1, 3); T = np.asarray(tris, np.int64).reshape(-1, 3)
    keep = participating(V, T)
    nq = len(q)
    dist = np.full(nq, np.inf, f); tri = np.full(nq, -1, np.int32); point = np.full((nq, 3), np.nan, f)
    qok = np.isfinite(q).all(1)
    if len(keep):
        a, b, c = (V[T[keep, k]].astype(f)[None] for k in range(3))
        for s in range(0, nq, chunk):
            qq = np.where(qok[s:s + chunk, None], q[s:s + chunk], f(0))
            d2, p = tri_candidates(qq[:, None, :], a, b, c)
            d2 = np.where(np.isnan(d2), f(np.inf), d2)
            j = d2.argmin(1)                                    # (the first of equal minima: the lowest index)
            r = np.arange(len(qq))
            got = d2[r, j] < np.inf
            dist[s:s + chunk] = np.where(got, np.sqrt(d2[r, j]), f(np.inf)).astype(f)
            tri[s:s + chunk] = np.where(got, keep[j], -1)
            point[s:s + chunk] = np.where(got[:, None], p[r, j], f(np.nan))
    dist[~qok] = np.nan; tri[~qok] = -1; point[~qok] = np.nan
    return dist, tri, point


# ---- an independent closest point: Ericson, Real-Time Collision Detection 5.1.5, the region form, in float64 --------------------------
def ericson_closest(q, a, b, c):
    """q [m, 1, 3], a / b / c [1, T, 3] float64 -> the closest point [m, T, 3] of every triangle"""
    ab = b - a; ac = c - a
    ap = q - a
    d1 = (ab * ap).sum(-1); d2 = (ac * ap).sum(-1)
    bp = q - b
    d3 = (ab * bp).sum(-1); d4 = (ac * bp).sum(-1)
    cp = q - c
    d5 = (ab * cp).sum(-1); d6 = (ac * cp).sum(-1)
    vc = d1 * d4 - d3 * d2; vb = d5 * d2 - d1 * d6; va = d3 * d6 - d5 * d4
    shape = np.broadcast_shapes(q.shape, a.shape)
    out = np.empty(shape); done = np.zeros(shape[:-1], bool)

    def put(mask, value):
        m = mask & ~done
        out[m] = np.broadcast_to(value, shape)[m]
        done[m] = True
    with np.errstate(all="ignore"):
        put((d1 <= 0) & (d2 <= 0), a)
        put((d3 >= 0) & (d4 <= d3), b)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[..., None] * ab)
        put((d6 >= 0) & (d5 <= d6), c)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[..., None] * ac)
        put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b))
        den = 1.0 / (va + vb + vc)
        put(np.ones(shape[:-1], bool), a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None])
    return out


def ericson_mesh_nearest(query, verts, tris):
    """float64 distances [nq] from every query to the mesh by the region form, over the participating triangles"""
    q = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3)
    V = np.asarray(verts, np.float32).astype(np.float64); T = np.asarray(tris, np.int64)
    keep = participating(verts, tris)
    a, b, c = (V[T[keep, k]][None] for k in range(3))
    p = ericson_closest(q[:, None, :], a, b, c)
    return np.sqrt(((q[:, None, :] - p) ** 2).sum(-1)).min(1)


# ---- the grid, in plain numpy: registration by box and the shell walk with the strict stop -----------------------------------------
def _planes(lo, h, dim):
    f = np.float32
    return (f(lo) + (np.arange(dim + 1, dtype=f) * f(h)).astype(f)).astype(f)


def _cell_axis(x, planes, dim):
    """the largest cell k of [0, dim) with P(k) <= x, cell 0 when there is none"""
    if dim == 1:
        return np.zeros(np.shape(x), np.int64)
    return np.maximum(np.searchsorted(planes[:dim], x, side="right") - 1, 0)


def grid_mesh_nearest(query, verts, tris, h, wide_cells=64):
    """the search of nsk_mesh_nearest without its bookkeeping: a grid of edge h over the participating vertices, every triangle
    registered in the cells its box overlaps (more than wide_cells of them: the wide list), every query walking shells of growing
    radius around its own cell and stopping when best < fl(m m) strictly or when the block covers the grid.  What a shell brings is
    evaluated by tri_candidates.  -> (dist, tri, point) float32, and the largest radius any query reached"""
    f = np.float32
    q = np.asarray(query, f).reshape(-1, 3); V = np.asarray(verts, f); T = np.asarray(tris, np.int64)
    keep = participating(V, T)
    a, b, c = (V[T[keep, k]] for k in range(3))
    tlo = np.minimum(np.minimum(a, b), c); thi = np.maximum(np.maximum(a, b), c)
    lo = tlo.min(0); ext = thi.max(0).astype(np.float64) - lo
    h = f(h); inv_h = f(1) / h
    dim = [int(np.floor(ext[k] / float(h))) + 1 if ext[k] >= float(h) else 1 for k in range(3)]
    planes = [_planes(lo[k], h, dim[k]) for k in range(3)]
    c0 = np.stack([_cell_axis(tlo[:, k], planes[k], dim[k]) for k in range(3)], 1)
    c1 = np.stack([_cell_axis(thi[:, k], planes[k], dim[k]) for k in range(3)], 1)
    wide = (c1 - c0 + 1).prod(1) > wide_cells
    nq = len(q)
    dist = np.full(nq, np.inf, f); tri = np.full(nq, -1, np.int32); point = np.full((nq, 3), np.nan, f)
    reach = 0

    def merge(i, sel, state):
        if not sel.any():
            return state
        d2, p = tri_candidates(q[i][None, None, :], a[sel][None], b[sel][None], c[sel][None])
        d2 = np.where(np.isnan(d2[0]), f(np.inf), d2[0])
        j = int(d2.argmin())
        t = int(np.flatnonzero(sel)[j])
        if d2[j] < state[0] or (d2[j] == state[0] and state[1] >= 0 and t < state[1]):
            return (d2[j], t, p[0, j])
        return state
    for i in range(nq):
        state = (f(np.inf), -1, np.full(3, np.nan, f))
        state = merge(i, wide, state)
        cq = [int(np.floor(((q[i, k] - lo[k]).astype(f) * inv_h).astype(f))) if dim[k] > 1 else 0 for k in range(3)]
        r = max(0, max(max(-cq[k], cq[k] - (dim[k] - 1)) for k in range(3)))
        tried = wide.copy()
        while True:
            inblock = np.ones(len(keep), bool)
            for k in range(3):
                inblock &= (c1[:, k] >= cq[k] - r) & (c0[:, k] <= cq[k] + r)
            state = merge(i, inblock & ~tried, state)
            tried |= inblock
            m = f(np.inf)
            for k in range(3):
                if dim[k] == 1:
                    continue
                klo, khi = cq[k] - r, cq[k] + r + 1
                if klo >= 1:
                    m = min(m, max(f(0), (q[i, k] - planes[k][klo]).astype(f)))
                if khi <= dim[k] - 1:
                    m = min(m, max(f(0), (planes[k][khi] - q[i, k]).astype(f)))
            if m == np.inf or state[0] < f(m * m):
                break
            r += 1
        reach = max(reach, r)
        if state[1] >= 0:
            dist[i] = np.sqrt(state[0]); tri[i] = keep[state[1]]; point[i] = state[2]
    return dist, tri, point, reach, int(wide.sum()), dim


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
def _normals(verts, tris, idx):
    """(n float64 [n, 3] by n = (b - a) x (c - a), each operation on its own; ok bool [n])"""
    V = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3); T = np.asarray(tris, np.int64).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < len(T))
    t = T[np.where(ok, idx, 0)] if len(T) else np.zeros((len(idx), 3), np.int64)
    ok &= ((t >= 0) & (t < len(V))).all(1)
    t = np.where(ok[:, None], t, 0)
    if not len(V):
        return np.zeros((len(idx), 3)), np.zeros(len(idx), bool)
    a, b, c = (V[t[:, k]] for k in range(3))
    with np.errstate(all="ignore"):
        return _cross(b - a, c - a), ok


def normal_terms(va, ta, ia, vb, tb, ib):
    """[n, 3]: cos_i = |n_A . n_B| / (|n_A| |n_B|), 1 where the pair counts, 1 where it is skipped"""
    na, oka = _normals(va, ta, ia); nb, okb = _normals(vb, tb, ib)
    with np.errstate(all="ignore"):
        la = np.sqrt(_dot(na, na)); lb = np.sqrt(_dot(nb, nb))
        ok = oka & okb & (la > 0) & (la < np.inf) & (lb > 0) & (lb < np.inf)
        cos = np.where(ok, np.abs(_dot(na, nb)) / (la * lb), 0.0)
    return np.stack([cos, ok.astype(np.float64), (~ok).astype(np.float64)], 1)


def normal_stats(va, ta, ia, vb, tb, ib):
    """dict(sum, count, skipped) in the row reduction's association (rows_checks.reduce)"""
    terms = normal_terms(va, ta, ia, vb, tb, ib)
    s = rows.reduce(terms) if len(terms) else np.zeros(3)
    return dict(sum=float(s[0]), count=int(s[1]), skipped=int(s[2]))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def tilt(verts, angles=(0.3, -0.7, 1.1), shift=(0.0, 0.0, 0.0)):
    """the vertices rotated by angles (rad) about x, then y, then z, and moved by shift, in float64 -> float32"""
    ax, ay, az = angles
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return (np.asarray(verts, np.float64) @ (Rz @ Ry @ Rx).T + np.asarray(shift, np.float64)).astype(np.float32)


ANGLES = (0.3, -0.7, 1.1)


def tilted_sheets(gap=0.03, shift=(0.0, 0.0, 0.0), angles=ANGLES):
    """the default sheet and a second one with the same outline `gap` above it, both tilted and shifted alike -> (mesh, mesh)"""
    v0, t0 = rc.sheet()
    v1, t1 = rc.sheet(nx=11, ny=13, origin=(0.0, 0.0, gap), seed=1)
    return (tilt(v0, angles, shift), t0), (tilt(v1, angles, shift), t1)


def slivers(height):
    """two triangles of base 1 and the given height sharing their long edge"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.4, height, 0], [0.6, -height, 0]], np.float64)
    return tilt(v, ANGLES, (0.2, 0.1, -0.3)), np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def box_queries(verts, n, factor, seed):
    """n points uniform in a box `factor` times the mesh's size around its centre"""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64)
    mid = 0.5 * (v.min(0) + v.max(0)); half = 0.5 * (v.max(0) - v.min(0)).max() * factor
    return (mid + rng.uniform(-half, half, (n, 3))).astype(np.float32)


def write_ply(path, v, t):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), len(t))).encode())
        f.write(np.ascontiguousarray(v, "<f4").tobytes())
        rec = np.zeros(len(t), dtype=[("n", "u1"), ("i", "<i4", 3)]); rec["n"] = 3; rec["i"] = t
        f.write(rec.tobytes())

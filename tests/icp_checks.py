"""numpy restatement of the alignment rule (include/nsk.h: nsk_cloud_pair_sums, nsk_rigid_from_sums, nsk_cloud_icp, nsk_cloud_transform) and
the scene its tests share.  tests/test_icp_cpu.py proves these helpers; tests/test_gpu_icp.py holds the device to them."""
import functools

import numpy as np

import recon_checks as rc


def transform(M, pts):
    """s'_a = ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3] in float64 from the float32 point, one rounding to float32; a point with a
    non-finite component is passed on unchanged"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    ok = np.isfinite(p).all(1)
    d = np.where(ok[:, None], p, np.float32(0)).astype(np.float64)
    out = np.empty_like(p)
    with np.errstate(over="ignore"):
        for a in range(3):
            out[:, a] = (((M[a, 0] * d[:, 0] + M[a, 1] * d[:, 1]) + M[a, 2] * d[:, 2]) + M[a, 3]).astype(np.float32)
    out[~ok] = p[~ok]
    return out


def pairs(S, T, M, threshold):
    """(s' float32 [ns, 3], dist float32 [ns], index int32 [ns], counts bool [ns]) of one evaluation"""
    sp = transform(M, S)
    dist, idx = rc.brute_nearest(sp, T)
    with np.errstate(invalid="ignore"):
        counts = np.isfinite(sp).all(1) & (idx >= 0) & (dist <= np.float32(threshold))
    return sp, dist, idx, counts


def sums_of(sp, dist, idx, counts, T):
    """the 17 pair sums in float64 (numpy's own summation order: compare with a relative tolerance)"""
    s = sp[counts].astype(np.float64); t = np.asarray(T, np.float32).reshape(-1, 3)[idx[counts]].astype(np.float64)
    d = dist[counts].astype(np.float64)
    out = np.zeros(17)
    out[0] = counts.sum(); out[1] = (d * d).sum(); out[2:5] = s.sum(0); out[5:8] = t.sum(0)
    out[8:17] = (s[:, :, None] * t[:, None, :]).sum(0).reshape(9)
    return out


def pair_sums(S, T, M, threshold):
    sp, dist, idx, counts = pairs(S, T, M, threshold)
    return sums_of(sp, dist, idx, counts, T), dist, idx


def kabsch(sums):
    """the rigid update of the rule from the 17 sums with numpy's SVD -> (U [4, 4] float64, rank)"""
    sums = np.asarray(sums, np.float64)
    U4 = np.eye(4)
    n = sums[0]
    if not n > 0:
        return U4, 0
    ms, mt = sums[2:5] / n, sums[5:8] / n
    Cm = sums[8:17].reshape(3, 3) / n - np.outer(ms, mt)
    Us, sig, Vt = np.linalg.svd(Cm)
    V = Vt.T
    rank = int((sig > 1e-12 * sig[0]).sum()) if sig[0] > 0 else 0
    d = 1.0 if np.linalg.det(V @ Us.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ Us.T
    U4[:3, :3] = R; U4[:3, 3] = mt - R @ ms
    return U4, rank


def mul4(A, B):
    """A B with every product and sum on its own, k ascending"""
    out = np.empty((4, 4))
    for i in range(4):
        for j in range(4):
            acc = A[i, 0] * B[0, j]
            for k in range(1, 4):
                acc = acc + A[i, k] * B[k, j]
            out[i, j] = acc
    return out


def icp(S, T, threshold=0.1, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, init=None, solve=kabsch):
    """the loop of the rule -> (M, info); info["history"] holds (fitness, rmse) of every evaluation, info["margin"] the smallest
    |d - threshold| in float32 ulps of the threshold over all sources and evaluations"""
    M = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    ns = len(S)
    th = np.float32(threshold)
    ulp = float(np.spacing(th))
    margin = np.inf

    def evaluate(M):
        nonlocal margin
        sp, dist, idx, counts = pairs(S, T, M, threshold)
        fin = np.isfinite(dist)
        if fin.any():
            margin = min(margin, float(np.abs(dist[fin].astype(np.float64) - float(th)).min()) / ulp)
        s = sums_of(sp, dist, idx, counts, T)
        return s, s[0] / ns, (np.sqrt(s[1] / s[0]) if s[0] > 0 else 0.0)

    s, fit, err = evaluate(M)
    hist = [(fit, err)]
    updates, converged, degenerate = 0, False, False
    while updates < max_iter and s[0] > 0:
        U, rank = solve(s)
        degenerate |= rank <= 1
        M = mul4(U, M); updates += 1
        s, f2, e2 = evaluate(M)
        hist.append((f2, e2))
        still = abs(f2 - fit) < rel_fitness and abs(e2 - err) < rel_rmse
        fit, err = f2, e2
        if s[0] > 0 and still:
            converged = True
            break
    return M, dict(iterations=updates, fitness=fit, rmse=err, correspondences=int(s[0]), converged=converged, degenerate=bool(degenerate),
                   history=hist, margin=margin)


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
def height(x, y):
    """a heightfield over the unit square that constrains all six freedoms"""
    return 0.1 * np.sin(3 * x) + 0.05 * np.cos(5 * y) + 0.1 * x * y


def motion(deg, axis, trans):
    """the 4x4 of a rotation by deg degrees about axis (through the origin) followed by the translation trans"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = trans
    return M


def corner_shift(A, B, lo=(0.0, 0.0, -0.15), hi=(1.0, 1.0, 0.25)):
    """the largest distance between A c and B c over the corners c of the scene's box"""
    c = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    return float(np.linalg.norm((c @ np.asarray(A).T - c @ np.asarray(B).T)[:, :3], axis=1).max())


NT, NS = 4000, 5000
MOVE = motion(1.5, (0.5, -0.3, 0.8), (0.012, -0.011, 0.012))      # about 1.5 degrees about an oblique axis and about 2 cm


def heightfield_points(n, seed):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    return np.stack([x, y, height(x, y)], 1).astype(np.float32)


def scene():
    """(source [NS, 3], target [NT, 3], truth).  The source is the target's own points -- each once, in another order, and 1000 of them a
    second time -- moved by MOVE, so truth = MOVE^-1 is what the alignment should find.  Every source has an exact partner: once the
    correspondences are right the next solve is exact and the loop stops on a step of 1e-9, not on one that hovers about the tolerance (two
    samplings of the surface from different seeds slide towards each other with steps that shrink by a fifth per update and cross 1e-6
    slowly: test_icp_cpu.py asserts the conditions that rule such a scene out)."""
    T = heightfield_points(NT, 23)
    rng = np.random.default_rng(102)
    pick = np.concatenate([rng.permutation(NT), rng.integers(0, NT, NS - NT)])
    return transform(MOVE, T[pick]), T, np.linalg.inv(MOVE)


@functools.lru_cache(maxsize=None)
def scene_icp():
    """the restatement's result on the scene, computed once for all tests: (M, info)"""
    S, T, _ = scene()
    return icp(S, T)


def heightfield_mesh(nx, ny, seed=None, jitter=0.3):
    """the heightfield as a triangle mesh: rc.sheet's grid over the unit square (the inner nodes jittered with `seed`), lifted onto it"""
    v, t = rc.sheet(nx, ny, jitter=jitter if seed is not None else 0.0, seed=seed or 0)
    v = v.astype(np.float64)
    v[:, 2] = height(v[:, 0], v[:, 1])
    return v.astype(np.float32), t


def mesh_scene(nx=31, ny=29):
    """the end-to-end scene: gt = the heightfield mesh; rec0 = the same surface re-triangulated (its vertices in another order, every cell
    cut along the other diagonal); rec = rec0 moved by MOVE.  -> (gt, rec0, rec, truth), each mesh (verts float32, tris int32)"""
    gv, gt = heightfield_mesh(nx, ny, seed=0)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(gv))                                # new index -> old index
    inv = np.argsort(perm)
    i, k = np.meshgrid(np.arange(nx), np.arange(ny))
    v00 = (k * (nx + 1) + i).reshape(-1); v10 = v00 + 1; v01 = v00 + nx + 1; v11 = v01 + 1
    tris = inv[np.concatenate([np.stack([v00, v10, v01], 1), np.stack([v10, v11, v01], 1)])].astype(np.int32)
    rv0 = gv[perm]
    return (gv, gt), (rv0, tris), (transform(MOVE, rv0), tris), np.linalg.inv(MOVE)


@functools.lru_cache(maxsize=None)
def mesh_scene_icp():
    """the restatement on the end-to-end scene's vertices: (M, info, e_mesh = its residual displacement over the box's corners)"""
    gt, _, rec, truth = mesh_scene()
    M, info = icp(rec[0], gt[0])
    return M, info, corner_shift(M, truth)

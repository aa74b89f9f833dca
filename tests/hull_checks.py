"""The rule of nsk_points_hull and nsk_lattice_in_hull (include/nsk.h) restated with numpy and Python integers, the exact checks a hull
has to pass whatever produced it, and the seeded clouds the hull tests share.

The restatement is independent of the library: it keeps each face's outside set as an index array and moves points between them, where
the library walks one list of outside points on the device and keeps the face table on the host.  Every decision is an int64 (numpy) or
Python integer comparison, so there is nothing to tolerate: the library's vertices, faces and counts equal these."""
import numpy as np

QMAX = (1 << 20) - 1


# ---- the clouds ------------------------------------------------------------------------------------------------------------------------
def cloud(name, seed=0):
    """a seeded float32 cloud [n, 3] by name"""
    r = np.random.default_rng(seed)
    if name == "lattice5":                      # every tie rule matters: 125 points, 98 of them on the boundary, 8 corners
        g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
        return r.permutation(g).astype(np.float32)
    if name == "ball2000":
        d = r.normal(size=(2000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return (d * r.random((2000, 1)) ** (1 / 3) * 1.7 + [0.3, -0.2, 1.1]).astype(np.float32)
    if name == "sphere300":                     # every point is a hull vertex
        d = r.normal(size=(300, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True) * 2.5).astype(np.float32)
    if name == "box70000":
        return (r.random((70000, 3)) * [4.0, 3.0, 2.5] - [2.0, 1.5, 0.5]).astype(np.float32)
    if name == "repeated":                      # 50 points, three times each
        p = (r.random((50, 3)) * 3.0 - 1.0).astype(np.float32)
        return np.concatenate([p, p, p])[r.permutation(150)]
    if name == "walls":                         # 5000 points on the six lattice-aligned walls of a room, on a 1/8 lattice
        n = np.array([40, 28, 20])
        p = r.integers(0, n + 1, size=(5000, 3))
        a = r.integers(0, 3, size=5000)
        p[np.arange(5000), a] = r.integers(0, 2, size=5000) * n[a]
        return (p * 0.125 - [2.5, 1.75, 0.0]).astype(np.float32)
    raise KeyError(name)


def flat_cloud(rank):
    """a line (rank 1) or a plane (rank 2) that stays one after the quantisation: integer coordinates with an extent of 15, which divides
    2^20 - 1, so the quantised coordinates are 69905 times the integers"""
    if rank == 1:
        return (np.outer(np.arange(16), [1.0, 1.0, -1.0]) + [2.0, -7.0, 15.0]).astype(np.float32)
    return np.array([[x, y, 15 - x - y] for x in range(16) for y in range(16 - x)], np.float32)


GENERAL = ("ball2000", "sphere300", "box70000")            # general position: the vertex set is unique
CLOUDS = ("lattice5",) + GENERAL + ("repeated", "walls")


# ---- the hull rule -----------------------------------------------------------------------------------------------------------------------
def quantise(points):
    """steps 1 and 2 -> (q [N, 3] int64, finite [N] bool, E, lo [3]); q is None without a finite point or with E == 0"""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    finite = np.isfinite(p).all(axis=1)
    if not finite.any():
        return None, finite, 0.0, None
    pd = p.astype(np.float64)
    lo, hi = pd[finite].min(0), pd[finite].max(0)
    E = float((hi - lo).max())
    if E == 0.0:
        return None, finite, 0.0, lo
    s = np.float64(QMAX) / np.float64(E)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint((np.where(finite[:, None], pd, 0.0) - lo) * s).astype(np.int64)
    return q, finite, E, lo


def _first_max(score, finite):
    s = np.where(finite, score, -1)
    return int(np.argmax(s)), int(s.max())


def _normal(q, a, b, c):
    return np.cross(q[b] - q[a], q[c] - q[a])


def hull(points, extra=None):
    """nsk_points_hull -> dict(vertices int32 [nv], faces int32 [nf, 3], info int64 [8] (info[7] = 0: the re-compactions are the
    library's business), q, finite)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if extra is not None:
        p = np.concatenate([p, np.asarray(extra, np.float32).reshape(-1, 3)])
    info = np.zeros(8, np.int64)
    out = dict(vertices=np.zeros(0, np.int32), faces=np.zeros((0, 3), np.int32), info=info, q=None, finite=None)
    if p.shape[0] == 0:
        return out
    q, finite, E, _ = quantise(p)
    out["q"], out["finite"] = q, finite
    info[0], info[1] = int(finite.sum()), int((~finite).sum())
    if q is None:
        return out
    info[6] = np.array([E / QMAX], np.float64).view(np.int64)[0]
    # step 4
    key = (q[:, 0] << 40) | (q[:, 1] << 20) | q[:, 2]
    i0 = int(np.argmin(np.where(finite, key, np.int64(1) << 62)))
    d = q - q[i0]
    i1, m = _first_max((d * d).sum(1), finite)
    if m == 0:
        return out
    info[2] = 1
    i2, m = _first_max(np.abs(np.cross(q[i1] - q[i0], d)).max(1), finite)
    if m == 0:
        return out
    info[2] = 2
    n012 = _normal(q, i0, i1, i2)
    i3, m = _first_max(np.abs(d @ n012), finite)
    if m == 0:
        return out
    info[2] = 3
    if int((q[i3] - q[i0]) @ n012) > 0:
        i1, i2 = i2, i1
    faces = [(i0, i1, i2), (i0, i3, i1), (i1, i3, i2), (i2, i3, i0)]
    live = [True] * 4
    normals = [_normal(q, *f) for f in faces]
    edge = {}
    for f, (a, b, c) in enumerate(faces):
        edge[(a, b)] = f; edge[(b, c)] = f; edge[(c, a)] = f
    # step 5
    outside = []
    rest = np.flatnonzero(finite)
    for f in range(4):
        on = (q[rest] - q[faces[f][0]]) @ normals[f] > 0
        outside.append(rest[on])
        rest = rest[~on]
    # step 6
    F, insertions = 0, 0
    while True:
        while F < len(faces) and not (live[F] and outside[F].size):
            F += 1
        if F == len(faces):
            break
        pts = outside[F]
        det = (q[pts] - q[faces[F][0]]) @ normals[F]
        apex = int(pts[det == det.max()].min())
        lv = np.flatnonzero(np.array(live))
        A = q[np.array([faces[f][0] for f in lv])]
        N = np.array([normals[f] for f in lv])
        visible = [int(f) for f in lv[((q[apex] - A) * N).sum(1) > 0]]
        vset = set(visible)
        new = []
        for f in visible:
            a, b, c = faces[f]
            for u, v in ((a, b), (b, c), (c, a)):
                if edge[(v, u)] not in vset:
                    new.append((u, v, apex))
        moved = np.sort(np.concatenate([outside[f] for f in visible]))
        moved = moved[moved != apex]
        for f in visible:
            live[f] = False
            outside[f] = np.zeros(0, np.int64)
            a, b, c = faces[f]
            del edge[(a, b)], edge[(b, c)], edge[(c, a)]
        for (u, v, w) in new:
            f = len(faces)
            faces.append((u, v, w)); live.append(True); normals.append(_normal(q, u, v, w))
            edge[(u, v)] = f; edge[(v, w)] = f; edge[(w, u)] = f
            on = (q[moved] - q[u]) @ normals[f] > 0
            outside.append(moved[on])
            moved = moved[~on]
        insertions += 1
    tri = np.array([faces[f] for f in range(len(faces)) if live[f]], np.int32).reshape(-1, 3)
    out["faces"] = tri
    out["vertices"] = np.unique(tri).astype(np.int32)
    info[3], info[4], info[5] = out["vertices"].size, tri.shape[0], insertions
    return out


# ---- exact checks of any hull over the quantised points ---------------------------------------------------------------------------------
def _ints(q):
    return [tuple(int(x) for x in row) for row in np.asarray(q)]


def det_int(a, b, c, p):
    """((b - a) x (c - a)) . (p - a) in Python integers"""
    ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    vx, vy, vz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
    return (uy * vz - uz * vy) * (p[0] - a[0]) + (uz * vx - ux * vz) * (p[1] - a[1]) + (ux * vy - uy * vx) * (p[2] - a[2])


def closed_manifold(faces):
    """every directed edge once, its twin once, V - E + F = 2, one component"""
    faces = np.asarray(faces).reshape(-1, 3)
    directed = set()
    for a, b, c in faces.tolist():
        for e in ((a, b), (b, c), (c, a)):
            if e in directed or e[0] == e[1]:
                return False
            directed.add(e)
    if any((v, u) not in directed for (u, v) in directed):
        return False
    V, E, F = np.unique(faces).size, len(directed) // 2, faces.shape[0]
    return V - E + F == 2


def points_outside(q, finite, faces):
    """the number of (finite point, face) pairs with det > 0: int64 numpy per face, which the bound on the coordinates keeps exact, and
    Python integers on the pairs closest to a violation"""
    q = np.asarray(q, np.int64)
    idx = np.flatnonzero(finite)
    bad = 0
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        d = (q[idx] - q[a]) @ np.cross(q[b] - q[a], q[c] - q[a])
        k = int(np.argmax(d))
        assert int(d[k]) == det_int(*_ints(q[[a, b, c, idx[k]]]))
        bad += int((d > 0).sum())
    return bad


def volume6(q, faces):
    """six times the enclosed volume, exactly"""
    rows = _ints(q)
    o = (0, 0, 0)
    return sum(-det_int(rows[a], rows[b], rows[c], o) for a, b, c in np.asarray(faces).reshape(-1, 3).tolist())


# ---- the mask -------------------------------------------------------------------------------------------------------------------------
def mask_planes(xyz, faces_local, scale):
    """the scaled hull's planes -> (n [nf, 3], A' [nf, 3], box lo [3], box hi [3]) in float64; xyz: the hull vertices' float32
    coordinates in ascending index order, faces_local: positions in it"""
    V = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    c = np.cumsum(V, axis=0)[-1] / np.float64(V.shape[0])          # (cumsum adds left to right; np.sum pairs)
    Vs = c + np.float64(scale) * (V - c)
    f = np.asarray(faces_local).reshape(-1, 3)
    A, B, C = Vs[f[:, 0]], Vs[f[:, 1]], Vs[f[:, 2]]
    u, v = B - A, C - A
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    return n, A, Vs.min(0), Vs.max(0)


def lattice_points(origin, step, nx, ny, nz):
    """the node points as nsk_eval_lattice forms them (float32: the product rounded, then the sum), [nz, ny, nx, 3] float64"""
    o, s = np.asarray(origin, np.float32), np.asarray(step, np.float32)
    ax = [o[a] + np.arange(n).astype(np.float32) * s[a] for a, n in enumerate((nx, ny, nz))]
    P = np.empty((nz, ny, nx, 3), np.float64)
    P[..., 0] = ax[0][None, None, :]; P[..., 1] = ax[1][None, :, None]; P[..., 2] = ax[2][:, None, None]
    return P


def lattice_in_hull(origin, step, nx, ny, nz, xyz, faces_local, scale, want_margin=False):
    """nsk_lattice_in_hull -> uint8 [nz, ny, nx] (and, asked for, each node's smallest distance to a face's plane)"""
    P = lattice_points(origin, step, nx, ny, nz)
    if len(faces_local) == 0:
        z = np.zeros((nz, ny, nx), np.uint8)
        return (z, np.full((nz, ny, nx), np.inf)) if want_margin else z
    n, A, lo, hi = mask_planes(xyz, faces_local, scale)
    inside = ((P >= lo) & (P <= hi)).all(-1)
    margin = np.full((nz, ny, nx), np.inf)
    for k in range(n.shape[0]):
        w = P - A[k]
        s = (w[..., 0] * n[k, 0] + w[..., 1] * n[k, 1]) + w[..., 2] * n[k, 2]
        inside &= ~(s > 0)
        if want_margin:
            margin = np.minimum(margin, np.abs(s) / np.linalg.norm(n[k]))
    out = inside.astype(np.uint8)
    return (out, margin) if want_margin else out


def local_faces(vertices, faces):
    """faces as positions in the ascending vertex list"""
    return np.searchsorted(np.asarray(vertices), np.asarray(faces)).astype(np.int32)

"""The rule of nsk_mesh_vertex_normals and nsk_normal_rays (include/nsk.h) restated in numpy, operation by operation, and the meshes the
tests of both run on.  numpy rounds every elementwise product, difference and sum on its own (no FMA), and np.add.at adds its operands one
after the other in the order given: the sequential, in-order sum the rule asks for."""
import numpy as np

import raster_checks as rc

f32 = np.float32


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def face_normals(verts, tris, dtype=np.float32):
    """n_t = (b - a) x (c - a), each component fl(fl(xy) - fl(zw)) -> (n [nt, 3] with NaN rows for an index out of range, take [nt]: the
    triangles that take part)"""
    v = np.asarray(verts, np.float32).astype(dtype).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    nv = len(v)
    inside = ((t >= 0) & (t < nv)).all(axis=1)
    n = np.full((len(t), 3), np.nan, dtype)
    ti = t[inside]
    if len(ti) and nv:
        a, b, c = v[ti[:, 0]], v[ti[:, 1]], v[ti[:, 2]]
        with np.errstate(invalid="ignore", over="ignore"):
            e0, e1 = b - a, c - a
            n[inside] = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1],
                                  e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2],
                                  e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], axis=1)
    return n, inside & np.isfinite(n).all(axis=1)


def vertex_normals(verts, tris, dtype=np.float32):
    """-> (normals [nv, 3] of dtype, info = [triangles left out, vertices without a normal, the largest number of namings, 0])"""
    nv = len(np.asarray(verts).reshape(-1, 3))
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    n, take = face_normals(verts, t, dtype)
    corners = t[take].reshape(-1)                           # (triangle, corner) in ascending order: triangle-major
    acc = np.zeros((nv, 3), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(acc, corners, np.repeat(n[take], 3, axis=0))
        nn = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
        zero = ~(np.isfinite(nn) & (nn > 0))
        out = acc / np.sqrt(nn)[:, None]
    out[zero] = 0
    valence = int(np.bincount(corners, minlength=max(nv, 1)).max()) if len(corners) else 0
    return out.astype(dtype), [int(len(t) - take.sum()), int(zero.sum()), valence, 0]


def normal_rays(verts, normals, length):
    """-> (rays_o [n, 3], rays_d [n, 3], gt_depth [n], has_ray [n] uint8), float32"""
    v, n = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)
    ok = np.isfinite(v).all(axis=1) & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.where(ok[:, None], v + f32(length) * n, v).astype(np.float32)
        d = np.where(ok[:, None], -n, np.array([0, 0, -1], np.float32)).astype(np.float32)
    return o, d, np.full(len(v), length, np.float32), ok.astype(np.uint8)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def uv_sphere(rings=15, sectors=24, radius=0.8, centre=(0.3, -0.2, 0.5)):
    """a closed, welded sphere wound outwards: two poles named by `sectors` triangles each, `rings` rings of `sectors` vertices
    (15 x 24: 362 vertices, 720 triangles)"""
    th = np.pi * np.arange(1, rings + 1) / (rings + 1)
    ph = 2 * np.pi * np.arange(sectors) / sectors
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.cos(th)[:, None] * np.ones(sectors)[None]], -1)
    v = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    idx = lambda r, s: 1 + r * sectors + s % sectors
    south = 1 + rings * sectors
    t = []
    for s in range(sectors):
        t.append((0, idx(0, s), idx(0, s + 1)))
        for r in range(rings - 1):
            t.append((idx(r, s), idx(r + 1, s), idx(r + 1, s + 1)))
            t.append((idx(r, s), idx(r + 1, s + 1), idx(r, s + 1)))
        t.append((south, idx(rings - 1, s + 1), idx(rings - 1, s)))
    return v.astype(np.float32), np.array(t, np.int32)


def fan(n=1000, seed=5):
    """one hub named by n triangles -- more than a workgroup has threads -- around an uneven rim of n + 1 vertices"""
    rng = np.random.default_rng(seed)
    a = 1.9 * np.pi * np.arange(n + 1) / n
    r = rng.uniform(0.8, 1.2, n + 1)
    rim = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.2, 0.2, n + 1)], -1)
    v = np.concatenate([[[0.0, 0.0, 0.1]], rim]).astype(np.float32)
    k = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + k, 2 + k], 1).astype(np.int32)


DIRTY_INFO = [3, 6, 8, 0]           # what the construction below implies: left out, without a normal, most namings


def dirty_mesh():
    """raster_checks.blob() (121 vertices, 200 triangles, an interior vertex named by 6) with every defect the rule speaks of:
      vertex 121           isolated: no normal
      vertex 122           a NaN component; its one triangle (122, 0, 1) is left out: no normal
      vertices 123 .. 126  collinear; the triangles (123, 124, 125), (126, 123, 124), (126, 124, 125) have no area and take part: no normal
      triangle (60, 60, 17)    names the interior vertex 60 twice, takes part with an exactly zero normal: 60 is named 8 times
      triangles (-1, 3, 4), (2, 127, 7)    an index of -1 and one of n_vertices: left out"""
    v, t = rc.blob()
    assert len(v) == 121 and len(t) == 200 and int(np.bincount(t.reshape(-1)).max()) == 6 and int(np.bincount(t.reshape(-1))[60]) == 6
    extra_v = np.array([[0.2, 0.1, 2.0], [np.nan, 0.5, 0.5], [3, 0, 0], [4, 0, 0], [5, 0, 0], [6, 0, 0]], np.float32)
    v = np.concatenate([v, extra_v])
    nv = len(v)
    extra_t = np.array([[122, 0, 1], [123, 124, 125], [126, 123, 124], [126, 124, 125], [60, 60, 17], [-1, 3, 4], [2, nv, 7]], np.int32)
    # the defects sit between the good triangles, not behind them
    t = np.concatenate([t[:50], extra_t[:3], t[50:120], extra_t[3:5], t[120:], extra_t[5:]]).astype(np.int32)
    return v, t


def shuffled(tris, seed=11):
    return np.ascontiguousarray(np.asarray(tris)[np.random.default_rng(seed).permutation(len(tris))])


def read_ply(path):
    """a PLY of Mesher::write_ply: float x y z, [float nx ny nz], [uchar red green blue], list uchar int vertex_indices
    -> (xyz, normals or None, rgb or None, triangles)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    nv = nf = 0
    props, cur = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            cur = w[1]
            if cur == "vertex":
                nv = int(w[2])
            elif cur == "face":
                nf = int(w[2])
        elif w[0] == "property" and cur == "vertex":
            props.append((w[1], w[2]))
        elif w[0] == "property" and cur == "face":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"], ln
    P, N, C = [("float", k) for k in "xyz"], [("float", "n" + k) for k in "xyz"], [("uchar", k) for k in ("red", "green", "blue")]
    has_n = props[3:6] == N
    has_c = props[3 + 3 * has_n:] == C
    assert props == P + (N if has_n else []) + (C if has_c else []), props
    vdt = np.dtype([("p", "<f4", 3)] + ([("n", "<f4", 3)] if has_n else []) + ([("c", "u1", 3)] if has_c else []))
    v = np.frombuffer(data, vdt, nv, end)
    off = end + nv * vdt.itemsize
    fdt = np.dtype([("k", "u1"), ("i", "<i4", 3)])
    fa = np.frombuffer(data, fdt, nf, off)
    assert off + nf * fdt.itemsize == len(data), "trailing bytes"
    assert (fa["k"] == 3).all()
    return v["p"].copy(), (v["n"].copy() if has_n else None), (v["c"].copy() if has_c else None), fa["i"].copy()

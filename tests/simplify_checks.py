"""The rule of nsk_mesh_simplify (include/nsk.h) restated in numpy, one int64 / float64 operation per operation of the rule, and the small
meshes the simplification tests share.  Nothing here imports the product.

  1. cell finite and > 0; a vertex with a non-finite coordinate is left out; a triangle with an index out of range or naming such a
     vertex is invalid;
  2. lo / hi: the finite vertices' box in float64;  g = (float64(p) - lo) / float64(cell);  c = floor(g);  n = c(hi) + 1;
     cell index (c_z n_y + c_y) n_x + c_x;  more than 2^28 cells, or more than 2^21 - 1 along an axis: SimplifyError;
  3. q = rint((g - c) 2^20) (to even);  per cell count and sums of q over all its finite vertices in int64;  m = sum / count;
     position float32(lo + (c + m / 2^20) cell);
  4. collapsed: two corners in one cell;  duplicate (unless keep_duplicates): an earlier survivor with the same corner cells in the
     same cyclic order;  the mirrored triple is none;
  5. output vertices: the cells a kept triangle names, ascending;  vertex_map: the output vertex of every input vertex or -1;
  6. info: finite, left out, invalid, collapsed, duplicates, occupied cells, cells, n_x | n_y << 21 | n_z << 42."""
import numpy as np

F = np.float32
MAX_CELLS = 1 << 28
MAX_AXIS = (1 << 21) - 1
FRAC = float(1 << 20)


class SimplifyError(ValueError):
    pass


def rotate_smallest_first(tri):
    """[n, 3] -> the same cyclic triples with their smallest entry in front"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    m = np.argmin(tri, axis=1)
    r = np.arange(len(tri))
    return np.stack([tri[r, m], tri[r, (m + 1) % 3], tri[r, (m + 2) % 3]], 1)


def simplify(verts, tris, cell, keep_duplicates=False):
    """-> dict(verts [m, 3] float32, tris [k, 3] int32, vertex_map [nv] int32, info [8] int64, cell_of_vertex [nv] int64 (-1: left out))"""
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    cell = F(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise SimplifyError("cell = %r" % cell)
    nv, nt = len(v), len(t)
    info = np.zeros(8, np.int64)
    fin = np.isfinite(v).all(axis=1)
    info[0], info[1] = fin.sum(), nv - fin.sum()
    vcell = np.full(nv, -1, np.int64)
    out = dict(verts=np.zeros((0, 3), F), tris=np.zeros((0, 3), np.int32), vertex_map=np.full(nv, -1, np.int32), info=info, cell_of_vertex=vcell,
               named_cells=np.zeros(0, np.int64))
    if info[0] == 0:
        info[2] = nt
        return out
    cd = np.float64(cell)
    lo, hi = v[fin].min(axis=0).astype(np.float64), v[fin].max(axis=0).astype(np.float64)
    top = np.floor((hi - lo) / cd)                                  # c(hi), still a float: it may be past int64
    cells = int(top[0] + 1) * int(top[1] + 1) * int(top[2] + 1)     # (Python integers)
    if cells > MAX_CELLS:
        raise SimplifyError("%d cells" % cells)
    n = top.astype(np.int64) + 1
    if n.max() > MAX_AXIS:
        raise SimplifyError("%s cells per axis" % n)
    g = (v[fin].astype(np.float64) - lo) / cd
    c = np.floor(g)
    q = np.rint((g - c) * FRAC).astype(np.int64)
    c = c.astype(np.int64)
    assert (c >= 0).all() and (c < n).all()
    cidx = (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0]
    vcell[fin] = cidx
    occupied, rank = np.unique(cidx, return_inverse=True)            # ascending cell index
    rank = rank.reshape(-1)
    count = np.bincount(rank, minlength=len(occupied)).astype(np.int64)
    sums = np.zeros((len(occupied), 3), np.int64)
    for a in range(3):
        np.add.at(sums[:, a], rank, q[:, a])
    m = sums.astype(np.float64) / count.astype(np.float64)[:, None]
    oc = np.stack([occupied % n[0], (occupied // n[0]) % n[1], occupied // (n[0] * n[1])], 1)
    with np.errstate(over="ignore"):
        pos = (lo + (oc.astype(np.float64) + m / FRAC) * cd).astype(F)
    info[5], info[6], info[7] = len(occupied), cells, int(n[0]) | (int(n[1]) << 21) | (int(n[2]) << 42)
    # triangles
    t64 = t.astype(np.int64)
    inr = ((t64 >= 0) & (t64 < nv)).all(axis=1)
    tc = np.full((nt, 3), -1, np.int64)
    tc[inr] = vcell[t64[inr]]
    valid = inr & (tc >= 0).all(axis=1)
    collapsed = valid & ((tc[:, 0] == tc[:, 1]) | (tc[:, 1] == tc[:, 2]) | (tc[:, 0] == tc[:, 2]))
    surv = valid & ~collapsed
    info[2], info[3] = (~valid).sum(), collapsed.sum()
    keep = surv.copy()
    if not keep_duplicates and surv.any():
        idx = np.flatnonzero(surv)
        keys = rotate_smallest_first(tc[idx])
        _, first = np.unique(keys, axis=0, return_index=True)        # the first (lowest input index) of every rotated triple
        keep[:] = False
        keep[idx[first]] = True
        info[4] = surv.sum() - keep.sum()
    kc = tc[keep]
    named = np.unique(kc)                                            # ascending cell index
    out["verts"] = np.ascontiguousarray(pos[np.searchsorted(occupied, named)])
    out["tris"] = np.ascontiguousarray(np.searchsorted(named, kc).astype(np.int32).reshape(-1, 3))
    vm = np.full(nv, -1, np.int64)
    at = np.searchsorted(named, vcell[fin])
    at[at >= len(named)] = 0
    hit = len(named) > 0
    if hit:
        vm[fin] = np.where(named[at] == vcell[fin], at, -1)
    out["vertex_map"] = vm.astype(np.int32)
    out["named_cells"] = named
    return out


def unpack_dims(info):
    p = int(info[7])
    return p & MAX_AXIS, (p >> 21) & MAX_AXIS, (p >> 42) & MAX_AXIS


# ---- what an output must satisfy -------------------------------------------------------------------------------------------------
def directed_edge_excess(tris):
    """{(u, v): count(u, v) - count(v, u)} over the directed sides of the triangles, the positive entries only: empty = balanced"""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    cnt = {}
    for a, b in zip(tris.reshape(-1).tolist(), tris[:, [1, 2, 0]].reshape(-1).tolist()):
        cnt[a, b] = cnt.get((a, b), 0) + 1
    return {e: k - cnt.get((e[1], e[0]), 0) for e, k in cnt.items() if k > cnt.get((e[1], e[0]), 0)}


def check_output(res, keep_duplicates):
    """no collapsed triangle; no same-orientation duplicate; every output vertex referenced; ascending cell order"""
    tr, nv = res["tris"].astype(np.int64), len(res["verts"])
    if len(tr) == 0:
        assert nv == 0
        return
    assert tr.min() >= 0 and tr.max() < nv
    assert (tr[:, 0] != tr[:, 1]).all() and (tr[:, 1] != tr[:, 2]).all() and (tr[:, 0] != tr[:, 2]).all(), "a collapsed triangle"
    if not keep_duplicates:
        keys = rotate_smallest_first(tr)
        assert len(np.unique(keys, axis=0)) == len(keys), "a same-orientation duplicate"
    assert len(np.unique(tr)) == nv, "an output vertex no triangle names"
    named = res["named_cells"]
    assert len(named) == nv and (np.diff(named) > 0).all(), "output vertices are not in ascending cell order"
    vm, vc = res["vertex_map"], res["cell_of_vertex"]
    on = vm >= 0
    assert (named[vm[on]] == vc[on]).all() and not np.isin(vc[~on], named).any()


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def icosphere(level=3, radius=1.0, centre=(0.1, -0.2, 0.3)):
    """a closed mesh wound outwards: the icosahedron subdivided `level` times -> (verts float32 [10 4^level + 2, 3], tris int32 [20 4^level, 3])"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, g = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.array(v) * radius + np.array(centre)).astype(F), np.array(f, np.int32)


def sphere_volume(n=24, radius=0.37):
    """[n, n, n] float32: positive inside a sphere about a point off the lattice's centre, on the unit cube's lattice"""
    x = np.linspace(0.0, 1.0, n)
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij")
    return (radius - np.sqrt((X - 0.52) ** 2 + (Y - 0.47) ** 2 + (Z - 0.5) ** 2)).astype(F)


def two_tetrahedra():
    """two closed tetrahedra over one base's cells (cell = 1): their base triangles fall into the same three cells in the same order, the
    apexes D and E into different cells on the same side -> the base is a same-orientation duplicate whose removal unbalances its sides"""
    v = np.array([[0.2, 0.2, 0.2], [2.2, 0.2, 0.2], [0.2, 2.2, 0.2], [0.3, 0.3, 2.2],          # A B C D
                  [0.4, 0.4, 0.4], [2.4, 0.4, 0.4], [0.4, 2.4, 0.4], [1.4, 1.4, 3.4]], F)       # A' B' C' E
    tet = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)                        # wound outwards
    return v, np.concatenate([tet, tet + 4])


def fan(n_rim, cell=1.0):
    """a fan of n_rim - 1 triangles about a centre in the grid's first cell; every rim vertex has a cell of its own, so every triangle
    of the fan is registered under the centre's cell -> (verts, tris)"""
    k = np.arange(n_rim)
    rim = np.stack([1.5 + (k % 40), 1.5 + (k // 40), np.full(n_rim, 0.5)], 1) * cell
    v = np.concatenate([[[0.25 * cell, 0.25 * cell, 0.25 * cell]], rim]).astype(F)
    t = np.stack([np.zeros(n_rim - 1, np.int64), 1 + k[:-1], 2 + k[:-1]], 1).astype(np.int32)
    return v, t


def write_ply(path, verts, tris):
    """the PLY Mesher::write_ply writes without colours"""
    verts, tris = np.ascontiguousarray(verts, "<f4").reshape(-1, 3), np.ascontiguousarray(tris, "<i4").reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(tris)))
    rec = np.zeros(len(tris), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    rec["n"], rec["i"] = 3, tris
    with open(path, "wb") as f:
        f.write(head.encode("ascii") + verts.tobytes() + rec.tobytes())

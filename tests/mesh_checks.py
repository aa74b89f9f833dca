"""What a marching-cubes mesh must satisfy, computed from the VOLUME alone (pure numpy, nothing imported from the product), and the
checks of a 256-case triangle table.  Conventions restated from include/nsk.h:
  volume[k, j, i] (x fastest), node (i, j, k) at origin + (i, j, k) * step in float32 (product rounded, then the sum);
  a node is inside when value > level; a cell is processed when its 8 corners are finite and valid;
  corner c of a cell has the offsets (x, y, z) = (c & 1, (c >> 1) & 1, c >> 2), bit c of the case index = corner c inside;
  edge e = 4 * axis + idx runs along axis from the corner whose other two offsets (in axis order) are (idx & 1, idx >> 1);
  every lattice edge belongs to its lower node; vertex index = rank of node_index * 3 + axis among the crossing edges of processed cells."""
import numpy as np

CORNER = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]


def edge_ends(e):
    """the two corners (lower, upper) of cube edge e"""
    a, idx = e >> 2, e & 3
    others = [d for d in range(3) if d != a]
    lo = [0, 0, 0]
    lo[others[0]], lo[others[1]] = idx & 1, idx >> 1
    hi = list(lo)
    hi[a] = 1
    return lo[0] + 2 * lo[1] + 4 * lo[2], hi[0] + 2 * hi[1] + 4 * hi[2]


def edge_faces(e):
    """the two cube faces (axis, side) edge e lies in"""
    lo, _ = edge_ends(e)
    return {(d, CORNER[lo][d]) for d in range(3) if d != (e >> 2)}


def edge_mid(e):
    lo, hi = edge_ends(e)
    return (np.array(CORNER[lo], float) + np.array(CORNER[hi], float)) / 2


def face_signs(case, axis, side):
    """inside bits of the four corners of face (axis, side), keyed by the corner's two in-face offsets"""
    return {tuple(CORNER[c][d] for d in range(3) if d != axis): (case >> c) & 1 for c in range(8) if CORNER[c][axis] == side}


def edge_in_face_key(e, axis):
    """an edge of a face, named without the face's own coordinate (so that it can be compared across the two cells that share the face)"""
    lo, hi = edge_ends(e)
    drop = lambda c: tuple(CORNER[c][d] for d in range(3) if d != axis)
    return (drop(lo), drop(hi))


def face_segments(tris, axis, side):
    """directed triangle sides of a case that lie in face (axis, side), in face-local edge names"""
    out = []
    for t in tris:
        for q in range(3):
            a, b = t[q], t[(q + 1) % 3]
            if (axis, side) in edge_faces(a) and (axis, side) in edge_faces(b):
                out.append((edge_in_face_key(a, axis), edge_in_face_key(b, axis)))
    return out


def check_table(table):
    """table: list of 256 lists of triangles (edge triples).  Raises AssertionError with the case at fault."""
    assert len(table) == 256
    assert table[0] == [] and table[255] == [], "cases 0 and 255 must be empty"
    segs = {}
    for case in range(256):
        tris = table[case]
        crossing = {e for e in range(12) if ((case >> edge_ends(e)[0]) & 1) != ((case >> edge_ends(e)[1]) & 1)}
        used = {e for t in tris for e in t}
        assert all(0 <= e < 12 for e in used), case
        assert used == crossing, "case %d: triangles use edges %s, the crossing edges are %s" % (case, sorted(used), sorted(crossing))
        sides = {}
        for t in tris:
            assert len(set(t)) == 3, "case %d: degenerate triangle %s" % (case, t)
            for q in range(3):
                s = (t[q], t[(q + 1) % 3])
                sides[s] = sides.get(s, 0) + 1
        for (a, b), n in sides.items():
            assert n == 1, "case %d: directed side %s used %d times" % (case, (a, b), n)
            if edge_faces(a) & edge_faces(b):        # lies in a cube face: the neighbouring cell supplies the opposite direction
                assert (b, a) not in sides, "case %d: side %s lies in a face and is used in both directions" % (case, (a, b))
            else:
                assert (b, a) in sides, "case %d: inner side %s has no partner" % (case, (a, b))
        for axis in range(3):
            for side in range(2):
                segs[case, axis, side] = sorted(face_segments(tris, axis, side))
    # what a case leaves on a face = reversed what ANY case with the same four signs leaves on the opposite face (the neighbour's view)
    by_signs = {}
    for case in range(256):
        for axis in range(3):
            for side in range(2):
                by_signs.setdefault((axis, side, tuple(sorted(face_signs(case, axis, side).items()))), []).append(case)
    n_cmp = 0
    for case in range(256):
        for axis in range(3):
            for side in range(2):
                mine = segs[case, axis, side]
                signs = tuple(sorted(face_signs(case, axis, side).items()))
                for other in by_signs[axis, 1 - side, signs]:
                    theirs = sorted((b, a) for a, b in segs[other, axis, 1 - side])
                    assert mine == theirs, "face (%d,%d) of case %d against face (%d,%d) of case %d: %s vs %s" % (axis, side, case, axis, 1 - side, other, mine, theirs)
                    n_cmp += 1
    assert n_cmp == 256 * 6 * 16
    # the complement: on a face that is not ambiguous it leaves the same segments the other way round
    for case in range(256):
        for axis in range(3):
            for side in range(2):
                s = face_signs(case, axis, side)
                if sum(s.values()) == 2 and s[0, 0] == s[1, 1]:
                    continue
                assert segs[case, axis, side] == sorted((b, a) for a, b in segs[255 - case, axis, side]), (case, axis, side)
    # winding: for one inside corner the normal points away from it
    for c in range(8):
        tris = table[1 << c]
        assert len(tris) == 1, (c, tris)
        p = [edge_mid(e) for e in tris[0]]
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.dot(nrm, (p[0] + p[1] + p[2]) / 3 - np.array(CORNER[c], float)) > 0, "case %d: normal points into the inside corner" % (1 << c)
    return max(len(t) for t in table)


# ---- a mesh against its volume --------------------------------------------------------------------------------
def lattice_coords(origin, step, n):
    return [(np.float32(origin[a]) + np.arange(n[a]).astype(np.float32) * np.float32(step[a])).astype(np.float32) for a in range(3)]


def lattice_points(origin, step, nx, ny, nz):
    """[nz * ny * nx, 3] float32, x fastest"""
    cx, cy, cz = lattice_coords(origin, step, (nx, ny, nz))
    P = np.empty((nz, ny, nx, 3), np.float32)
    P[..., 0] = cx[None, None, :]; P[..., 1] = cy[None, :, None]; P[..., 2] = cz[:, None, None]
    return P.reshape(-1, 3)


def processed_cells(vol, valid=None):
    ok = np.isfinite(vol)
    if valid is not None:
        ok &= np.asarray(valid).reshape(vol.shape) != 0
    p = np.ones(tuple(s - 1 for s in vol.shape), bool)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                p &= ok[dz:vol.shape[0] - 1 + dz, dy:vol.shape[1] - 1 + dy, dx:vol.shape[2] - 1 + dx]
    return p


def cell_cases(vol, level, proc):
    """case index of every processed cell (1-D)"""
    ins = vol > np.float32(level)
    code = np.zeros(proc.shape, np.int32)
    for c, (dx, dy, dz) in enumerate(CORNER):
        code |= ins[dz:vol.shape[0] - 1 + dz, dy:vol.shape[1] - 1 + dy, dx:vol.shape[2] - 1 + dx].astype(np.int32) << c
    return code[proc]


def reference_vertices(vol, origin, step, level, valid=None):
    """(keys, positions): keys = node_index * 3 + axis of every crossing edge of a processed cell, ascending; positions [n, 3] float32 by
    p0 + t (p1 - p0), t = (level - v0) / (v1 - v0), every operation in float32"""
    nz, ny, nx = vol.shape
    level = np.float32(level)
    proc = processed_cells(vol, valid)
    pp = np.zeros((nz + 1, ny + 1, nx + 1), bool)          # pp[k + 1, j + 1, i + 1] = cell (i, j, k) processed; False outside
    pp[1:nz, 1:ny, 1:nx] = proc
    ins = vol > level
    has = np.zeros((nz, ny, nx, 3), bool)
    # x edges: cells (i, j-1..j, k-1..k)
    has[:, :, :nx - 1, 0] = (ins[:, :, :-1] != ins[:, :, 1:]) & (pp[1:, 1:, 1:nx] | pp[1:, :-1, 1:nx] | pp[:-1, 1:, 1:nx] | pp[:-1, :-1, 1:nx])
    has[:, :ny - 1, :, 1] = (ins[:, :-1, :] != ins[:, 1:, :]) & (pp[1:, 1:ny, 1:] | pp[1:, 1:ny, :-1] | pp[:-1, 1:ny, 1:] | pp[:-1, 1:ny, :-1])
    has[:nz - 1, :, :, 2] = (ins[:-1, :, :] != ins[1:, :, :]) & (pp[1:nz, 1:, 1:] | pp[1:nz, 1:, :-1] | pp[1:nz, :-1, 1:] | pp[1:nz, :-1, :-1])
    keys = np.flatnonzero(has.reshape(-1)).astype(np.int64)
    node, axis = keys // 3, keys % 3
    i, j, k = node % nx, (node // nx) % ny, node // (nx * ny)
    idx = np.stack([i, j, k], 1)
    coords = lattice_coords(origin, step, (nx, ny, nz))
    pos = np.stack([coords[a][idx[:, a]] for a in range(3)], 1).astype(np.float32)
    up = idx.copy()
    up[np.arange(len(keys)), axis] += 1
    v0 = vol[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float32)
    v1 = vol[up[:, 2], up[:, 1], up[:, 0]].astype(np.float32)
    with np.errstate(all="ignore"):
        t = ((level - v0).astype(np.float32) / (v1 - v0).astype(np.float32)).astype(np.float32)
        for a in range(3):
            m = axis == a
            p0 = pos[m, a]
            p1 = coords[a][up[m, a]]
            pos[m, a] = (p0 + (t[m] * (p1 - p0).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return keys, pos


def ulp_distance(a, b):
    """largest distance in float32 steps between two arrays of finite numbers"""
    def ordered(x):
        u = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7fffffff), u)
    if a.size == 0:
        return 0
    return int(np.abs(ordered(a) - ordered(b)).max())


def check_vertices(verts, vol, origin, step, level, valid=None, max_ulp=0):
    keys, pos = reference_vertices(vol, origin, step, level, valid)
    assert verts.shape == pos.shape, "vertex count %s, the volume has %s crossing edges in processed cells" % (verts.shape, pos.shape)
    assert np.isfinite(pos).all() == np.isfinite(verts).all()
    fin = np.isfinite(pos)
    assert (fin == np.isfinite(verts)).all()
    d = ulp_distance(verts[fin], pos[fin])
    assert d <= max_ulp, "vertex positions differ from the float32 formula by %d ulp (allowed %d)" % (d, max_ulp)
    return keys


def check_topology(tris, keys, vol, valid=None):
    """tris [nt, 3] vertex indices, keys = lattice edge of every vertex (check_vertices).  Returns the number of boundary sides."""
    nz, ny, nx = vol.shape
    nv = len(keys)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if len(tris) == 0:
        assert nv == 0, "vertices without triangles"
        return 0
    assert tris.min() >= 0 and tris.max() < nv
    assert (tris[:, 0] != tris[:, 1]).all() and (tris[:, 1] != tris[:, 2]).all() and (tris[:, 0] != tris[:, 2]).all(), "degenerate index triple"
    assert len(np.unique(tris)) == nv, "a vertex no triangle uses"
    proc = processed_cells(vol, valid)
    node, axis = keys // 3, keys % 3
    nidx = np.stack([node % nx, (node // nx) % ny, node // (nx * ny)], 1)            # [nv, 3] node of the owning lower end
    lo = nidx - (np.arange(3)[None, :] != axis[:, None])                               # cells an edge touches: [lo, hi] per axis
    hi = nidx
    tlo = lo[tris].max(axis=1)
    thi = hi[tris].min(axis=1)
    assert (tlo == thi).all(), "a triangle whose three edges do not single out one cell (%d of them)" % int((tlo != thi).any(axis=1).sum())
    cell = tlo
    dims = np.array([nx - 1, ny - 1, nz - 1])
    assert (cell >= 0).all() and (cell < dims).all()
    assert proc[cell[:, 2], cell[:, 1], cell[:, 0]].all(), "a triangle in a cell that is not processed"
    lin = (cell[:, 2] * ny + cell[:, 1]) * nx + cell[:, 0]
    assert (np.diff(lin) >= 0).all(), "triangles are not ordered by cell"
    # sides
    a = tris.reshape(-1)
    b = tris[:, [1, 2, 0]].reshape(-1)
    scell = np.repeat(cell, 3, axis=0)
    code = a * nv + b
    assert len(np.unique(code)) == len(code), "a directed side used twice"
    has_rev = np.isin(b * nv + a, code)
    # a side lies in a cell face when both lattice edges lie in one plane d = const (d the axis of neither); the neighbour across supplies its partner
    expect = np.ones(len(a), bool)
    for d in range(3):
        inface = (axis[a] != d) & (axis[b] != d) & (nidx[a, d] == nidx[b, d])
        ncell = scell.copy()
        ncell[:, d] += np.where(nidx[a, d] == scell[:, d], -1, 1)
        inside = ((ncell >= 0) & (ncell < dims)).all(axis=1)
        nproc = np.zeros(len(a), bool)
        nproc[inside] = proc[ncell[inside, 2], ncell[inside, 1], ncell[inside, 0]]
        expect &= ~inface | nproc
    bad = has_rev != expect
    assert not bad.any(), "%d sides: partner %s where %s was due" % (int(bad.sum()), has_rev[bad][:4], expect[bad][:4])
    return int((~expect).sum())


def euler_characteristic(tris, nv):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.sort(np.stack([tris.reshape(-1), tris[:, [1, 2, 0]].reshape(-1)], 1), axis=1)
    return nv - len(np.unique(e[:, 0] * nv + e[:, 1])) + len(tris)


def signed_volume(verts, tris):
    """divergence theorem; positive when the normals point out of the enclosed solid"""
    v = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def read_ply(path):
    """binary little-endian PLY with float x y z [uchar red green blue] vertices and `list uchar int vertex_indices` faces"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    nv = nf = 0
    props = []
    cur = None
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
    names = [p[1] for p in props]
    assert names[:3] == ["x", "y", "z"] and all(p[0] == "float" for p in props[:3])
    color = names[3:] == ["red", "green", "blue"]
    assert color or len(names) == 3, names
    vdt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if color else []))
    v = np.frombuffer(data, vdt, nv, end)
    off = end + nv * vdt.itemsize
    fdt = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    fa = np.frombuffer(data, fdt, nf, off)
    assert off + nf * fdt.itemsize == len(data), "trailing bytes"
    assert (fa["n"] == 3).all()
    return v["p"].copy(), (v["c"].copy() if color else None), fa["i"].copy()


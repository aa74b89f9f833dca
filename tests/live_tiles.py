"""numpy model of the backward's dead-tile skip (include/nsk.h, nsk_set_mask): which grid cells have a marked corner voxel, which samples
fall in such cells, and how many 16-sample tiles of a given slot order hold at least one such sample.

Everything is float32 with one rounding per operation, the operation sequence of the kernels' cell_index / tri_setup (itself that of
F::grid_sample with align_corners, border padding), so cell indices agree with the device bit for bit."""
import numpy as np

LEVEL_BIT = {"middle": 1, "fine": 2, "color": 4}
F = np.float32


def cell_coords(shape_zyx, bound, pts):
    """[n, 3] int (ix, iy, iz): the lower corner voxel of the cell holding each point, clamped into the grid (tri_setup's i0)"""
    Z, Y, X = shape_zyx
    dims = (X, Y, Z)
    b = np.asarray(bound, F).reshape(3, 2)
    p = np.asarray(pts, F).reshape(-1, 3)
    out = np.zeros(p.shape, np.int64)
    for k in range(3):
        lo, hi = b[k, 0], b[k, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            u = (p[:, k] - lo) / F(hi - lo) * F(2) - F(1)
            x = (u + F(1)) / F(2) * F(dims[k] - 1)
        mx = F(dims[k] - 1)
        x = np.where(x <= 0, F(0), np.where(x >= mx, mx, x))          # a NaN stays a NaN here and is clamped below, as on the device
        i = np.where(np.isfinite(x), np.floor(x), 0).astype(np.int64)
        out[:, k] = np.clip(i, 0, dims[k] - 1)
    return out


def cell_index(shape_zyx, bound, pts):
    Z, Y, X = shape_zyx
    c = cell_coords(shape_zyx, bound, pts)
    return (c[:, 2] * Y + c[:, 1]) * X + c[:, 0]


def cell_live(mask_zyx):
    """[Z, Y, X] bool: the OR of the mask over the cell's eight corner voxels, the neighbour along an axis clamped into the grid"""
    m = np.asarray(mask_zyx).astype(bool)
    out = np.zeros_like(m)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                s = m
                if dz:
                    s = np.concatenate([s[1:], s[-1:]], 0)
                if dy:
                    s = np.concatenate([s[:, 1:], s[:, -1:]], 1)
                if dx:
                    s = np.concatenate([s[:, :, 1:], s[:, :, -1:]], 2)
                out |= s
    return out


def sample_points(rays_o, rays_d, z):
    """[N * S, 3] float32: p = o + d z, the product rounded, then the sum (reference src/Renderer.cpp:121)"""
    ro, rd, z = np.asarray(rays_o, F), np.asarray(rays_d, F), np.asarray(z, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)


def sample_bytes(bound, shapes_zyx, masks, pts):
    """[n] uint8: bit 0 middle, 1 fine, 2 colour -- the point's cell at that level has a marked corner; a level without a mask (None or
    absent) has its bit set everywhere"""
    b = np.zeros(len(pts), np.uint8)
    for name, bit in LEVEL_BIT.items():
        m = masks.get(name)
        if m is None or name not in shapes_zyx:
            b |= np.uint8(bit)
            continue
        live = cell_live(m).ravel()
        b |= np.where(live[cell_index(shapes_zyx[name], bound, pts)], np.uint8(bit), np.uint8(0)).astype(np.uint8)
    return b


def sample_bytes_brute(bound, shapes_zyx, masks, pts):
    """the same by the definition: per sample, its eight (clamped) corner voxels looked up in the mask one by one"""
    b = np.zeros(len(pts), np.uint8)
    for name, bit in LEVEL_BIT.items():
        m = masks.get(name)
        if m is None or name not in shapes_zyx:
            b |= np.uint8(bit)
            continue
        Z, Y, X = shapes_zyx[name]
        m = np.asarray(m).astype(bool)
        c = cell_coords(shapes_zyx[name], bound, pts)
        for s in range(len(pts)):
            on = False
            for corner in range(8):
                ix = min(c[s, 0] + (corner & 1), X - 1)
                iy = min(c[s, 1] + ((corner >> 1) & 1), Y - 1)
                iz = min(c[s, 2] + (corner >> 2), Z - 1)
                on = on or bool(m[iz, iy, ix])
            if on:
                b[s] |= np.uint8(bit)
    return b


def live_tiles(slot_bytes, bit):
    """number of 16-slot tiles with at least one slot whose byte has `bit`; the last tile may be ragged (its missing slots count for nothing)"""
    v = (np.asarray(slot_bytes, np.uint8) & np.uint8(bit)) != 0
    n = len(v)
    pad = (-n) % 16
    if pad:
        v = np.concatenate([v, np.zeros(pad, bool)])
    return int(v.reshape(-1, 16).any(axis=1).sum())


def cell_order(bound, key_shape_zyx, parent_shape_zyx, pts):
    """a stable order of the samples by key-level cell and, inside it, by the parity of the parent-level cell: the order class the device's
    cell sort produces (its order inside a key is arrival order, which no tile count here depends on much)"""
    key = cell_index(key_shape_zyx, bound, pts) * 8
    if parent_shape_zyx is not None:
        c = cell_coords(parent_shape_zyx, bound, pts)
        key = key + ((c[:, 0] & 1) | ((c[:, 1] & 1) << 1) | ((c[:, 2] & 1) << 2))
    return np.argsort(key, kind="stable")

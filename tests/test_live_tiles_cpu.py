"""The numpy model of the dead-tile skip (tests/live_tiles.py) that the GPU tests and tools/live_tiles.py rely on, against the definition
applied sample by sample.  Needs no GPU."""
import numpy as np

import live_tiles as lt
import scenes

SHAPES = {k: scenes.SMALL_GRID_SHAPES[k][1:] for k in ("middle", "fine", "color")}


def _points(seed, n):
    """points inside the bound, on its faces, outside it and non-finite: the clamps of tri_setup all get exercised"""
    rng = np.random.default_rng(seed)
    b = scenes.REF_BOUND
    p = (b[:, 0] + rng.random((n, 3)) * (b[:, 1] - b[:, 0])).astype(np.float32)
    p[0] = b[:, 0]; p[1] = b[:, 1]; p[2] = b[:, 1] + 1.0; p[3] = b[:, 0] - 1.0
    p[4] = [np.nan, 0.0, 0.0]; p[5] = [np.inf, -np.inf, 0.0]
    p[6] = [b[0, 1], b[1, 0], 0.5 * (b[2, 0] + b[2, 1])]
    return p


def _masks(rng):
    out = {}
    for k, s in SHAPES.items():
        out[k] = rng.random(s) < 0.15
    return out


def test_cell_live_is_the_or_of_the_clamped_corners():
    rng = np.random.default_rng(1)
    for s in SHAPES.values():
        m = rng.random(s) < 0.1
        live = lt.cell_live(m)
        Z, Y, X = s
        for iz in range(Z):
            for iy in range(Y):
                for ix in range(X):
                    want = any(m[min(iz + dz, Z - 1), min(iy + dy, Y - 1), min(ix + dx, X - 1)] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
                    assert live[iz, iy, ix] == want, (s, iz, iy, ix)
    one = np.zeros(SHAPES["fine"], bool)
    one[-1, -1, -1] = True                                       # the far corner voxel: the 8 cells around it, no wrap-around
    assert lt.cell_live(one).sum() == 8
    assert lt.cell_live(np.zeros(SHAPES["fine"], bool)).sum() == 0 and lt.cell_live(np.ones(SHAPES["fine"], bool)).all()


def test_sample_bytes_match_the_per_sample_corner_test():
    p = _points(2, 600)
    rng = np.random.default_rng(3)
    for masks in (_masks(rng), {"middle": None, "fine": _masks(rng)["fine"], "color": np.zeros(SHAPES["color"], bool)}, {}):
        a = lt.sample_bytes(scenes.REF_BOUND, SHAPES, masks, p)
        b = lt.sample_bytes_brute(scenes.REF_BOUND, SHAPES, masks, p)
        assert np.array_equal(a, b)
    assert (lt.sample_bytes(scenes.REF_BOUND, SHAPES, {}, p) == 7).all()


def test_cells_of_out_of_bound_and_non_finite_points_stay_in_the_grid():
    p = _points(4, 16)
    for s in SHAPES.values():
        c = lt.cell_coords(s, scenes.REF_BOUND, p)
        Z, Y, X = s
        assert (c >= 0).all() and (c[:, 0] < X).all() and (c[:, 1] < Y).all() and (c[:, 2] < Z).all()
        assert tuple(c[0]) == (0, 0, 0) and tuple(c[1]) == (X - 1, Y - 1, Z - 1) and tuple(c[2]) == (X - 1, Y - 1, Z - 1) and tuple(c[3]) == (0, 0, 0)
        assert c[4, 0] == 0                                      # NaN: cell 0 along that axis, as the device's conversion gives


def test_live_tiles_counts_whole_and_ragged_tiles():
    b = np.zeros(40, np.uint8)
    assert lt.live_tiles(b, 2) == 0
    b[15] = 2; b[16] = 1; b[39] = 2
    assert lt.live_tiles(b, 2) == 2 and lt.live_tiles(b, 1) == 1 and lt.live_tiles(b, 4) == 0
    assert lt.live_tiles(np.full(33, 7, np.uint8), 4) == 3
    # against a plain loop over the tiles
    rng = np.random.default_rng(5)
    v = (rng.random(203 * 48) < 0.02).astype(np.uint8) * 4
    want = sum(1 for t in range(0, len(v), 16) if v[t:t + 16].any())
    assert lt.live_tiles(v, 4) == want


def test_cell_order_groups_the_samples_of_a_cell():
    p = _points(6, 500)
    order = lt.cell_order(scenes.REF_BOUND, SHAPES["fine"], SHAPES["middle"], p)
    assert sorted(order) == list(range(500))
    cells = lt.cell_index(SHAPES["fine"], scenes.REF_BOUND, p)[order]
    assert (np.diff(cells) >= 0).all()

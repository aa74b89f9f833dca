"""GPU tests of the row reductions (csrc/nsk_reduce.h) through the public entry points that end in them: the device's sums must be, bytes
for bytes, what tests/rows_checks.py computes over the stated tree (tests/test_rows_cpu.py proves that restatement).  Sizes: a partial
wave and a second wave (1, 63, 64, 65), a second row (255, 256, 257) and the row cap, where one lane takes a second element."""
import numpy as np
import pytest
import torch

import icp_checks as ic
import recon_checks as rc
import rows_checks as rw
from gpu_util import cu

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1024 * 256 + 1]             # (1024: IMG_MAX_ROWS = CLOUD_MAX_ROWS)
PIX = [1, 63, 64, 65, 255, 256, 257, 64 * 256 + 1]                  # (64: RASTER_STAT_ROWS)


@pytest.fixture(scope="module")
def ctx():
    import nice_slam_cpp_amd as pkg
    return pkg.Context(0)


def mixed(rng, shape):
    """float32 magnitudes over [1e-3, 1e3]: another association of the sums shows in the low bits"""
    return np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape)).astype(np.float32)


def spoil(rng, a, every=37):
    """NaN, +inf and -inf at a few places (none when the array is too short to keep a finite entry beside them)"""
    flat = a.reshape(-1)
    if flat.size >= 63:
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            flat[5 + 3 * k::every * (k + 1)] = v
    return a


def same(got, want):
    return (rw.bits(got) == rw.bits(want)).all()


@pytest.mark.parametrize("n", SIZES)
def test_cloud_stats(ctx, n):
    rng = np.random.default_rng(n)
    d = spoil(rng, mixed(rng, n))
    want = rw.reduce(rw.cloud_stats_terms(d, 1.0), rw.CLOUD_STATS_OPS)
    got = ctx.cloud_stats(cu(d), 1.0)
    print("n %d: sum %r (tree %r, numpy %r)" % (n, got["sum"], want[0], float(np.sum(d[np.isfinite(d)].astype(np.float64)))))
    assert same([got["sum"], got["max"]], want[[0, 3]]) and got["count"] == want[1] and got["below"] == want[2]
    fin = d[np.isfinite(d)]
    assert got["count"] == len(fin) and got["below"] == (fin < 1).sum() and got["max"] == (fin.max() if len(fin) else 0)


@pytest.mark.parametrize("n", SIZES)
def test_image_metrics(ctx, n):
    rng = np.random.default_rng(100 + n)
    rgb, gc = spoil(rng, mixed(rng, (1, n, 3)), 101), spoil(rng, mixed(rng, (1, n, 3)), 89)
    d, g = spoil(rng, mixed(rng, (1, n))), spoil(rng, mixed(rng, (1, n)), 53)
    if n >= 63:
        g[0, 7::11] = 0.0                                           # no measurement
    want = rw.reduce(rw.image_metrics_terms(rgb, d, g, gc))
    m = ctx.image_metrics(cu(rgb), cu(d), cu(g), cu(gc))
    print("n %d: depth sum %r (tree %r), colour sum %r (tree %r)" % (n, m["depth_sum"], want[1], m["color_sum"], want[3]))
    assert same([m["depth_sum"], m["color_sum"]], want[[1, 3]])
    assert (m["pixels"], m["depth_pixels"], m["color_terms"], m["nonfinite"]) == (n, want[0], want[2], want[4])
    assert m["h_out"][6:] == [0.0, 0.0]
    if n >= 63:
        assert 0 < m["nonfinite"] < n and 0 < m["depth_pixels"] < n - m["nonfinite"]


@pytest.mark.parametrize("n", SIZES)
def test_cloud_pair_sums(ctx, n):
    rng = np.random.default_rng(200 + n)
    M = ic.motion(30.0, (1.0, 2.0, -1.0), (0.3, -0.2, 0.5))
    T = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    T[::41, 1] = np.nan
    S = (rng.uniform(-1, 1, (n, 3)) * mixed(rng, (n, 1)) / 30).astype(np.float32)       # most within the threshold of a target, some far out
    if n >= 63:
        S[3] = [3e38, 3e38, 3e38]                                   # finite, but not under the transform
        S[11, 0] = np.nan
    dS, dT = cu(S), cu(T)
    got, dist, idx = ctx.cloud_pair_sums(dS, dT, M, 0.5, want_pairs=True)
    skipped = ctx.last_skipped
    terms = rw.icp_terms(ic.transform(M, S), dist.cpu().numpy(), idx.cpu().numpy(), T, 0.5)
    want = rw.reduce(terms)
    print("n %d: %d pairs, sum d^2 %r (tree %r)" % (n, got[0], got[1], want[1]))
    assert same(got, want[:17]) and skipped == 8
    _, info = ctx.cloud_icp(dS, dT, 0.5, 0, init=M)                  # no update: the evaluation under M, and its eighteenth column
    assert info["source_nonfinite"] == want[17] == (2 if n >= 63 else 0) and info["correspondences"] == want[0]
    if n >= 255:
        assert 0 < want[0] < n - 2                                   # pairs on both sides of the threshold


@pytest.mark.parametrize("n_pix", PIX)
def test_depth_pair_stats(ctx, n_pix):
    V = 3
    rng = np.random.default_rng(300 + n_pix)
    a, b = spoil(rng, mixed(rng, (V, n_pix))), spoil(rng, mixed(rng, (V, n_pix)), 43)
    if n_pix >= 63:
        a[:, 2::7] = 0.0; b[:, 1::5] = 0.0                          # nothing hit
        a[1] *= 3                                                   # the views differ
    want = np.stack([rw.reduce(rw.depth_pair_terms(a[v], b[v]), cap=64) for v in range(V)])
    got = ctx.depth_pair_stats(cu(a), cu(b))
    print("n_pix %d: sums %r (tree %r)" % (n_pix, got[:, 0].tolist(), want[:, 0].tolist()))
    assert got.shape == (V, 4) and same(got, want)


@pytest.mark.parametrize("n", SIZES)
def test_box_of_the_targets(ctx, n):
    """the box has no order to restate: its count against numpy, and the grid built on it through the nearest distances"""
    rng = np.random.default_rng(400 + n)
    T = (rng.uniform(-1, 1, (n, 3)) * mixed(rng, (n, 1))).astype(np.float32)
    if n >= 63:
        T[::29, 2] = np.nan; T[7, 0] = np.inf; T[13, 1] = -np.inf
    q = (rng.uniform(-1, 1, (32, 3)) * mixed(rng, (32, 1))).astype(np.float32)
    q[:4] = T[:4]
    want_d, want_i = rc.brute_nearest(q, T, chunk=32)
    d, i = ctx.cloud_nearest(cu(q), cu(T), want_index=True)
    assert ctx.last_skipped == (~np.isfinite(T).all(1)).sum()
    d = d.cpu().numpy()
    assert (d.view(np.uint32) == want_d.view(np.uint32))[~np.isnan(want_d)].all() and (np.isnan(d) == np.isnan(want_d)).all()
    assert (i.cpu().numpy() == want_i).all()
    box = ctx.depth_views(cu(T), 0)                                 # the same kernel behind nsk_depth_views
    fin = T[np.isfinite(T).all(1)]
    assert ctx.last_box.tobytes() == np.concatenate([fin.min(0), fin.max(0)]).astype(np.float32).tobytes() and box.shape == (0, 4, 4)

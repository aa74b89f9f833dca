"""tests/rows_checks.py against a plain Python loop over the tree it states, and the proof that the tree is not numpy's own summation."""
import math

import numpy as np
import pytest

import rows_checks as rw


def _op(name):
    # fmin / fmax as the device has them: a NaN operand is dropped
    if name == rw.SUM:
        return lambda a, b: a + b
    pick = min if name == rw.MIN else max
    return lambda a, b: b if math.isnan(a) else (a if math.isnan(b) else pick(a, b))


def loop_reduce(terms, ops, block, cap):
    """thread by thread, wave by wave, row by row"""
    x = np.asarray(terms, np.float64)
    if x.ndim == 2:
        x = x[:, None, :]
    n, K, cols = x.shape
    nrows = min((n + block - 1) // block, cap)
    out = []
    for c in range(cols):
        op = _op(ops[c])
        rows = []
        for b in range(nrows):
            acc = [0.0] * block
            for t in range(block):
                p = b * block + t
                while p < n:
                    for k in range(K):
                        acc[t] = op(acc[t], float(x[p, k, c]))
                    p += nrows * block
            waves = []
            for w in range(block // 64):
                v = acc[64 * w:64 * w + 64]
                for s in (32, 16, 8, 4, 2, 1):
                    v = [op(v[lane], v[lane ^ s]) for lane in range(64)]
                waves.append(v[0])
            r = waves[0]
            for w in waves[1:]:
                r = op(r, w)
            rows.append(r)
        if ops[c] == rw.SUM:
            r = 0.0
            for v in rows:
                r = r + v
        else:
            r = rows[0]
            for v in rows[1:]:
                r = op(r, v)
        out.append(r)
    return np.array(out, np.float64)


def _mixed(rng, shape):
    """magnitudes over six decades, so that another association shows in the low bits"""
    return np.exp(rng.uniform(np.log(1e-3), np.log(1e3), shape))


# a partial wave, a second wave, a second row, the cap with a second pass of the lanes (and a third for some), several terms per element
@pytest.mark.parametrize("n,block,cap,K", [(1, 256, 1024, 1), (63, 256, 1024, 1), (65, 256, 1024, 1), (257, 256, 1024, 1), (700, 256, 2, 1),
                                             (300, 128, 1, 1), (520, 256, 1, 3), (200, 64, 2, 2)])
def test_restatement_equals_the_plain_loop(n, block, cap, K):
    rng = np.random.default_rng(n + cap)
    x = _mixed(rng, (n, K, 4))
    x[:, :, 2] = -x[:, :, 2]
    x[rng.random((n, K)) < 0.1] = 0.0                               # skipped elements
    ops = (rw.SUM, rw.MAX, rw.MIN, rw.SUM)
    terms = x if K > 1 else x[:, 0]
    got, want = rw.reduce(terms, ops, block, cap), loop_reduce(terms, ops, block, cap)
    assert (rw.bits(got) == rw.bits(want)).all()
    assert got[1] == x[:, :, 1].max() and got[2] == x[:, :, 2].min()        # (+0.0, where the lanes start, lies outside neither)
    assert abs(got[0] - math.fsum(x[:, :, 0].reshape(-1))) <= 1e-12 * got[0]


def test_rows_follow_the_cap():
    assert [rw.n_rows(n) for n in (1, 256, 257, 1024 * 256, 1024 * 256 + 1)] == [1, 1, 2, 1024, 1024]
    assert rw.n_rows(64 * 256 + 1, cap=64) == 64


def test_the_tree_is_not_numpys_sum():
    """the same terms, another association, other bits: a device that summed in any other order would be caught"""
    rng = np.random.default_rng(7)
    x = _mixed(rng, (5000, 1))
    tree = rw.reduce(x)[0]
    assert rw.bits(tree) != rw.bits(np.sum(x[:, 0]))
    assert rw.bits(tree) != rw.bits(rw.reduce(x[::-1])[0])          # nor is it blind to the order of the elements
    assert abs(tree - math.fsum(x[:, 0])) <= 1e-12 * tree


def test_entry_point_terms():
    """the terms each entry point feeds in, on inputs small enough to check by eye"""
    inf, nan = np.inf, np.nan
    t = rw.cloud_stats_terms(np.array([0.5, nan, 2.0, inf], np.float32), 1.0)
    assert t.tolist() == [[0.5, 1, 1, 0.5], [0, 0, 0, 0], [2.0, 1, 0, 2.0], [0, 0, 0, 0]]
    a = np.array([1.0, 0.0, 2.0, inf, nan], np.float32); b = np.array([1.5, 1.0, 0.0, inf, 1.0], np.float32)
    assert rw.depth_pair_terms(a, b).tolist() == [[0.5, 1, 0.5, 1], [1.0, 0, 0, 0], [2.0, 0, 0, 1], [0, 1, 0, 1], [0, 0, 0, 0]]
    rgb = np.array([[0.5, 0.5, 0.5], [nan, 0.5, 0.5], [1.0, 0.0, 0.5]], np.float32); gc = np.full((3, 3), 0.5, np.float32)
    m = rw.image_metrics_terms(rgb, np.array([1.0, 1.0, 3.0], np.float32), np.array([2.0, 2.0, 0.0], np.float32), gc)
    assert m[:, 0, [0, 1, 4]].tolist() == [[1, 1.0, 0], [0, 0, 1], [0, 0, 0]]
    assert m[:, :, 2].tolist() == [[1, 1, 1], [0, 0, 0], [1, 1, 1]] and m[:, :, 3].tolist() == [[0, 0, 0], [0, 0, 0], [0.25, 0.25, 0]]
    s = np.array([[1, 2, 3], [nan, 0, 0], [4, 5, 6], [7, 8, 9]], np.float32); tg = np.array([[1, 1, 1], [2, 0, 0]], np.float32)
    i = rw.icp_terms(s, np.array([0.5, nan, 3.0, 1.0], np.float32), np.array([1, -1, 0, 0]), tg, 1.0)
    assert i[0].tolist() == [1, 0.25, 1, 2, 3, 2, 0, 0, 2, 0, 0, 4, 0, 0, 6, 0, 0, 0]
    assert i[1].tolist() == [0] * 17 + [1] and not i[2].any()
    assert i[3].tolist() == [1, 1, 7, 8, 9, 1, 1, 1, 7, 7, 7, 8, 8, 8, 9, 9, 9, 0]

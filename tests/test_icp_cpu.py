"""The alignment rule without a GPU: nsk_rigid_from_sums (host only, through ctypes) against a numpy Kabsch, host/test/rigid_test under
AddressSanitizer + UndefinedBehaviorSanitizer, and the numpy restatement of the loop (tests/icp_checks.py) on the scene the GPU tests use,
with the conditions that scene must meet so that the device's iteration count does not hinge on a last bit."""
import os
import subprocess

import numpy as np
import pytest

import icp_checks as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")


def rigid(sums):
    import nice_slam_cpp_amd as pkg
    return pkg.nsk.rigid_from_sums(sums)


def sums_under(M, s):
    """the 17 sums of the points s [n, 3] (float64) paired with t = M s, formed in float64"""
    t = s @ M[:3, :3].T + M[:3, 3]
    out = np.zeros(17)
    out[0] = len(s); out[1] = ((s - t) ** 2).sum(); out[2:5] = s.sum(0); out[5:8] = t.sum(0)
    out[8:17] = (s[:, :, None] * t[:, None, :]).sum(0).reshape(9)
    return out


def proper(U):
    R = U[:3, :3]
    return np.isfinite(U).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14 \
        and (U[3] == [0, 0, 0, 1]).all()


MOTIONS = [(1.5, (0.5, -0.3, 0.8), (0.012, -0.011, 0.012)), (30.0, (1, 2, -1), (0.3, -0.2, 0.5)), (179.0, (-1, 0.2, 0.1), (-1, 2, 0.25)),
           (0.0, (0, 0, 1), (0, 0, 0)), (120.0, (1, 1, 1), (0.1, 0.1, 0.1))]


@pytest.mark.parametrize("k", range(len(MOTIONS)))
def test_rigid_solve_equals_numpy_kabsch_and_recovers_the_motion(k):
    rng = np.random.default_rng(k)
    M = ic.motion(*MOTIONS[k])
    s = rng.uniform(-1, 1, (1000, 3))
    sums = sums_under(M, s)
    U, rank = rigid(sums)
    want, want_rank = ic.kabsch(sums)
    print("motion %d: |U - numpy| %.3g, |U - truth| %.3g, rank %d" % (k, np.abs(U - want).max(), np.abs(U - M).max(), rank))
    assert rank == want_rank == 3
    assert np.abs(U - want).max() < 1e-12
    assert np.abs(U - M).max() < 1e-12                           # exact pairs: the motion itself
    assert proper(U)
    # noisy pairs (no motion fits them): still numpy's answer
    noisy = sums.copy()
    t = s @ M[:3, :3].T + M[:3, 3] + rng.normal(0, 0.01, s.shape)
    noisy[5:8] = t.sum(0); noisy[8:17] = (s[:, :, None] * t[:, None, :]).sum(0).reshape(9)
    U, _ = rigid(noisy)
    assert np.abs(U - ic.kabsch(noisy)[0]).max() < 1e-12 and proper(U)


def test_reflection_case_gives_a_rotation():
    rng = np.random.default_rng(7)
    s = np.stack([rng.uniform(-1, 1, 500), rng.uniform(0, 1, 500), np.zeros(500)], 1)
    # a planar cloud and its mirror image: the orthogonal map that fits best has det -1
    sums = sums_under(np.diag([-1.0, 1.0, 1.0, 1.0]), s)
    n = sums[0]
    Cm = sums[8:17].reshape(3, 3) / n - np.outer(sums[2:5] / n, sums[5:8] / n)
    Us, _, Vt = np.linalg.svd(Cm)
    U, rank = rigid(sums)
    want, _ = ic.kabsch(sums)
    print("det before the fix %.3f, after %.15f, rank %d" % (np.linalg.det(Vt.T @ Us.T), np.linalg.det(U[:3, :3]), rank))
    assert rank == 2 and proper(U)
    assert np.abs(U - want).max() < 1e-12                          # (rank 2 determines R, whichever sign the third singular vectors carry)
    # planar under a true motion: rank 2 determines R
    M = ic.motion(30.0, (1, 2, -1), (0.3, -0.2, 0.5))
    s[:, 2] = 0.25 * s[:, 0] - 0.5 * s[:, 1] + 0.1
    U, rank = rigid(sums_under(M, s))
    assert rank == 2 and np.abs(U - M).max() < 1e-12 and proper(U)


def test_degenerate_sums_give_a_finite_proper_rotation():
    rng = np.random.default_rng(8)
    M = ic.motion(20.0, (1, 2, -1), (0.3, -0.2, 0.5))
    u = rng.uniform(0, 1, 300)
    U, rank = rigid(sums_under(M, np.stack([u, 1 - 2 * u, 0.5 * u], 1)))
    assert rank == 1 and proper(U)
    p = np.array([[0.3, -0.2, 0.9]])
    U, rank = rigid(sums_under(M, p))
    assert rank <= 1 and proper(U)
    assert np.abs(U[:3, :3] @ p[0] + U[:3, 3] - (M[:3, :3] @ p[0] + M[:3, 3])).max() < 1e-14     # the means still meet
    U, rank = rigid(sums_under(M, np.tile(p, (1000, 1))))
    assert rank <= 1 and proper(U)
    U, rank = rigid(np.zeros(17))
    assert rank == 0 and (U == np.eye(4)).all()


def test_a_sum_that_is_not_finite_is_refused():
    import nice_slam_cpp_amd as pkg
    s = np.zeros(17); s[0] = 3; s[9] = np.nan
    with pytest.raises(pkg.NskError):
        rigid(s)
    assert (rigid(np.zeros(17))[0] == np.eye(4)).all()


def test_rigid_test_under_the_sanitizers():
    subprocess.check_call(["make", "-s", "-C", HOST, "rigid_test"])
    r = subprocess.run([os.path.join(HOST, "rigid_test")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "rigid_test: ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_the_restated_transform_is_the_rule():
    rng = np.random.default_rng(3)
    p = rng.uniform(-2, 2, (500, 3)).astype(np.float32)
    p[5] = [np.nan, 1, 2]; p[9] = [0, np.inf, 1]; p[11] = [1, 2, -np.inf]
    M = ic.motion(30.0, (1, 2, -1), (0.3, -0.2, 0.5))
    got = ic.transform(M, p)
    for i in (0, 17, 499):
        x, y, z = (float(v) for v in p[i])
        for a in range(3):
            assert got[i, a] == np.float32(((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3])
    for i in (5, 9, 11):                                           # non-finite points pass through with their bits
        assert (got[i].view(np.uint32) == p[i].view(np.uint32)).all()
    assert (ic.transform(np.eye(4), p).view(np.uint32) == p.view(np.uint32)).all()
    A, B = ic.motion(10, (1, 0, 0), (1, 2, 3)), ic.motion(20, (0, 1, 0), (0, 1, 0))
    assert np.abs(ic.mul4(A, B) - A @ B).max() < 1e-15


def test_the_restatement_recovers_the_motion_and_the_scene_meets_its_conditions():
    S, T, truth = ic.scene()
    assert len(S) == ic.NS and len(T) == ic.NT
    M, info = ic.scene_icp()
    h = info["history"]
    steps = [(abs(h[k][0] - h[k - 1][0]), abs(h[k][1] - h[k - 1][1])) for k in range(1, len(h))]
    e_ref = ic.corner_shift(M, truth)
    print("updates %d, fitness %.6f, rmse %.3e, e_ref %.3e m, nearest |d - threshold| %.3g ulp" % (
        info["iterations"], info["fitness"], info["rmse"], e_ref, info["margin"]))
    for k, (df, de) in enumerate(steps):
        print("  evaluation %d: |d fitness| %.3e, |d rmse| %.3e" % (k + 1, df, de))
    assert info["converged"] and info["iterations"] < 30
    assert steps[-1][0] < 1e-7 and steps[-1][1] < 1e-7
    assert all(max(df, de) > 1e-5 for df, de in steps[:-1])
    assert info["margin"] > 4                                      # no distance within 4 ulp of the threshold, counting or not
    assert ic.corner_shift(np.eye(4), truth) > 0.02                # the scene starts centimetres off ...
    assert e_ref < 1e-6                                            # ... and ends where it belongs
    R = M[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-13
    # the loop's edges: no update asked for, and a start at the answer
    M0, i0 = ic.icp(S, T, max_iter=0)
    assert (M0 == np.eye(4)).all() and i0["iterations"] == 0 and not i0["converged"] and i0["fitness"] == h[0][0]
    M1, i1 = ic.icp(S, T, init=truth)
    assert i1["iterations"] <= 1 and i1["converged"]

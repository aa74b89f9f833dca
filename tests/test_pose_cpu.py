"""The pose checks checked, on the CPU (tests/pose_checks.py; the GPU side is tests/test_gpu_pose.py).

The backward kernels are emulated in numpy float32 in their own order -- k_rays_backward: a partial per thread t over r = t, t + 256, ..., an xor
butterfly over the 64 lanes of a wave, ((s0 + s1) + s2) + s3 over the four wave partials; camera_matrix_backward: statement by statement --
without FMA and with every multiply-add contracted, and must stay inside both derived bounds on every case of the builders.  Then the same
emulation with a defect planted in it must be flagged, by an error / bound ratio above 1 or by a wrong byte in the one-hot coverage check:
that is the evidence that the GPU tests would notice a subtly wrong kernel.

Worst emulated error / bound (pytest -s prints them): rays 0.10 (N = 1 ... 4999, three gradient kinds, modes 0-3, plain and contracted),
camera 0.12 and radial identity 0.05 (300 quaternions of the six kinds, two kinds of g_c2w, plain and contracted); the planted defects reach
4e2 ... 3e5, or a wrong byte."""
import math

import numpy as np
import pytest

import pose_checks as pc
from pose_checks import F32

LANES = np.arange(64)


# ---- the kernels' order in numpy float32 ---------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once (the product of two float32 is exact in fp64; the sum is rounded to fp64 and then to fp32)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emu_dirs(pi, pj, intr, mode, defect=None):
    if defect == "truncation_omitted":
        return pc.dirs_f32(pi, pj, intr, mode & 1)
    if defect == "j_for_i_in_mode_1" and (mode & 1):
        d = pc.dirs_f32(pi, pj, intr, mode)
        fx, fy, cx, cy = pc.intrinsics_f32(intr, mode)
        d[:, 1] = (np.asarray(pj).astype(np.float32) - cy) / fy
        return d
    return pc.dirs_f32(pi, pj, intr, mode)


def emu_rays_backward(pi, pj, intr, g_ro, g_rd, mode, fma=False, defect=None):
    """k_rays_backward -> g_c2w [3, 4] float32"""
    n = len(pi)
    d = emu_dirs(pi, pj, intr, mode, defect)
    g_ro, g_rd = np.asarray(g_ro, np.float32).copy(), np.asarray(g_rd, np.float32).copy()
    if defect == "last_ray_dropped":
        n -= 1
    if defect == "ray_256_skipped" and n > 256:
        g_ro[256], g_rd[256] = 0, 0                          # adding zeros is exact: the same as never visiting the ray
    S = math.ceil(n / pc.BLOCK) if n else 0
    pad = lambda a: np.concatenate([a[:n], np.zeros((S * pc.BLOCK - n,) + a.shape[1:], np.float32)]).reshape((S, pc.BLOCK) + a.shape[1:])
    go, gd, dd = pad(g_ro), pad(g_rd), pad(d)
    acc = np.zeros((pc.BLOCK, 3, 4), np.float32)
    for s in range(S):                                       # the thread-strided partials, 256 threads at a time
        if fma:
            acc[:, :, :3] = _fma(gd[s][:, :, None], dd[s][:, None, :], acc[:, :, :3])
        else:
            acc[:, :, :3] = acc[:, :, :3] + gd[s][:, :, None] * dd[s][:, None, :]
        acc[:, :, 3] = acc[:, :, 3] + go[s]
    v = acc.reshape(4, 64, 12)
    for o in (32, 16, 8, 4, 2, 1):                           # wave_sum: v += shfl_xor(v, o)
        v = v + v[:, LANES ^ o, :]
    s = v[:, 0, :]
    if defect == "wave_partial_left_out":
        s = s.copy()
        s[1] = 0
    out = ((s[0] + s[1]) + s[2]) + s[3]
    assert out.dtype == np.float32
    return out.reshape(3, 4)


def emu_camera_backward(cams, G, fma=False, defect=None):
    """camera_matrix_backward on a batch: cams [n, 7], G [n, 3, 4] float32 -> g_cam [n, 7] float32"""
    cams, G = np.asarray(cams, np.float32), np.asarray(G, np.float32)
    q = [cams[:, k] for k in range(4)]
    qr, qi, qj, qk = q
    mad = _fma if fma else (lambda a, b, c: a * b + c)
    n2 = mad(q[3], q[3], mad(q[2], q[2], mad(q[1], q[1], q[0] * q[0]))) if fma else ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    two_s = F32(2) / n2
    M = [-mad(qj, qj, qk * qk), mad(qi, qj, -(qk * qr)), mad(qi, qk, qj * qr), mad(qi, qj, qk * qr), -mad(qi, qi, qk * qk),
         mad(qj, qk, -(qi * qr)), mad(qi, qk, -(qj * qr)), mad(qj, qk, qi * qr), -mad(qi, qi, qj * qj)]
    z, m2 = np.zeros_like(qr), F32(-2)
    dM = [[z, z, m2 * qj, m2 * qk], [-qk, qj, qi, -qr], [qj, qk, qr, qi], [qk, qj, qi, qr], [z, m2 * qi, z, m2 * qk],
          [-qi, -qr, qk, qj], [-qj, qk, -qr, qi], [qi, qr, qk, qj], [z, m2 * qi, m2 * qj, z]]
    if defect == "dM_sign_flipped":
        dM[1][0] = qk
    out = np.empty((len(cams), 7), np.float32)
    for c in range(4):
        dts = ((-two_s if defect == "dts_without_2" else m2 * two_s) * q[c]) / n2
        s = np.zeros_like(qr)
        for ab in range(9):
            s = mad(G[:, ab // 3, ab % 3], mad(dts, M[ab], two_s * dM[ab][c]), s)
        out[:, c] = s
    out[:, 4:] = G[:, :, 3]
    assert n2.dtype == np.float32 and dts.dtype == np.float32
    return out


def _rays_ratio(n, kind, mode, fma=False, defect=None, seed=0):
    pi, pj = pc.pixels(n, seed)
    g_ro, g_rd = pc.ray_gradients(kind, n, seed)
    ref, A = pc.rays_backward_f64(pi, pj, pc.INTR, g_ro, g_rd, mode)
    got = emu_rays_backward(pi, pj, pc.INTR, g_ro, g_rd, mode, fma, defect)
    return pc.ratio(got.astype(np.float64) - ref, pc.rays_bound(n, A))


def _camera_ratios(kind, gkind, n, fma=False, defect=None):
    cams = pc.quaternions(kind, n)
    G = np.stack([pc.c2w_gradients(gkind, k) for k in range(n)])
    got = emu_camera_backward(cams, G, fma, defect)
    worst, radial = 0.0, 0.0
    for k in range(n):
        ref, B = pc.camera_backward_f64(cams[k], G[k])
        assert np.array_equal(got[k, 4:], G[k][:, 3])                    # the translation gradient is column 3, to the byte
        worst = max(worst, pc.ratio(got[k, :4].astype(np.float64) - ref[:4], pc.camera_bound(B)))
        radial = max(radial, pc.radial_ratio(cams[k], got[k], B))
    return worst, radial


# ---- the references themselves ---------------------------------------------------------------------------------------------------------------
def test_forward_restatements_agree_with_fp64():
    """camera_from_tensor_f32 / rays_f32 against the reference's op sequence in fp64 (oracle/torch_ref.py): each element within a few u of
    the sum of its absolute terms, so the restatements compute the right thing before any byte is compared with them"""
    import torch
    from oracle import torch_ref as T
    pi, pj = pc.pixels(300, 3)
    for kind in pc.QUAT_KINDS:
        for cam in pc.quaternions(kind, 20):
            c32 = pc.camera_from_tensor_f32(cam)
            c64 = T.get_camera_from_tensor(torch.tensor(cam.astype(np.float64))).numpy()
            assert np.abs(c32 - c64).max() <= 16 * pc.U * 3.0, (kind, cam)         # |R_ab| <= 1 = 1 - t with t <= 2: terms below 3
            assert np.array_equal(c32[:, 3], cam[4:])
            for mode in range(4):
                ro, rd = pc.rays_f32(pi, pj, pc.INTR, c32, mode)
                fx, fy, cx, cy = (float(F32(x)) for x in pc.INTR)
                ro64, rd64 = T.rays_from_pixels(torch.tensor(pi), torch.tensor(pj), fx, fy, cx, cy, torch.tensor(c32.astype(np.float64)), mode)
                assert np.array_equal(ro, ro64.numpy().astype(np.float32))
                scale = np.abs(pc.dirs_f64(pi, pj, pc.INTR, mode)) @ np.abs(c32[:, :3].astype(np.float64)).T
                assert (np.abs(rd - rd64.numpy()) <= 6 * pc.U * scale).all(), (kind, mode)
    a, b = pc.dirs_f32(pi, pj, pc.INTR, 0), pc.dirs_f32(pi, pj, pc.INTR, 2)
    assert (a[:, 0] != b[:, 0]).all() and (a[:, 1] != b[:, 1]).all()              # the intrinsics are such that the truncation shows


def test_autograd_reference_equals_the_hand_written_jacobian():
    """fp64 autograd through the reference's op sequence == the hand-written fp64 Jacobian, to 1e-12 of the sum of the absolute terms B (fp64
    leaves about 32 * 2^-53 = 4e-15 of it): the reference of the camera check is pinned from two independent sides"""
    worst = 0.0
    for kind in pc.QUAT_KINDS:
        for gk in pc.C2W_GRAD_KINDS:
            for k, cam in enumerate(pc.quaternions(kind, 25, seed=5)):
                G = pc.c2w_gradients(gk, 100 + k)
                auto, B = pc.camera_backward_f64(cam, G)
                hand = pc.camera_backward_hand_f64(cam, G.astype(np.float64))
                assert np.array_equal(auto[4:], hand[4:])
                assert (B > 0).all()
                r = float((np.abs(auto[:4] - hand[:4]) / B).max())
                worst = max(worst, r)
                assert r <= 1e-12, (kind, gk, cam, r)
    print("autograd vs hand Jacobian, worst |diff| / B: %.2e" % worst)


def test_case_builders():
    for kind in pc.QUAT_KINDS:
        q = pc.quaternions(kind, 50)
        assert q.dtype == np.float32 and q.shape == (50, 7) and np.isfinite(q).all()
        n = np.linalg.norm(q[:, :4].astype(np.float64), axis=1)
        if kind == "scaled":
            assert n.min() < 0.1 and n.max() > 10
        else:
            assert np.abs(n - 1).max() < 1e-3
    assert (pc.quaternions("half_turn", 5)[:, 0] == 0).all() and (pc.quaternions("near_half_turn", 5)[:, 0] == F32(1e-7)).all()
    wins = pc.frame_windows()
    assert len(wins["thirty_two"]["first"]) == pc.MAX_POSE_FRAMES and set(wins["thirty_two"]["count"]) == {0, 1, 64, 257}
    assert wins["five_gaps_first_inactive"]["active"][0] == 0 and not any(wins["three_all_inactive"]["active"])
    assert any(f % 256 for f in wins["five_gaps"]["first"])
    for name, w in wins.items():
        spans = sorted((f, f + c) for f, c in zip(w["first"], w["count"]) if c)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), name
        rays = pc.window_rays(w)
        live = np.zeros(rays["n"], bool)
        for f, c, a in zip(w["first"], w["count"], w["active"]):
            if a:
                live[f:f + c] = True
        assert np.isfinite(rays["g_rd"][live]).all() and np.isnan(rays["g_rd"][~live]).all() and np.isnan(rays["g_ro"][~live]).all(), name
        assert (~live).any(), name


# ---- the emulated kernels stay inside the bounds ----------------------------------------------------------------------------------------------
def test_emulated_rays_backward_inside_the_bound():
    worst = {}
    for n in pc.SIZES:
        for kind in pc.GRAD_KINDS:
            for mode in range(4):
                for fma in (False, True):
                    r = _rays_ratio(n, kind, mode, fma)
                    assert r <= 1.0, (n, kind, mode, fma, r)
                    worst[n] = max(worst.get(n, 0.0), r)
    print("emulated rays_backward error / bound per N: " + ", ".join("%d: %.3f" % kv for kv in worst.items()))
    print("emulated rays_backward worst error / bound: %.3f" % max(worst.values()))


def test_emulated_camera_backward_inside_the_bound():
    worst, radial = {}, 0.0
    for kind in pc.QUAT_KINDS:
        for gk in pc.C2W_GRAD_KINDS:
            for fma in (False, True):
                w, r = _camera_ratios(kind, gk, 50, fma)
                assert w <= 1.0 and r <= 1.0, (kind, gk, fma, w, r)
                worst[kind] = max(worst.get(kind, 0.0), w)
                radial = max(radial, r)
    print("emulated camera_backward error / bound per kind: " + ", ".join("%s: %.3f" % kv for kv in worst.items()))
    print("emulated camera_backward worst error / bound: %.3f, radial identity: %.3f" % (max(worst.values()), radial))


def _one_hot_bytes_ok(n, r, mode, defect=None):
    pi, pj = pc.pixels(n, 7)
    rng = np.random.default_rng([n, r, mode])
    go, gd = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    go[r], gd[r] = rng.standard_normal(3), rng.standard_normal(3)
    want = pc.one_hot_expected(pi, pj, pc.INTR, mode, r, go[r], gd[r])
    return all(emu_rays_backward(pi, pj, pc.INTR, go, gd, mode, fma, defect).tobytes() == want.tobytes() for fma in (False, True))


def test_one_hot_coverage_on_the_emulation():
    """a single ray's gradient comes out as its own fp32 products, byte for byte, wherever the ray sits"""
    for n in pc.SIZES:
        for r in pc.one_hot_rows(n):
            for mode in range(4):
                assert _one_hot_bytes_ok(n, r, mode), (n, r, mode)


# ---- planted defects: each must be flagged on its stated case ---------------------------------------------------------------------------------
def test_planted_defects_in_the_reduction_are_flagged():
    """stated cases: N = 257 (two strides, the last ray alone in its stride), normal gradients, mode 0, for the ratio; the one-hot rays N - 1,
    256 and 64 (wave 1) for the bytes"""
    for defect, hot in (("last_ray_dropped", 256), ("ray_256_skipped", 256), ("wave_partial_left_out", 64)):
        r = _rays_ratio(257, "normal", 0, defect=defect)
        ok = _one_hot_bytes_ok(257, hot, 0, defect)
        print("defect %-22s rays error / bound %.3g (N 257, normal), one-hot ray %d bytes %s" % (defect, r, hot, "equal" if ok else "DIFFER"))
        assert r > 1.0 and not ok, defect
    # the nine-decade kind may hide a small dropped ray under the bound of the large ones: there the one-hot bytes are the check
    assert not _one_hot_bytes_ok(4999, 4998, 0, "last_ray_dropped")


def test_planted_defects_in_the_ray_directions_are_flagged():
    """stated cases: N = 257, normal gradients, mode 2 (truncation omitted) and mode 1 (j used for i): the backward leaves its bound, the
    one-hot bytes differ, and the forward rays differ from rays_f32 in bytes"""
    pi, pj = pc.pixels(257, 0)
    c2w = pc.camera_from_tensor_f32(pc.quaternions("unit", 1)[0])
    for defect, mode in (("truncation_omitted", 2), ("truncation_omitted", 3), ("j_for_i_in_mode_1", 1), ("j_for_i_in_mode_1", 3)):
        r = _rays_ratio(257, "normal", mode, defect=defect)
        ok = _one_hot_bytes_ok(257, 63, mode, defect)
        d = emu_dirs(pi, pj, pc.INTR, mode, defect)
        rd_bad = np.stack([(d[:, 0] * c2w[a, 0] + d[:, 1] * c2w[a, 1]) + d[:, 2] * c2w[a, 2] for a in range(3)], -1)
        same = rd_bad.tobytes() == pc.rays_f32(pi, pj, pc.INTR, c2w, mode)[1].tobytes()
        print("defect %-22s mode %d: rays error / bound %.3g, one-hot bytes %s, forward bytes %s"
              % (defect, mode, r, "equal" if ok else "DIFFER", "equal" if same else "DIFFER"))
        assert r > 1.0 and not ok and not same, (defect, mode)
    # and the unplanted emulation of the forward is rays_f32, so "differs" above is the defect's doing
    d = emu_dirs(pi, pj, pc.INTR, 1)
    assert np.array_equal(d, pc.dirs_f32(pi, pj, pc.INTR, 1))


@pytest.mark.parametrize("defect", ["dM_sign_flipped", "dts_without_2"])
def test_planted_defects_in_the_camera_jacobian_are_flagged(defect):
    """stated cases: unit quaternions, both kinds of g_c2w (a wrong dts moves the gradient along q, so the radial identity sees it too)"""
    for gk in pc.C2W_GRAD_KINDS:
        w, radial = _camera_ratios("unit", gk, 20, defect=defect)
        print("defect %-16s g_c2w %-13s camera error / bound %.3g, radial %.3g" % (defect, gk, w, radial))
        assert w > 1.0, (defect, gk)
        if defect == "dts_without_2":
            assert radial > 1.0, gk

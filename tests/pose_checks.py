"""The pose chain, component by component: fp32 restatements of the forward kernels, fp64 references of the two backward kernels, a derived
bound on what fp32 may differ from them, and the cases (quaternions, ray gradients, frame tables) the CPU and GPU tests share.

The chain (csrc/nsk.hip): k_camera_from_tensor (camera_matrix: 7-vector -> 3x4), k_rays_from_pixels / k_rays_from_camera (pixel -> ray),
k_rays_backward (ray gradients -> d c2w, one block of 256 threads), k_camera_backward (camera_matrix_backward: d c2w -> d 7-vector) and the
fused k_pose_step / k_pose_multi (the two backward kernels and Adam on the pose in one launch; a frame per block).

Forward: to the bit.  camera_matrix forbids contraction (#pragma clang fp contract(off)) and the ray direction is written with add_rn / mul_rn /
sub_rn / div_rn, so every operation rounds on its own and the result is DEFINED: camera_from_tensor_f32 and rays_f32 restate the same operations
in numpy float32 (numpy fuses nothing; its float32 divide is correctly rounded, as the device's is) and the GPU tests compare bytes.

Backward: under a bound.  The order of a reduction is the kernel's business, so the two backward kernels are compared with fp64 values of the
same fp32 inputs.  u = 2^-24 is the relative error of one correctly rounded fp32 operation.  An fp32 sum of terms t_k, however ordered, differs
from the exact sum by at most (roundings on the longest path through the sum) * u * sum |t_k| to first order, and a term formed with j roundings
carries j * u |t_k| itself.  Both bounds below count operations; no factor was fitted to any output, and contraction into FMAs only removes
roundings from the count.

  rays_bound = (ceil(N / 256) + 12) * u * A,      A[a, b] = sum_r |g_rd[r, a] * dir_r[b]|   (b < 3),    A[a, 3] = sum_r |g_ro[r, a]|
      A thread adds at most ceil(N / 256) terms in sequence (r = t, t + 256, ...), the xor butterfly over the 64 lanes adds 6 levels, the four wave
      partials take 3 more adds: ceil(N / 256) + 9 roundings on the longest path.  A term g * dir carries 3: the subtraction i - cx, the division
      by fx, the product.  (The translation column adds g_ro itself: no rounding in the term, same path.)
  camera_bound = 32 * u * B,      B[c] = sum_ab |G_ab| * (|dts_c| * Mabs_ab + |two_s| * |dM_ab,c|)
      with R = I + two_s * M, n2 = |q|^2, two_s = 2 / n2, dts_c = d two_s / d q_c = -2 two_s q_c / n2, dM the table of d M_ab / d q_c, and Mabs_ab
      the sum of the absolute values of the products that make up M_ab (|qi qj| + |qk qr| for M_01, qj^2 + qk^2 for M_00).  g_cam[c] is a sum of
      9 terms (9 adds); a term G * (dts * M + two_s * dM) carries: n2 (4 products, 3 adds -- 4 roundings on its longest path), two_s (1), dts (3:
      two products and a division), M_ab (3: two products and an add, relative to Mabs), dM (1: the factor 2), the two inner products (2), their
      sum (1) and the product with G (1) -- about 20 once n2 and two_s are counted for both inner products.  9 + 20 = 29 <= 32.
      g_cam[4:7] is column 3 of G, copied: exact.

  The radial identity: R does not depend on |q|, so sum_c q_c * g_cam[c] = 0 exactly in real arithmetic, whatever G; in fp32
  |sum_c q_c g_c| <= 32 u sum_c |q_c| B_c (each g_c within its bound of a set of values whose weighted sum is zero).

This module imports nothing from the device path."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
INTR = (360.7, 355.2, 320.5, 239.5)          # non-integer on purpose: mode & 2 truncates all four, so modes 2 and 3 differ from 0 and 1
WIDTH, HEIGHT = 640, 480
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4999)
BLOCK = 256                                   # threads of the reducing block
QUAT_KINDS = ("unit", "near_identity", "scaled", "half_turn", "near_half_turn", "near_quarter_turn")
GRAD_KINDS = ("normal", "alternating", "decades")
C2W_GRAD_KINDS = ("normal", "near_identity")
MAX_POSE_FRAMES = 32                          # NSK_MAX_POSE_FRAMES
SENTINEL = F32(-77.25)


# ---- forward, fp32, operation by operation -------------------------------------------------------------------------------------------------
def camera_from_tensor_f32(cam):
    """camera_matrix (quad2rotation + the translation column) in float32, every product and sum rounded on its own, in the kernel's order"""
    c = np.asarray(cam, np.float32)
    qr, qi, qj, qk = c[0], c[1], c[2], c[3]
    rr, ii, jj, kk = qr * qr, qi * qi, qj * qj, qk * qk
    ssum = ((rr + ii) + jj) + kk
    two_s = F32(2) / ssum
    ij, ik, jk, ir, jr, kr = qi * qj, qi * qk, qj * qk, qi * qr, qj * qr, qk * qr
    s0, s1, s2 = jj + kk, ii + kk, ii + jj
    a01, a02, a10, a12, a20, a21 = ij - kr, ik + jr, ij + kr, jk - ir, ik - jr, jk + ir
    t0, t1, t2 = two_s * s0, two_s * s1, two_s * s2
    R = [F32(1) - t0, two_s * a01, two_s * a02, two_s * a10, F32(1) - t1, two_s * a12, two_s * a20, two_s * a21, F32(1) - t2]
    out = np.empty((3, 4), np.float32)
    out[:, :3] = np.array(R, np.float32).reshape(3, 3)
    out[:, 3] = c[4:7]
    assert all(isinstance(x, np.float32) for x in R)
    return out


def intrinsics_f32(intr, mode):
    """the four float32 intrinsics the kernels see: mode & 2 truncates them towards zero first (intr(), D10)"""
    v = [F32(x) for x in intr]
    if mode & 2:
        v = [F32(int(x)) for x in v]
    return v


def dirs_f32(pi, pj, intr, mode):
    """camera-frame directions [N, 3] float32: div_rn(sub_rn(i, cx), fx), the mode & 1 form of the second, -1"""
    fx, fy, cx, cy = intrinsics_f32(intr, mode)
    i, j = np.asarray(pi).astype(np.float32), np.asarray(pj).astype(np.float32)
    d0 = (i - cx) / fx
    d1 = (i - cy) / fy if (mode & 1) else -((j - cy) / fy)
    return np.stack([d0, d1, np.full_like(d0, -1)], -1)


def rays_f32(pi, pj, intr, c2w, mode):
    """k_rays_from_pixels in float32 -> (rays_o, rays_d): rd[a] = add_rn(add_rn(mul_rn(d0, c[a,0]), mul_rn(d1, c[a,1])), mul_rn(-1, c[a,2]))"""
    c = np.asarray(c2w, np.float32).reshape(3, 4)
    d = dirs_f32(pi, pj, intr, mode)
    rd = np.stack([(d[:, 0] * c[a, 0] + d[:, 1] * c[a, 1]) + d[:, 2] * c[a, 2] for a in range(3)], -1)
    ro = np.broadcast_to(c[:, 3], rd.shape).copy()
    assert rd.dtype == np.float32
    return ro, rd


# ---- backward, fp64, with the sums of absolute terms ---------------------------------------------------------------------------------------
def dirs_f64(pi, pj, intr, mode):
    """the directions in fp64 from the fp32 pixel and intrinsic values (truncated first if mode & 2)"""
    fx, fy, cx, cy = (float(x) for x in intrinsics_f32(intr, mode))
    i, j = np.asarray(pi).astype(np.float64), np.asarray(pj).astype(np.float64)
    d0 = (i - cx) / fx
    d1 = (i - cy) / fy if (mode & 1) else -(j - cy) / fy
    return np.stack([d0, d1, np.full_like(d0, -1)], -1)


def rays_backward_f64(pi, pj, intr, g_ro, g_rd, mode):
    """-> (g_c2w [3, 4] fp64, A [3, 4]: per element the sum of the absolute values of its terms)"""
    d = dirs_f64(pi, pj, intr, mode)
    go, gd = np.asarray(g_ro, np.float32).astype(np.float64), np.asarray(g_rd, np.float32).astype(np.float64)
    t = gd[:, :, None] * d[:, None, :]                      # [N, a, b]
    g, A = np.empty((3, 4)), np.empty((3, 4))
    g[:, :3], A[:, :3] = t.sum(0), np.abs(t).sum(0)
    g[:, 3], A[:, 3] = go.sum(0), np.abs(go).sum(0)
    return g, A


def rays_bound(n, A):
    """(ceil(N / 256) + 12) u A -- module docstring"""
    return (math.ceil(n / BLOCK) + 12) * U * np.asarray(A, np.float64)


def camera_parts_f64(cam):
    """the pieces of camera_matrix_backward in fp64: dict(q, n2, two_s, M [9], Mabs [9], dM [9, 4], dts [4])"""
    q = np.asarray(cam, np.float32).astype(np.float64)[:4]
    qr, qi, qj, qk = q
    n2 = float(q @ q)
    two_s = 2.0 / n2
    M = np.array([-(qj * qj + qk * qk), qi * qj - qk * qr, qi * qk + qj * qr, qi * qj + qk * qr, -(qi * qi + qk * qk),
                  qj * qk - qi * qr, qi * qk - qj * qr, qj * qk + qi * qr, -(qi * qi + qj * qj)])
    a = abs
    Mabs = np.array([qj * qj + qk * qk, a(qi * qj) + a(qk * qr), a(qi * qk) + a(qj * qr), a(qi * qj) + a(qk * qr), qi * qi + qk * qk,
                     a(qj * qk) + a(qi * qr), a(qi * qk) + a(qj * qr), a(qj * qk) + a(qi * qr), qi * qi + qj * qj])
    dM = np.array([[0, 0, -2 * qj, -2 * qk], [-qk, qj, qi, -qr], [qj, qk, qr, qi], [qk, qj, qi, qr], [0, -2 * qi, 0, -2 * qk],
                   [-qi, -qr, qk, qj], [-qj, qk, -qr, qi], [qi, qr, qk, qj], [0, -2 * qi, -2 * qj, 0]], np.float64)
    dts = -2.0 * two_s * q / n2
    return dict(q=q, n2=n2, two_s=two_s, M=M, Mabs=Mabs, dM=dM, dts=dts)


def camera_backward_hand_f64(cam, g_c2w):
    """the hand-written Jacobian in fp64 (the kernel's own table): only there to pin the autograd reference, tests/test_pose_cpu.py"""
    P = camera_parts_f64(cam)
    G = np.asarray(g_c2w, np.float64).reshape(3, 4)
    J = P["dts"][None, :] * P["M"][:, None] + P["two_s"] * P["dM"]             # [9, 4]
    return np.concatenate([G[:, :3].reshape(9) @ J, G[:, 3]])


def camera_backward_f64(cam, g_c2w):
    """-> (g_cam [7] fp64, B [4]).  g_cam[0:4]: torch fp64 autograd through the reference's op sequence (oracle/torch_ref.py
    get_camera_from_tensor), independent of the kernel's dM table; g_cam[4:7]: column 3 of g_c2w; B: module docstring"""
    import torch
    from oracle import torch_ref as T
    G = np.asarray(g_c2w, np.float32).astype(np.float64).reshape(3, 4)
    x = torch.tensor(np.asarray(cam, np.float32).astype(np.float64), dtype=torch.float64, requires_grad=True)
    (T.get_camera_from_tensor(x) * torch.tensor(G, dtype=torch.float64)).sum().backward()
    g = x.grad.numpy().copy()
    g[4:7] = G[:, 3]
    P = camera_parts_f64(cam)
    aG = np.abs(G[:, :3]).reshape(9)
    B = aG @ (np.abs(P["dts"])[None, :] * P["Mabs"][:, None] + abs(P["two_s"]) * np.abs(P["dM"]))
    return g, B


def camera_bound(B):
    """32 u B -- module docstring"""
    return 32 * U * np.asarray(B, np.float64)


def ratio(err, bound):
    """largest |err| / bound; 0 where the error is 0, inf where the bound is 0 and the error is not"""
    err, bound = np.abs(np.asarray(err, np.float64)).ravel(), np.asarray(bound, np.float64).ravel()
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    r = np.where(np.isfinite(err), r, np.inf)
    return float(r.max()) if r.size else 0.0


def radial_ratio(cam, g_cam, B):
    """|sum_c q_c g_c| / (32 u sum_c |q_c| B_c)"""
    q = np.asarray(cam, np.float32).astype(np.float64)[:4]
    g = np.asarray(g_cam, np.float64)[:4]
    return ratio(abs(float(q @ g)), 32 * U * float(np.abs(q) @ np.asarray(B, np.float64)))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def quaternions(kind, n, seed=0):
    """n pose 7-vectors [n, 7] float32 of one kind; the translation is N(0, 1)"""
    rng = np.random.default_rng([seed, QUAT_KINDS.index(kind)])
    unit = rng.standard_normal((n, 4))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    if kind == "unit":
        q = unit
    elif kind == "near_identity":
        q = np.array([1.0, 0, 0, 0]) + 1e-4 * rng.standard_normal((n, 4))
    elif kind == "scaled":                                  # what Adam leaves: nothing renormalises the pose
        q = unit * 10.0 ** rng.uniform(-2, 2, (n, 1))
    elif kind in ("half_turn", "near_half_turn"):           # qr = 0 and qr = 1e-7: rotations by 180 degrees
        q = unit.copy()
        q[:, 0] = 0.0
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q[:, 0] = 0.0 if kind == "half_turn" else 1e-7
    elif kind == "near_quarter_turn":
        q = np.array([math.sqrt(0.5), math.sqrt(0.5), 0, 0]) + 1e-6 * rng.standard_normal((n, 4))
    else:
        raise KeyError(kind)
    return np.concatenate([q, rng.standard_normal((n, 3))], 1).astype(np.float32)


def pixels(n, seed=0):
    rng = np.random.default_rng([seed, 101])
    return rng.integers(0, WIDTH, n).astype(np.int32), rng.integers(0, HEIGHT, n).astype(np.int32)


def ray_gradients(kind, n, seed=0):
    """(g_ro, g_rd) [n, 3] float32 of one kind"""
    rng = np.random.default_rng([seed, 202, GRAD_KINDS.index(kind)])
    x = rng.standard_normal((2, n, 3))
    if kind == "alternating":                               # a converging Tracker: residuals of either sign that nearly cancel
        x = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[None, :, None] + 1e-3 * x
    elif kind == "decades":
        x = x * 10.0 ** rng.uniform(-6, 3, (1, n, 1))
    elif kind != "normal":
        raise KeyError(kind)
    return x[0].astype(np.float32), x[1].astype(np.float32)


def c2w_gradients(kind, seed=0):
    """g_c2w [3, 4] float32: normal, or I + 1e-3 noise in the rotation block (the cancelling kind: sum_ab R_ab dR_ab = 0)"""
    rng = np.random.default_rng([seed, 303, C2W_GRAD_KINDS.index(kind)])
    g = rng.standard_normal((3, 4))
    if kind == "near_identity":
        g[:, :3] = np.eye(3) + 1e-3 * g[:, :3]
    return g.astype(np.float32)


def one_hot_rows(n):
    """the rays at which the exact-coverage check plants its single gradient: the edges of a wave, of the block, of the batch"""
    return sorted({r for r in (0, 63, 64, 255, 256, n - 1) if 0 <= r < n})


def one_hot_expected(pi, pj, intr, mode, r, g_ro_r, g_rd_r):
    """g_c2w [3, 4] float32 of a batch whose only non-zero gradient is at ray r: the fp32 products fl(g * dir) and the planted g_ro.  Every other
    term is an exact zero, and fl(g * dir + 0) = fl(g * dir), so a contracted evaluation gives the same bytes; 0 + x also turns a -0 product
    into +0, as the kernel's accumulator (which starts at +0) does"""
    d = dirs_f32(pi[r:r + 1], pj[r:r + 1], intr, mode)[0]
    g = np.zeros((3, 4), np.float32)
    g[:, :3] = F32(0) + np.asarray(g_rd_r, np.float32)[:, None] * d[None, :]
    g[:, 3] = F32(0) + np.asarray(g_ro_r, np.float32)
    return g


def frame_windows():
    """the frame tables of k_pose_multi: name -> dict(first, count, active) (lists of nf ints)"""
    cyc = (0, 1, 64, 257)
    w = {}
    w["one"] = dict(first=[0], count=[257], active=[1])
    w["three_contiguous"] = dict(first=[0, 100, 357], count=[100, 257, 64], active=[1, 1, 1])
    w["five_gaps"] = dict(first=[7, 300, 777, 1100, 1500], count=[200, 65, 256, 1, 333], active=[1, 1, 1, 1, 1])
    w["five_gaps_first_inactive"] = dict(w["five_gaps"], active=[0, 1, 0, 1, 1])
    w["three_all_inactive"] = dict(w["three_contiguous"], active=[0, 0, 0])
    w["active_empty"] = dict(first=[5, 70, 70], count=[65, 0, 63], active=[1, 1, 1])
    first, count, at = [], [], 3
    for f in range(MAX_POSE_FRAMES):
        first.append(at); count.append(cyc[f % 4])
        at += cyc[f % 4] + (f % 3)                          # gaps of 0, 1, 2 rays
    w["thirty_two"] = dict(first=first, count=count, active=[1] * MAX_POSE_FRAMES)
    w["thirty_two_mixed"] = dict(first=first, count=count, active=[int(f % 3 != 1) for f in range(MAX_POSE_FRAMES)])
    return w


def window_rays(win, seed=0):
    """the ray arrays of a window: dict(pi, pj, g_ro, g_rd, n).  A ray that belongs to no frame, or to an inactive one, carries NaN in g_ro and
    g_rd: whatever reads it shows in the output"""
    n = max(f + c for f, c in zip(win["first"], win["count"])) + 9
    pi, pj = pixels(n, seed + 1)
    g_ro, g_rd = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
    for k, (f, c, a) in enumerate(zip(win["first"], win["count"], win["active"])):
        if a and c:
            go, gd = ray_gradients(GRAD_KINDS[k % 3], c, seed + 10 + k)
            g_ro[f:f + c], g_rd[f:f + c] = go, gd
    return dict(pi=pi, pj=pj, g_ro=g_ro, g_rd=g_rd, n=n)

"""The pose chain on the device, component by component (-m gpu): k_camera_from_tensor, k_rays_from_pixels / k_rays_from_camera, k_rays_backward,
k_camera_backward and the fused k_pose_step / k_pose_multi against tests/pose_checks.py.  The forward kernels are compared to the bit with
their float32 restatements; the two backward kernels element by element with fp64 values of the same inputs, inside bounds derived from
operation counts (pose_checks' docstring; tests/test_pose_cpu.py shows that planted defects leave them); the fused kernels to the bit with
their parts, and k_pose_multi's frame table on windows whose unowned rays carry NaN.  The context is only a handle here.

Worst device error / bound on the MI355X (pytest -m gpu -s prints them): rays_backward 0.10 (per N: 1: 0.094, 63: 0.099, 64: 0.099, 65: 0.096,
255: 0.078, 256: 0.062, 257: 0.053, 1000: 0.028, 4999: 0.015 -- the figures of the numpy emulation, digit for digit), camera_backward 0.12 (unit
0.111, near identity 0.084, far from unit 0.098, half turn 0.063, near half turn 0.062, near quarter turn 0.122), radial identity 0.05, the pose
under Adam 0.74 of adam_checks' bound.

What the first run of this module found: k_pose_step and k_pose_multi did not equal their parts.  camera_matrix_backward was contracted into
FMAs differently in each kernel it is inlined into (rotation gradients off in the last bits, at N = 1 already), and the device assembly showed
k_pose_multi fusing the two moment updates of Adam that k_pose_step and k_adam_scalar leave as rounded products and a sum (the gradients failed
first, so no run saw that one fail).  csrc/nsk.hip now has one uncontracted body
for each of the three pieces (rays_backward_block, camera_matrix_backward, adam_scalar_update)."""
import numpy as np
import pytest
import torch

import adam_checks as ac
import pose_checks as pc
import scenes
from gpu_util import cu, make_ctx

pytestmark = pytest.mark.gpu
LR = 1e-3


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx(scenes.make_scene(1, scenes.SMALL_GRID_SHAPES))
    yield c
    c.close()


def ci(a):
    return cu(a, torch.int32)


def host(t):
    return t.detach().cpu().numpy()


def same(a, b):
    """byte for byte (NaN payloads and the sign of zero included)"""
    a = host(a) if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    b = host(b) if isinstance(b, torch.Tensor) else np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- a. forward, to the bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.QUAT_KINDS)
def test_forward_to_the_bit(ctx, kind):
    """camera_from_tensor == camera_from_tensor_f32, rays_from_pixels == rays_f32 (rays_o AND rays_d, modes 0-3, intrinsics the truncation of
    mode & 2 changes), rays_from_camera == the two-step form and hands back the same matrix: all byte for byte, 257 rays (two blocks)"""
    n = 257
    pi, pj = pc.pixels(n, 1)
    d_pi, d_pj = ci(pi), ci(pj)
    for cam in pc.quaternions(kind, 8, seed=1):
        d_cam = cu(cam)
        c2w = ctx.camera_from_tensor(d_cam)
        want = pc.camera_from_tensor_f32(cam)
        assert same(c2w, want), (kind, cam, host(c2w), want)
        for mode in range(4):
            ro, rd = ctx.rays_from_pixels(d_pi, d_pj, pc.INTR, c2w, mode)
            ro_ref, rd_ref = pc.rays_f32(pi, pj, pc.INTR, want, mode)
            assert same(ro, ro_ref), (kind, cam, mode)
            assert same(rd, rd_ref), (kind, cam, mode, int((host(rd) != rd_ref).sum()))
            ro2, rd2, c2w2 = ctx.rays_from_camera(d_pi, d_pj, pc.INTR, d_cam, mode, want_c2w=True)
            assert same(ro2, ro) and same(rd2, rd) and same(c2w2, c2w), (kind, cam, mode)
            ro3, rd3 = ctx.rays_from_camera(d_pi, d_pj, pc.INTR, d_cam, mode)
            assert same(ro3, ro) and same(rd3, rd)


# ---- b. rays_backward under the bound --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.SIZES)
def test_rays_backward_inside_the_bound(ctx, n):
    """every N x gradient kind x mode: each of the 12 elements within (ceil(N / 256) + 12) u A of the fp64 value"""
    pi, pj = pc.pixels(n, 0)
    d_pi, d_pj = ci(pi), ci(pj)
    worst = 0.0
    for kind in pc.GRAD_KINDS:
        g_ro, g_rd = pc.ray_gradients(kind, n, 0)
        d_go, d_gd = cu(g_ro), cu(g_rd)
        for mode in range(4):
            got = host(ctx.rays_backward(d_pi, d_pj, pc.INTR, d_go, d_gd, mode)).astype(np.float64)
            ref, A = pc.rays_backward_f64(pi, pj, pc.INTR, g_ro, g_rd, mode)
            r = pc.ratio(got - ref, pc.rays_bound(n, A))
            worst = max(worst, r)
            assert r <= 1.0, (n, kind, mode, r, got, ref)
    print("rays_backward error / bound N=%d: %.3f" % (n, worst))


# ---- c. exact coverage -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.SIZES)
def test_rays_backward_counts_every_ray_once(ctx, n):
    """one ray with a gradient, at the edges of a wave, of the block and of the batch: g_c2w is that ray's own fp32 products and its g_ro, byte
    for byte -- the other terms are exact zeros, so a ray counted twice or never is a wrong byte whatever its size"""
    pi, pj = pc.pixels(n, 7)
    d_pi, d_pj = ci(pi), ci(pj)
    for r in pc.one_hot_rows(n):
        for mode in range(4):
            rng = np.random.default_rng([n, r, mode])
            go, gd = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
            go[r], gd[r] = rng.standard_normal(3), rng.standard_normal(3)
            got = ctx.rays_backward(d_pi, d_pj, pc.INTR, cu(go), cu(gd), mode)
            want = pc.one_hot_expected(pi, pj, pc.INTR, mode, r, go[r], gd[r])
            assert same(got, want), (n, r, mode, host(got), want)


# ---- d. camera_backward under the bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.QUAT_KINDS)
def test_camera_backward_inside_the_bound(ctx, kind):
    """components 0-3 within 32 u B of fp64 autograd through the reference's op sequence, 4-6 exact, and the radial identity"""
    worst, radial = 0.0, 0.0
    for gk in pc.C2W_GRAD_KINDS:
        for k, cam in enumerate(pc.quaternions(kind, 16, seed=2)):
            G = pc.c2w_gradients(gk, k)
            got = host(ctx.camera_backward(cu(cam), cu(G)))
            ref, B = pc.camera_backward_f64(cam, G)
            assert same(got[4:], G[:, 3]), (kind, gk, cam)
            r = pc.ratio(got[:4].astype(np.float64) - ref[:4], pc.camera_bound(B))
            rr = pc.radial_ratio(cam, got, B)
            worst, radial = max(worst, r), max(radial, rr)
            assert r <= 1.0 and rr <= 1.0, (kind, gk, cam, r, rr, got, ref)
    print("camera_backward error / bound %s: %.3f, radial identity %.3f" % (kind, worst, radial))


# ---- e. pose_step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unit", "scaled", "half_turn"])
def test_pose_step_equals_its_parts_and_follows_adam(ctx, kind):
    """steps 1..5 and one at step 1000, N = 257, a new batch of gradients (kinds and modes cycling) each step: g_cam_out == camera_backward(
    rays_backward) and cam, m, v == the adam_vector path byte for byte; cam, m, v inside adam_checks' bound of the fp64 trajectory fed the
    device's own gradients"""
    n = 257
    pi, pj = pc.pixels(n, 3)
    d_pi, d_pj = ci(pi), ci(pj)
    cam0 = pc.quaternions(kind, 1, seed=3)[0]
    cam_a, m_a, v_a = cu(cam0), torch.zeros(7, device="cuda"), torch.zeros(7, device="cuda")
    cam_b, m_b, v_b = cam_a.clone(), m_a.clone(), v_a.clone()
    track = ac.AdamTrack(cam0)
    ratios = []
    for t, step in enumerate((1, 2, 3, 4, 5, 1000)):
        mode = t % 4
        g_ro, g_rd = pc.ray_gradients(pc.GRAD_KINDS[t % 3], n, 20 + t)
        d_go, d_gd = cu(g_ro), cu(g_rd)
        g_cam = ctx.camera_backward(cam_a, ctx.rays_backward(d_pi, d_pj, pc.INTR, d_go, d_gd, mode))
        ctx.adam_vector(cam_a, g_cam, m_a, v_a, LR, step)
        g_out = torch.full((7,), float(pc.SENTINEL), device="cuda")
        ctx.pose_step(d_pi, d_pj, pc.INTR, d_go, d_gd, cam_b, m_b, v_b, LR, step, mode, g_cam_out=g_out)
        ctx.sync()
        assert same(g_out, g_cam), (kind, step, host(g_out), host(g_cam))
        assert same(cam_b, cam_a) and same(m_b, m_a) and same(v_b, v_a), (kind, step)
        assert np.isfinite(host(g_out)).all() and np.isfinite(host(cam_b)).all()
        track.step(host(g_out), LR, step)
        assert not track.near_range_edge().any()
        for what, dev in (("p", cam_b), ("m", m_b), ("v", v_b)):
            r = track.compare(host(dev), what=what)
            assert r["excluded"] == 0 and r["nonfinite"] == 0 and r["ratio"] <= 1.0, (kind, step, what, r)
            ratios.append(r["ratio"])
    print("pose_step Adam error / bound %s: %.3f" % (kind, max(ratios)))


def test_pose_step_gradient_equals_its_parts_at_every_size(ctx):
    """the fused kernel carries its own copy of the reduction: its g_cam_out == camera_backward(rays_backward) byte for byte at every N of the
    sweep (one step from planted moments, gradient kinds and modes cycling)"""
    for k, n in enumerate(pc.SIZES):
        pi, pj = pc.pixels(n, 4)
        d_pi, d_pj = ci(pi), ci(pj)
        g_ro, g_rd = pc.ray_gradients(pc.GRAD_KINDS[k % 3], n, 30 + k)
        d_go, d_gd = cu(g_ro), cu(g_rd)
        cam = pc.quaternions(pc.QUAT_KINDS[k % len(pc.QUAT_KINDS)], 1, seed=4)[0]
        mode = k % 4
        g_cam = ctx.camera_backward(cu(cam), ctx.rays_backward(d_pi, d_pj, pc.INTR, d_go, d_gd, mode))
        g_out = torch.full((7,), float(pc.SENTINEL), device="cuda")
        ctx.pose_step(d_pi, d_pj, pc.INTR, d_go, d_gd, cu(cam), torch.zeros(7, device="cuda"), torch.zeros(7, device="cuda"), LR, 1, mode, g_cam_out=g_out)
        assert same(g_out, g_cam), (n, mode, host(g_out), host(g_cam))


# ---- f. pose_step_multi: the frame table ------------------------------------------------------------------------------------------------------
def _window_state(nf, seed):
    """cams, m, v [nf, 8] float32: quaternion kinds cycling over the frames, planted moments, the unused eighth float a sentinel"""
    rng = np.random.default_rng([seed, 505])
    cams = np.full((nf, 8), pc.SENTINEL, np.float32)
    for f in range(nf):
        cams[f, :7] = pc.quaternions(pc.QUAT_KINDS[f % len(pc.QUAT_KINDS)], 1, seed=seed + f)[0]
    m, v = np.full((nf, 8), pc.SENTINEL, np.float32), np.full((nf, 8), pc.SENTINEL, np.float32)
    m[:, :7], v[:, :7] = rng.standard_normal((nf, 7)) * 0.1, rng.random((nf, 7)) * 0.01
    return cams, m, v


def _check_window(ctx, win, dev, cams0, m0, v0, step, mode, with_moments, keep=None):
    """one launch of pose_step_multi and every assertion on what it wrote; -> g_cams (host)"""
    first, count, active = win["first"], win["count"], win["active"]
    nf = len(first)
    cams, m, v = cu(cams0), cu(m0), cu(v0)
    g = torch.full((8 * nf + 8,), float(pc.SENTINEL), device="cuda")
    ctx.pose_step_multi(first, count, active, dev["pi"], dev["pj"], pc.INTR, dev["g_ro"], dev["g_rd"], cams, m if with_moments else None,
                        v if with_moments else None, lr=LR, step=step, mode=mode, g_cams=g, keep=keep)
    ctx.sync()
    tag = (nf, step, mode)
    hg, hc, hm, hv = host(g), host(cams), host(m), host(v)
    for name, a in (("g_cams", hg), ("cams", hc), ("m", hm), ("v", hv)):
        assert not np.isnan(a).any(), (tag, name)                                   # a ray outside every active range was read
    assert same(hc[:, 7], cams0[:, 7]) and same(hm[:, 7], m0[:, 7]) and same(hv[:, 7], v0[:, 7]), tag
    if step == 0:
        assert same(hc, cams0) and same(hm, m0) and same(hv, v0), tag
    for f in range(nf):
        row = hg[8 * f:8 * f + 8]
        assert row[7] == 0, (tag, f)
        if not active[f]:
            assert (row == 0).all(), (tag, f, row)
            assert same(hc[f], cams0[f]) and same(hm[f], m0[f]) and same(hv[f], v0[f]), (tag, f)
            continue
        cam7, m7, v7 = cu(cams0[f, :7]), cu(m0[f, :7]), cu(v0[f, :7])
        if count[f] == 0:
            assert (row == 0).all(), (tag, f, row)
            if step:
                ctx.adam_vector(cam7, torch.zeros(7, device="cuda"), m7, v7, LR, step)
        else:
            s = slice(first[f], first[f] + count[f])
            g7 = torch.full((7,), float(pc.SENTINEL), device="cuda")
            ctx.pose_step(dev["pi"][s].clone(), dev["pj"][s].clone(), pc.INTR, dev["g_ro"][s].clone(), dev["g_rd"][s].clone(), cam7, m7, v7, LR,
                          max(step, 1), mode, g_cam_out=g7)
            assert same(row[:7], g7), (tag, f, row, host(g7))
        if step:
            assert same(hc[f, :7], cam7) and same(hm[f, :7], m7) and same(hv[f, :7], v7), (tag, f)
    return hg


@pytest.mark.parametrize("name", list(pc.frame_windows()))
def test_pose_step_multi_frame_table(ctx, name):
    """every active frame == pose_step on a contiguous copy of its slice (gradient; with step >= 1 cam, m, v too), a count-0 active frame ==
    adam_vector with a zero gradient, inactive frames zero gradients and untouched state, slot 8 f + 7 zero, the row after the last frame
    untouched without `keep`, step 0 leaves the poses alone and needs no moments, and no NaN of an unowned ray anywhere"""
    win = pc.frame_windows()[name]
    nf = len(win["first"])
    rays = pc.window_rays(win, seed=nf)
    dev = dict(pi=ci(rays["pi"]), pj=ci(rays["pj"]), g_ro=cu(rays["g_ro"]), g_rd=cu(rays["g_rd"]))
    cams0, m0, v0 = _window_state(nf, seed=nf)
    for step, mode, with_moments in ((0, 0, False), (0, 3, True), (1, 2, True), (7, 1, True)):
        hg = _check_window(ctx, win, dev, cams0, m0, v0, step, mode, with_moments)
        assert (hg[8 * nf:] == pc.SENTINEL).all(), (name, step, hg[8 * nf:])


@pytest.mark.parametrize("n_keep", [1, 255, 256, 257, 4999])
def test_pose_step_multi_counts_the_kept_rays(ctx, n_keep):
    """with `keep`: slot 8 nf + 1 == keep.sum() (random, all-zero and all-one masks), the other seven slots of that row stay untouched, the
    frames' gradients are what they are without it"""
    win = pc.frame_windows()["three_contiguous"]
    nf = len(win["first"])
    rays = pc.window_rays(win, seed=9)
    dev = dict(pi=ci(rays["pi"]), pj=ci(rays["pj"]), g_ro=cu(rays["g_ro"]), g_rd=cu(rays["g_rd"]))
    cams0, m0, v0 = _window_state(nf, seed=9)
    plain = _check_window(ctx, win, dev, cams0, m0, v0, 0, 0, False)
    rng = np.random.default_rng(n_keep)
    for mask in ((rng.random(n_keep) < 0.6), np.zeros(n_keep, bool), np.ones(n_keep, bool)):
        keep = cu(mask.astype(np.uint8), torch.uint8)
        hg = _check_window(ctx, win, dev, cams0, m0, v0, 0, 0, False, keep=keep)
        tail = hg[8 * nf:]
        assert tail[1] == float(mask.sum()), (n_keep, tail, int(mask.sum()))
        assert (np.delete(tail, 1) == pc.SENTINEL).all(), (n_keep, tail)
        assert same(hg[:8 * nf], plain[:8 * nf])

"""The reference's Tracker and bundle-adjustment iterations on ATen-CPU (oracle/torch_ref.py: the reference's op sequence, autograd for the
backward, torch.optim.Adam for the step), and the data they run on.  Shared by the GPU tests (tests/test_gpu_aten.py) and the CPU self-check
of these chains against the fp32 and fp64 oracles (tests/test_oracle.py).  No GPU needed here.

  tracking_frame  a constructed frame on which every mask of the Tracker does something: ground truth is the scene's own rendering at the
                  true pose (iterated, so that the residual at the true pose is small), with noise, dynamic outliers, zero depths and rays
                  whose ground truth lies beyond the box exit; the pose to optimise starts perturbed
  ba_window       three frames of bundle adjustment (the oldest one fixed), rays split unevenly, some beyond the box exit
"""
import numpy as np
import torch

import scenes
from oracle import torch_ref as T

TRACK_LR = 1e-2                     # src/Tracker.cpp:104 (torch::optim::AdamOptions(1e-2))
BA_CAM_LR = 1e-3                    # mapping.BA_cam_lr


def cam7_from_c2w(c2w):
    """get_tensor_from_camera (quaternion qw, qx, qy, qz + translation) of a rotation with positive trace"""
    R = np.asarray(c2w, np.float64)[:3, :3]
    qw = np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([qw, (R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw)])
    return np.concatenate([q, np.asarray(c2w, np.float64)[:3, 3]])


def perturb_cam(cam, rng, dq=0.001, dt=0.005):
    """a start pose near `cam`: every quaternion component moved by ~dq and the norm scaled by 1.2 (quad2rotation normalises), the
    translation moved by ~dt"""
    c = np.asarray(cam, np.float64).copy()
    c[:4] = (c[:4] + rng.uniform(-dq, dq, 4)) * 1.2
    c[4:] += rng.uniform(-dt, dt, 3)
    return c.astype(np.float32)


def torch_scene(sc):
    return (torch.tensor(np.asarray(sc["bound"], np.float32)), {k: torch.tensor(v[None].copy()) for k, v in sc["grids"].items()},
            {k: torch.tensor(v.copy()) for k, v in sc["decoders"].items()})


def _box_exit(bound, ro, rd):
    return scenes._ray_box_far(np.asarray(bound, np.float64), np.asarray(ro, np.float64), np.asarray(rd, np.float64))


def k5_scene():
    return scenes.make_scene(81, scenes.grid_shapes_for(scenes.K5_BOUND), bound=scenes.K5_BOUND, grid_std=0.2, bias_std=0.05)


def tracking_frame(sc, n, seed=83, render_iters=20, damping=0.3, noise=0.01, dyn_frac=0.10, zero_frac=0.05, beyond_frac=0.05, cam=scenes.CAM_TUM):
    """n pixels of one frame (CAM_TUM, 20-pixel edge) and their ground truth:
      depth   the scene's own rendering at the true pose: gt <- gt + damping (render(gt) - gt), `render_iters` times (the render depends on gt
              through the surface samples, Renderer.cpp:80-99; undamped, the iteration oscillates on this scene with a median residual of
              0.1-0.3 m, damped it settles at ~6 mm);
              then 1 % multiplicative noise; `dyn_frac` of the rays at 0.5 x depth (dynamic outliers); the `zero_frac` zero depths of make_rays
              stay 0; `beyond_frac` of the rays get 1.3 x their box exit (the inside filter drops them); every other ray is kept at most at
              0.9 x its box exit, so that the start pose's filter cannot flip it
      colour  make_rays' colour of the room
    and a start pose perturbed from the true one."""
    intr = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    r = scenes.make_rays(seed, n, sc["bound"], n_frames=1, edge=20, up="z", zero_frac=zero_frac, **cam)
    cam_true = cam7_from_c2w(r["c2w"][0]).astype(np.float32)
    bound, grids, decs = torch_scene(sc)
    with torch.no_grad():
        ro, rd = T.rays_from_pixels(torch.tensor(r["pix_i"]), torch.tensor(r["pix_j"]), *intr, T.get_camera_from_tensor(torch.tensor(cam_true)))
        gd = torch.tensor(r["gt_depth"])
        zero = gd == 0
        for _ in range(render_iters):
            _, d, _, _ = T.render_batch_ray(grids, decs, rd, ro, "color", gd, bound)
            gd = torch.where(zero, torch.zeros_like(d), gd + damping * (d - gd))
    rng = np.random.default_rng(seed + 1000)
    exit_ = _box_exit(sc["bound"], ro.numpy(), rd.numpy())
    g = gd.numpy().astype(np.float64) * (1 + noise * rng.standard_normal(n))
    g = np.minimum(g, 0.9 * exit_)
    nz = np.flatnonzero(g > 0)
    pick = rng.permutation(nz)
    n_dyn, n_out = int(round(dyn_frac * n)), int(round(beyond_frac * n))
    dyn, beyond = pick[:n_dyn], pick[n_dyn:n_dyn + n_out]
    g[dyn] *= 0.5
    g[beyond] = 1.3 * exit_[beyond]
    g[~(g > 0)] = 0.0
    return dict(pix_i=r["pix_i"], pix_j=r["pix_j"], gt_depth=g.astype(np.float32), gt_color=r["gt_color"], intr=intr, cam_true=cam_true,
                cam0=perturb_cam(cam_true, rng), n_dyn=len(dyn), n_beyond=len(beyond))


def first_rays(fr, n):
    """the frame restricted to its first n rays (an odd count on the same data)"""
    return select_rays(fr, np.arange(len(fr["gt_depth"])) < n)


def select_rays(fr, sel):
    """the frame's rays where sel [n] is set (every per-ray array of the frame)"""
    return {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == fr["gt_depth"].shape else v) for k, v in fr.items()}


def aten_track(sc, fr, handle_dynamic=True, detach_var=True, use_color=True, iters=1, w_color=0.5, lr=TRACK_LR):
    """Tracker::optimize_cam_in_batch (src/Tracker.cpp:41-89) `iters` times on the frame's fixed pixels: a 7-vector leaf ->
    get_camera_from_tensor -> rays_from_pixels -> the detached inside filter, compacting -> render_batch_ray -> loss_track -> backward ->
    torch.optim.Adam on the pose.  Returns what the first iteration saw and the pose after the last."""
    bound, grids, decs = torch_scene(sc)
    pi, pj = torch.tensor(fr["pix_i"]), torch.tensor(fr["pix_j"])
    gd_all, gc_all = torch.tensor(fr["gt_depth"]), torch.tensor(fr["gt_color"])
    cam = torch.tensor(fr["cam0"]).requires_grad_(True)
    opt = torch.optim.Adam([cam], lr=lr)
    out = dict(hist=[])
    for it in range(iters):
        opt.zero_grad()
        ro, rd = T.rays_from_pixels(pi, pj, *fr["intr"], T.get_camera_from_tensor(cam))
        keep = T.inside_mask(bound, ro, rd, gd_all)
        ro, rd, gd, gc = ro[keep], rd[keep], gd_all[keep], gc_all[keep]
        rgb, depth, var, _ = T.render_batch_ray(grids, decs, rd, ro, "color", gd, bound)
        loss = T.loss_track(depth, rgb, var, gd, gc, w_color, use_color, handle_dynamic, detach_var)
        loss.backward()
        if it == 0:
            tmp = torch.abs(gd - depth).detach()
            out.update(keep=keep.numpy(), loss=float(loss.detach()), grad=cam.grad.numpy().copy(), median=float(tmp.median()),
                       dyn_dropped=int(((tmp >= 10 * tmp.median()) & (gd > 0)).sum()))
        opt.step()
        out["hist"].append((float(loss.detach()), cam.grad.numpy().copy(), cam.detach().numpy().copy(), int(keep.sum())))
        if it == 0:
            out["cam1"] = cam.detach().numpy().copy()
    out["cam"] = cam.detach().numpy().copy()
    return out


def ba_window(sc, counts=(300, 450, 250), seed=90, beyond_frac=0.05, cam=scenes.CAM_TUM):
    """a K5 mapping window of len(counts) frames (rays split unevenly; frame 0 is the oldest, its pose fixed): make_rays' room ground truth
    at each frame's true pose, `beyond_frac` of every frame's rays beyond the box exit, the optimised poses perturbed"""
    intr = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    rng = np.random.default_rng(seed + 1000)
    frames = []
    for f, n in enumerate(counts):
        r = scenes.make_rays(seed + f, n, sc["bound"], n_frames=1, edge=20, up="z", **cam)
        gd = r["gt_depth"].astype(np.float64)
        exit_ = _box_exit(sc["bound"], r["rays_o"], r["rays_d"])
        out = rng.permutation(np.flatnonzero(gd > 0))[:int(round(beyond_frac * n))]
        gd[out] = 1.3 * exit_[out]
        c = cam7_from_c2w(r["c2w"][0]).astype(np.float32)
        frames.append(dict(pix_i=r["pix_i"], pix_j=r["pix_j"], gt_depth=gd.astype(np.float32), gt_color=r["gt_color"],
                           cam0=c if f == 0 else perturb_cam(c, rng), active=f > 0))
    return dict(frames=frames, intr=intr, counts=list(counts))


def aten_ba(sc, win, lr, w_color=0.5, ba_lr=BA_CAM_LR):
    """one colour-stage Mapper::optimize_map iteration with BA (src/Mapper.cpp:305-329,430-446): a 7-vector leaf per active frame (the
    oldest frame's pose a constant), rays of every frame concatenated, the detached inside filter compacting, render_batch_ray, loss_map,
    backward, and torch.optim.Adam over the groups decoders (colour), middle, fine, colour and camera.  lr: the 6 group rates of
    include/nsk.h (the camera entry is replaced by ba_lr)."""
    bound, grids, decs = torch_scene(sc)
    levels = ("middle", "fine", "color")
    for k in levels:
        grids[k].requires_grad_(True)
    decs["color"].requires_grad_(True)
    cams = [torch.tensor(f["cam0"]).requires_grad_(bool(f["active"])) for f in win["frames"]]
    ro, rd = zip(*[T.rays_from_pixels(torch.tensor(f["pix_i"]), torch.tensor(f["pix_j"]), *win["intr"], T.get_camera_from_tensor(c))
                   for f, c in zip(win["frames"], cams)])
    ro, rd = torch.cat(ro), torch.cat(rd)
    gd = torch.tensor(np.concatenate([f["gt_depth"] for f in win["frames"]]))
    gc = torch.tensor(np.concatenate([f["gt_color"] for f in win["frames"]]))
    keep = T.inside_mask(bound, ro, rd, gd)
    rgb, depth, var, _ = T.render_batch_ray(grids, decs, rd[keep], ro[keep], "color", gd[keep], bound)
    loss = T.loss_map(depth, rgb, gd[keep], gc[keep], w_color, True)
    opt = torch.optim.Adam([{"params": [decs["color"]], "lr": lr[0]}] + [{"params": [grids[k]], "lr": lr[i]} for i, k in ((2, "middle"), (3, "fine"), (4, "color"))]
                           + [{"params": [c for c in cams if c.requires_grad], "lr": ba_lr}])
    opt.zero_grad()
    loss.backward()
    out = dict(keep=keep.numpy(), loss=float(loss.detach()), rgb=rgb.detach().numpy(), depth=depth.detach().numpy(),
               g_grids={k: grids[k].grad[0].numpy().copy() for k in levels}, g_dec=decs["color"].grad.numpy().copy(),
               g_cams=[c.grad.numpy().copy() if c.grad is not None else np.zeros(7, np.float32) for c in cams])
    opt.step()
    out.update(grids={k: grids[k].detach()[0].numpy().copy() for k in levels}, dec=decs["color"].detach().numpy().copy(),
               cams=[c.detach().numpy().copy() for c in cams])
    return out

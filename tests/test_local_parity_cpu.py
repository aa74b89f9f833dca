"""CPU side of the localised comparison (tests/local_parity.py) on the edge scenes (tests/edge_scenes.py): the reference is pinned on these
inputs before the GPU is judged by it (tests/test_gpu_edges.py).

  * the oracle's running-error scale R against a numpy restatement;
  * kappa_ref = fp32 oracle against fp64 oracle, same forced branches, per scene and stage (printed: run with -s), the oracle's non-finite rays
    exactly the rays constructed to be so and at most 5 % of a scene, every border voxel of the lattice scene touched;
  * fp32 oracle == ATen (oracle/torch_ref.py: the reference's op sequence) per ray on every edge scene.

Measured here (fp32 oracle vs fp64 oracle on the fp32 oracle's own branches; worst grid level and stage; kappa's denominator is R_v + 2^-24 max R,
tests/local_parity.py): lattice 3.6e-5, outside-on-bound 2.0e-4, thin-grids 7.4e-5, one-cell (512 rays) 3.6e-7, max-spread 6.5e-3 (one sample per
fine voxel: a weight's absolute rounding meets weights of 1e-5).

What ATen does at the edges (established by test_fp32_oracle_matches_aten_per_ray, documented in include/nsk.h):
  * a ray INSIDE a face (origin on the face, zero direction component across it) has 0/0 in the box exit.  torch.max / torch.min propagate the NaN,
    so ATen renders every such ray non-finite.  The oracle's and the HIP kernel's `t0 > t1 ? t0 : t1` / `m < far` comparisons drop a NaN
    except in the first axis' upper-face slot (x = hi, d_x = 0: m = t1 = NaN becomes `far` unconditionally): they render the other in-face
    rays finite, with the exit of the remaining axes.  The oracle is NOT changed to ATen's behaviour: the product renders strictly more rays
    than the reference would, and the rays it does not render are the oracle's; the test pins exactly this difference.
  * 1-voxel dimensions: align_corners scales by dim - 1 = 0, ATen reads voxel 0 with weight 1 and a zero spatial gradient; the oracle agrees.
"""
import numpy as np
import pytest
import torch

import edge_scenes as E
import local_parity as LP
import scenes
from aten_chains import torch_scene
from oracle import torch_ref as T

W_COLOR = 0.5
SCENES = {"lattice": E.lattice, "outside-on-bound": E.outside_and_on_bound, "thin-grids": E.thin_grids, "one-cell": lambda: E.one_cell(512),
          "max-spread": E.max_spread}


def in_face(bound, ro, rd):
    """bool [N, 3, 2]: the origin lies on face (axis, side) and the direction has a zero component across it"""
    b = np.asarray(bound, np.float32)
    return (ro[:, :, None] == b[None, :, :]) & (rd[:, :, None] == 0)


def own_branches(o, sc, rays, stage, gmax, e):
    """the branches of oracle o's own forward: hidden-ReLU bits per decoder, relu(sigma), and the L1 seed gradients of its outputs"""
    op = o.opts(sc["bound"], n_samples=e["n_samples"], n_surface=e["n_surface"])
    args = (rays["rays_o"], rays["rays_d"], rays["gt_depth"], gmax)
    fw = o.render_forward(op, sc["grids"], sc["decoders"], stage, *args, want_aux=True)
    which = {"coarse": ["coarse"], "middle": ["middle"], "fine": ["middle", "fine"], "color": ["middle", "fine", "color"]}[stage]
    bits = {k: o.preacts(op, sc["grids"], sc["decoders"], stage, k, *args) > 0 for k in which}
    _, g_d, g_c = o.loss_map(fw["depth"], fw["rgb"], rays["gt_depth"], rays["gt_color"], W_COLOR, stage == "color")
    return fw, bits, fw["raw"][..., 3].reshape(-1) > 0, g_d, g_c


def compact(rays, keep):
    return {k: v[keep] for k, v in rays.items()}


def test_lattice_coordinates_are_exact_in_fp32():
    """pitch exactly 1: tri_setup's normalise -> unnormalise chain returns the world coordinate itself for every multiple of 1/4 in the bound"""
    q = np.arange(0, 33) / 4.0
    p = np.stack(np.meshgrid(q, q[:17], q, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    x = E.lattice_coordinates_fp32(E.LATTICE_BOUND, (9, 5, 9), p)
    assert (x == p).all()
    e = E.lattice()
    assert e["rays"]["rays_o"].shape[0] <= 512
    d = e["rays"]["rays_d"]
    assert ((d == 0).sum(axis=1) == 2).sum() >= 36 and ((d == 0).sum(axis=1) == 1).sum() >= 72


def test_running_error_scale_against_numpy(oracle64):
    """R > 0 exactly on the voxels a numpy restatement says are touched with a non-zero weight by a sample that carries gradient (occupancy
    compositing: alpha = sigmoid(10 sigma) sends a gradient to every in-bound sample), and R == that restatement's sum there"""
    o = oracle64
    sc = scenes.make_scene(5, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    rays = scenes.make_rays(6, 24, sc["bound"], zero_frac=0.0)
    op = o.opts(sc["bound"], occupancy=True)
    N = 24
    rng = np.random.default_rng(0)
    g_d, g_c = rng.standard_normal(N), np.zeros((N, 3))
    fw = o.render_forward(op, sc["grids"], sc["decoders"], "middle", rays["rays_o"], rays["rays_d"], rays["gt_depth"], want_aux=True)
    bw = o.render_backward(op, sc["grids"], sc["decoders"], "middle", rays["rays_o"], rays["rays_d"], rays["gt_depth"], -1.0, g_c, g_d, want_scale=True)
    plain = o.render_backward(op, sc["grids"], sc["decoders"], "middle", rays["rays_o"], rays["rays_d"], rays["gt_depth"], -1.0, g_c, g_d)
    assert (plain["g_grids"]["middle"] == bw["g_grids"]["middle"]).all()          # the scaled entry point computes the same gradient
    R = bw["r_grids"]["middle"]
    Cc, Z, Y, X = sc["grids"]["middle"].shape
    b = sc["bound"].astype(np.float64)
    p = rays["rays_o"][:, None, :].astype(np.float64) + rays["rays_d"][:, None, :].astype(np.float64) * fw["z"][:, :, None]
    inb = ((p > b[:, 0]) & (p < b[:, 1])).all(axis=-1)
    touched = np.zeros((Z, Y, X), bool)
    wsum = np.zeros((Z, Y, X))
    x = [np.clip((p[..., k] - b[k, 0]) / (b[k, 1] - b[k, 0]) * 2 - 1, -1, 1) for k in range(3)]
    x = [np.clip((x[k] + 1) / 2 * (d - 1), 0, d - 1) for k, d in enumerate((X, Y, Z))]
    i0 = [np.floor(v).astype(int) for v in x]
    t = [v - i for v, i in zip(x, i0)]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (t[0] if dx else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                ix, iy, iz = i0[0] + dx, i0[1] + dy, i0[2] + dz
                ok = inb & (w != 0) & (ix < X) & (iy < Y) & (iz < Z)
                np.add.at(wsum, (iz[ok], iy[ok], ix[ok]), w[ok])
                touched[iz[ok], iy[ok], ix[ok]] = True
    assert ((R > 0) == touched).all(), (int((R > 0).sum()), int(touched.sum()))
    assert (~touched).any() and touched.any()
    # where R == 0 the gradient is exactly zero, elsewhere it is bounded by R (|sum w g| <= sum w max|g|)
    g = bw["g_grids"]["middle"]
    assert (g[:, ~touched] == 0).all()
    assert (np.abs(g).max(axis=0) <= R * (1 + 1e-12)).all()
    # same for the decoder parameters and the rays
    assert (np.abs(bw["g_decoders"]["middle"]) <= bw["r_decoders"]["middle"] * (1 + 1e-9) + 1e-300).all()
    assert (np.abs(bw["g_rays_o"]).max(axis=1) <= bw["r_rays_o"] * (1 + 1e-9)).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_kappa_ref_per_scene(name, oracle32, oracle64):
    """kappa_ref per scene, stage and level; the oracle's non-finite rays are exactly the constructed ones (<= 5 %); lattice: every border voxel touched"""
    e = SCENES[name]()
    sc, rays = e["sc"], e["rays"]
    N = rays["rays_o"].shape[0]
    gmax = float(rays["gt_depth"].max())
    assert e["made_nonfinite"].mean() <= 0.05
    for stage in e["stages"]:
        op32 = oracle32.opts(sc["bound"], n_samples=e["n_samples"], n_surface=e["n_surface"])
        with np.errstate(all="ignore"):
            fw = oracle32.render_forward(op32, sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"], rays["gt_depth"], gmax)
        bad = ~(np.isfinite(fw["depth"]) & np.isfinite(fw["var"]) & np.isfinite(fw["rgb"]).all(axis=1) & np.isfinite(fw["weights"]).all(axis=1))
        assert (bad == e["made_nonfinite"]).all(), (name, stage, np.flatnonzero(bad), np.flatnonzero(e["made_nonfinite"]))
        assert bad.mean() <= 0.05
        kept = compact(rays, ~bad)
        fw32, bits, sig_on, g_d, g_c = own_branches(oracle32, sc, kept, stage, gmax, e)
        kw = dict(n_samples=e["n_samples"], n_surface=e["n_surface"])
        r32 = LP.forced_reference(oracle32, sc, kept, stage, gmax, g_c, g_d, None, bits, sig_on, **kw)
        r64 = LP.forced_reference(oracle64, sc, kept, stage, gmax, g_c, g_d, None, bits, sig_on, **kw)
        levels = list(r64["g_grids"]) if stage != "coarse" else ["coarse"]
        levels = [k for k in levels if k in bits]
        fig = LP.compare_backward(r32, r32, r64, levels, "%s/%s fp32 oracle" % (name, stage), decoders=[k for k in levels], check=False)
        for k in levels:
            kr = fig["grid " + k][1]
            # the reference itself must resolve the scale it judges by.  (max-spread: ~1 sample per fine voxel, so a weight's ABSOLUTE rounding -- 64 voxels x
            # 2^-24 per axis -- meets weights of 1e-5 at corners a sample barely touches: kappa_ref 1.5e-2 there, 1e-4 and below everywhere else)
            assert np.isfinite(kr) and kr < (0.1 if name == "max-spread" else 1e-3), (name, stage, k, kr)
            pv = LP.per_voxel(r32["g_grids"][k], r64["g_grids"][k], r64["r_grids"][k])
            assert pv["leak"] == 0
            if name == "lattice":
                border = E.border_voxels(r64["r_grids"][k].shape)
                assert (r64["r_grids"][k][border] > 0).all(), (stage, k, np.argwhere(border & ~(r64["r_grids"][k] > 0))[:5])
        for k in ("g_rays_o", "g_rays_d"):
            assert fig[k][1] <= LP.RAY_TOL, (name, stage, k, fig[k])
    if name == "max-spread":
        z = oracle32.render_forward(op32, sc["grids"], sc["decoders"], "fine", rays["rays_o"], rays["rays_d"], rays["gt_depth"], gmax, want_aux=True)["z"]
        cells = E.distinct_cells_per_group(sc["bound"], sc["grids"]["fine"].shape[:0:-1], z, rays["rays_o"], rays["rays_d"])
        print("max-spread: distinct fine cells per 8-ray workgroup: min %d, max %d" % (min(cells), max(cells)))
        assert min(cells) > 300


@pytest.mark.parametrize("name", list(SCENES))
def test_fp32_oracle_matches_aten_per_ray(name, oracle32):
    e = SCENES[name]()
    sc, rays = e["sc"], e["rays"]
    bound, grids, decs = torch_scene(sc)
    ro, rd, gd = torch.tensor(rays["rays_o"]), torch.tensor(rays["rays_d"]), torch.tensor(rays["gt_depth"])
    face = in_face(sc["bound"], rays["rays_o"], rays["rays_d"])
    for stage in e["stages"]:
        with torch.no_grad():
            rgb, depth, var, w = T.render_batch_ray(grids, decs, rd, ro, stage, gd, bound, n_samples=e["n_samples"], n_surface=e["n_surface"])
        aten = dict(rgb=rgb.numpy(), depth=depth.numpy(), var=var.numpy(), weights=w.numpy())
        with np.errstate(all="ignore"):
            fw = oracle32.render_forward(oracle32.opts(sc["bound"], n_samples=e["n_samples"], n_surface=e["n_surface"]), sc["grids"], sc["decoders"], stage,
                                         rays["rays_o"], rays["rays_d"], rays["gt_depth"])
        bad_aten = ~np.isfinite(aten["depth"])
        bad_orc = ~np.isfinite(fw["depth"])
        # ATen: non-finite exactly on the in-face rays (0/0 propagates through torch.max / torch.min); the oracle: only x = hi with d_x = 0
        assert (bad_aten == face.any(axis=(1, 2))).all(), (name, stage, np.flatnonzero(bad_aten != face.any(axis=(1, 2))))
        assert (bad_orc == face[:, 0, 1]).all() and (bad_orc == e["made_nonfinite"]).all()
        both = ~bad_aten
        print("%s/%s: %d rays, ATen non-finite %d, oracle non-finite %d" % (name, stage, len(bad_aten), bad_aten.sum(), bad_orc.sum()))
        LP.compare_forward({k: v[both] for k, v in fw.items()}, {k: v[both] for k, v in aten.items()}, "%s/%s fp32 oracle vs ATen" % (name, stage))


def test_principal_point_rays_hold_exact_zeros(oracle32):
    pi, pj, intr, c2w = E.principal_point()
    for mode in (0, 2):
        ro, rd = oracle32.rays_from_pixels(pi, pj, *intr, c2w, mode)
        to, td = T.rays_from_pixels(torch.tensor(pi), torch.tensor(pj), *intr, torch.tensor(c2w[:3]), mode)
        assert (rd == td.numpy()).all() and (ro == to.numpy()).all()               # (== : the oracle's zeros carry the sign of -(j - cy), ATen's sum makes them +0)
        col, row = pi == int(intr[2]), pj == int(intr[3])
        assert col.any() and row.any() and (rd[col, 0] == 0).all() and (rd[row, 1] == 0).all()


def test_miss_rays_without_gt_match_aten(oracle32):
    """gt_depth None on rays that miss the bound (far < 0 unclamped, descending z, negative distances): what ATen renders there -- weights of 1e21,
    inf / NaN on part of the rays -- is what the fp32 oracle renders: same non-finite rays, the rest per ray"""
    sc, ro, rd = E.misses_without_gt()
    bound, grids, decs = torch_scene(sc)
    for stage in ("middle", "color"):
        with torch.no_grad():
            rgb, depth, var, w = T.render_batch_ray(grids, decs, torch.tensor(rd), torch.tensor(ro), stage, None, bound)
        with np.errstate(all="ignore"):
            fw = oracle32.render_forward(oracle32.opts(sc["bound"]), sc["grids"], sc["decoders"], stage, ro, rd, None, want_aux=True)
        assert (np.diff(fw["z"][:24], axis=1) < 0).all() and (fw["z"][:24, -1] < 0).all()           # descending, ending behind the origin
        LP.compare_forward(fw, dict(rgb=rgb.numpy(), depth=depth.numpy(), var=var.numpy(), weights=w.numpy()), "misses without gt/%s fp32 oracle vs ATen" % stage)

"""Localised comparisons: the worst RAY and the worst VOXEL ROW instead of one relative L2 over a whole array, in which one wrong ray in
5000 or one voxel row that received its neighbour's sum disappears (the aggregate checks sit at 1e-4 with measured figures of 1e-6 .. 1e-7).

  per ray      err_n = max |a_n - ref_n| / (max |ref_n| + floor): a ray is normalised by its own reference magnitude; the floor (default: the rms
               of the reference over the batch; for ray gradients the oracle's per-ray running-error scale) keeps rays whose reference is
               (nearly) zero comparable.
  per voxel    kappa = max_v max_c |g[v][c] - g64[v][c]| / R_v with R_v = sum_samples w(sample, v) max_c |g_feat(sample)[c]| from the fp64 oracle
               (oracle/nso.c nso_render_backward_scaled): the scale of what ANY fp32 evaluation of the sum may lose at that voxel.  A voxel with
               R == 0 is touched by no sample: anything but an exact zero there is gradient that landed in a wrong row ("leak").
               The denominator is R_v + 2^-24 max_v R: an error below one fp32 unit roundoff of the level's largest scale is not resolved.  It
               matters for voxels fed only by samples behind a masked one (occ = 100 outside the bound, Renderer.cpp:36): there alpha = 1 - exp(-100 dist)
               rounds to 1 in fp32, the compositing's 1 - alpha + 1e-10 is 1e-10 where the exact value is 4.7e-10, and after a few such samples the fp32
               REFERENCE's own gradient is off by a factor of 100 at a scale of 1e-31 (measured: kappa_ref 0.19 without the floor).
  per weight   the same with sum |activation| |g| per decoder parameter.

Limits.  kappa_ref is the fp32 oracle against the fp64 oracle with the SAME forced branches (hidden ReLUs, relu(sigma), L1 signs), so that both
evaluate one smooth function.  The GPU gets KAPPA_FACTOR = 8 times kappa_ref: 4 for the two operand bits the two fp16 pieces of a backward
chain drop (2^-22 against 2^-24), 2 for the order of the atomic sums.  The per-ray limit is the suite's contract tolerance RAY_TOL = 1e-4
(relative L2 over an array until now), applied to every single ray.  Nothing here is calibrated from the GPU's own figures.
"""
import numpy as np

from edge_scenes import position_in_grid

KAPPA_FACTOR = 8.0
RAY_TOL = 1e-4
U32 = 2.0 ** -24


def per_ray(a, ref, floor=None):
    """(worst err_n, index of the worst ray, err [N]); a, ref [N] or [N, K]; rays where the reference is not finite are left out (the caller
    asserts separately that they are the same rays on both sides)"""
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    fin = np.isfinite(ref).all(axis=1)
    mag = np.abs(ref).max(axis=1)
    if floor is None:
        floor = float(np.sqrt((ref[fin] ** 2).mean())) if fin.any() else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - ref).max(axis=1) / (mag + floor)
    err = np.where(np.isnan(err) & fin, np.inf, err)             # a non-finite result on a finite reference is the worst error there is
    err = np.where(fin, np.where(mag + floor > 0, err, np.where(np.abs(a).max(axis=1) > 0, np.inf, 0.0)), 0.0)
    n = int(np.argmax(err)) if len(err) else -1
    return (float(err[n]) if n >= 0 else 0.0), n, err


def per_voxel(g, g64, R):
    """g, g64 [C,Z,Y,X], R [Z,Y,X] -> dict(kappa, index (z,y,x) of the worst voxel, where (interior / face / edge / corner), leak = number of
    voxels with R == 0 that are not exactly zero in g, leak_index, n_touched)"""
    g, g64, R = np.asarray(g, np.float64), np.asarray(g64, np.float64), np.asarray(R, np.float64)
    err = np.abs(g - g64).max(axis=0)
    err = np.where(np.isnan(err), np.inf, err)
    touched = R > 0
    ratio = np.zeros_like(R)
    ratio[touched] = err[touched] / (R[touched] + U32 * R.max())
    idx = np.unravel_index(int(np.argmax(ratio)), R.shape)
    leak = (~touched) & (np.abs(np.nan_to_num(g, nan=1.0)).max(axis=0) != 0)
    lidx = tuple(int(i) for i in np.argwhere(leak)[0]) if leak.any() else None
    return dict(kappa=float(ratio[idx]), index=tuple(int(i) for i in idx), where=position_in_grid(idx, R.shape), leak=int(leak.sum()),
                leak_index=lidx, n_touched=int(touched.sum()))


def per_weight(gp, gp64, rP):
    """packed decoder gradients against the per-parameter scale sum |activation| |g| -> dict(kappa, index, leak)"""
    gp, gp64, rP = np.asarray(gp, np.float64), np.asarray(gp64, np.float64), np.asarray(rP, np.float64)
    err = np.abs(gp - gp64)
    err = np.where(np.isnan(err), np.inf, err)
    touched = rP > 0
    ratio = np.zeros_like(rP)
    ratio[touched] = err[touched] / (rP[touched] + U32 * rP.max())
    i = int(np.argmax(ratio))
    return dict(kappa=float(ratio[i]), index=i, leak=int(((~touched) & (np.nan_to_num(gp, nan=1.0) != 0)).sum()))


def samples_touching(bound, shape_zyx, idx_zyx, z, rays_o, rays_d):
    """(ray, sample) pairs whose trilinear footprint contains voxel idx: what to look at when a voxel fails"""
    b = np.asarray(bound, np.float64)
    p = rays_o[:, None, :].astype(np.float64) + rays_d[:, None, :].astype(np.float64) * np.asarray(z, np.float64)[:, :, None]
    hit = np.ones(p.shape[:2], bool)
    for k, (i, s) in enumerate(zip(idx_zyx[::-1], shape_zyx[::-1])):             # k = x, y, z
        x = np.clip((p[..., k] - b[k, 0]) / (b[k, 1] - b[k, 0]) * (s - 1), 0, s - 1)
        hit &= np.abs(x - i) < 1
    return np.argwhere(hit)


def forced_reference(o, sc, rays, stage, gmax, g_rgb, g_depth, g_var, bits, sigma_on, n_samples=32, n_surface=16, decoders=True):
    """oracle `o`'s backward with every branch given and the running-error scales alongside"""
    return o.render_backward(o.opts(sc["bound"], n_samples=n_samples, n_surface=n_surface), sc["grids"], sc["decoders"], stage, rays["rays_o"], rays["rays_d"],
                             rays["gt_depth"], gmax, g_rgb, g_depth, g_var, want_decoders=decoders, relu=bits, sigma_on=sigma_on, want_scale=True)


def compare_backward(got, ref32, ref64, levels, label, decoders=(), ray_floor=True, check=True, out=print):
    """got: dict(g_grids, g_decoders, g_rays_o, g_rays_d) of the evaluation under test (entries may be missing / None); ref32 / ref64: forced_reference of
    the fp32 and the fp64 oracle on the same branches.  Prints every figure, then (check) asserts them; returns the figures."""
    fig = {}
    fails = []
    for k in levels:
        R = ref64["r_grids"][k]
        kr = per_voxel(ref32["g_grids"][k], ref64["g_grids"][k], R)
        kg = per_voxel(got["g_grids"][k], ref64["g_grids"][k], R)
        fig["grid " + k] = (kg["kappa"], kr["kappa"])
        out("%s: d/d grid %-6s kappa %.2e at voxel %s (%s), kappa_ref %.2e at %s (%s), ratio %.2f; %d voxels touched, %d untouched voxels not exactly zero%s" % (
            label, k, kg["kappa"], kg["index"], kg["where"], kr["kappa"], kr["index"], kr["where"], kg["kappa"] / max(kr["kappa"], 1e-300), kg["n_touched"],
            kg["leak"], "" if not kg["leak"] else " (first: %s, %s)" % (kg["leak_index"], position_in_grid(kg["leak_index"], R.shape))))
        if kg["leak"]:
            fails.append("%s grid %s: gradient in %d voxels no sample touches, first %s" % (label, k, kg["leak"], kg["leak_index"]))
        if not kg["kappa"] <= KAPPA_FACTOR * kr["kappa"]:
            fails.append("%s grid %s: kappa %.3e > %g x kappa_ref %.3e at voxel %s (%s)" % (label, k, kg["kappa"], KAPPA_FACTOR, kr["kappa"], kg["index"], kg["where"]))
    for k in decoders:
        rP = ref64["r_decoders"][k]
        kr = per_weight(ref32["g_decoders"][k], ref64["g_decoders"][k], rP)
        kg = per_weight(got["g_decoders"][k], ref64["g_decoders"][k], rP)
        fig["decoder " + k] = (kg["kappa"], kr["kappa"])
        out("%s: d/d decoder %-6s kappa %.2e at parameter %d, kappa_ref %.2e, ratio %.2f, %d leaks" % (label, k, kg["kappa"], kg["index"], kr["kappa"],
                                                                                                          kg["kappa"] / max(kr["kappa"], 1e-300), kg["leak"]))
        if kg["leak"]:
            fails.append("%s decoder %s: %d parameters with a gradient and no contribution" % (label, k, kg["leak"]))
        if not kg["kappa"] <= KAPPA_FACTOR * kr["kappa"]:
            fails.append("%s decoder %s: kappa %.3e > %g x kappa_ref %.3e at parameter %d" % (label, k, kg["kappa"], KAPPA_FACTOR, kr["kappa"], kg["index"]))
    for k in ("g_rays_o", "g_rays_d"):
        if got.get(k) is None:
            continue
        scale = ref64["r_" + k[2:]]
        # floor: the oracle's per-ray running-error scale sum_samples |d loss / d sample point| (x |z| for the direction): a clipped or
        # cancelled ray gradient is judged by the size of the terms it was summed from
        e, n, _ = per_ray_scaled(got[k], ref64[k], scale)
        er, nr, _ = per_ray_scaled(ref32[k], ref64[k], scale)
        fig[k] = (e, er)
        out("%s: %s worst ray %d: %.2e of its scale (fp32 oracle: ray %d, %.2e)" % (label, k, n, e, nr, er))
        if not e <= RAY_TOL:
            fails.append("%s %s: ray %d off by %.3e of its scale %.3e: %s against %s (fp32 oracle %s)" % (label, k, n, e, scale[n], got[k][n], ref64[k][n], ref32[k][n]))
    if check:
        assert not fails, "\n".join(fails)
    return fig


def per_ray_scaled(a, ref, scale):
    """ray gradients [N,3] against the oracle's per-ray scale [N]: err_n = max |a_n - ref_n| / (scale_n + rms of the scale over the batch x 1e-6);
    a ray with scale 0 must be exactly zero"""
    a, ref, scale = np.asarray(a, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    fin = np.isfinite(ref).all(axis=1) & np.isfinite(scale)
    tiny = 1e-6 * float(np.sqrt((scale[fin] ** 2).mean())) if fin.any() else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - ref).max(axis=1) / (scale + tiny)
    err = np.where(fin, np.where(np.isnan(err), np.where(np.abs(a - ref).max(axis=1) == 0, 0.0, np.inf), err), 0.0)
    n = int(np.argmax(err)) if len(err) else -1
    return (float(err[n]) if n >= 0 else 0.0), n, err


def compare_forward(got, ref, label, keys=("depth", "var", "rgb", "weights"), check=True, out=print):
    """per-ray forward outputs against a reference (dicts of arrays [N, ...]); the non-finite rays must be the same set"""
    fig = {}
    fails = []
    for k in keys:
        a, r = np.asarray(got[k]), np.asarray(ref[k])
        fa = np.isfinite(a.reshape(len(a), -1)).all(axis=1)
        fr = np.isfinite(r.reshape(len(r), -1)).all(axis=1)
        if (fa != fr).any():
            fails.append("%s %s: non-finite rays differ: %s against the reference's %s" % (label, k, np.flatnonzero(~fa)[:8], np.flatnonzero(~fr)[:8]))
        e, n, _ = per_ray(a, r)
        fig[k] = e
        out("%s: %-7s worst ray %d: %.2e (%d non-finite rays in the reference)" % (label, k, n, e, int((~fr).sum())))
        if not e <= RAY_TOL:
            fails.append("%s %s: ray %d off by %.3e" % (label, k, n, e))
    if check:
        assert not fails, "\n".join(fails)
    return fig

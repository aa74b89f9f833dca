"""CPU tests (-m "not gpu") of the importance-sampling rule as tests/importance_checks.py restates it (include/nsk.h, nsk_set_importance):
against its own fp64 form, against a torch statement of upstream's sample_pdf, and on hand cases; the configuration key
rendering.N_importance through the host classes' constructors (host/importance_test --config)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import importance_checks as IC

EPS = 2.0 ** -24            # unit roundoff of fp32


def _random_case(seed, N, S1, Ni, floor=0.05):
    """sorted depths in (0.1, 6) and weights in [floor, 1] / S1 (their sum stays below 1, as compositing weights do)"""
    rng = np.random.default_rng(seed)
    z = np.sort(rng.uniform(0.1, 6.0, (N, S1)), 1).astype(np.float32)
    w = (rng.uniform(floor, 1.0, (N, S1)) / S1).astype(np.float32)
    return z, w, IC.u_values(N, Ni, det=False, seed=seed)


def _torch_sample_pdf(z, w, u):
    """upstream NICE-SLAM's sample_pdf (src/common.py) on z_vals_mid and weights[..., 1:-1], with its u given"""
    z, w, u = torch.tensor(z), torch.tensor(w), torch.tensor(u)
    bins = .5 * (z[..., 1:] + z[..., :-1])
    weights = w[..., 1:-1] + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    inds_g = torch.stack([below, above], -1)
    shape = [inds_g.shape[0], inds_g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(shape), 2, inds_g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return (bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])).numpy()


def _bound(z, w):
    """How far the fp32 rule may be from its fp64 form.  q has one rounding, total S1 - 3 more, pdf one more: pdf is off by at most
    (S1 - 1) eps relatively; cdf[k] sums k of them with k - 1 roundings and stays <= 1, so every knot of the cdf is off by at most
    dc = 2 S1 eps.  The inverse of the cdf is continuous and piecewise linear in (u, knots) with slope (bins[k+1] - bins[k]) / pdf[k] in
    segment k (a u that falls into the neighbouring segment in one of the two forms still moves along one of the two slopes), so moving the
    two knots of a segment and u - cdf[below] (one rounding, and the quotient's) moves zs by at most slope * (3 dc + 3 eps); bins, the product
    and the sum add four roundings of a value <= max z.  Needs pdf well above the 1e-5 switch of step 9 (the cases' weight floor sees to it)."""
    z64, w64 = z.astype(np.float64), w.astype(np.float64)
    S1 = z.shape[1]
    bins = 0.5 * (z64[:, 1:] + z64[:, :-1])
    q = w64[:, 1:-1] + 1e-5
    pdf = q / q.sum(1, keepdims=True)
    assert pdf.min() > 1e-3
    slope = ((bins[:, 1:] - bins[:, :-1]) / pdf).max()
    return slope * (3 * 2 * S1 + 3) * EPS + 4 * EPS * float(z64.max())


CASES = [(1, 64, 48, 16), (2, 64, 32, 16), (3, 64, 13, 5), (4, 64, 3, 1), (5, 64, 4, 7)]


def test_fp32_rule_against_its_fp64_form():
    """The rule in fp32 against the same rule in fp64 (same u, same constants) on random weights, (S1, Ni) = (48, 16), (32, 16), (13, 5),
    (3, 1), (4, 7), 64 rays each.  The assertion is _bound's (its docstring derives it); measured worst |zs32 - zs64| 9.8e-6 / 6.7e-6 / 4.6e-6 /
    2.5e-7 / 5.9e-7, at most 0.05 of the bound (2.1e-3 / 1.3e-3 / 6.3e-4 / 4.9e-6 / 4.3e-5: the steepest segment of a case sets it)."""
    worst, worst_rel = 0.0, 0.0
    for seed, N, S1, Ni in CASES:
        z, w, u = _random_case(seed, N, S1, Ni)
        a = IC.sample_zs(z, w, u, np.float32)
        b = IC.sample_zs(z, w, u, np.float64)
        assert a.dtype == np.float32 and b.dtype == np.float64
        d, lim = float(np.abs(a.astype(np.float64) - b).max()), _bound(z, w)
        print("fp32 rule against fp64, S1 = %d, Ni = %d: worst %.2e, bound %.2e" % (S1, Ni, d, lim))
        worst, worst_rel = max(worst, d), max(worst_rel, d / lim)
        assert d <= lim, (S1, Ni, d, lim)
    print("worst %.2e (%.3f of the bound)" % (worst, worst_rel))


# twice the worst |rule - torch| measured on the cases above with torch's CPU kernels (1.36e-5 at S1 = 48): the two differ in the order of
# torch.sum (vectorised partial sums) against the rule's left-to-right sum, which moves every knot of the cdf by a few ulp
TORCH_LIMIT = 2 * 1.36e-5


def test_fp32_rule_against_torch_sample_pdf():
    """The rule in fp32 against a torch statement of upstream's sample_pdf (torch.sum, torch.cumsum, torch.searchsorted(right=True)) on the
    same inputs.  Measured worst difference 1.36e-5 (S1 = 48; 7.6e-6 at 32, 4.3e-6 at 13, 0 at S1 = 3 and 4: no sum to reorder); the limit is twice
    that.  (The fp32 rule is as far from its own fp64 form: 9.8e-6 at S1 = 48.)"""
    torch.set_num_threads(1)
    worst = 0.0
    for seed, N, S1, Ni in CASES:
        z, w, u = _random_case(seed, N, S1, Ni)
        a = IC.sample_zs(z, w, u, np.float32)
        b = _torch_sample_pdf(z, w, u)
        d = float(np.abs(a - b).max())
        print("fp32 rule against torch sample_pdf, S1 = %d, Ni = %d: worst %.2e" % (S1, Ni, d))
        worst = max(worst, d)
    assert worst <= TORCH_LIMIT, worst


def test_equal_weights_give_evenly_spaced_quantiles():
    """all weights equal: the cdf is linear over the bins' indices, so u[j] lands at the (S1 - 2) u[j]-th bin, linearly between its neighbours"""
    S1, Ni = 18, 9
    z = np.linspace(1.0, 3.0, S1, dtype=np.float32)[None] ** 2          # uneven bins
    w = np.full((1, S1), 0.03, np.float32)
    u = IC.u_values(1, Ni)
    zs = IC.sample_zs(z, w, u)[0]
    bins = (np.float32(0.5) * (z[0, 1:] + z[0, :-1])).astype(np.float32)
    want = np.interp(u[0].astype(np.float64) * (S1 - 2), np.arange(S1 - 1), bins.astype(np.float64))
    assert np.abs(zs - want).max() < 1e-5, np.abs(zs - want).max()      # (16 knots of a cdf off by a few ulp, slopes of ~1 x 16)
    assert zs[0] == bins[0] and bins[-2] < zs[-1] <= bins[-1]


def test_one_weight_carrying_everything():
    """weight k carries everything: its pdf entry k - 1 is ~1, so every sample lies between bins[k - 1] and bins[k], the two bins around z[k]"""
    S1, Ni, k = 20, 16, 7
    z = np.linspace(0.5, 4.0, S1, dtype=np.float32)[None]
    w = np.zeros((1, S1), np.float32); w[0, k] = 1.0
    u = IC.u_values(1, Ni, det=False, seed=3)
    u = np.clip(u, 0.01, 0.99).astype(np.float32)                        # (the first and last 2e-4 of the cdf belong to the empty bins)
    zs = IC.sample_zs(z, w, u)[0]
    bins = 0.5 * (z[0, 1:] + z[0, :-1])
    assert (zs >= bins[k - 1]).all() and (zs <= bins[k]).all(), (zs, bins[k - 1], bins[k])
    z2 = IC.resample(z, w, Ni, det=False, seed=3)
    assert z2.shape == (1, S1 + Ni) and (np.diff(z2[0]) >= 0).all()


def test_u_one_returns_the_last_bin():
    """u = 1 counts every cdf entry (inds = S1 - 1), below = above = S1 - 2, the clamped denominator is 1 and t multiplies 0: bins[S1 - 2]
    exactly.  That is the rule wherever the rounded cdf ends at or below 1 (always at S1 = 3, where it ends at q / q = 1); a cdf whose
    rounded sum ends an ulp above 1 leaves u = 1 inside the last segment."""
    seen_exact = 0
    for S1 in (3, 4, 5, 48):
        z, w, _ = _random_case(7, 32, S1, 1)
        zs = IC.sample_zs(z, w, np.ones((32, 1), np.float32))[:, 0]
        bins = (np.float32(0.5) * (z[:, 1:] + z[:, :-1])).astype(np.float32)
        ends = IC.cdf_of(w)[:, -1]
        exact = ends <= 1
        seen_exact += int(exact.sum())
        assert exact.all() or S1 > 3
        assert np.array_equal(zs[exact], bins[exact, -1])
        assert (zs[~exact] <= bins[~exact, -1]).all() and (zs[~exact] > bins[~exact, -2]).all()
    assert seen_exact > 64


def test_single_importance_sample():
    """Ni = 1: linspace of one step is 0, so the sample is bins[0]; the merged set has S1 + 1 sorted depths with it in place"""
    z, w, _ = _random_case(8, 5, 9, 1)
    assert np.array_equal(IC.u_values(5, 1), np.zeros((5, 1), np.float32))
    z2 = IC.resample(z, w, 1)
    b0 = (np.float32(0.5) * (z[:, 1] + z[:, 0])).astype(np.float32)
    assert z2.shape == (5, 10)
    assert np.array_equal(z2[:, 1], b0) and np.array_equal(z2[:, 0], z[:, 0]) and np.array_equal(z2[:, 2:], z[:, 1:])


def test_helpers_restate_the_device_forms():
    """linspace01 is at::linspace's two-sided form: 0 first, 1 last, the upper half the lower one's mirror; the hash gives 24-bit u in
    [0, 1); a NaN depth sorts last"""
    assert np.array_equal(IC.linspace01(1), [0.0])
    for n in (2, 5, 16, 31):
        t = IC.linspace01(n)
        step = np.float32(1) / np.float32(n - 1)
        assert t.dtype == np.float32 and t[0] == 0 and t[-1] == 1 and (np.diff(t) > 0).all(), n
        assert np.array_equal(t[:n // 2], step * np.arange(n // 2, dtype=np.float32)), n
        assert np.array_equal(t[n // 2:], np.float32(1) - step * np.arange(n - 1 - n // 2, -1, -1, dtype=np.float32)), n
    u = IC.u_values(3, 16, det=False, seed=11)
    assert u.min() >= 0 and u.max() < 1 and len(np.unique(u)) == 48
    assert np.array_equal(u * np.float32(16777216.0), np.round(u * np.float32(16777216.0)))
    zc = np.array([[2.0, np.nan, 1.0, 1.0, np.inf]], np.float32)
    out = IC.rank_sort(zc)
    assert np.array_equal(out[0, :3], [1.0, 1.0, 2.0]) and np.isnan(out[0, 3]) and np.isinf(out[0, 4])


_NS_YAML = """coarse: True
tracking:
  ignore_edge_W: 4
  ignore_edge_H: 4
  use_color_in_tracking: True
  handle_dynamic: True
  w_color_loss: 0.5
  lr: 0.001
  pixels: 100
  iters: 3
mapping:
  color_refine: True
  middle_iter_ratio: 0.4
  fine_iter_ratio: 0.6
  BA: True
  BA_cam_lr: 0.001
  fix_fine: True
  fix_color: False
  keyframe_every: 50
  mapping_window_size: 5
  w_color_loss: 0.2
  frustum_feature_selection: True
  keyframe_selection_method: 'overlap'
  lr_first_factor: 5
  lr_factor: 1
  pixels: 200
  iters_first: 10
  iters: 5
"""
_CF_YAML = """mapping:
  pixels: 200
cam:
  H: 48
  W: 64
  fx: 40.0
  fy: 40.0
  cx: 32.0
  cy: 24.0
"""


@pytest.mark.parametrize("block, want", [
    ("rendering:\n  N_importance: 16\n", 16),
    ("rendering:\n  N_samples: 32   # N_importance absent from the block\n", 0),
    ("", 0),
])
def test_config_key_reaches_every_host_renderer(tmp_path, block, want):
    """rendering.N_importance of a configuration file is what a Renderer, a Tracker's and a Mapper's carry (host/importance_test --config,
    no device); an absent key or block means 0"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nice-slam-cpp_amd", "host", "importance_test")
    if not os.path.exists(exe):
        pytest.fail("importance_test is not built (run __graft_entry__.build())")
    ns, cf = tmp_path / "ns.yaml", tmp_path / "cf.yaml"
    ns.write_text(_NS_YAML + block)
    cf.write_text(_CF_YAML)
    r = subprocess.run([exe, "--config", str(ns), str(cf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"renderer": want, "tracker": want, "mapper": want}

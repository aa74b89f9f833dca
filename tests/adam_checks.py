"""Adam, element by element: an fp64 reference of the optimiser launch, a derived bound on what fp32 may differ from it, planted gradients.

The device formula (k_adam_multi, k_adam_scalar, k_pose_step, k_pose_multi; oracle/nso.c nso_adam_step), all operands fp32:

    m' = b1 m + (1 - b1) g                     v' = b2 v + (1 - b2) g g
    p' = p - step_size * (m' / (sqrtf(v') / bc2s + eps))
    step_size = lr / (1 - b1^t),  bc2s = sqrtf(1 - b2^t)        (host: adam_consts -- float32 of a double pow, float32 divide, sqrtf)

Reference (adam_ref, AdamTrack).  The same formula in fp64 on the values the device holds: float32(b1), float32(b2), float32(eps), float32(lr),
the float32 differences 1 - b1 and 1 - b2, and step_size / bc2s restated operation by operation as the host computes them (adam_consts below), so
the constants are the device's own and need no slack.  The fp32 RANGE is kept: a moment, quotient, update or parameter whose fp64 value rounds
to an infinite float32 is infinite in the reference (v' after g g overflowed, say, or m' / d for a caller's large m and tiny v); below the
range nothing is flushed -- the bound carries a subnormal spacing.

Bound (AdamTrack), derived, no constant fitted to any output.  u = 2^-24 is the relative error of one correctly rounded fp32 operation on a
normal result, s = 2^-149 the absolute error of one that lands among the subnormals (denormals are kept on gfx950).  The device moments cannot
be read back, so their errors em, ev (device minus reference, absolute) are carried from step to step; every operation below is counted once for
the uncontracted evaluation, and a contracted one (-ffp-contract=fast: a multiply fused into the following add or subtract) only removes a
rounding, so both lie inside.

  m':  t1 = fl(b1 m), t2 = fl((1-b1) g), m' = fl(t1 + t2): two roundings on each term's path.  The roundings are relative to the TERMS, not to
       their possibly cancelling sum, so the bound uses |b1 m| + |(1-b1) g| with |m| <= A + em, where A' = b1 A + (1-b1)|g| is a second
       recurrence on |g| (A >= |m| always):
           em' = b1 em + 3u (b1 (A + em) + (1-b1)|g|) + 2s                  (3u >= (1+u)^2 - 1 with room for the second order)
  v':  w1 = fl((1-b2) g), w2 = fl(w1 g), t = fl(b2 v), v' = fl(t + w2): three roundings on the g g path, two on the v path; w1 may be subnormal
       (error s, then multiplied by |g|), w2 and t may be (error s each) -- g g underflows to zero inside this term:
           ev' = b2 ev + 4u (b2 (v + ev) + (1-b2) g g) + s (|g| + 3)
  sqrt: S = sqrt(v').  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt a + sqrt b) <= sqrt|a - b|, so the carried ev' moves S by at most
           es0 = min(ev' / (S + sqrt(max(v' - ev', 0))), sqrt(ev'));           es = es0 + 2u (S + es0)
       (a correctly rounded sqrtf costs u; 2u leaves room for a faithfully rounded one -- decided before any run, like the divides below)
  q = S / bc2s:        eq = es / bc2s + 2u (q + es / bc2s) + s
  d = q + eps:         ed = eq + u (d + eq)
  r = m' / d:          |m^/d^ - m'/d| <= (em' d + |m'| ed) / (d (d - ed))   exactly, for d - ed > 0 (eps > 0 keeps it so; otherwise the
                       bound is infinite and the element counts as excluded, which the CPU test forbids):
                       er = that + 2u (|r| + that) + s
  upd = step_size r:   eu = |step_size| er + u (|upd| + |step_size| er) + s
  p' = p - upd:        ep' = ep + eu + u (|p'| + ep + eu)                   (u x >= half an ulp of any fp32 of magnitude <= x: the final
                       subtraction's rounding, or the single rounding of the fused p - step_size r)
  Where the reference v' is infinite the device's is too (tests/test_adam_cpu.py asserts no planted value comes near the edge of the range), the
  quotient is exactly 0 for a finite m' and the step adds no error; a non-finite m' makes p' NaN in the reference and the element is then only
  required to be non-finite on the device.  A voxel a mask leaves unmarked, and a float4 the "never touched" shortcut skips (g = m = v = 0:
  the update is exactly 0), keep p, moments and errors unchanged -- for them the bound stays 0 and the comparison is for equality.

Planted gradients (planted): seeded, new data every step, laid out by float4 group so that every voxel (8 groups) of a grid and every run of a
decoder carries several kinds:
  kinds 0..3   one group per position k: g[k] != 0 at the first step only (moderate size), zero everywhere else and ever after -- from the second
               step on m[k] and v[k] are the group's only non-zero values and the float must keep moving
  kinds 4..7   the same with g[k] ~ 1e-30: g g underflows, so from the second step on m[k] ALONE of the twelve values g[0..3], m[0..3], v[0..3]
               is non-zero (v[k] alone cannot be reached through gradients: m is non-zero whenever v is -- planted_state sets it directly
               where the caller owns the moments, nsk_adam_vector)
  kinds 8, 9   all zero from the start: must stay byte-identical
  kinds 10, 11 magnitudes as below, the sign of every element flips at every step
  kinds 12..22 magnitudes in decades 1e-30 .. 1e+15 and 1e+20, 1e+25, 3e+38 (g g underflows below 1e-19 and overflows to inf above 1.8e+19), random
               mantissa and sign, 8 % exact zeros, 4 % -0.0; kind 22 gets +inf, -inf, NaN in its first float at the LAST step (the steps
               before it still render with finite parameters)
  lr per step: 1e-3, 0, 1e-2, 5e-3 -- the second step must advance moments and step count without moving anything.
"""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24
SUB = 2.0 ** -149
FMAX = float(np.finfo(np.float32).max)
LRS = (1e-3, 0.0, 1e-2, 5e-3)
N_KINDS = 23
DECADES = tuple(10.0 ** k for k in range(-30, 16)) + (1e20, 1e25, 3e38)


def adam_consts(lr, b1, b2, step):
    """(step_size, bc2s) as float32, operation by operation what the host's adam_consts does"""
    lr, b1, b2 = F32(lr), F32(b1), F32(b2)
    bc1 = F32(1) - F32(math.pow(float(b1), int(step)))
    bc2 = F32(1) - F32(math.pow(float(b2), int(step)))
    with np.errstate(all="ignore"):
        return F32(lr / bc1), F32(np.sqrt(bc2))


def _range32(x):
    """fp64 values that round to an infinite float32 are infinite (the device's range); nothing else changes"""
    with np.errstate(all="ignore"):
        y = x.astype(np.float32)
    return np.where(np.isinf(y), y.astype(np.float64), x)


def adam_ref(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8, mask=None, parts=None):
    """one step in fp64 on the device's fp32 inputs -> (p', m', v'); mask (bool per element): False keeps p, m, v; parts (a dict) receives
    the quotient r and the update step_size r"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    fb1, fb2, feps = float(F32(b1)), float(F32(b2)), float(F32(eps))
    c1, c2 = float(F32(1) - F32(b1)), float(F32(1) - F32(b2))
    ss, bc2s = (float(x) for x in adam_consts(lr, b1, b2, step))
    with np.errstate(all="ignore"):
        m1 = _range32(fb1 * m + c1 * g)
        v1 = _range32(fb2 * v + _range32(c2 * g * g))
        r = _range32(m1 / _range32(_range32(np.sqrt(v1) / bc2s) + feps))
        upd = _range32(ss * r)
        p1 = _range32(p - upd)
    if mask is not None:
        mask = np.asarray(mask, bool)
        p1, m1, v1 = np.where(mask, p1, p), np.where(mask, m1, m), np.where(mask, v1, v)
    if parts is not None:
        parts["r"], parts["upd"] = r, upd
    return p1, m1, v1


class AdamTrack:
    """the fp64 reference trajectory of a parameter vector and, beside it, the running bound of |device - reference| (module docstring)"""

    def __init__(self, p0, b1=0.9, b2=0.999, eps=1e-8):
        self.b1, self.b2, self.eps = b1, b2, eps
        self.p = np.asarray(p0, np.float32).astype(np.float64).ravel().copy()
        self.ep = np.zeros_like(self.p)
        self.reset()

    def reset(self):
        """nsk_adam_reset: zero moments (and nothing known wrong about them); the parameters and their error stay"""
        z = np.zeros_like(self.p)
        self.m, self.v, self.A, self.em, self.ev = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()

    def step(self, g, lr, step, mask=None):
        g = np.asarray(g, np.float32).astype(np.float64).ravel()
        b1, b2, eps = float(F32(self.b1)), float(F32(self.b2)), float(F32(self.eps))
        c1, c2 = float(F32(1) - F32(self.b1)), float(F32(1) - F32(self.b2))
        ss, bc2s = (float(x) for x in adam_consts(lr, self.b1, self.b2, step))
        self.parts = {}
        p1, m1, v1 = adam_ref(self.p, g, self.m, self.v, lr, step, self.b1, self.b2, self.eps, parts=self.parts)
        ag = np.abs(g)
        with np.errstate(all="ignore"):
            A1 = b1 * self.A + c1 * ag
            em = b1 * self.em + 3 * U * (b1 * (self.A + self.em) + c1 * ag) + 2 * SUB
            ev = b2 * self.ev + 4 * U * (b2 * (self.v + self.ev) + c2 * g * g) + SUB * (ag + 3)
            m_bad, v_inf = ~np.isfinite(m1), np.isinf(v1)
            em = np.where(m_bad, 0.0, em)                 # p' is NaN there: the element is compared for being non-finite only
            ev = np.where(v_inf | np.isnan(v1), 0.0, ev)
            S = np.sqrt(v1)
            es0 = np.minimum(np.where(ev > 0, ev / (S + np.sqrt(np.maximum(v1 - ev, 0.0))), 0.0), np.sqrt(ev))
            es = es0 + 2 * U * (S + es0)
            q = S / bc2s
            eq = es / bc2s + 2 * U * (q + es / bc2s) + SUB
            d = q + eps
            ed = eq + U * (d + eq)
            r = m1 / d
            e0 = np.where(d - ed > 0, (em * d + np.abs(m1) * ed) / (d * (d - ed)), np.inf)
            er = e0 + 2 * U * (np.abs(r) + e0) + SUB
            er = np.where(v_inf & ~m_bad, 0.0, er)        # m' / inf = 0 exactly
            eu = abs(ss) * er + U * (np.abs(ss * r) + abs(ss) * er) + SUB
            eu = np.where(v_inf & ~m_bad, 0.0, eu)
            ep = self.ep + eu + U * (np.abs(p1) + self.ep + eu)
            ep = np.where(np.isfinite(p1), ep, np.nan)
        # the "never touched" shortcut changes nothing where the formula changes nothing, so it needs no case of its own -- but there the bound
        # stays what it was (0 for a parameter that never moved): equality is asked for, not closeness
        still = (g == 0) & (self.m == 0) & (self.v == 0)
        keep = still if mask is None else (still | ~np.asarray(mask, bool).ravel())
        sel = lambda new, old: np.where(keep, old, new)
        self.p, self.m, self.v, self.A = sel(p1, self.p), sel(m1, self.m), sel(v1, self.v), sel(A1, self.A)
        self.em, self.ev, self.ep = sel(em, self.em), sel(ev, self.ev), sel(ep, self.ep)

    def near_range_edge(self):
        """elements where a finite reference value of the last step (moments, quotient, update, parameter) stands so close to the edge of the
        fp32 range that the device may round to the other side"""
        with np.errstate(all="ignore"):
            edge = lambda x: np.isfinite(x) & (np.abs(x) > 0.99 * FMAX)
            return edge(self.v) | edge(self.m) | edge(self.p) | edge(self.parts["r"]) | edge(self.parts["upd"])

    def set_moments(self, m, v):
        """moments the caller owns (nsk_adam_vector): known exactly, so nothing is carried"""
        self.reset()
        self.m, self.v = np.asarray(m, np.float32).astype(np.float64).ravel(), np.asarray(v, np.float32).astype(np.float64).ravel()
        self.A = np.abs(self.m)

    def compare(self, dev, sel=None, what="p"):
        """dev: what the device holds (float32) of the parameters (what = "m", "v": of a moment).  -> dict(ratio: largest |dev - ref| / bound
        over the finite reference elements (inf where the bound is 0 and the values differ), compared: how many those were, nonfinite:
        reference elements that are inf / NaN, nonfinite_ok: the device is non-finite at every one of them, excluded: finite reference
        elements without a finite bound, worst: index of the largest ratio)"""
        dev = np.asarray(dev, np.float32).astype(np.float64).ravel()
        idx = np.arange(self.p.size) if sel is None else np.flatnonzero(np.asarray(sel).ravel())
        full_ref, full_ep = {"p": (self.p, self.ep), "m": (self.m, self.em), "v": (self.v, self.ev)}[what]
        ref, ep, dv = full_ref[idx], full_ep[idx], dev[idx]
        fin = np.isfinite(ref)
        with np.errstate(all="ignore"):
            err = np.abs(dv[fin] - ref[fin])
            bound = ep[fin]
            ratio = np.where(err == 0, 0.0, np.where(np.isfinite(bound) & (bound > 0), err / bound, np.inf))
            ratio = np.where(np.isfinite(err), ratio, np.inf)
        worst = int(idx[fin][np.argmax(ratio)]) if ratio.size else -1
        return dict(ratio=float(ratio.max()) if ratio.size else 0.0, compared=int(fin.sum()), nonfinite=int((~fin).sum()),
                    nonfinite_ok=bool((~np.isfinite(dv[~fin])).all()), excluded=int((~np.isfinite(ep[fin])).sum()), worst=worst)


# ---- planted data -----------------------------------------------------------------------------------------------------------------------------
def kinds(n):
    """kind (module docstring) of every element of a vector of n floats, n a multiple of 4"""
    assert n % 4 == 0
    return np.repeat(np.arange(n // 4) % N_KINDS, 4)


def planted(n, steps=4, seed=0, nonfinite=True):
    """dict(g [steps][n] float32, p0 [n] float32, lr [steps], kind [n]): the planted sequence of the module docstring"""
    rng = np.random.default_rng(seed)
    kind, pos = kinds(n), np.arange(n) % 4
    grp = np.arange(n) // 4
    base_sign = rng.choice([-1.0, 1.0], n)
    g = np.zeros((steps, n), np.float32)
    for t in range(steps):
        dec, mant = rng.choice(DECADES, n), rng.uniform(1.0, 9.99, n)
        # 1e20: (1 - b2) g g stays finite, and with mantissas up to 2.5 so does v after five such steps (0.005 * 6.25e40 < 0.99 FLT_MAX) -- no
        # planted value stands at the edge of the fp32 range, where the device could round to the other side of it than the reference
        mag = np.minimum(dec * np.where(dec == 1e20, 1.0 + (mant - 1.0) / 6.0, mant), 3.0e38)
        sign = np.where((kind == 10) | (kind == 11), base_sign * (1.0 if t % 2 == 0 else -1.0), rng.choice([-1.0, 1.0], n))
        gt = (sign * mag).astype(np.float32)
        z = rng.random(n)
        gt[z < 0.08] = 0.0
        gt[(z >= 0.08) & (z < 0.12)] = -0.0
        one = rng.choice([-1.0, 1.0], n) * np.where(kind < 4, 10.0 ** rng.uniform(-3, 3, n), 1e-30 * rng.uniform(1.0, 9.99, n))
        gt = np.where(kind < 8, np.where((t == 0) & (pos == kind % 4), one, 0.0), gt).astype(np.float32)
        gt[(kind == 8) | (kind == 9)] = 0.0
        if nonfinite and t == steps - 1:
            first = (kind == 22) & (pos == 0)
            gt[first] = np.array([np.inf, -np.inf, np.nan], np.float32)[(grp[first] // N_KINDS) % 3]
        g[t] = gt
    p0 = (rng.standard_normal(n) * 0.01).astype(np.float32)
    z = rng.random(n)
    p0[z < 0.05] = 0.0
    p0[(z >= 0.05) & (z < 0.08)] = -0.0
    return dict(g=g, p0=p0, lr=[LRS[t % len(LRS)] for t in range(steps)], kind=kind)


def planted_state(n, seed):
    """one step of a vector whose moments the caller owns (nsk_adam_vector), any n: dict(p0, g, m0, v0) with the planted magnitudes in all
    three of g, m0 and v0 (v0 >= 0, a fifth of it zero, kept below 1e31 so that only g g takes v' out of the range).  Here the moments can be
    set apart: in the groups of kinds 0..3 m0[k] alone is non-zero, in those of kinds 4..7 v0[k] alone (g = 0 in both)"""
    seq = planted((n + 3) & ~3, steps=3, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    kind, pos = seq["kind"][:n], np.arange(n) % 4
    m0 = np.where(np.isfinite(seq["g"][0][:n]), seq["g"][0][:n], 0).astype(np.float32)
    v0 = np.minimum(np.abs(seq["g"][1][:n]), 1e31).astype(np.float32)
    v0[rng.random(n) < 0.2] = 0.0
    lone_v = (kind >= 4) & (kind < 8)
    m0[lone_v] = 0.0
    v0[lone_v & (pos == kind % 4)] = (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)[lone_v & (pos == kind % 4)]
    return dict(p0=seq["p0"][:n].copy(), g=seq["g"][2][:n].copy(), m0=m0, v0=v0)


def garbage(n, seed):
    """what the slab may hold at voxels a mask leaves unmarked: large finite values and NaN"""
    rng = np.random.default_rng(seed)
    x = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(20, 38, n)).astype(np.float32)
    x[rng.random(n) < 0.25] = np.nan
    return x


def voxel_masks(nvox, seed=0):
    """the mask cases of a level: name -> uint8 [nvox] (None: no mask)"""
    rng = np.random.default_rng(seed)
    one = lambda idx: np.bincount(np.atleast_1d(idx), minlength=nvox).astype(bool).astype(np.uint8)
    return {"none": None, "all": np.ones(nvox, np.uint8), "empty": np.zeros(nvox, np.uint8), "first": one(0), "last": one(nvox - 1),
            "33": one(rng.choice(nvox, min(33, nvox), replace=False)), "half": (rng.random(nvox) < 0.5).astype(np.uint8)}


def voxels_to_floats(mask):
    return None if mask is None else np.repeat(np.asarray(mask, bool), 32)


# ---- the kernel's formula in fp32 numpy, and wrong variants of it --------------------------------------------------------------------------
MUTANTS = ("eps_in_sqrt", "step_off_by_one", "bias_on_v_inside_sqrt", "betas_exchanged", "abs_g_for_g2", "shortcut_on_g_zero",
           "lr0_freezes_moments", "unmarked_voxel_moves", "last_marked_of_block_missing")


def marked_list(mask_vox, mutant=None):
    """k_mask_index's ascending list of marked voxels -- or a wrong one"""
    idx = np.flatnonzero(np.asarray(mask_vox, bool))
    if mutant == "unmarked_voxel_moves":
        off = np.flatnonzero(~np.asarray(mask_vox, bool))
        idx = np.sort(np.append(idx, off[len(off) // 2]))
    if mutant == "last_marked_of_block_missing":
        nvox = len(mask_vox)
        last = [idx[(idx >= b) & (idx < b + 1024)].max() for b in range(0, nvox, 1024) if ((idx >= b) & (idx < b + 1024)).any()]
        idx = np.setdiff1d(idx, last[-1:])
    return idx


def kernel_step(p, m, v, g, lr, step, b1=0.9, b2=0.999, eps=1e-8, fma=False, mutant=None, mask_vox=None):
    """k_adam_multi's arithmetic on float32 arrays -> (p', m', v').  fma: every multiply-add as one fp64 operation rounded once (a contracted
    evaluation); mask_vox: uint8 per voxel of 32 floats; mutant: a name of MUTANTS"""
    p, m, v, g = (np.asarray(a, np.float32) for a in (p, m, v, g))
    if mutant == "lr0_freezes_moments" and lr == 0:
        return p.copy(), m.copy(), v.copy()
    fb1, fb2 = (F32(b2), F32(b1)) if mutant == "betas_exchanged" else (F32(b1), F32(b2))
    c1, c2, feps = F32(1) - fb1, F32(1) - fb2, F32(eps)
    ss, bc2s = adam_consts(lr, fb1, fb2, step + 1 if mutant == "step_off_by_one" else step)
    d64 = lambda a: np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        gg = np.abs(g) if mutant == "abs_g_for_g2" else (c2 * g) * g
        if mutant == "abs_g_for_g2":
            gg = c2 * gg
        if fma:
            mm = (d64(fb1) * d64(m) + d64(c1 * g)).astype(np.float32)
            vv = (d64(fb2) * d64(v) + d64(gg)).astype(np.float32)
        else:
            mm = fb1 * m + c1 * g
            vv = fb2 * v + gg
        if mutant == "eps_in_sqrt":
            denom = np.sqrt(vv + feps) / bc2s
        elif mutant == "bias_on_v_inside_sqrt":
            denom = np.sqrt(vv / bc2s) + feps
        else:
            denom = np.sqrt(vv) / bc2s + feps
        r = mm / denom
        pp = (d64(p) - d64(ss) * d64(r)).astype(np.float32) if fma else p - ss * r
    if p.size % 4:                  # k_adam_scalar: a plain vector, no float4 shortcut
        return pp, mm, vv
    z4 = lambda a: np.repeat((a.reshape(-1, 4) == 0).all(axis=1), 4)
    skip = z4(g) if mutant == "shortcut_on_g_zero" else (z4(g) & z4(m) & z4(v))
    if mask_vox is not None:
        on = np.zeros(len(mask_vox), bool)
        on[marked_list(mask_vox, mutant)] = True
        skip = skip | ~np.repeat(on, 32)
    return np.where(skip, p, pp), np.where(skip, m, mm), np.where(skip, v, vv)

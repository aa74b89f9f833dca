"""CPU tests of tests/adam_checks.py: the fp64 reference agrees with the project's oracle, the kernel's formula in fp32 (plain and with
contracted multiply-adds) stays inside the derived bound on every planted sequence, every wrong variant leaves it, nothing is excluded."""
import numpy as np
import pytest

import adam_checks as ac

N = 23 * 4 * 24            # every kind 24 times
NVOX = 1100                # one full block of 1024 voxels and a partial one


def _run(seq, fma=False, mutant=None, mask_vox=None, unmask_last=False):
    """the emulated kernel beside the reference over a planted sequence -> list of compare() results, one per step"""
    n = seq["p0"].size
    tr = ac.AdamTrack(seq["p0"])
    p, m, v = seq["p0"].copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    out = []
    steps = len(seq["lr"])
    for t in range(steps):
        mk = None if (unmask_last and t == steps - 1) else mask_vox
        g = seq["g"][t].copy()
        if mk is not None:
            off = ~ac.voxels_to_floats(mk)
            g[off] = ac.garbage(n, 100 + t)[off]
        p, m, v = ac.kernel_step(p, m, v, g, seq["lr"][t], t + 1, fma=fma, mutant=mutant, mask_vox=mk)
        tr.step(seq["g"][t], seq["lr"][t], t + 1, mask=ac.voxels_to_floats(mk))
        assert not tr.near_range_edge().any()
        out.append(tr.compare(p))
    return out, tr


def test_reference_agrees_with_the_oracle(oracle64):
    seq = ac.planted(N, steps=4, seed=1, nonfinite=False)
    tame = (np.abs(seq["g"]) <= 1e15).all(axis=0)          # the oracle's fp64 has no fp32 range to leave
    p = seq["p0"].astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    po, mo, vo = p.copy(), m.copy(), v.copy()
    f = lambda x: float(np.float32(x))
    for t in range(4):
        before = p.copy()
        p, m, v = ac.adam_ref(p, seq["g"][t], m, v, seq["lr"][t], t + 1)
        oracle64.adam_step(po, seq["g"][t].astype(np.float64), mo, vo, f(seq["lr"][t]), t + 1, b1=f(0.9), b2=f(0.999), eps=f(1e-8))
        # the oracle forms 1 - b^t in fp64, the device's host code in fp32: 2^-24 relative on a bias correction of at least 1e-3
        tol = 2e-4 * np.abs(p - before) + 1e-300
        assert (np.abs(p - po)[tame] <= tol[tame] + 1e-12 * np.abs(p[tame])).all(), t
        assert np.allclose(m[tame], mo[tame], rtol=1e-12, atol=0) and np.allclose(v[tame], vo[tame], rtol=1e-12, atol=0)
        po[:], mo[:], vo[:] = p, m, v                     # (both start every step from the same state: the comparison is per step)
    assert (p != seq["p0"])[tame & (seq["kind"] < 8)].any()


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_fp32_formula_stays_inside_the_bound(fma, masked):
    n = NVOX * 32 if masked else N
    worst = 0.0
    for seed in range(3):
        seq = ac.planted(n, steps=4, seed=seed)
        mk = ac.voxel_masks(NVOX, seed)["half"] if masked else None
        res, tr = _run(seq, fma=fma, mask_vox=mk, unmask_last=masked)
        planted_bad = int((~np.isfinite(seq["g"][-1])).sum())
        assert planted_bad > 0
        for t, r in enumerate(res):
            # nothing is excluded: every element is compared but those the reference itself makes inf / NaN -- the planted ones of the last step
            assert r["excluded"] == 0 and r["compared"] + r["nonfinite"] == n
            assert r["nonfinite"] == (planted_bad if t == len(res) - 1 else 0), (t, r)
            assert r["nonfinite_ok"]
            assert r["ratio"] <= 1.0, (seed, t, r)
            worst = max(worst, r["ratio"])
        zero = (seq["kind"] == 8) | (seq["kind"] == 9)
        assert np.array_equal(tr.p[zero].astype(np.float32).view(np.uint32), seq["p0"][zero].view(np.uint32))
        # the one-value groups keep moving after their only gradient (kinds 0..3: on m and v, kinds 4..7: on m alone)
        hot = (seq["kind"] < 8) & (seq["g"][0] != 0)
        assert hot.sum() == (seq["kind"] < 8).sum() // 4
        if not masked:
            t2 = ac.AdamTrack(seq["p0"])
            t2.step(seq["g"][0], seq["lr"][0], 1)
            p1 = t2.p.copy()
            t2.step(seq["g"][1], seq["lr"][1], 2)
            assert np.array_equal(t2.p, p1)                                  # lr = 0 moves nothing ...
            t2.step(seq["g"][2], seq["lr"][2], 3)
            # ... and the next step moves on moments two steps old (a 1e-30 gradient moves by ~1e-25: visible only on a parameter that small)
            assert (t2.p[hot & (seq["kind"] < 4)] != p1[hot & (seq["kind"] < 4)]).all() and (t2.m[hot] != 0).all()
            assert (t2.v[hot & (seq["kind"] >= 4)] < 2.0 ** -149).all()      # g g underflowed: fp32 holds v = 0 there
    print("largest error / bound, fma=%s masked=%s: %.3f" % (fma, masked, worst))
    assert worst > 0.01          # the bound is not vacuous: fp32 uses a visible share of it


@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    masked = mutant in ("unmarked_voxel_moves", "last_marked_of_block_missing")
    caught = 0
    for fma in (False, True):
        seq = ac.planted(NVOX * 32 if masked else N, steps=4, seed=5)
        mk = ac.voxel_masks(NVOX, 5)["half"] if masked else None
        res, _ = _run(seq, fma=fma, mutant=mutant, mask_vox=mk)
        assert max(r["ratio"] for r in res) > 1.0 or not all(r["nonfinite_ok"] for r in res), (mutant, fma)
        caught += 1
    print("mutant %s: caught (plain and contracted)" % mutant)
    assert caught == 2


@pytest.mark.parametrize("fma", [False, True])
def test_single_steps_from_planted_moments(fma):
    """the states tests/test_gpu_adam.py hands to nsk_adam_vector: p, m and v of the fp32 formula inside the single-step bound, none of them at
    the edge of the range, a wrong step count outside"""
    for n in (1, 7, 255, 256, 257, 1000):
        for j, step in enumerate((1, 2, 1000, 100000)):
            st = ac.planted_state(n, 71 + j)
            tr = ac.AdamTrack(st["p0"])
            tr.set_moments(st["m0"], st["v0"])
            tr.step(st["g"], ac.LRS[j], step)
            assert not tr.near_range_edge().any(), (n, step)
            for mutant in (None, "step_off_by_one"):
                p, m, v = ac.kernel_step(st["p0"], st["m0"], st["v0"], st["g"], ac.LRS[j], step, fma=fma, mutant=mutant)
                res = [tr.compare(x, what=w) for w, x in (("p", p), ("m", m), ("v", v))]
                assert all(r["excluded"] == 0 and r["compared"] + r["nonfinite"] == n and r["nonfinite_ok"] for r in res)
                if mutant is None:
                    assert max(r["ratio"] for r in res) <= 1.0, (n, step, res)
                elif n >= 255 and ac.LRS[j] > 0 and step < 100000:        # (at step 100000 both bias corrections are 1 either way)
                    assert res[0]["ratio"] > 1.0, (n, step)


def test_constants_are_the_hosts():
    """step_size and bc2s are float32 and close to the fp64 values: rounding b^t to float32 moves 1 - b^t by at most u absolutely, the
    subtraction is then exact or rounds once, the divide / sqrt round once"""
    for step in (1, 2, 1000, 100000):
        ss, bc2s = ac.adam_consts(1e-3, 0.9, 0.999, step)
        assert ss.dtype == np.float32 and bc2s.dtype == np.float32
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        assert abs(float(ss) - float(np.float32(1e-3)) / bc1) <= (ac.U / bc1 + 2 * ac.U) * float(ss)
        assert abs(float(bc2s) - np.sqrt(bc2)) <= (ac.U / bc2 + 2 * ac.U) * float(bc2s)

"""CPU proof of the operand-range helpers (tests/operand_range.py) and the ATen expectation for non-finite values in the map, before any GPU
is involved (tests/test_gpu_operand_range.py builds on both)."""
import numpy as np
import pytest

import operand_range as OR
import scenes

SC = OR.op_scene()
PTS = OR.op_points(SC)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("which", scenes.LEVELS)
def test_rebalance_is_exact_in_both_oracles(which, oracle32, oracle64):
    """(a) For every decoder, every block i and a in {-12, 12} (and 20, the over-range tests' reach): the hidden pre-activations of block i are
    bit for bit 2^a times the unscaled ones, those of every other block and the outputs bit-identical -- in the fp32 and in the fp64 oracle
    (oracle/nso.c has its own make_layout: this pins the packing offsets of rebalance).  Stage = the decoder's own (fine runs middle + fine,
    colour all three), so the untouched decoders are checked through the outputs."""
    for o in (oracle32, oracle64):
        base_raw = o.eval_points(SC["bound"], SC["grids"], SC["decoders"], which, PTS)
        base_pre = o.point_preacts(SC["bound"], SC["grids"], SC["decoders"], which, which, PTS)
        assert np.isfinite(base_raw).all() and np.abs(base_pre).max() > 0
        for i in range(5):
            for a in (-12, 12, 20):
                decs = dict(SC["decoders"], **{which: OR.rebalance(SC["decoders"][which], which, i, a)})
                raw = o.eval_points(SC["bound"], SC["grids"], decs, which, PTS)
                pre = o.point_preacts(SC["bound"], SC["grids"], decs, which, which, PTS)
                assert np.array_equal(_bits(raw), _bits(base_raw)), (which, i, a)
                want = base_pre.copy()
                want[:, i] *= o.dt(2.0) ** a
                assert np.array_equal(_bits(pre), _bits(want)), (which, i, a)
        exps = [7, -7, 7, -7, 7]
        decs = dict(SC["decoders"], **{which: OR.rebalance_all(SC["decoders"][which], which, exps)})
        assert np.array_equal(_bits(o.eval_points(SC["bound"], SC["grids"], decs, which, PTS)), _bits(base_raw))
        pre = o.point_preacts(SC["bound"], SC["grids"], decs, which, which, PTS)
        assert np.array_equal(_bits(pre), _bits(base_pre * (o.dt(2.0) ** np.array(exps, o.dt))[None, :, None]))


@pytest.mark.parametrize("stage", scenes.LEVELS)
def test_scale_features_is_exact_in_both_oracles(stage, oracle32, oracle64):
    """the same for scale_features on every level the stage reads: outputs and every hidden pre-activation bit-identical (the trilinear
    lookup of a grid times 2^a is the lookup times 2^a, and the fc columns take the factor back)"""
    for o in (oracle32, oracle64):
        base_raw = o.eval_points(SC["bound"], SC["grids"], SC["decoders"], stage, PTS)
        for level in OR.DECODERS_OF[stage]:
            for a in (-12, 12, 19):
                g, d = OR.scale_features(SC["grids"], SC["decoders"], level, a)
                assert np.array_equal(g[level], SC["grids"][level] * np.float32(2.0) ** a)
                assert np.array_equal(_bits(o.eval_points(SC["bound"], g, d, stage, PTS)), _bits(base_raw)), (stage, level, a)
                for which in OR.DECODERS_OF[stage]:
                    assert np.array_equal(_bits(o.point_preacts(SC["bound"], g, d, stage, which, PTS)),
                                          _bits(o.point_preacts(SC["bound"], SC["grids"], SC["decoders"], stage, which, PTS)))


def test_exponent_window_keeps_weights_below_the_limit():
    for which in scenes.LEVELS:
        P = SC["decoders"][which]
        for i in range(5):
            lo, hi = OR.exponent_window(P, which, i)
            assert lo < -10 and hi > 10
            for a, inside in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False)):
                assert (OR.max_weight(OR.rebalance(P, which, i, a), which) < 2.0 ** OR.W_LIMIT) == inside, (which, i, a)


def test_point_evaluation_is_the_sample_evaluation(oracle32):
    """Oracle.eval_points goes through render_forward with one-sample rays of zero direction, so that the sample is the point bit for bit.
    Checked against the samples of real rays (raw at the sample (o, d, z) = eval_points at the float32 point o + d z), against the
    "100 outside the bound" rule and against ATen's eval_points."""
    rays = OR.op_rays(SC)
    fw = oracle32.render_forward(oracle32.opts(SC["bound"]), SC["grids"], SC["decoders"], "color", rays["rays_o"], rays["rays_d"], rays["gt_depth"], want_aux=True)
    p = (rays["rays_o"][:, None, :] + rays["rays_d"][:, None, :] * fw["z"][:, :, None]).astype(np.float32).reshape(-1, 3)
    assert np.array_equal(_bits(oracle32.eval_points(SC["bound"], SC["grids"], SC["decoders"], "color", p)), _bits(fw["raw"].reshape(-1, 4)))
    raw = oracle32.eval_points(SC["bound"], SC["grids"], SC["decoders"], "color", PTS)
    b = SC["bound"]
    inb = np.all((PTS < b[:, 1]) & (PTS > b[:, 0]), axis=1)
    assert inb.sum() > 100 and (~inb).sum() > 10 and (raw[~inb, 3] == 100).all() and (raw[inb, 3] != 100).all()
    assert scenes.rel_l2(raw[inb], OR.aten_eval_points(SC, "color", PTS)[inb]) < 1e-5


def _footprint(sc, level, zyx, pts):
    """points whose trilinear footprint (F.grid_sample, align_corners, border padding) includes voxel zyx"""
    b = np.asarray(sc["bound"], np.float64)
    dims = sc["grids"][level].shape[1:][::-1]                       # X, Y, Z
    hit = np.ones(len(pts), bool)
    for k in range(3):
        x = np.clip((pts[:, k].astype(np.float64) - b[k, 0]) / (b[k, 1] - b[k, 0]) * (dims[k] - 1), 0, dims[k] - 1)
        i0 = np.floor(x)
        v = zyx[2 - k]
        hit &= (i0 == v) | ((i0 + 1 == v) & (i0 + 1 <= dims[k] - 1))
    return hit


@pytest.mark.parametrize("stage", scenes.LEVELS)
def test_aten_propagates_a_nan_voxel_to_every_point_that_touches_it(stage):
    """(b) The expectation for non-finite values in the map comes from ATen on the CPU (oracle/torch_ref.py: the ops the reference calls), NOT
    from oracle/nso.c: torch::relu propagates a NaN, the plain-C oracle's `s > 0 ? s : 0` turns it into 0 (a comparison with NaN is false), so
    in nso.c a NaN that reaches a hidden ReLU without a later fc term -- the coarse decoder's last block -- comes out finite.  That is the very
    defect these tests look for in the kernels, so the plain-C oracle cannot be the reference of this file.
    With one voxel row set to NaN, every point inside the bound whose trilinear footprint includes that voxel has a non-finite occupancy (colour
    stage: non-finite colour when the colour level is hit), every other output is bit-identical to the clean scene's: the "touched" set."""
    clean = OR.aten_eval_points(SC, stage, PTS)
    b = SC["bound"]
    inb = np.all((PTS < b[:, 1]) & (PTS > b[:, 0]), axis=1)
    assert np.isfinite(clean).all()
    for level in OR.DECODERS_OF[stage]:
        zyx = OR.central_voxel(SC, level)
        raw = OR.aten_eval_points(SC, stage, PTS, grids=OR.poison_voxel(SC["grids"], level, zyx, "nan+"))
        hit = _footprint(SC, level, zyx, PTS)
        assert (hit & inb).sum() >= 3 and (~hit & inb).sum() >= 3
        ch = slice(0, 3) if level == "color" else 3
        bad = ~np.isfinite(raw[:, ch]).reshape(len(PTS), -1).all(axis=1)
        assert np.array_equal(bad[inb], hit[inb]), (stage, level)
        touched = ~np.isfinite(raw).all(axis=1)
        assert np.array_equal(_bits(raw[~touched]), _bits(clean[~touched]))
        if level == "color":
            assert np.array_equal(touched, hit)                      # the colour has no "100 outside" rule

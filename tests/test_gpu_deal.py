"""GPU tests (-m gpu) of the backward's queue dealing: in k_decode_bwd_multi a skipping frozen role deals the first part of its tiles statically
and claims the rest, a few consecutive tiles at a time, from a cursor in device memory (the trainable role and the 16-wave kernel of the all-frozen
launches deal statically).  Every comparison is this build against this build with nsk_set_tuning("static_deal", 1), which deals every tile as
tile_of does.

Bounds (none of them new): two runs that differ only in the order of their atomic adds agree to 1e-5 in their gradients and in the parameters
after Adam (test_gpu_dead_skip.py, test_gpu_split.py: the same comparison); the loss does not depend on the backward and is bit-equal.  The
frozen roles' tile counters equal numpy's count on the step's own slot order (live_tiles.py) under both dealings: a tile dealt twice or not at
all would move them.

Sizes (x 48 samples, 16 per tile): 2 rays = 6 tiles, one group, most workgroups get nothing; 203 rays = 609 tiles, a ragged last group, fewer
groups than workgroups; 700 rays = 2100 tiles, about one round of the launch's waves; 1400 rays = 4200 tiles, more than two rounds, so the
claimed tail and the claims two ahead are exercised past the first round.

What claims and what does not.  A role claims only with liveness bytes (a mask on its level) and, by default, with 24 rounds of tiles per wave or
more, which takes a K3-size batch: no test here runs a dealt launch at that default; the queue is switched on with "deal_min_rounds" 0.  So the
mask-"none" cases (no role skips) and the plain fine-stage case (k_decode_bwd_frozen never claims) compare static dealing with static dealing:
they hold the keys to changing nothing there.  The claiming kernel runs in the colour-stage cases with a mask and in the fine-stage cases with
"no_frozen_kernel"."""
import numpy as np
import pytest
import torch

import scenes
import test_gpu_dead_skip as ds
from scenes import rel_l2

pytestmark = pytest.mark.gpu
LEVELS = ds.LEVELS
LR = ds.LR
MASKS = ["none", "frustum", "half", "ones", "zeros"]
SIZES = [2, 203, 700, 1400]
BOUND = 1e-5
QUEUE = {"deal_min_rounds": 0}      # by default a role claims only where its waves have 24 rounds of tiles or more: none of these sizes has


def _masks(kind):
    return None if kind == "none" else ds._masks(kind)


def _rays(n):
    """exactly n rays (make_rays deals n // n_frames pixels to each camera): 203 = 7 cameras x 29"""
    key = ("deal_rays", n)
    if key not in ds._cache:
        ds._cache[key] = scenes.make_rays(60 + n, n, ds._scene()["bound"], n_frames=7 if n % 7 == 0 else (5 if n % 5 == 0 else 1))
        assert ds._cache[key]["rays_o"].shape[0] == n
    return ds._cache[key]


def _run(stage, masks, r, tune, sort_mode, steps=1, graph=False):
    """`steps` mapping steps (map_step + adam_step) of one batch; what the LAST step left: loss, gradients (downloaded before its Adam step when
    the steps are eager), the parameters after Adam, the frozen roles' tile counters (checked against numpy on the way)"""
    ctx = ds._new_ctx(stage, masks, tune, sort_mode)
    ro, rd, gd, gc = ds._tensors(r)
    loss = torch.zeros(1, device="cuda")
    color = stage == "color"
    levels = LEVELS if color else ("middle", "fine")
    out = {}
    with torch.cuda.stream(ctx.tstream):
        def step(last):
            ctx.map_step(stage, ro, rd, gd, gc, -1.0, 0.5, color, flags=3 if color else 1, loss=loss)
            if last and not graph:
                ctx.sync()
                out["g"] = {k: ctx.grid_download(k, grad=True) for k in levels}
                out["dec_g"] = ctx.decoder_download("color", grad=True) if color else None
                out["counts"] = ds._check_counts(ctx, stage, masks, r, 48, ["middle", "fine"])
            ctx.adam_step(LR)
        if graph:
            step(False)                                   # an eager step first (it sizes the workspaces): the first of `steps`
            ctx.graph_begin(); step(False); gid = ctx.graph_end()
            for _ in range(steps - 1):
                ctx.graph_launch(gid)
        else:
            for i in range(steps):
                step(i == steps - 1)
    ctx.sync()
    if graph:
        out["counts"] = ds._check_counts(ctx, stage, masks, r, 48, ["middle", "fine"])
    out["loss"] = float(loss)
    out["p"] = {k: ctx.grid_download(k) for k in levels}
    out["dec_p"] = ctx.decoder_download("color") if color else None
    ctx.close()
    return out


def _agree(a, b, what, grads=True):
    figs = {}
    if grads:
        for k in a["g"]:
            figs["g_" + k] = rel_l2(a["g"][k], b["g"][k])
        if a["dec_g"] is not None:
            figs["g_dec"] = rel_l2(a["dec_g"], b["dec_g"])
    for k in a["p"]:
        figs["p_" + k] = rel_l2(a["p"][k], b["p"][k])
    if a["dec_p"] is not None:
        figs["p_dec"] = rel_l2(a["dec_p"], b["dec_p"])
    print(what, "loss", a["loss"], b["loss"], {k: float("%.3g" % v) for k, v in figs.items()})
    for k, v in figs.items():
        assert v < BOUND, (what, k, v)


@pytest.mark.parametrize("n_rays", SIZES)
@pytest.mark.parametrize("kind", MASKS)
def test_queue_dealt_step_equals_the_statically_dealt_step(kind, n_rays):
    masks, r = _masks(kind), _rays(n_rays)
    ntiles = (n_rays * 48 + 15) // 16
    # the fine stage twice: through its own 16-wave kernel (k_decode_bwd_frozen, which deals statically whatever the key says) and, with
    # "no_frozen_kernel", through k_decode_bwd_multi, where its two roles claim their tails as they do beside the colour role
    for stage, tune in (("color", {}), ("fine", {}), ("fine", {"no_frozen_kernel": 1})):
        for sort_mode in (1, 0):
            what = "%s%s %s %d rays, %s order:" % (stage, " (multi kernel)" if tune else "", kind, n_rays, "cell" if sort_mode else "ray")
            q = _run(stage, masks, r, dict(tune, **QUEUE), sort_mode)
            s = _run(stage, masks, r, dict(tune, static_deal=1), sort_mode)
            assert q["loss"] == s["loss"], (what, q["loss"], s["loss"])
            _agree(q, s, what)
            # _check_counts held the counters of either run to numpy's count of its own slot order; the order-free cases here as well
            if kind in ("none", "ones"):
                assert q["counts"][0] == s["counts"][0] == ntiles and q["counts"][1] == s["counts"][1] == ntiles, (what, q["counts"], s["counts"])
            if kind == "zeros":
                assert q["counts"][0] == s["counts"][0] == 0 and q["counts"][1] == s["counts"][1] == 0, (what, q["counts"], s["counts"])
                assert all(not g.any() for g in q["g"].values()), what          # the colour grid's gradient slab among them: untouched
                if stage == "color":
                    assert np.abs(q["dec_g"]).max() > 0 or n_rays < 100, what
            if sort_mode == 0:                            # ray order is the same slot order in both runs
                assert q["counts"].tolist() == s["counts"].tolist(), (what, q["counts"], s["counts"])


@pytest.mark.parametrize("stage,tune", [("color", {}), ("fine", {"no_frozen_kernel": 1})])
def test_a_replayed_graph_gives_the_eager_steps(stage, tune):
    """the cursors are armed by a launch inside the captured step, so every replay starts them at zero: an eager step and three replays of the
    captured step (map_step + adam_step) leave what four eager steps leave, and the last replay's tile counters are exact"""
    masks, r = ds._masks("frustum"), _rays(1400)
    for sort_mode in (1, 0):
        what = "%s graph, %s order:" % (stage, "cell" if sort_mode else "ray")
        g = _run(stage, masks, r, dict(tune, **QUEUE), sort_mode, steps=4, graph=True)
        e = _run(stage, masks, r, dict(tune, **QUEUE), sort_mode, steps=4)
        s = _run(stage, masks, r, dict(tune, static_deal=1), sort_mode, steps=4)
        assert abs(g["loss"] - e["loss"]) <= 1e-6 * abs(e["loss"]), (what, g["loss"], e["loss"])
        _agree(g, e, what + " replayed against eager", grads=False)
        _agree(e, s, what + " eager against static")


def test_static_deal_is_what_the_deterministic_mode_and_no_dead_skip_run():
    """the fixed paths: the deterministic mode stays bit-reproducible with and without the key, and with no_dead_skip nothing is claimed or skipped
    (every tile counted, the gradients those of the skipping run)"""
    masks, r = ds._masks("half"), _rays(203)
    d0 = ds._step("color", masks, r, tune={"deterministic": 1})
    d1 = ds._step("color", masks, r, tune={"deterministic": 1, "static_deal": 1})
    ds._same_step(d0, d1, exact=True)
    full = ds._step("color", masks, r, tune={"no_dead_skip": 1}, check=True)
    assert full["counts"][3] == 0 and full["counts"][0] == 609 and full["counts"][1] == 609 and full["counts"][2] == -1
    ds._same_step(ds._step("color", masks, r), full, exact=False)

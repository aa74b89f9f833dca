"""GPU tests (-m gpu) of the backward's dead-tile skip: with an optimiser mask on a level (nsk_set_mask / nsk_frustum_mask) a frozen decoder's
backward does not run a 16-sample tile none of whose samples touches a marked voxel.  Every comparison is this build with the skip against
this build with nsk_set_tuning("no_dead_skip", 1); the oracle tests cover the rest.

Bounds (none of them new): gradients of two runs that differ only in the order of their atomic adds agree to 1e-5 (test_gpu_dist.py::
test_deterministic_debug_mode_is_bit_reproducible), parameters after Adam to 5e-3 of the update (test_map_prepare_gives_the_unprepared_steps),
ray gradients to 1e-6 (test_gpu_parity.py, the Tracker's three forms); the deterministic mode is bit equality."""
import numpy as np
import pytest
import torch

import live_tiles as lt
import scenes
from gpu_util import cu, make_ctx
from scenes import rel_l2

pytestmark = pytest.mark.gpu
LEVELS = ("middle", "fine", "color")
SHAPES = {k: scenes.SMALL_GRID_SHAPES[k][1:] for k in LEVELS}
LR = [0.005, 0.0, 0.005, 0.005, 0.005, 0.0]
LR0 = [0.0] * 6
MASK_KINDS = ["frustum", "ones", "zeros", "single", "half", "upper"]
_cache = {}


def _scene():
    if "sc" not in _cache:
        _cache["sc"] = scenes.make_scene(5, scenes.SMALL_GRID_SHAPES, grid_std=0.05, bias_std=0.1)
    return _cache["sc"]


def _rays(n=320, seed=6):
    key = ("rays", n, seed)
    if key not in _cache:
        _cache[key] = scenes.make_rays(seed, n, _scene()["bound"], n_frames=5 if n >= 100 else 1)
    return _cache[key]


def _masks(kind):
    """a mask per level; "frustum" is built on the device from the last camera of the 320-ray batch (and cached as host arrays)"""
    if kind in _cache:
        return _cache[kind]
    out = {}
    if kind == "frustum":
        r = _rays()
        c2w = r["c2w"][-1]
        H, W = r["HW"]
        fx, fy, cx, cy = r["intr"]
        depth = torch.tensor(scenes.frame_depth_image(_scene()["bound"], c2w, H, W, fx, fy, cx, cy), device="cuda")
        ctx = make_ctx(_scene())
        out = {k: np.asarray(ctx.frustum_mask(k, depth, r["intr"], c2w)).astype(bool).reshape(SHAPES[k]) for k in LEVELS}
        ctx.close()
    for k in (LEVELS if kind != "frustum" else ()):
        Z, Y, X = SHAPES[k]
        m = np.zeros((Z, Y, X), bool)
        if kind == "ones":
            m[:] = True
        elif kind == "single":
            m[Z // 2, Y // 2, X // 2] = True
        elif kind == "half":                  # the plane x = const between voxels: the cells across it have marked and unmarked corners
            m[:, :, : X // 2] = True
        elif kind == "upper":                 # only voxels on the grid's upper faces: reached through tri_setup's clamp alone
            m[-1, :, :] = True; m[:, -1, :] = True; m[:, :, -1] = True
        out[k] = m
    _cache[kind] = out
    return out


def _tensors(r):
    return [cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]


def _new_ctx(stage, masks, tune=(), sort_mode=1, sc=None, **opts):
    ctx = make_ctx(sc or _scene(), trainable=["color"] if stage == "color" else [], **opts)
    for k, v in dict(tune).items():
        ctx.set_tuning(k, v)
    if not dict(tune).get("deterministic"):
        ctx.set_sort_mode(sort_mode)
    for k, m in (masks or {}).items():
        ctx.set_mask(k, m)
    return ctx


def _check_counts(ctx, stage, masks, r, S, frozen, skip=True, want_order=False):
    """the device's liveness bytes and tile counters against numpy on the step's own z values, slot order and the masks: exactly"""
    N = r["rays_o"].shape[0]
    M = N * S
    counts, perm, lb = ctx.debug_live_tiles(M)
    z = ctx.debug_fetch("z", M).reshape(N, S)
    want = lt.sample_bytes(_scene()["bound"], SHAPES, {k: (masks or {}).get(k) for k in frozen + ([] if stage != "color" else ["color"])},
                           lt.sample_points(r["rays_o"], r["rays_d"], z))
    assert sorted(perm.tolist()) == list(range(M))
    skipping = skip and any((masks or {}).get(k) is not None for k in frozen)
    assert counts[3] == (1 if skipping else 0)
    ntiles = (M + 15) // 16
    for k in LEVELS:
        i = LEVELS.index(k)
        if k not in frozen:
            assert counts[i] == -1, (k, counts)
        elif (masks or {}).get(k) is None or not skip:
            assert counts[i] == ntiles, (k, counts)
        else:
            bit = lt.LEVEL_BIT[k]
            assert np.array_equal(lb & bit, want[perm] & bit), k
            assert counts[i] == lt.live_tiles(want[perm], bit), (k, counts, lt.live_tiles(want[perm], bit), ntiles)
    assert counts[7] == ntiles
    return (counts[:4], perm, lb) if want_order else counts[:4]


def _step(stage, masks, r, tune=(), sort_mode=1, check=False, S=48, **opts):
    ctx = _new_ctx(stage, masks, tune, sort_mode, **opts)
    ro, rd, gd, gc = _tensors(r)
    loss = torch.zeros(1, device="cuda")
    ctx.map_step(stage, ro, rd, gd, gc, -1.0, 0.5, stage == "color", flags=3 if stage == "color" else 1, loss=loss)
    ctx.sync()
    frozen = ["middle", "fine"]
    out = dict(loss=float(loss), g={k: ctx.grid_download(k, grad=True) for k in (LEVELS if stage == "color" else frozen)},
               dec=ctx.decoder_download("color", grad=True) if stage == "color" else None)
    if check:
        out["counts"] = _check_counts(ctx, stage, masks, r, S, frozen, skip=not dict(tune).get("no_dead_skip"))
    ctx.close()
    return out


def _same_step(a, b, exact):
    for k in a["g"]:
        if exact:
            assert np.array_equal(a["g"][k], b["g"][k]), k
        else:
            assert rel_l2(a["g"][k], b["g"][k]) < 1e-5, (k, rel_l2(a["g"][k], b["g"][k]))
    if exact:
        assert a["loss"] == b["loss"] and (a["dec"] is None or np.array_equal(a["dec"], b["dec"]))
    else:
        assert abs(a["loss"] - b["loss"]) <= 1e-6 * abs(b["loss"])
        assert a["dec"] is None or rel_l2(a["dec"], b["dec"]) < 1e-5


@pytest.mark.parametrize("stage", ["color", "fine"])
@pytest.mark.parametrize("kind", MASK_KINDS)
def test_marked_gradients_are_unchanged_and_the_counters_are_exact(kind, stage):
    """tests 1 and 4 of the issue: 320 rays x 48 samples of five cameras, colour stage (k_decode_bwd_multi) and fine stage (k_decode_bwd_frozen);
    the downloads (marked voxels; the rest reads as zero) of the skipping and the all-live run agree to the atomic-order bound, in the
    deterministic mode bit for bit, loss and decoder gradient included; the tile counters equal numpy's count on the same z, perm and masks.
    (The skip is off in the deterministic mode -- its waves meet at barriers in every round -- so the deterministic arms run the same code
    twice: they check that the mode stays bit-reproducible and untouched by the liveness machinery around it, not the skip itself.)"""
    masks, r = _masks(kind), _rays()
    skip = _step(stage, masks, r, check=True)
    full = _step(stage, masks, r, tune={"no_dead_skip": 1}, check=True)
    _same_step(skip, full, exact=False)
    ntiles = 320 * 48 // 16
    assert full["counts"][3] == 0 and full["counts"][0] == ntiles and full["counts"][1] == ntiles
    if kind == "zeros":
        assert skip["counts"][0] == 0 and skip["counts"][1] == 0
        assert all(not g.any() for g in skip["g"].values())
        if stage == "color":
            assert np.abs(skip["dec"]).max() > 0
    if kind == "ones":
        assert skip["counts"][0] == ntiles and skip["counts"][1] == ntiles
    if kind in ("frustum", "half", "single", "upper"):
        assert 0 < skip["counts"][1] < ntiles, skip["counts"]          # the case does skip something, and not everything
    det = _step(stage, masks, r, tune={"deterministic": 1})
    det_full = _step(stage, masks, r, tune={"deterministic": 1, "no_dead_skip": 1})
    _same_step(det, det_full, exact=True)
    _same_step(skip, det, exact=False)


def test_no_mask_runs_every_tile():
    r = _rays()
    out = _step("color", None, r, check=True)
    assert out["counts"][3] == 0 and out["counts"][0] == 960 and out["counts"][1] == 960 and out["counts"][2] == -1
    one = _step("color", {"fine": _masks("half")["fine"]}, r, check=True)          # a mask on one level only: the other role is not skipping
    assert one["counts"][3] == 1 and one["counts"][0] == 960 and 0 < one["counts"][1] < 960
    _same_step(one, _step("color", {"fine": _masks("half")["fine"]}, r, tune={"no_dead_skip": 1}), exact=False)


def test_parameters_after_adam_and_a_mask_change():
    """test 2: three optimiser steps under a mask -- marked voxels as in the all-live run, unmarked ones byte-identical to the upload; then another
    mask and one step: the gradients a fresh context with the same parameters and that mask computes (gradient clear, cell_live rebuilt)"""
    sc, r, masks, masks2 = _scene(), _rays(), _masks("frustum"), _masks("half")
    ro, rd, gd, gc = _tensors(r)
    res = {}
    for name, tune in (("skip", {}), ("full", {"no_dead_skip": 1})):
        ctx = _new_ctx("color", masks, tune)
        loss = torch.zeros(1, device="cuda")
        for _ in range(3):
            ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss)
            ctx.adam_step(LR)
        ctx.sync()
        res[name] = ({k: ctx.grid_download(k) for k in LEVELS}, ctx.decoder_download("color"))
        if name == "skip":
            for k, m in masks2.items():
                ctx.set_mask(k, m)
            ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss)
            ctx.sync()
            after = {k: ctx.grid_download(k, grad=True) for k in LEVELS}
            _check_counts(ctx, "color", masks2, r, 48, ["middle", "fine"])
        ctx.close()
    for k in LEVELS:
        up, m = sc["grids"][k], np.broadcast_to(masks[k][None], sc["grids"][k].shape)
        for name in res:
            assert np.array_equal(res[name][0][k][~m].view(np.uint32), up[~m].view(np.uint32)), (name, k)
        if m.any():
            assert rel_l2(res["skip"][0][k][m] - up[m], res["full"][0][k][m] - up[m]) < 5e-3, k
    assert rel_l2(res["skip"][1] - sc["decoders"]["color"], res["full"][1] - sc["decoders"]["color"]) < 5e-3
    sc2 = dict(bound=sc["bound"], grids=dict(sc["grids"], **res["skip"][0]), decoders=dict(sc["decoders"], color=res["skip"][1]))
    ctx = _new_ctx("color", masks2, {"no_dead_skip": 1}, sc=sc2)
    loss = torch.zeros(1, device="cuda")
    ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=3, loss=loss)
    ctx.sync()
    for k in LEVELS:
        assert rel_l2(after[k], ctx.grid_download(k, grad=True)) < 1e-5, k
    ctx.close()


@pytest.mark.parametrize("what", ["track", "ba"])
def test_ray_gradients_are_untouched_by_the_mask(what):
    """test 3: d/dp flows through every sample whatever the voxel mask says -- with NSK_GRAD_RAYS nothing is skipped"""
    r, masks = _rays(200, 8), _masks("single")
    ro, rd, gd, gc = _tensors(r)
    out = {}
    for name, tune in (("skip", {}), ("full", {"no_dead_skip": 1})):
        ctx = _new_ctx("color", masks, tune, sort_mode=1 if what == "ba" else -1)
        if what == "track":
            ctx.decoder_set_trainable("color", False)
        g_ro, g_rd, loss = torch.zeros_like(ro), torch.zeros_like(rd), torch.zeros(1, device="cuda")
        if what == "track":
            ctx.track_step("color", ro, rd, gd, gc, -1.0, 0.5, True, True, True, flags=4, loss=loss, g_rays=(g_ro, g_rd))
        else:
            ctx.map_step("color", ro, rd, gd, gc, -1.0, 0.5, True, flags=7, loss=loss, g_rays=(g_ro, g_rd))
        ctx.sync()
        counts, _, _ = ctx.debug_live_tiles(200 * 48)
        assert counts[3] == 0 and counts[0] == 600 and counts[1] == 600 and counts[2] == (600 if what == "track" else -1), counts
        out[name] = (float(loss), g_ro.cpu().numpy(), g_rd.cpu().numpy())
        ctx.close()
    assert np.abs(out["full"][1]).max() > 0 and np.abs(out["full"][2]).max() > 0
    assert out["skip"][0] == out["full"][0]
    assert rel_l2(out["skip"][1], out["full"][1]) < 1e-6 and rel_l2(out["skip"][2], out["full"][2]) < 1e-6


@pytest.mark.parametrize("path", ["prepared", "unprepared", "ray-order", "dropped", "render-between", "graph", "graph-ray-order"])
def test_every_path_that_feeds_the_bytes(path):
    """test 5: however the batch's sampling came about -- riding in the previous step's launches, on its own, in ray order, after another
    registration was dropped, with a render in between, recorded in a graph -- its step gives the all-live step's gradients and exact counters.

    A replayed graph's counter over three launches: every launch's counts equal numpy's for that launch's own slot order, exactly -- nothing is
    carried from one launch to the next -- and whenever two launches have the same slot order their counts are equal.  In ray order the slot
    order is fixed, so there the three counts ARE equal.  In cell order they need not be: k_sort_scan places its 256-cell chunks in the order its
    workgroups arrive (one returning add on a cursor; nsk_device.h), so the same samples sit at other slots from launch to launch, the 16-slot
    tile boundaries fall elsewhere in the cells, and the number of tiles holding a live sample moves with them (measured on this case, 14 runs of
    three launches: 681 / 540 tiles in most launches, 678 / 537 in some; an assertion of plain equality failed 3 runs of 14).  What is equal
    from launch to launch in cell order is what does not depend on the order: the samples' bytes."""
    masks, A, B, C = _masks("frustum"), _rays(), _rays(320, 16), _rays(320, 26)
    ray_order = path.endswith("ray-order")
    ref = _step("color", masks, A, tune={"no_dead_skip": 1}, sort_mode=0 if ray_order else 1)
    ctx = _new_ctx("color", masks, sort_mode=0 if ray_order else 1)
    tA, tB, tC = _tensors(A), _tensors(B), _tensors(C)
    loss = torch.zeros(1, device="cuda")
    step = lambda t: ctx.map_step("color", t[0], t[1], t[2], t[3], -1.0, 0.5, True, flags=3, loss=loss)
    prep = lambda t: ctx.map_prepare("color", t[0], t[1], t[2], -1.0, flags=3)
    frozen = ["middle", "fine"]
    with torch.cuda.stream(ctx.tstream):
        if path in ("prepared", "render-between"):
            prep(tA); step(tB)
            if path == "render-between":
                ctx.render_forward("color", tC[0], tC[1], tC[2], -1.0)
            ctx.adam_step(LR0)
        elif path == "dropped":
            prep(tC); step(tB); prep(tA); step(tB); ctx.adam_step(LR0)
        ctx.zero_grads()
        if path.startswith("graph"):
            step(tA); ctx.zero_grads()
            ctx.graph_begin(); step(tA); gid = ctx.graph_end()
            seen = []
            for _ in range(3):
                ctx.zero_grads()
                ctx.graph_launch(gid)
                seen.append(_check_counts(ctx, "color", masks, A, 48, frozen, want_order=True))        # exact for this launch's own order
            for c, perm, lb in seen[1:]:
                by_sample = np.empty_like(lb); by_sample[perm] = lb
                first = np.empty_like(seen[0][2]); first[seen[0][1]] = seen[0][2]
                assert np.array_equal(by_sample, first)                                                  # the same byte for every sample
                if np.array_equal(perm, seen[0][1]):
                    assert c.tolist() == seen[0][0].tolist(), (c, seen[0][0])
            if ray_order:
                assert all(np.array_equal(perm, np.arange(320 * 48)) for _, perm, _ in seen)
                assert seen[0][0].tolist() == seen[1][0].tolist() == seen[2][0].tolist(), [c.tolist() for c, _, _ in seen]
        else:
            step(tA)
    ctx.sync()
    _check_counts(ctx, "color", masks, A, 48, frozen)
    # (a replayed graph leaves the decoder's gradient in the per-workgroup slabs for its own Adam node: only an eager step's is read back here)
    got = dict(loss=float(loss), g={k: ctx.grid_download(k, grad=True) for k in LEVELS}, dec=None if path.startswith("graph") else ctx.decoder_download("color", grad=True))
    ctx.close()
    _same_step(got, ref, exact=False)


@pytest.mark.parametrize("n_rays,n_samples,n_surface", [(203, 32, 16), (17, 8, 8), (17, 8, 5)])
@pytest.mark.parametrize("stage", ["color", "fine"])
def test_ragged_sizes(stage, n_rays, n_samples, n_surface):
    """test 6: sample counts that are no multiple of the workgroup's 128 samples, and (17 x 13) of the 16-sample tile: the padding lanes of the last
    tile repeat the last slot, and must neither make a dead tile live nor hide a live sample -- the counters stay exact"""
    S = n_samples + n_surface
    r = _rays(n_rays, 40 + n_rays + S)
    for kind in ("half", "single"):
        masks = _masks(kind)
        opts = dict(n_samples=n_samples, n_surface=n_surface)
        skip = _step(stage, masks, r, check=True, S=S, **opts)
        full = _step(stage, masks, r, tune={"no_dead_skip": 1}, **opts)
        _same_step(skip, full, exact=False)

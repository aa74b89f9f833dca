"""GPU tests (-m gpu) of the optimiser launch, element by element (tests/adam_checks.py: reference, derived bound, planted gradients).

nsk_grad_slab hands out the device gradient slab after completing the pending slab sum, and the slab is writable: a test that overwrites it
decides exactly what k_adam_multi reads.  Every parameter is then compared with the fp64 reference under the running bound; nothing is
measured here but the printed error / bound ratios.  The derived images of a trainable decoder (what the MFMA kernels read) are compared
byte for byte with what an upload of the same parameters builds (nsk_debug_decoder_images).

Shapes: 45, 315, 2431 and 1147 voxels -- no multiple of 1024, two levels above 1024, the colour level one voxel thin; 16 rays."""
import numpy as np
import pytest
import torch

import adam_checks as ac
import scenes
from gpu_util import cu

pytestmark = pytest.mark.gpu
LEVELS = ("coarse", "middle", "fine", "color")
SHAPES = {"coarse": (3, 3, 5), "middle": (5, 7, 9), "fine": (11, 13, 17), "color": (1, 37, 31)}      # Z, Y, X
NVOX = {k: int(np.prod(SHAPES[k])) for k in LEVELS}
DEC_N = {k: scenes.decoder_param_count(k) for k in LEVELS}
DEC_N4 = {k: (DEC_N[k] + 3) & ~3 for k in LEVELS}
TRAIN_SETS = {"color": ("color",), "middle": ("middle",), "fine": ("fine",), "mfc": ("middle", "fine", "color"), "all8": LEVELS}
_cache = {}


def _scene():
    if "sc" not in _cache:
        sc = scenes.make_scene(3, {k: (32,) + SHAPES[k] for k in LEVELS}, grid_std=0.05, bias_std=0.1)
        # the compositing takes relu(sigma): with the seeded output bias the coarse decoder's sigma is negative at every sample of the 16 rays and
        # a coarse step leaves no gradient at all -- a positive output bias (the packed vector's last float) lets the real steps of (d) train it
        sc["decoders"]["coarse"][-1] = 0.5
        _cache["sc"] = sc
    return _cache["sc"]


def _rays():
    if "rays" not in _cache:
        r = scenes.make_rays(7, 16, _scene()["bound"])
        _cache["rays"] = [cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]
    return _cache["rays"]


def _seq(name, n, steps, seed, nonfinite=True):
    key = ("seq", name, n, steps, seed, nonfinite)
    if key not in _cache:
        _cache[key] = ac.planted(n, steps=steps, seed=seed, nonfinite=nonfinite)
    return _cache[key]


def _offsets():
    """the gradient slab: the four levels voxel-major, the four decoders padded to whole float4, four loss floats (include/nsk.h)"""
    off, n = {}, 0
    for k in LEVELS:
        off["grid", k] = n
        n += NVOX[k] * 32
    for k in LEVELS:
        off["dec", k] = n
        n += DEC_N4[k]
    return off, n + 4


def _czyx(flat, level):
    Z, Y, X = SHAPES[level]
    return np.ascontiguousarray(np.asarray(flat).reshape(Z, Y, X, 32).transpose(3, 0, 1, 2))


def _flat(czyx):
    return np.ascontiguousarray(np.asarray(czyx).reshape(32, -1).T).ravel()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ctx(grids=None, decoders=None, trainable=(), mode=None):
    import nice_slam_cpp_amd as pkg
    sc = _scene()
    ctx = pkg.Context(0)
    ctx.set_render_opts(n_samples=8, n_surface=4)
    if mode is not None:
        ctx.set_matmul_mode(mode)
    ctx.load_scene(sc["bound"], dict(sc["grids"], **(grids or {})), dict(sc["decoders"], **(decoders or {})))
    for k in trainable:
        ctx.decoder_set_trainable(k, True)
    return ctx


def _touch(ctx, stages, flags=3):
    """small steps that leave gradients (and the groups touched): no optimiser step in between"""
    ro, rd, gd, gc = _rays()
    loss = torch.zeros(1, device="cuda")
    for st in stages:
        ctx.map_step(st, ro, rd, gd, gc, -1.0, 0.5, True, flags=flags, loss=loss)


def _plant(slab, off, values):
    slab[off:off + values.size].copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(slab.device))


def _read(slab, off, n):
    return slab[off:off + n].cpu().numpy()


def _report(name, ratios):
    print("adam error/bound %s: %.3f" % (name, max(ratios) if ratios else 0.0))


# ---- a. planted steps on the grids, under every mask case -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["none", "all", "empty", "first", "last", "33", "half"])
def test_planted_grid_steps(case):
    """four planted steps under the mask, then one with the mask removed: every parameter inside the bound, unmarked voxels byte-identical
    while unmarked and stepping from zero moments at the level's step count once marked, the slab zero where it was read"""
    off, total = _offsets()
    seqs = {k: _seq("grid", NVOX[k] * 32, 5, 11 + i) for i, k in enumerate(LEVELS)}
    masks = {k: ac.voxel_masks(NVOX[k], 21 + i)[case] for i, k in enumerate(LEVELS)}
    ctx = _ctx(grids={k: _czyx(seqs[k]["p0"], k) for k in LEVELS})
    for k in LEVELS:
        if masks[k] is not None:
            ctx.set_mask(k, masks[k])
    track = {k: ac.AdamTrack(seqs[k]["p0"]) for k in LEVELS}
    ratios, compared = [], 0
    for t in range(5):
        if t == 4:
            for k in LEVELS:
                if masks[k] is not None:
                    ctx.set_mask(k, None)
            masks = {k: None for k in LEVELS}
        _touch(ctx, ["coarse", "color"])
        slab = ctx.grad_slab()
        assert slab.numel() == total
        want = {}
        for i, k in enumerate(LEVELS):
            g = seqs[k]["g"][t].copy()
            on = ac.voxels_to_floats(masks[k])
            if on is not None:
                g[~on] = ac.garbage(g.size, 31 + 7 * t + i)[~on]
            _plant(slab, off["grid", k], g)
            want[k] = g if on is None else np.where(on, g, np.float32(0))
        for k in LEVELS:          # the layout: a gradient download sees what was planted (zeros where the mask discards it)
            assert np.array_equal(_bits(_flat(ctx.grid_download(k, grad=True))), _bits(want[k])), (k, t)
        lr = seqs["coarse"]["lr"][t]
        ctx.adam_step([lr] * 6)
        ctx.sync()
        for k in LEVELS:
            on = ac.voxels_to_floats(masks[k])
            p = _flat(ctx.grid_download(k))
            track[k].step(seqs[k]["g"][t], lr, t + 1, mask=on)
            assert not track[k].near_range_edge().any()
            r = track[k].compare(p)
            assert r["excluded"] == 0 and r["nonfinite_ok"] and r["ratio"] <= 1.0, (k, t, r)
            assert r["nonfinite"] == (int((~np.isfinite(seqs[k]["g"][4])).sum()) if t == 4 else 0), (k, t, r)
            ratios.append(r["ratio"])
            compared += r["compared"]
            after = _read(slab, off["grid", k], p.size)
            if on is None:
                assert not after.any(), (k, t)
            else:
                assert not after[on].any(), (k, t)
                assert np.array_equal(_bits(p[~on]), _bits(seqs[k]["p0"][~on])), (k, t)       # never marked so far: the upload's bytes
            zero = (seqs[k]["kind"] == 8) | (seqs[k]["kind"] == 9)
            assert np.array_equal(_bits(p[zero]), _bits(seqs[k]["p0"][zero])), (k, t)
    ctx.close()
    assert compared > 0
    _report("grids, mask %s" % case, ratios)


# ---- b. per-group step counts ------------------------------------------------------------------------------------------------------------------
def test_groups_keep_their_own_step_counts():
    """steps that touch different levels: every level follows the reference with its own count, an untouched level keeps its bytes;
    nsk_adam_reset restarts all of them from zero moments and count 0"""
    off, _ = _offsets()
    seqs = {k: _seq("grid", NVOX[k] * 32, 5, 41 + i, False) for i, k in enumerate(LEVELS)}
    ctx = _ctx(grids={k: _czyx(seqs[k]["p0"], k) for k in LEVELS})
    track = {k: ac.AdamTrack(seqs[k]["p0"]) for k in LEVELS}
    count = {k: 0 for k in LEVELS}
    used = {k: 0 for k in LEVELS}
    plan = [(["middle"], ["middle"]), (["color"], ["middle", "fine", "color"]), (["coarse", "fine"], ["coarse", "middle", "fine"]),
            "reset", (["coarse", "color"], list(LEVELS)), (["middle"], ["middle"])]
    ratios = []
    for j, item in enumerate(plan):
        if item == "reset":
            ctx.adam_reset()
            for k in LEVELS:
                track[k].reset()
                count[k] = 0
            continue
        stages, touched = item
        before = {k: _flat(ctx.grid_download(k)) for k in LEVELS}
        _touch(ctx, stages)
        slab = ctx.grad_slab()
        for k in touched:
            _plant(slab, off["grid", k], seqs[k]["g"][used[k]])
        lr = ac.LRS[j % len(ac.LRS)]
        ctx.adam_step([lr] * 6)
        ctx.sync()
        for k in LEVELS:
            p = _flat(ctx.grid_download(k))
            if k not in touched:
                assert np.array_equal(_bits(p), _bits(before[k])), (k, j)
                continue
            count[k] += 1
            track[k].step(seqs[k]["g"][used[k]], lr, count[k])
            used[k] += 1
            r = track[k].compare(p)
            assert r["excluded"] == 0 and r["nonfinite"] == 0 and r["ratio"] <= 1.0, (k, j, count[k], r)
            ratios.append(r["ratio"])
    ctx.close()
    assert count == {"coarse": 1, "middle": 2, "fine": 1, "color": 1} and used["middle"] == 5
    _report("per-group counts", ratios)


# ---- c. trainable decoders, planted ----------------------------------------------------------------------------------------------------------
def _touch_stages(train):
    return (["coarse"] if "coarse" in train else []) + ["color"]


@pytest.mark.parametrize("name", list(TRAIN_SETS))
def test_planted_decoder_steps(name):
    """the planted procedure on the trainable decoders (15899 and 6337 parameters are no multiple of 4); "all8": four levels and four decoders,
    the eight segments one launch can carry.  Frozen decoders keep their bytes whatever their part of the slab holds."""
    train = TRAIN_SETS[name]
    off, _ = _offsets()
    sc = _scene()
    with_grids = name == "all8"
    dseq = {k: _seq("dec", DEC_N4[k], 4, 51 + i) for i, k in enumerate(train)}
    gseq = {k: _seq("grid", NVOX[k] * 32, 5, 11 + i, False) for i, k in enumerate(LEVELS)} if with_grids else {}
    ctx = _ctx(grids={k: _czyx(gseq[k]["p0"], k) for k in gseq}, trainable=train)
    dtrack = {}
    for k in train:
        p0 = np.zeros(DEC_N4[k], np.float32)
        p0[:DEC_N[k]] = sc["decoders"][k]
        dtrack[k] = ac.AdamTrack(p0)
    gtrack = {k: ac.AdamTrack(gseq[k]["p0"]) for k in gseq}
    ratios = []
    for t in range(4):
        _touch(ctx, _touch_stages(train), flags=3 if with_grids else 2)
        slab = ctx.grad_slab()
        for i, k in enumerate(LEVELS):
            _plant(slab, off["dec", k], dseq[k]["g"][t] if k in train else ac.garbage(DEC_N4[k], 61 + i + 5 * t))
        for k in gseq:
            _plant(slab, off["grid", k], gseq[k]["g"][t])
        for k in train:
            assert np.array_equal(_bits(ctx.decoder_download(k, grad=True)), _bits(dseq[k]["g"][t][:DEC_N[k]])), (k, t)
        lr = ac.LRS[t]
        ctx.adam_step([lr] * 6)
        ctx.sync()
        for k in LEVELS:
            p = ctx.decoder_download(k)
            if k not in train:
                assert np.array_equal(_bits(p), _bits(sc["decoders"][k])), (k, t)
                continue
            dtrack[k].step(dseq[k]["g"][t], lr, t + 1)
            assert not dtrack[k].near_range_edge().any()
            pad = np.zeros(DEC_N4[k], np.float32)
            pad[:DEC_N[k]] = p
            real = np.arange(DEC_N4[k]) < DEC_N[k]
            r = dtrack[k].compare(pad, sel=real)
            assert r["excluded"] == 0 and r["nonfinite_ok"] and r["ratio"] <= 1.0, (k, t, r)
            assert r["compared"] + r["nonfinite"] == DEC_N[k]
            assert r["nonfinite"] == (int((~np.isfinite(dseq[k]["g"][3][:DEC_N[k]])).sum()) if t == 3 else 0), (k, t, r)
            ratios.append(r["ratio"])
            assert not _read(slab, off["dec", k], DEC_N[k]).any(), (k, t)
        for k in gseq:
            gtrack[k].step(gseq[k]["g"][t], lr, t + 1)
            r = gtrack[k].compare(_flat(ctx.grid_download(k)))
            assert r["excluded"] == 0 and r["nonfinite"] == 0 and r["ratio"] <= 1.0, (k, t, r)
            ratios.append(r["ratio"])
    ctx.close()
    _report("decoders %s" % name, ratios)


# ---- d. the images follow the parameters ------------------------------------------------------------------------------------------------------
def _images(ctx, train):
    return {(k, w): ctx.debug_decoder_images(k, w) for k in train for w in ctx.DECODER_IMAGES}


def _outputs(ctx):
    ro, rd, gd, _ = _rays()
    rgb, depth, var, w = ctx.render_forward("color", ro, rd, gd)
    pts = ro + rd * gd.clamp(min=0.5)[:, None]
    raw = ctx.eval_points("color", pts.contiguous())
    ctx.sync()
    return [x.cpu().numpy() for x in (rgb, depth, var, w, raw)]


@pytest.mark.parametrize("name", list(TRAIN_SETS))
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_images_follow_the_parameters(mode, name):
    """after three real steps the four device images of every trainable decoder are, byte for byte, what an upload of the downloaded parameters
    builds in a fresh context -- with the decoder gradient still in per-workgroup slabs when the optimiser runs (single trainable decoder)
    and with it flushed first; a matmul-mode round trip, which rebuilds the forward images, changes no byte"""
    train = TRAIN_SETS[name]
    fresh = _ctx(trainable=train, mode=mode)
    img_0 = _images(fresh, train)
    fresh.close()
    for flushed in (False, True):
        A = _ctx(trainable=train, mode=mode)
        for _ in range(3):
            _touch(A, _touch_stages(train))
            if flushed:
                A.grad_slab()
            A.adam_step([1e-3] * 6)
        A.sync()
        img_a = _images(A, train)
        grids = {k: A.grid_download(k) for k in LEVELS}
        decs = {k: A.decoder_download(k) for k in LEVELS}
        assert all((decs[k] != _scene()["decoders"][k]).any() for k in train)
        assert all(np.isfinite(decs[k]).all() for k in train)
        B = _ctx(grids=grids, decoders=decs, trainable=train, mode=mode)
        img_b = _images(B, train)
        for key in img_a:
            assert img_a[key].size == img_b[key].size and (img_a[key].size > 0 or key[0] == "coarse"), key
            diff = np.flatnonzero(img_a[key] != img_b[key])
            assert diff.size == 0, (key, flushed, diff.size, diff[:8] // 4)
            assert img_a[key].size == 0 or (img_a[key] != img_0[key]).mean() > 0.05, key     # the read-back sees images that moved
        for a, b in zip(_outputs(A), _outputs(B)):
            assert np.array_equal(_bits(a), _bits(b)), flushed
        A.set_matmul_mode(0 if mode == 2 else 2)
        A.set_matmul_mode(mode)
        again = _images(A, train)
        for key in img_a:
            assert np.array_equal(img_a[key], again[key]), (key, flushed)
        A.close()
        B.close()


# ---- e. nsk_adam_vector ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 255, 256, 257, 1000])
def test_adam_vector_single_steps(n):
    """the caller owns p, g, m and v: one step at a time from planted moments, p, m and v each inside the single-step bound"""
    ctx = _ctx()
    ratios = []
    for j, step in enumerate((1, 2, 1000, 100000)):
        st = ac.planted_state(n, 71 + j)
        g, p0, m0, v0 = st["g"], st["p0"], st["m0"], st["v0"]
        lr = ac.LRS[j]
        p, m, v = cu(p0), cu(m0), cu(v0)
        ctx.adam_vector(p, cu(g), m, v, lr, step)
        ctx.sync()
        tr = ac.AdamTrack(p0)
        tr.set_moments(m0, v0)
        tr.step(g, lr, step)
        assert not tr.near_range_edge().any()
        for what, dev in (("p", p), ("m", m), ("v", v)):
            r = tr.compare(dev.cpu().numpy(), what=what)
            assert r["excluded"] == 0 and r["nonfinite_ok"] and r["ratio"] <= 1.0, (n, step, what, r)
            assert r["compared"] + r["nonfinite"] == n
            ratios.append(r["ratio"])
    ctx.close()
    _report("adam_vector n=%d" % n, ratios)

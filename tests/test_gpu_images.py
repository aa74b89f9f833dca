"""GPU tests (-m gpu) of the decoder images against a specification: every image read through nsk_debug_decoder_images is, byte for byte, what
numpy builds from the downloaded parameters and the index table of nsk_decoder_image_table by the rules of include/nsk.h, restated here:

- entry t of a table holds parameter idx[t], or zero for -1; the fp32 images (0, 1) are that gather;
- images 2 and 3 keep np 16-bit pieces per entry: piece p of entry t = fg * 512 + lane * 8 + j is unsigned short ((fg * np + p) * 64 + lane) * 8 + j;
- np = 2: high = fp16(x), low = fp16((x - high) * 2048); np = 3: three successive bf16 pieces of x and of what the earlier ones left; every
  conversion rounds to nearest even, fp16 results below the smallest normal stay subnormals (numpy's float16 conversion does the same);
- the tail is the last tail_n floats of the fp32 sibling (740 after image 2, 416 after image 3).
Image 2 has 2 pieces under matmul mode 2 and 3 under modes 0 and 1; image 3 always 2.

No rendering: decoders of the scene tests/test_gpu_adam.py uses, uploaded into one small context per test.  The second parameter set spreads
magnitudes over 2^-30 .. 2^4 so that high and low pieces reach fp16's subnormal range and zero."""
import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu
LEVELS = ("coarse", "middle", "fine", "color")
SHAPES = {"coarse": (3, 3, 5), "middle": (5, 7, 9), "fine": (11, 13, 17), "color": (1, 37, 31)}
TAIL_N = {2: 740, 3: 416}
_cache = {}


def _params(which):
    """A: the scene's decoders.  B: other values, magnitudes spread over 34 octaves, some exact zeros and negative zeros"""
    if "A" not in _cache:
        sc = scenes.make_scene(3, {k: (32,) + SHAPES[k] for k in LEVELS}, grid_std=0.05, bias_std=0.1)
        _cache["A"] = {k: np.asarray(sc["decoders"][k], np.float32).copy() for k in LEVELS}
        rng = np.random.default_rng(5)
        B = {}
        for k in LEVELS:
            n = _cache["A"][k].size
            b = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 5, n))).astype(np.float32)
            b[rng.integers(0, n, 40)] = 0.0
            b[rng.integers(0, n, 40)] = -0.0
            B[k] = b
        _cache["B"] = B
    return _cache[which]


def _ctx(mode, params):
    import nice_slam_cpp_amd as pkg
    ctx = pkg.Context(0)
    ctx.set_matmul_mode(mode)
    for k in LEVELS:
        ctx.decoder_upload(k, params[k])
    return ctx


def _bf16(x):
    """round to nearest even to 8 significant bits: (the 16 bits, their value as float32); finite inputs"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    h = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return h.astype(np.uint16), (h << 16).astype(np.uint32).view(np.float32)


def _pieces(x, n_pieces):
    x = np.ascontiguousarray(x, np.float32)
    if n_pieces == 2:
        h = x.astype(np.float16)
        low = ((x - h.astype(np.float32)) * np.float32(2048)).astype(np.float16)
        return [h.view(np.uint16), low.view(np.uint16)]
    h, hf = _bf16(x)
    r1 = x - hf
    m, mf = _bf16(r1)
    low, _ = _bf16(r1 - mf)
    return [h, m, low]


def _expected(P, which, what, pieces):
    """the bytes of image `what` of decoder `which` holding parameters P"""
    import nice_slam_cpp_amd as pkg
    idx = pkg.nsk.decoder_image_table(which, what, pieces)
    if idx.size == 0:
        return np.zeros(0, np.uint8)
    vals = np.where(idx >= 0, P[np.maximum(idx, 0)], np.float32(0)).astype(np.float32)
    if what < 2:
        return vals.view(np.uint8)
    n_pieces = pieces if what == 2 else 2
    frag = np.stack([p.reshape(-1, 512) for p in _pieces(vals, n_pieces)], axis=1)          # [fragment group, piece, lane * 8 + j]
    tail = _expected(P, which, what - 2, pieces)[-4 * TAIL_N[what]:]
    return np.concatenate([np.ascontiguousarray(frag, "<u2").reshape(-1).view(np.uint8), tail])


def _check(ctx, which, what, pieces, P=None):
    P = ctx.decoder_download(which) if P is None else P
    got, want = ctx.debug_decoder_images(which, what), _expected(P, which, what, pieces)
    assert got.size == want.size, (which, what, got.size, want.size)
    assert got.size > 0 or (which == "coarse" and what >= 2)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (which, what, diff.size, diff[:8])
    return got


@pytest.mark.parametrize("which", LEVELS)
@pytest.mark.parametrize("mode", [2, 1, 0])
def test_fresh_upload_builds_the_specified_images(mode, which):
    for name in ("A", "B"):
        ctx = _ctx(mode, _params(name))
        P = ctx.decoder_download(which)
        assert np.array_equal(P.view(np.uint32), _params(name)[which].view(np.uint32))
        for what in range(4):
            _check(ctx, which, what, 2 if mode == 2 else 3)
        ctx.close()


def test_the_second_parameter_set_reaches_the_subnormal_pieces():
    """what the comparison above covered: fp16 high and low pieces that are subnormal, and ones that are zero beside a nonzero value"""
    x = _params("B")["middle"]
    h, low = (p.view(np.float16) for p in _pieces(x, 2))
    sub = lambda p: (np.abs(p) < np.float16(2.0 ** -14)) & (p != 0)
    assert sub(h).sum() > 100 and sub(low).sum() > 100 and ((h == 0) & (x != 0)).sum() > 100


@pytest.mark.parametrize("which", ["middle", "fine", "color"])
def test_a_second_upload_rebuilds_the_lazy_image(which):
    """image 3 is built when first read; an upload must mark it stale again"""
    A, B = _params("A"), _params("B")
    ctx = _ctx(2, A)
    first = _check(ctx, which, 3, 2, A[which])
    ctx.decoder_upload(which, B[which])
    second = _check(ctx, which, 3, 2, B[which])
    assert (first != second).mean() > 0.05
    for what in range(3):
        _check(ctx, which, what, 2, B[which])
    ctx.close()


def test_a_matmul_mode_round_trip_restores_the_forward_image():
    ctx = _ctx(2, _params("A"))
    before = {k: _check(ctx, k, 2, 2) for k in LEVELS}
    ctx.set_matmul_mode(1)
    for k in LEVELS[1:]:
        three = _check(ctx, k, 2, 3)
        assert three.size == (before[k].size - 4 * TAIL_N[2]) * 3 // 2 + 4 * TAIL_N[2]
    ctx.set_matmul_mode(2)
    for k in LEVELS:
        assert np.array_equal(ctx.debug_decoder_images(k, 2), before[k]), k
    ctx.close()

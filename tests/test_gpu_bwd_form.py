"""GPU tests (-m gpu): which backward launch a step sends out (csrc/nsk_split.h: bwd_form, bwd_deal_role, bwd_grid, median_form) is what the
build before that decision had one home sent out.  A table of cases crosses stage, gradient flags, trainable decoders, backward mode, the
deterministic mode, the tuning keys that change the form (no_frozen_kernel, static_deal, no_dead_skip, no_fused_median, no_deferred_median),
an optimiser mask and, for Tracker steps, handle_dynamic.  Every case takes a fresh context, runs ONE step and nsk_sync, and compares all
16 integers of nsk_debug_last_split(dir = 1) and the bits of the step's loss with tests/golden/bwd_launch_records.txt.  One step per context:
the first step of a kind assumes every tile runs, so the record does not depend on when liveness counts arrive.

The golden file was recorded from the parent build, never from the tree under test (its first line names the commit):

    NSK_LIB=<the parent's libnsk.so> python tests/test_gpu_bwd_form.py --record <commit> <output file>

The records hold workgroup counts, so they are those of a 256-CU device.  A step the library refuses is recorded with its error text.

Shapes: 64 and 200 rays x 16 samples on the suite's toy grids, and one case each at the smallest sizes on either side of two thresholds:
  deal_min_rounds       colour stage, colour decoder trainable, masks on every level: 6072 / 6073 tiles.  At 6073 the planner gives the frozen
                        roles 33 workgroups each, 24 rounds of 8 waves (the default deal_min_rounds); at 6072, 23 rounds.  The record has no field
                        for dealing (both are form "multi"): the case shows that either launch goes out and sums the same loss.
  (N + 3) / 4 <= CUs    Tracker steps at 1024 / 1025 rays, with and without no_deferred_median: the deferred and the barrier form reach to 1024.
                        The record tells the deferred form from the others (form "track", median_wg 1); it cannot tell the barrier form from
                        the three-launch form (same record, same loss bits), and on 256 CUs this threshold coincides with the 1024-ray cap.
What the record cannot show on either threshold, a >= turned into a > in bwd_deal_role or a barrier beyond one workgroup per CU, is held by
host/test/split_test.cpp's form_sweep (tests/test_split_cpu.py), which enumerates both sides of both on 50 and 256 CUs."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwd_launch_records.txt")
STAGE_DECODERS = {"coarse": ["coarse"], "middle": ["middle"], "fine": ["middle", "fine"], "color": ["middle", "fine", "color"]}
MASK_LEVELS = ("middle", "fine", "color")
pytestmark = pytest.mark.gpu


def _case(kind, stage, flags, trainable=(), bmode=2, det=0, tune=(), mask=0, hd=1, n=64):
    return dict(kind=kind, stage=stage, flags=flags, trainable=tuple(trainable), bmode=bmode, det=det, tune=tuple(tune), mask=mask, hd=hd, n=n)


def _name(c):
    return "%s %s flags=%d train=%s bmode=%d det=%d tune=%s mask=%d hd=%d n=%d" % (
        c["kind"], c["stage"], c["flags"], "+".join(c["trainable"]) or "-", c["bmode"], c["det"], "+".join(c["tune"]) or "-", c["mask"], c["hd"], c["n"])


def _groups():
    """group name -> cases.  flags: 1 grids, 3 grids + decoders, 5 grids + rays, 7 all three (a Tracker step also runs 4 and 6: no grids)"""
    g = {"map": [], "map-knobs": [], "track": [], "track-knobs": [], "edges": []}
    for stage, decs in STAGE_DECODERS.items():
        # none trainable; the stage's last decoder (the one trainable role, or the fine decoder: separate launches); every decoder of the stage
        subsets = [(), (decs[-1],)] + ([tuple(decs)] if len(decs) > 1 else []) + ([("middle",)] if stage == "color" else [])
        modes = ((2, 0), (0, 0), (2, 1))            # (backward mode, deterministic)
        g["map"].append(_case("map", stage, 2))         # decoder gradients alone, none trainable: nothing to do
        g["track"].append(_case("track", stage, 2))
        for flags in (1, 3, 5, 7):
            for trainable in subsets:
                for bmode, det in modes:
                    g["map"].append(_case("map", stage, flags, trainable, bmode, det))
        for flags in (4, 5, 6, 7, 1):
            for trainable in subsets[:2]:
                for bmode, det in modes:
                    g["track"].append(_case("track", stage, flags, trainable, bmode, det))
                g["track"].append(_case("track", stage, flags, trainable, hd=0))
    for stage in ("fine", "color"):
        trainable = ("color",) if stage == "color" else ()
        for flags in (1, 3):
            for n in (64, 200):
                for mask in (0, 1):
                    for tune in ((), ("no_frozen_kernel",), ("static_deal",), ("no_dead_skip",), ("no_frozen_kernel", "static_deal")):
                        g["map-knobs"].append(_case("map", stage, flags, trainable, tune=tune, mask=mask, n=n))
        for flags in (4, 6):
            for tr in sorted({(), trainable}):
                for n in (64, 200):
                    for tune in ((), ("no_fused_median",), ("no_deferred_median",), ("no_fused_median", "no_deferred_median"), ("no_frozen_kernel",)):
                        g["track-knobs"].append(_case("track", stage, flags, tr, tune=tune, n=n, mask=1 if stage == "fine" else 0))
    for k in ("map-knobs", "track-knobs"):            # (a case without knob, mask or larger batch is in the first two groups already)
        g[k] = [c for c in g[k] if c["tune"] or c["mask"] or c["n"] != 64]
    for n in (6072, 6073):
        g["edges"].append(_case("map", "color", 3, ("color",), mask=1, n=n))
        g["edges"].append(_case("map", "color", 3, ("color",), mask=1, n=n, tune=("static_deal",)))
    for n in (1024, 1025):
        for tune in ((), ("no_deferred_median",)):
            g["edges"].append(_case("track", "color", 4, tune=tune, n=n))
    return g


GROUPS = _groups()
_cache = {}


def _inputs(n):
    import scenes
    from gpu_util import cu
    if "sc" not in _cache:
        _cache["sc"] = scenes.make_scene(5, scenes.SMALL_GRID_SHAPES, grid_std=0.05, bias_std=0.1)
    if n not in _cache:
        r = scenes.make_rays(6, n, _cache["sc"]["bound"], n_frames=1, zero_frac=0.1)
        _cache[n] = [cu(r[k]) for k in ("rays_o", "rays_d", "gt_depth", "gt_color")]
    return _cache["sc"], _cache[n]


def _masks(sc):
    """the plane x = const between voxels on every level (test_gpu_dead_skip.py's "half")"""
    import scenes
    out = {}
    for k in MASK_LEVELS:
        m = np.zeros(scenes.SMALL_GRID_SHAPES[k][1:], bool)
        m[:, :, : m.shape[2] // 2] = True
        out[k] = m
    return out


def run_case(c):
    """one step on a fresh context -> "i0 .. i15 | loss bits", or the library's error text"""
    import torch
    import nice_slam_cpp_amd as pkg
    from gpu_util import make_ctx
    sc, (ro, rd, gd, gc) = _inputs(c["n"])
    ctx = make_ctx(sc, n_samples=8, n_surface=8, trainable=c["trainable"])
    try:
        ctx.set_backward_mode(c["bmode"])
        if c["det"]:
            ctx.set_tuning("deterministic", 1)
        for k in c["tune"]:
            ctx.set_tuning(k, 1)
        if c["mask"]:
            for k, m in _masks(sc).items():
                ctx.set_mask(k, m)
        loss = torch.zeros(1, device="cuda")
        g_rays = (torch.empty_like(ro), torch.empty_like(rd)) if c["flags"] & 4 else None
        try:
            if c["kind"] == "map":
                ctx.map_step(c["stage"], ro, rd, gd, gc, -1.0, 0.5, c["stage"] == "color", flags=c["flags"], loss=loss, g_rays=g_rays)
            else:
                ctx.track_step(c["stage"], ro, rd, gd, gc, -1.0, 0.5, c["stage"] == "color", bool(c["hd"]), True, flags=c["flags"], loss=loss, g_rays=g_rays)
            ctx.sync()
        except pkg.NskError as e:
            return "error: %s" % " ".join(str(e).split())
        import ctypes as C
        h = (C.c_int * 16)()
        assert pkg.nsk.lib().nsk_debug_last_split(ctx.h, 1, h) == 0
        return "%s | %08x" % (" ".join(str(int(x)) for x in h), int(loss.cpu().numpy().view(np.uint32)[0]))
    finally:
        ctx.close()


def _golden():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            lines = [ln.rstrip("\n") for ln in f]
        assert lines[0].startswith("# recorded from commit "), lines[0]
        _cache["golden"] = dict(ln.split(" : ", 1) for ln in lines if ln and not ln.startswith("#"))
    return _cache["golden"]


def test_the_golden_file_covers_the_table():
    names = [_name(c) for cases in GROUPS.values() for c in cases]
    assert len(set(names)) == len(names) and set(names) == set(_golden())
    forms = {rec.split()[0] for rec in _golden().values() if not rec.startswith("error")}
    assert forms == {"0", "1", "2", "3", "4", "5"}, forms            # every NSK_SPLIT_BWD_* form, and "no launch", occurs


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_step_sends_the_launch_the_parent_sent(group):
    wrong = []
    for c in GROUPS[group]:
        got, want = run_case(c), _golden()[_name(c)]
        if got != want:
            wrong.append("%s\n    got  %s\n    want %s" % (_name(c), got, want))
    print("%s: %d cases, %d differ" % (group, len(GROUPS[group]), len(wrong)))
    assert not wrong, "\n".join(wrong[:20])


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--record" or "NSK_LIB" not in os.environ:
        sys.exit("usage: NSK_LIB=<the parent's libnsk.so> python tests/test_gpu_bwd_form.py --record <commit> <output file>")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[3], "w") as out:
        out.write("# recorded from commit %s (the parent build: NSK_LIB), 256-CU device, by tests/test_gpu_bwd_form.py --record\n" % sys.argv[2])
        out.write("# <case> : the 16 integers of nsk_debug_last_split(dir = 1) | the bits of the step's loss -- or the library's error text\n")
        for group, cases in GROUPS.items():
            for c in cases:
                out.write("%s : %s\n" % (_name(c), run_case(c)))
                out.flush()
    print("recorded %d cases" % sum(len(v) for v in GROUPS.values()))

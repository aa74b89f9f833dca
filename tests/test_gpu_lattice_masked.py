"""GPU tests of the lattice evaluation under a validity mask (nsk_eval_lattice_masked, Context.eval_lattice(valid=...), Mesher).
The bar is bit equality: a set node holds what the dense nsk_eval_lattice (or nsk_eval_points on the numpy float32 lattice) gives there,
every other node holds the bits of `fill`.  Every output tensor is prefilled with 7.0, so a node no pass wrote shows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_checks as mc
import mesh_cull_checks as cc
import scenes
from gpu_util import cu
from test_gpu_mesh import small_ctx  # noqa: F401  (the module-scoped fixture: SMALL_GRID_SHAPES, std 0.3)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nice-slam-cpp_amd", "host")

NX, NY, NZ = 37, 23, 29
NN = NX * NY * NZ
NAN_FILL = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
FILLS = (np.float32(100.0), np.float32(-0.0), NAN_FILL)
JUNK = 7.0


def ibits(t):
    """the int32 bits of a float32 cuda tensor or numpy array, flat, on the host"""
    if isinstance(t, torch.Tensor):
        return t.reshape(-1).view(torch.int32).cpu().numpy()
    return np.ascontiguousarray(t, np.float32).reshape(-1).view(np.int32)


def fbits(fill):
    return int(np.array([fill], np.float32).view(np.int32)[0])


@pytest.fixture(scope="module")
def lat(small_ctx):  # noqa: F811
    """the 37 x 23 x 29 lattice that sticks out of the bound by 0.3 on every side, and the dense volumes per stage (computed once)"""
    ctx, sc = small_ctx
    b = sc["bound"]
    origin = (b[:, 0] - np.float32(0.3)).astype(np.float32)
    step = ((b[:, 1] - b[:, 0] + np.float32(0.6)) / np.array([NX - 1, NY - 1, NZ - 1], np.float32)).astype(np.float32)
    pts = mc.lattice_points(origin, step, NX, NY, NZ)
    inb = ((pts > b[:, 0]) & (pts < b[:, 1])).all(axis=1)
    ctx.set_tuning("lattice_slab", 0)
    dense = {st: ibits(ctx.eval_lattice(st, origin, step, NX, NY, NZ)) for st in ("coarse", "middle", "fine", "color")}
    return dict(ctx=ctx, sc=sc, origin=origin, step=step, pts=pts, inb=inb, dense=dense)


def random_mask(seed=5):
    """half the nodes set; a tenth of the set bytes rewritten to 7 and to 255 (any non-zero byte counts)"""
    rng = np.random.default_rng(seed)
    valid = (rng.random(NN) < 0.5).astype(np.uint8)
    on = np.flatnonzero(valid)
    pick = rng.choice(on, len(on) // 10, replace=False)
    valid[pick[::2]] = 7
    valid[pick[1::2]] = 255
    return valid


def masked(lat, stage, valid, fill, slab=0):
    """-> (bits [NN] on the host, evaluated count)"""
    ctx = lat["ctx"]
    ctx.set_tuning("lattice_slab", slab)
    try:
        out = torch.full((NZ, NY, NX), JUNK, dtype=torch.float32, device="cuda")
        v = valid if isinstance(valid, torch.Tensor) else cu(valid, torch.uint8)
        got = ctx.eval_lattice(stage, lat["origin"], lat["step"], NX, NY, NZ, valid=v, fill=fill, out=out)
        assert got is out
        return ibits(out), ctx.last_evaluated
    finally:
        ctx.set_tuning("lattice_slab", 0)


def check(lat, stage, valid, fill, slab=0, label=""):
    got, n = masked(lat, stage, valid, fill, slab)
    on = np.asarray(valid).reshape(-1) != 0
    bad_set = int((got[on] != lat["dense"][stage][on]).sum())
    bad_unset = int((got[~on] != fbits(fill)).sum())
    print("%s stage %s slab %d fill %r: %d set nodes, %d of them differ from the dense volume, %d of %d unset nodes differ from fill"
          % (label, stage, slab, float(fill), int(on.sum()), bad_set, bad_unset, int((~on).sum())))
    assert bad_set == 0 and bad_unset == 0
    assert n == int(on.sum())
    return got


# ---- 1. bit equality under a random mask --------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["coarse", "middle", "fine", "color"])
def test_random_mask_bit_equal_to_dense_and_fill(lat, stage):
    valid = random_mask()
    on, inb = valid != 0, lat["inb"]
    dense = lat["dense"][stage]
    assert (on & inb).any() and (on & ~inb).any() and set(np.unique(valid).tolist()) == {0, 1, 7, 255}
    assert (dense[on & ~inb] == fbits(100.0)).all() and (dense[on & inb] != fbits(100.0)).any()
    n_set = int(on.sum())
    assert 2 * 5000 < n_set < 3 * 5000 and n_set % 5000 != 0          # slab 5000: three slabs, the last ragged
    for slab in (0, 5000):
        for fill in FILLS:
            check(lat, stage, valid, fill, slab, "random mask")
    # a bool mask is the same mask
    got, n = masked(lat, stage, cu(on, torch.bool), FILLS[0])
    assert (got[on] == dense[on]).all() and (got[~on] == fbits(100.0)).all() and n == n_set


# ---- 2. degenerate masks ----------------------------------------------------------------------------------------------
def test_all_zeros_launches_no_decoder(lat):
    ctx = lat["ctx"]
    stats = ctx.last_call_stats()
    valid = np.zeros(NN, np.uint8)
    for fill in FILLS:
        with torch.cuda.stream(ctx.tstream):
            ctx.profile_begin()
            got, n = masked(lat, "fine", valid, fill)
            prof = ctx.profile_end()
        assert (got == fbits(fill)).all() and n == 0
        assert sorted(prof) == ["lattice_compact"], prof
    assert ctx.last_call_stats() == stats


@pytest.mark.parametrize("name", ["all ones", "node 0", "last node", "one workgroup", "slab exactly", "slab + 1"])
def test_degenerate_masks(lat, name):
    valid = np.zeros(NN, np.uint8)
    slab = 0
    if name == "all ones":
        valid[:] = 1
    elif name == "node 0":
        valid[0] = 1
    elif name == "last node":
        valid[-1] = 1
    elif name == "one workgroup":
        valid[3 * 256:4 * 256] = 1                           # exactly 256 set nodes in one workgroup's range
    else:
        slab = 4096
        k = slab + (name == "slab + 1")
        valid[np.random.default_rng(8).choice(NN, k, replace=False)] = 1
        assert int(valid.sum()) == k
    for stage in ("fine", "coarse"):
        for fill in (FILLS[0], NAN_FILL):
            got = check(lat, stage, valid, fill, slab, name)
            if name == "all ones":
                assert (got == lat["dense"][stage]).all()


# ---- 3. scan depth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(41, 41, 41), (264, 256, 256)])
def test_scan_levels(lat, shape):
    """41^3 nodes are 270 workgroups (two scan levels), 264 x 256 x 256 are 67 584 (three).  Three whole z-planes and 0.2 % random nodes are
    set; there the middle stage must equal eval_points on the numpy float32 points bit for bit, everywhere else `fill`"""
    ctx, b = lat["ctx"], lat["sc"]["bound"]
    nx, ny, nz = shape
    nn = nx * ny * nz
    nb = (nn + 255) // 256 + 1
    assert (nb > 256) and ((nb > 65536) == (shape[0] == 264))
    origin = (b[:, 0] - np.float32(0.3)).astype(np.float32)
    step = ((b[:, 1] - b[:, 0] + np.float32(0.6)) / np.array([nx - 1, ny - 1, nz - 1], np.float32)).astype(np.float32)
    rng = np.random.default_rng(13)
    valid = (rng.random(nn) < 0.002).astype(np.uint8).reshape(nz, ny, nx)
    valid[0] = 1; valid[nz // 2] = 1; valid[-1] = 1
    valid = valid.reshape(-1)
    idx = np.flatnonzero(valid)
    cx, cy, cz = mc.lattice_coords(origin, step, (nx, ny, nz))       # mesh_checks.lattice_points, row by row, at the set indices only
    pts = np.stack([cx[idx % nx], cy[(idx // nx) % ny], cz[idx // (nx * ny)]], axis=1).astype(np.float32)
    if nn < 10 ** 6:
        assert (pts == mc.lattice_points(origin, step, nx, ny, nz)[idx]).all()
    want_set = ctx.eval_points("middle", cu(pts))[:, 3].contiguous().view(torch.int32)
    dvalid, didx = cu(valid, torch.uint8), torch.tensor(idx, device="cuda")
    for fill in (FILLS[0], NAN_FILL):
        out = torch.full((nz, ny, nx), JUNK, dtype=torch.float32, device="cuda")
        ctx.eval_lattice("middle", origin, step, nx, ny, nz, valid=dvalid, fill=fill, out=out)
        want = torch.full((nn,), fbits(fill), dtype=torch.int32, device="cuda")
        want[didx] = want_set
        ndiff = int((out.view(-1).view(torch.int32) != want).sum())
        print("%d x %d x %d: %d set nodes, %d workgroup counts, fill %r: %d nodes differ" % (nx, ny, nz, len(idx), nb, float(fill), ndiff))
        assert ndiff == 0 and ctx.last_evaluated == len(idx)
    assert bool((want_set != fbits(100.0)).any()) and bool((want_set == fbits(100.0)).any())


# ---- 4. the mesh does not see the difference ----------------------------------------------------------------------------
def test_mesh_from_masked_volume_equals_mesh_from_dense(lat):
    ctx = lat["ctx"]
    ks = cc.cull_scene(lat["sc"]["bound"], keyframes=(0,), params=((0, 0.25),))       # one look-at camera outside the lattice, cc.depth_image
    assert (ks["origin"] == lat["origin"]).all() and (ks["step"] == lat["step"]).all() and (ks["nx"], ks["ny"], ks["nz"]) == (NX, NY, NZ)
    valid, n_seen = ctx.lattice_seen(lat["origin"], lat["step"], NX, NY, NZ, cu(ks["depths"]), ks["intr"], ks["w2c"], 0, 0.25)
    dense = ctx.eval_lattice("fine", lat["origin"], lat["step"], NX, NY, NZ)
    share = mc.processed_cells(dense.cpu().numpy(), valid.cpu().numpy()).mean()
    print("seen mask: %d of %d nodes, %.1f %% of the cells processed" % (n_seen, NN, 100 * share))
    assert 0.05 < share < 0.9
    v0, t0 = ctx.extract_mesh(dense, lat["origin"], lat["step"], 0.0, valid)
    assert len(v0) > 100 and len(t0) > 100
    for fill in (FILLS[0], NAN_FILL):
        out = torch.full((NZ, NY, NX), JUNK, dtype=torch.float32, device="cuda")
        ctx.eval_lattice("fine", lat["origin"], lat["step"], NX, NY, NZ, valid=valid, fill=fill, out=out)
        assert ctx.last_evaluated == n_seen
        v, t = ctx.extract_mesh(out, lat["origin"], lat["step"], 0.0, valid)
        assert v.cpu().numpy().tobytes() == v0.cpu().numpy().tobytes() and t.cpu().numpy().tobytes() == t0.cpu().numpy().tobytes()


# ---- 5. determinism and error paths -------------------------------------------------------------------------------------
def test_two_runs_same_bytes_and_error_paths(lat):
    import nice_slam_cpp_amd as pkg
    ctx = lat["ctx"]
    L = pkg.nsk.lib()
    err = lambda: L.nsk_last_error().decode()
    valid = random_mask()
    a = check(lat, "fine", valid, NAN_FILL, 5000, "first run")
    b = check(lat, "fine", valid, NAN_FILL, 5000, "second run")
    assert a.tobytes() == b.tobytes()
    dv = cu(valid, torch.uint8)
    out = torch.full((NN,), JUNK, dtype=torch.float32, device="cuda")
    o = np.ascontiguousarray(lat["origin"]); s = np.ascontiguousarray(lat["step"]); neg = np.array([1, -1, 1], np.float32)
    op, sp = o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)
    n = C.c_longlong(-1)

    def call(stage=2, org=op, stp=sp, nx=NX, ny=NY, nz=NZ, vp=C.c_void_p(dv.data_ptr()), outp=C.c_void_p(out.data_ptr())):
        return L.nsk_eval_lattice_masked(ctx.h, stage, org, stp, nx, ny, nz, vp, C.c_float(100.0), outp, C.byref(n))
    assert call(vp=None) != 0 and "d_valid is NULL" in err() and "nsk_eval_lattice" in err()
    assert call(outp=None) != 0 and "d_volume is NULL" in err()
    assert call(stage=5) != 0 and "stage" in err()
    assert call(stage=-1) != 0 and "stage" in err()
    assert call(nx=0) != 0 and "at least 1 nodes" in err()
    assert call(org=None) != 0 and "null" in err()
    assert call(stp=neg.ctypes.data_as(C.c_void_p)) != 0 and "step[1]" in err()
    assert call(nx=1 << 10, ny=1 << 10, nz=(1 << 8) + 1) != 0 and "at most" in err()
    torch.cuda.synchronize()
    assert bool((out == JUNK).all()), "a refused call wrote to the volume"
    # a good call follows, without the optional count too
    assert L.nsk_eval_lattice_masked(ctx.h, 2, op, sp, NX, NY, NZ, C.c_void_p(dv.data_ptr()), C.c_float(100.0), C.c_void_p(out.data_ptr()), None) == 0
    assert call() == 0 and n.value == int((valid != 0).sum())
    ctx.sync()
    on = valid != 0
    got = ibits(out)
    assert (got[on] == lat["dense"]["fine"][on]).all() and (got[~on] == fbits(100.0)).all()
    assert (got[on] == a[on]).all()
    # the dense call is what it was
    assert (ibits(ctx.eval_lattice("fine", lat["origin"], lat["step"], NX, NY, NZ)) == lat["dense"]["fine"]).all() and ctx.last_evaluated is None


# ---- 6. C++ -----------------------------------------------------------------------------------------------------------------
def test_clean_mesh_cpp_evaluates_the_seen_nodes_only(tmp_path):
    """Mesher::get_clean_mesh on the scene of test_clean_mesh_cpp_equals_the_python_path: the decoders ran on as many nodes as the keyframes saw
    (the numpy float32 rule's count), fewer than the lattice has"""
    exe = os.path.join(HOST, "clean_mesh_test")
    if not os.path.exists(exe):
        pytest.fail("clean_mesh_test is not built (run __graft_entry__.build())")
    sc = scenes.make_scene(1, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    ks = cc.mesher_scene(sc["bound"])
    n = cc.MESHER_N
    want_seen = int(cc.seen_f32(ks["pts"], ks["depths"], ks["intr"], ks["w2c"], 0, 0.5).sum())
    d = str(tmp_path)
    np.save(os.path.join(d, "bound.npy"), sc["bound"].astype(np.float32))
    for k in scenes.LEVELS:
        np.save(os.path.join(d, "grid_%s.npy" % k), sc["grids"][k][None].astype(np.float32))
        np.save(os.path.join(d, "dec_%s.npy" % k), sc["decoders"][k].astype(np.float32))
    np.save(os.path.join(d, "depths.npy"), ks["depths"].astype(np.float32))
    np.save(os.path.join(d, "c2ws.npy"), ks["c2w"].astype(np.float32))
    np.save(os.path.join(d, "intr.npy"), np.array(ks["intr"], np.float32))
    r = subprocess.run([exe, d, str(n), "0", "0.1", "0.0", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "clean_mesh_test ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"(\d+) seen, (\d+) evaluated of (\d+) nodes", r.stdout)
    assert m, r.stdout
    seen, evaluated, nodes = [int(x) for x in m.groups()]
    print(r.stdout.strip())
    assert nodes == n ** 3 and evaluated == seen == want_seen and 0 < evaluated < nodes

"""CPU tests (-m "not gpu") of the depth-fusion checks themselves (tests/tsdf_checks.py): the float32 restatement of the rule sees what
mesh_cull_checks.seen_f32 sees, agrees with its float64 form within the bound that form derives, meshes the sphere scene within a cell of
the analytic sphere, and streams."""
import numpy as np
import pytest

import mesh_checks as mc
import mesh_cull_checks as cc
import scenes
import tsdf_checks as tc

F = np.float32


@pytest.fixture(scope="module")
def cull():
    sc = cc.cull_scene(scenes.REF_BOUND)
    sc["trunc"] = F(0.5)
    return sc


@pytest.fixture(scope="module")
def sphere():
    return tc.sphere_scene()


def both(sc, ks=None, edge=0, max_weight=64):
    ks = list(range(len(sc["depths"]))) if ks is None else ks
    a = (sc["pts"], sc["depths"][ks], sc["intr"], sc["w2c"][ks], edge, sc["trunc"])
    return tc.fuse_f32(*a, max_weight), tc.fuse_f64(*a, max_weight), cc.seen_f32(*a), cc.seen_f64(*a)


@pytest.mark.parametrize("name", ["cull", "sphere"])
def test_float32_rule_against_float64(name, cull, sphere):
    sc = cull if name == "cull" else sphere
    ks = [0, 1, 2, 0, 1, 0] if name == "cull" else None
    (T32, W32), (T64, W64, bound), seen32, (seen64, margin, _) = both(sc, ks)
    assert ((W32 > 0).astype(np.uint8) == seen32).all()                  # weight > 0 is the seen mask, at every node
    sure = margin > 1.0
    print("%s: %d nodes, %d observed, %.3f %% within the float32 bound of a decision" % (name, len(T32), int(seen32.sum()), 100 * (~sure).mean()))
    assert (~sure).mean() <= 0.01
    assert (W32[sure] == W64[sure]).all()
    err = np.abs(T32.astype(np.float64) - T64)[sure]
    worst = int(np.argmax(err - bound[sure]))
    print("%s: |T_f32 - T_f64| at most %.3g, the bound there %.3g, the largest bound %.3g" % (name, err.max(), bound[sure][int(np.argmax(err))], bound[sure].max()))
    assert (err <= bound[sure]).all(), (err[worst], bound[sure][worst])
    assert bound[sure].max() < 1e-4                                       # (the bound is a float32 rounding bound, not a loose one)
    assert 0 < seen32.sum() < seen32.size and W32.max() >= 2
    assert np.abs(T32[W32 > 0]).max() <= 1.0 + 1e-6 and (T32[W32 == 0] == 0).all()


def test_sphere_mesh_lies_on_the_sphere(sphere):
    sc = sphere
    a = (sc["pts"], sc["depths"], sc["intr"], sc["w2c"], 0, sc["trunc"])
    T64, W64, _ = tc.fuse_f64(*a)
    shape = (sc["nz"], sc["ny"], sc["nx"])
    vol, _ = tc.volume_of(T64, W64, 1, shape)
    _, pos = mc.reference_vertices(vol.astype(F), sc["origin"], sc["step"], 0.0)
    tc.check_sphere_mesh(pos, sc, "float64 volume")
    T32, W32 = tc.fuse_f32(*a)
    vol32, valid = tc.volume_of(T32, W32, 1, shape)
    assert vol32.dtype == F and (np.isfinite(vol32) == (valid != 0)).all()
    _, pos32 = mc.reference_vertices(vol32, sc["origin"], sc["step"], 0.0)
    tc.check_sphere_mesh(pos32, sc, "float32 volume")


def test_streaming_gives_the_bytes_of_one_pass(sphere):
    sc = sphere
    a = lambda ks: (sc["pts"], sc["depths"][ks], sc["intr"], sc["w2c"][ks], 0, sc["trunc"])
    T, W = tc.fuse_f32(*a(slice(0, 8)), 2)
    state = None
    for ks in (slice(0, 1), slice(1, 3), slice(3, 8)):
        state = tc.fuse_f32(*a(ks), 2, state)
    assert T.tobytes() == state[0].tobytes() and W.tobytes() == state[1].tobytes()
    assert W.max() == 2                                                   # (the cap was reached)


def test_volume_of_flips_the_sign_bit():
    T = np.array([0.0, -0.0, 0.25, -1.0, 0.5], F)
    W = np.array([1.0, 2.0, 0.0, 3.0, 1.0], F)
    vol, valid = tc.volume_of(T, W, 2, (1, 1, 5))
    assert valid.reshape(-1).tolist() == [0, 1, 0, 1, 0]
    assert np.isnan(vol.reshape(-1)[[0, 2, 4]]).all()
    assert vol.reshape(-1)[[1, 3]].tobytes() == np.array([0.0, 1.0], F).tobytes()
    vol, valid = tc.volume_of(T, W, 1, (1, 1, 5))
    assert np.signbit(vol.reshape(-1)[0]) and vol.reshape(-1)[0] == 0

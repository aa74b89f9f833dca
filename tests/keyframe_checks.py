"""fp64 numpy evaluations of the frame-level Mapper / Tracker operations, written from their definitions in include/nsk.h (not from
oracle/nso.c), the case tables of tests/test_keyframe_cpu.py and tests/test_gpu_keyframe.py, and for every boolean decision the fp64
MARGIN of each element.  No GPU, no ctypes.

Margin rule (frustum mask, keyframe overlap).  A decision compares a computed quantity q with a threshold T.  The fp32 evaluation (the
oracle's and the device's: the same operations, each rounded once) carries q32 = q64 + e with |e| <= bound, where `bound` is the first-order
propagation of one unit roundoff U = 2^-24 per fp32 operation through the rule, with the magnitudes that enter it taken per element.
`margin` is min over the thresholds of |q64 - T| / bound: a fp32 decision may differ from the fp64 one only where margin < 1.  The bounds
(nothing here is fitted to what the code gives):

  camera coordinates   cam = w2c p + t, p a voxel centre or a ray sample.  p carries e_p (below); the entries of w2c are rounded once
                       (the inverse is formed in double, then stored as fp32), each product once, the three adds once each:
                       e_cam <= |w2c| e_p + 5 U (|w2c| |p| + |t|)                               (componentwise, |.| of every entry)
  voxel centre         p = lo + (hi - lo) * linspace: sub, mul, add, and linspace01 itself two operations: e_p <= 5 U max(|lo|, |hi|)
  ray sample           p = o + d z,  z = near (1 - t) + far t: near, far, 1 - t, two products, one add, t two operations:
                       e_z <= 8 U max(near, far),  e_p <= |d| e_z + 2 U (|o| + |d| z)
  z                    zc = cam_z + 1e-5 (1e-5 rounds to fp32 with a relative U):  e_z <= e_cam_z + U (|cam_z| + 2e-5)
  pixel                u = (fx cam_x + cx cam_z) / zc: two products, one add, one division:
                       e_u <= (fx e_cam_x + |cx| e_cam_z + 3 U (fx |cam_x| + |cx| |cam_z|)) / |zc| + |u| (e_z / |zc| + U)
  sampled depth        bilinear in (u, v) with slopes at most D = max |image|, four taps of three products and one add each:
                       e_d <= D (e_u + e_v) + 8 U D      (0 where u +- e_u, v +- e_v leave all four taps outside the image: exactly 0)
  maximum depth        only a voxel whose d + e_d reaches the maximum can move it, by at most its own e_d:
                       e_dmax <= max { e_d[i] : d[i] + 2 e_d[i] >= dmax }
  depth test           -zc <= d + 0.5:  bound = e_z + e_d (or e_dmax where d == 0 took the maximum) + U (|d| + 0.5)
  zero-depth switch    d == 0 ? dmax : d is discontinuous.  It matters only where the test's outcome differs between d and dmax; there a
                       sample that is exactly zero on one side and not on the other needs (u, v) to cross a pixel line, so the margin is the
                       distance of u, v to the nearest integer over e_u, e_v.
  conjunctions         a rule that is an AND of comparisons is safely false as soon as ONE failing comparison is safe, and safely true only
                       when all are (and_margin); the frustum's  seen OR ball  the other way round.
  ball                 s = |p - c|^2 < 0.25: three subs, three products, two adds:  e_s <= 2 sqrt(s) sqrt(3) (e_p + U |c|) + 6 U s
"""
import numpy as np

import scenes

U32 = 2.0 ** -24
REF_BOUND = scenes.REF_BOUND
DYADIC_BOUND = np.array([[-4.0, 4.0], [-2.0, 2.0], [-3.0, 3.0]], np.float32)
CAP = 0.01                      # at most this share of a case's elements may have margin < 1


# ---- shared geometry -------------------------------------------------------------------------------------------------------------------
def pose(R, t):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = np.asarray(R, np.float64)
    m[:3, 3] = np.asarray(t, np.float64)
    return m


def turned(c2w):
    """the same camera turned by pi about its own up axis: it looks the other way"""
    m = c2w.astype(np.float64).copy()
    m[:3, :3] = m[:3, :3] @ np.diag([-1.0, 1.0, -1.0])
    return m.astype(np.float32)


def room_image(bound, c2w, H, W, intr, kind="walls"):
    """depth images of the case tables: the analytic room's walls (finite, clipped to [0, 20]), all zeros, every third row zero, negated"""
    with np.errstate(all="ignore"):
        d = scenes.frame_depth_image(bound, c2w, H, W, *intr)
    d = np.clip(np.nan_to_num(d, nan=0.0, posinf=20.0, neginf=0.0), 0.0, 20.0).astype(np.float32)
    if kind == "zeros":
        d[:] = 0.0
    elif kind == "rows":
        d[::3, :] = 0.0
    elif kind == "negative":
        d = -(d + np.float32(0.25))
    elif kind == "shallow":
        d = (d * np.float32(0.125)).astype(np.float32)
        d[::3, :] = 0.0
    else:
        assert kind == "walls", kind
    return np.ascontiguousarray(d)


def _project(w2c, P, e_p, intr):
    """camera coordinates, pixel and their fp32 error bounds (module docstring) for points P [n,3] with error e_p [n,3] or scalar"""
    fx, fy, cx, cy = (float(x) for x in intr)
    A, t = w2c[:3, :3], w2c[:3, 3]
    cam = P @ A.T + t
    e_cam = np.broadcast_to(e_p, P.shape) @ np.abs(A).T + 5 * U32 * (np.abs(P) @ np.abs(A).T + np.abs(t))
    cam[:, 0] *= -1
    z = cam[:, 2] + 1e-5
    e_z = e_cam[:, 2] + U32 * (np.abs(cam[:, 2]) + 2e-5)
    with np.errstate(all="ignore"):
        u = (fx * cam[:, 0] + cx * cam[:, 2]) / z
        v = (fy * cam[:, 1] + cy * cam[:, 2]) / z
        az = np.abs(z)
        e_u = (fx * e_cam[:, 0] + abs(cx) * e_cam[:, 2] + 3 * U32 * (fx * np.abs(cam[:, 0]) + abs(cx) * np.abs(cam[:, 2]))) / az + np.abs(u) * (e_z / az + U32)
        e_v = (fy * e_cam[:, 1] + abs(cy) * e_cam[:, 2] + 3 * U32 * (fy * np.abs(cam[:, 1]) + abs(cy) * np.abs(cam[:, 2]))) / az + np.abs(v) * (e_z / az + U32)
    return cam, z, u, v, e_z, e_u, e_v


def and_margin(conds, margins):
    """margin of a conjunction: true -- every operand must hold, the smallest margin counts; false -- one operand that fails safely is
    enough, the largest margin among the failing operands counts"""
    conds, margins = np.array(conds), np.array(margins)
    return np.where(conds.all(0), margins.min(0), np.where(conds, -np.inf, margins).max(0))


def _ratio(dist, bound):
    with np.errstate(all="ignore"):
        r = np.asarray(dist, np.float64) / np.asarray(bound, np.float64)
    return np.where(np.isnan(r), 0.0, r)          # 0 / 0: on the threshold with no error bound to speak of -- a tie


# ---- 1. frustum mask (nsk_frustum_mask) ---------------------------------------------------------------------------------------------------
def voxel_centres(bound, shape):
    """[Z*Y*X, 3] float64, x fastest: the centres are the end-point-inclusive linspace of the bound along each axis"""
    Z, Y, X = shape
    b = np.asarray(bound, np.float64)
    zz, yy, xx = np.meshgrid(np.linspace(b[2, 0], b[2, 1], Z), np.linspace(b[1, 0], b[1, 1], Y), np.linspace(b[0, 0], b[0, 1], X), indexing="ij")
    return np.stack([xx, yy, zz], -1).reshape(-1, 3)


def bilinear_zero(img, u, v):
    """bilinear sample at (u, v) with a zero border; non-finite coordinates sample nothing"""
    H, W = img.shape
    ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
    uu, vv = np.where(ok, u, -10.0), np.where(ok, v, -10.0)
    x0, y0 = np.floor(uu), np.floor(vv)
    ax, ay = uu - x0, vv - y0
    s = np.zeros_like(uu)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            tap = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.float64)
            s = s + np.where(inside, (ax if dx else 1 - ax) * (ay if dy else 1 - ay) * tap, 0.0)
    return s, ok


def frustum64(bound, shape, depth_img, intr, c2w):
    """the frustum rule of include/nsk.h in float64 -> dict(mask [Z,Y,X] bool, margin [Z,Y,X] (module docstring), ties: exact ties per criterion)"""
    H, W = depth_img.shape
    P = voxel_centres(bound, shape)
    c2w = np.asarray(c2w, np.float64).reshape(4, 4)
    w2c = np.linalg.inv(c2w)
    e_p = 5 * U32 * float(np.abs(np.asarray(bound, np.float64)).max())
    cam, z, u, v, e_z, e_u, e_v = _project(w2c, P, e_p, intr)
    d_raw, finite = bilinear_zero(depth_img, u, v)
    D = float(np.abs(depth_img).max())
    with np.errstate(all="ignore"):
        off_image = (u + e_u < -1) | (u - e_u > W) | (v + e_v < -1) | (v - e_v > H)      # all four taps outside in fp32 too: exactly 0, no error
    e_d = np.where(finite & ~off_image, D * (np.where(finite, e_u, 0.0) + np.where(finite, e_v, 0.0)) + 8 * U32 * D, 0.0)
    dmax = max(0.0, float(d_raw.max()))
    cand = d_raw + 2 * e_d >= dmax
    e_dmax = float(e_d[cand].max()) if cand.any() else 0.0
    zero = d_raw == 0
    d = np.where(zero, dmax, d_raw)
    with np.errstate(all="ignore"):
        in_img = (u > 0) & (u < W) & (v > 0) & (v < H)
        seen = in_img & (0 <= -z) & (-z <= d + 0.5)
        other = in_img & (0 <= -z) & (-z <= np.where(zero, d_raw, dmax) + 0.5)       # the outcome had the zero switch gone the other way
    c = c2w[:3, 3]
    s = ((P - c) ** 2).sum(1)
    ball = s < 0.25
    e_s = 2 * np.sqrt(s) * np.sqrt(3.0) * (e_p + U32 * np.abs(c).max()) + 6 * U32 * s
    with np.errstate(all="ignore"):
        m_dep = _ratio(np.abs(-z - d - 0.5), e_z + np.where(zero, e_dmax, e_d) + U32 * (np.abs(d) + 0.5))
        m_sw = np.where(seen != other, np.minimum(_ratio(np.abs(u - np.round(u)), e_u), _ratio(np.abs(v - np.round(v)), e_v)), np.inf)
        conds = [u > 0, u < W, v > 0, v < H, 0 <= -z, -z <= d + 0.5]
        margins = [_ratio(np.abs(u), e_u), _ratio(np.abs(u - W), e_u), _ratio(np.abs(v), e_v), _ratio(np.abs(v - H), e_v), _ratio(np.abs(z), e_z),
                   np.minimum(m_dep, m_sw)]
    m_seen = and_margin(conds, margins)
    m_ball = _ratio(np.abs(s - 0.25), e_s)
    # seen OR ball: a true outcome is as safe as its safest true operand, a false one as its least safe operand
    margin = np.where(seen & ball, np.maximum(m_seen, m_ball), np.where(seen, m_seen, np.where(ball, m_ball, np.minimum(m_seen, m_ball))))
    ties = dict(u0=int((u == 0).sum()), v0=int((v == 0).sum()), z0=int((cam[:, 2] == 0).sum()), ball=int((s == 0.25).sum()))
    return dict(mask=(seen | ball).reshape(shape), margin=margin.reshape(shape), ties=ties, dmax=dmax)


def _cam_case(name, bound, shape, HW, intr, c2w, expect_some=True, expect_all=False):
    return dict(name=name, bound=np.asarray(bound, np.float32), shape=tuple(shape), HW=HW, intr=intr, c2w=np.asarray(c2w, np.float32),
                some=("walls", "rows") if expect_some else (), dyadic=False)


INTR_A, HW_A = (80.0, 80.0, 79.5, 59.5), (120, 160)
FRUSTUM_KINDS = ("walls", "zeros", "rows")
SHAPES = [(1, 2, 3), (3, 5, 17), (4, 8, 8), (1, 1, 257), (17, 16, 15), (9, 8, 11)]


def _inside_camera(seed):
    return scenes.make_camera(np.random.default_rng(seed), REF_BOUND)


def _outside_camera():
    """2 m outside the upper z face, on the room's axis, looking along -z into the bound"""
    b = REF_BOUND.astype(np.float64)
    ctr = b.mean(1)
    return pose(scenes.look_rotation(0.05, -0.03, 0.02), [ctr[0], ctr[1], b[2, 1] + 2.0])


def frustum_cases():
    """the case table: (bound, shape, image size, intrinsics, pose); every case runs with each of FRUSTUM_KINDS"""
    cases = []
    for k, shape in enumerate(SHAPES):                                    # voxel counts around the launch geometry, a camera inside the bound
        thin = shape[0] == 1              # one z plane, the bound's lower z face: a camera 1 m from the centre towards it, pitched down towards its floor edge
        c2w = pose(scenes.look_rotation(0.1, -0.5, 0.05), REF_BOUND.mean(1) + np.array([0, 0, -1], np.float32)) if thin else _inside_camera(3 + k)
        cases.append(_cam_case("inside-%dx%dx%d" % shape, REF_BOUND, shape, HW_A, INTR_A, c2w))
        if shape == (1, 2, 3):
            cases[-1]["some"] = ("walls",)      # of its six voxels one is seen, and with every third image row zero its sampled depth falls short
    out = _outside_camera()
    cases.append(_cam_case("outside-looking-in", REF_BOUND, (17, 16, 15), HW_A, INTR_A, out))
    cases.append(_cam_case("outside-turned", REF_BOUND, (17, 16, 15), HW_A, INTR_A, turned(out), expect_some=False))
    on = voxel_centres(REF_BOUND, (9, 8, 11)).astype(np.float32)[(4 * 8 + 3) * 11 + 5]     # exactly a voxel centre as fp32 stores it
    cases.append(_cam_case("on-a-voxel", REF_BOUND, (9, 8, 11), HW_A, INTR_A, pose(scenes.look_rotation(0.3, 0.1, -0.1), on)))
    sc = _inside_camera(21).astype(np.float64)
    sc[:3, :3] *= 1.003                                                    # an unnormalised quaternion's rotation: the general inverse
    cases.append(_cam_case("scaled-rotation", REF_BOUND, (9, 8, 11), HW_A, INTR_A, sc))
    cases.append(_cam_case("1x1-image", REF_BOUND, (9, 8, 11), (1, 1), (1.0, 1.0, 0.5, 0.5), _inside_camera(22), expect_some=False))
    cases.append(_cam_case("fractional-intrinsics", REF_BOUND, (9, 8, 11), (31, 33), (20.0, 21.0, 16.1, 15.3), _inside_camera(23)))
    return cases


DYADIC_INTR, DYADIC_HW = (16.0, 16.0, 16.0, 12.0), (24, 32)


def dyadic_cases():
    """every voxel coordinate, the pose and the intrinsics are exact fp32 numbers: fp32 == fp64 at EVERY voxel, the exact ties included"""
    cases = []
    for t in ((0.0, 0.0, 1.5), (0.0, 0.0, 0.0), (1.0, 0.0, 3.0), (0.0, 0.0, 4.5)):
        for shape in ((9, 5, 9), (5, 3, 17)):
            c = _cam_case("dyadic-t%g,%g,%g-%dx%dx%d" % (t + shape), DYADIC_BOUND, shape, DYADIC_HW, DYADIC_INTR, pose(np.eye(3), t))
            c["dyadic"] = True
            cases.append(c)
    return cases


def frustum_image(case, kind):
    return room_image(case["bound"], case["c2w"], case["HW"][0], case["HW"][1], case["intr"], kind)


def check_frustum(got, case, kind, ref64):
    """the margin rule for one case: returns the excluded share; raises on a difference outside it or above the cap"""
    diff = got != ref64["mask"]
    low = ref64["margin"] < 1.0
    share = float(low.mean())
    label = "%s/%s" % (case["name"], kind)
    if case["dyadic"]:
        assert not diff.any(), (label, int(diff.sum()))
        return 0.0
    assert not (diff & ~low).any(), (label, int((diff & ~low).sum()), float(ref64["margin"][diff & ~low].min()))
    assert share <= CAP, (label, share)
    return share


# ---- 2. keyframe overlap (nsk_keyframe_overlap) ---------------------------------------------------------------------------------------------
OVERLAP_SIZES = [(1, 1, 1), (3, 2, 4), (67, 5, 4), (100, 16, 9), (1000, 16, 1), (100, 16, 33)]
OVERLAP_CAP = 2                 # points per keyframe whose margin may be below 1


def overlap_case(N, ns, K, seed=6, HW=HW_A):
    """rays of one frame (scenes.make_rays, 120 x 160, a fifth of the depths zero; pixels from inside the 20-pixel edge, since a pixel ON column
    20 or 140 projects onto the own pose's threshold itself, sixteen samples at a time) and K keyframes: [0] the frame's own pose, then -- as far
    as K reaches -- a random pose, the own pose turned by pi, a pose whose centre is a sample point of ray 0, further random poses.  The own
    pose need not rank first in general (a keyframe that also sees the frame's camera centre, where the samples of a zero depth start, can
    beat it: seed 5 at K = 33); the seed is one at which the fp32 oracle ranks it first in all six size cases"""
    H, W = HW_A
    fx, fy, cx, cy = INTR_A
    r = scenes.make_rays(seed, N, REF_BOUND, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, n_frames=1, zero_frac=0.2, edge=21)
    rng = np.random.default_rng(seed + 100)
    own = r["c2w"][0]
    z0 = overlap_depths(r["gt_depth"][:1], ns)[0, ns // 2]
    centre = (r["rays_o"][0].astype(np.float64) + r["rays_d"][0].astype(np.float64) * z0).astype(np.float32)
    at_point = scenes.make_camera(rng, REF_BOUND)
    at_point[:3, 3] = centre
    cams = [own, scenes.make_camera(rng, REF_BOUND), turned(own), at_point]
    while len(cams) < K:
        cams.append(scenes.make_camera(rng, REF_BOUND))
    names = (["own", "random", "turned", "at-point"] + ["random"] * K)[:K]
    return dict(rays=r, cams=np.stack(cams[:K]).astype(np.float32), names=names, intr=INTR_A, HW=HW, N=N, ns=ns, K=K)


def overlap_depths(gt_depth, ns):
    gd = np.asarray(gt_depth, np.float64)[:, None]
    t = np.linspace(0.0, 1.0, ns)[None, :] if ns > 1 else np.zeros((1, 1))
    return gd * 0.8 * (1 - t) + (gd + 0.5) * t


def overlap64(case):
    """per keyframe: the fp64 count of points inside the image (20-pixel edge, in front of the camera) and the number whose margin < 1"""
    r, (H, W) = case["rays"], case["HW"]
    z = overlap_depths(r["gt_depth"], case["ns"])
    o, d = r["rays_o"].astype(np.float64)[:, None, :], r["rays_d"].astype(np.float64)[:, None, :]
    P = (o + d * z[..., None]).reshape(-1, 3)
    gd = np.asarray(r["gt_depth"], np.float64)[:, None]
    e_z = 8 * U32 * np.maximum(gd * 0.8, gd + 0.5) * np.ones_like(z)
    e_p = (np.abs(d) * e_z[..., None] + 2 * U32 * (np.abs(o) + np.abs(d) * z[..., None])).reshape(-1, 3)
    counts, low = [], []
    for c2w in case["cams"]:
        w2c = np.linalg.inv(c2w.astype(np.float64))
        cam, zc, u, v, e_zc, e_u, e_v = _project(w2c, P, e_p, case["intr"])
        with np.errstate(all="ignore"):
            m = (u < W - 20) & (u > 20) & (v < H - 20) & (v > 20) & (zc < 0)
            margin = and_margin([u < W - 20, u > 20, v < H - 20, v > 20, zc < 0],
                                [_ratio(np.abs(u - (W - 20)), e_u), _ratio(np.abs(u - 20), e_u), _ratio(np.abs(v - (H - 20)), e_v),
                                 _ratio(np.abs(v - 20), e_v), _ratio(np.abs(zc), e_zc)])
        counts.append(int(m.sum()))
        low.append(int((margin < 1.0).sum()))
    return np.array(counts), np.array(low)


def check_overlap(got, case, ref64):
    """float32 fractions against the fp64 counts: round(p N ns) differs from the count by at most the number of low-margin points (<= cap)"""
    counts, low = ref64
    total = case["N"] * case["ns"]
    got_counts = np.rint(np.asarray(got, np.float64) * total).astype(np.int64)
    assert (low <= OVERLAP_CAP).all(), (case["names"], low)
    assert (np.abs(got_counts - counts) <= low).all(), (got_counts, counts, low)
    assert got[0] == np.max(got), got                                    # the frame's own pose ranks first
    for k, name in enumerate(case["names"]):
        if name == "turned":
            assert got[k] == 0.0, got[k]                                 # every point lies behind the turned camera
    return int(np.abs(got_counts - counts).sum()), int(low.sum())


# ---- 3. pixel draw and gather ---------------------------------------------------------------------------------------------------------------
WINDOWS = [(5, 6, 7, 8), (0, 1, 0, 64), (0, 64, 3, 4), (0, 680, 0, 1200), (20, 660, 20, 1180)]
PIXEL_COUNTS = [0, 1, 255, 256, 257, 1000]
PIXEL_HW = (680, 1200)


def pixel_images(seed=2):
    rng = np.random.default_rng(seed)
    H, W = PIXEL_HW
    return rng.uniform(0.5, 4.0, (H, W)).astype(np.float32), rng.random((H, W, 3)).astype(np.float32)


def check_pixels(pi, pj, window, ref=None):
    H0, H1, W0, W1 = window
    pi, pj = np.asarray(pi), np.asarray(pj)
    assert ((pi >= W0) & (pi < W1) & (pj >= H0) & (pj < H1)).all(), window
    if ref is not None:
        assert np.array_equal(pi, ref[0]) and np.array_equal(pj, ref[1]), window


def gather_np(pi, pj, depth, color=None):
    return depth[pj, pi], (None if color is None else color[pj, pi])


# ---- 4. inside filter (nsk_inside_filter, nsk_prepare_rays) ---------------------------------------------------------------------------------
FILTER_COUNTS = [1, 255, 256, 257]


def filter_np(bound, ro, rd, gt):
    """t = min over the axes of max over the two sides of (bound - o) / d, keep = t >= gt, in numpy float32 (every operation correctly
    rounded, as ATen's); np.maximum / np.minimum hand a NaN on as torch.max / torch.min do"""
    b = np.asarray(bound, np.float32)
    with np.errstate(all="ignore"):
        t = (b[None, :, :] - np.asarray(ro, np.float32)[:, :, None]) / np.asarray(rd, np.float32)[:, :, None]
        far = np.minimum.reduce(np.maximum(t[:, :, 0], t[:, :, 1]), axis=1)
        return far >= np.asarray(gt, np.float32), far


def filter_rays(bound):
    """(rays_o, rays_d, gt_depth, n_nan): every origin class x every pattern of zero direction components (+0 and -0) x the gt_depth classes;
    the first rays are the ones whose 0/0 the comparison form used to keep or drop by plane and axis"""
    b = np.asarray(bound, np.float32)
    lo, hi, mid = b[:, 0], b[:, 1], ((b[:, 0] + b[:, 1]) * np.float32(0.5)).astype(np.float32)
    inside = mid + np.array([0.25, -0.125, 0.5], np.float32)
    origins = [inside,
               [lo[0], inside[1], inside[2]], [hi[0], inside[1], inside[2]], [inside[0], lo[1], inside[2]], [inside[0], hi[1], inside[2]],
               [inside[0], inside[1], lo[2]], [inside[0], inside[1], hi[2]],                                  # the six faces
               [lo[0], hi[1], inside[2]], [hi[0], inside[1], lo[2]], [inside[0], lo[1], hi[2]],               # edges
               [hi[0], hi[1], lo[2]], [lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]],                           # corners
               [hi[0] + 1, inside[1], inside[2]], [inside[0], lo[1] - 2, inside[2]]]                          # outside
    comps = [0.0, -0.0, 0.3, -1.0]
    dirs = [(x, y, z) for x in comps for y in comps for z in comps]
    ro = [[lo[0], 0, 0], [hi[0], hi[1], 0]]
    rd = [[0, 0.3, -1], [0, 0, -1]]
    for o in origins:
        for d in dirs:
            ro.append(o); rd.append(d)
    ro, rd = np.array(ro, np.float32), np.array(rd, np.float32)
    _, far = filter_np(b, ro, rd, np.zeros(len(ro), np.float32))
    gt = np.ones(len(ro), np.float32)
    fin = np.isfinite(far)
    k = np.arange(len(ro))
    with np.errstate(all="ignore"):
        gt = np.where((k % 6 == 2) & fin, far, gt)                                                           # gt == t exactly: kept
        gt = np.where((k % 6 == 3) & fin, np.nextafter(far, np.float32(np.inf)), gt)                         # one ulp above: dropped
    gt = np.where(k % 6 == 4, np.float32(0), gt)
    gt = np.where(k % 12 == 5, np.float32(np.inf), gt)
    gt = np.where(k % 12 == 11, np.float32(np.nan), gt)
    gt[:2] = 1.0
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd), np.ascontiguousarray(gt.astype(np.float32)), int(np.isnan(far).sum())


def filter_tiled(rays, n):
    ro, rd, gt = rays[:3]
    idx = np.arange(n) % len(ro)
    return np.ascontiguousarray(ro[idx]), np.ascontiguousarray(rd[idx]), np.ascontiguousarray(gt[idx])


# ---- 5. Tracker median --------------------------------------------------------------------------------------------------------------------
MEDIAN_COUNTS = [1, 2, 3, 4, 255, 256, 257, 1023, 1024, 1025, 5000, 16384]
MEDIAN_LISTS = ["distinct", "equal", "zero", "half", "middle-third", "outliers"]
MEDIAN_LIMIT = 16384
FUSED_COUNTS = [255, 256, 257, 1023, 1024, 250, 258]   # the switches of lower_median_x10 and the fused limit; at 250 and 258 (pairs, an even
                                                       # median rank) the median is the FIRST of its pair: the element below it differs
RES_UNIT = 2.0 ** -10           # residuals are whole multiples of this: |gt - depth| is exact in fp32 around the depth below
BASE_DEPTH = 256.0


def lower_median_x10(r, keep=None):
    """10 x sort(r)[(n - 1) // 2] over the kept rays in float32; no kept ray: +inf (every masked residual sorts as +inf)"""
    r = np.asarray(r, np.float32)
    if keep is not None:
        r = r[np.asarray(keep, bool)]
    if r.size == 0:
        return np.float32(np.inf)
    return np.float32(10.0) * np.sort(r)[(r.size - 1) // 2]


def planted_residuals(kind, N, seed=0):
    """whole-number residuals (units of RES_UNIT) of the named list, shuffled"""
    rng = np.random.default_rng(seed + N)
    i = np.arange(1, N + 1, dtype=np.int64)
    if kind == "distinct":
        k = np.where(i > N - N // 8, 10 * i, i)                           # the upper eighth lies beyond 10 x median
        med = int(np.sort(k)[(N - 1) // 2])
        if N >= 16:                                                        # one value ON the threshold (dropped: the test is strict), one just below
            k[-1], k[-2] = 10 * med, 10 * med - 1
    elif kind == "equal":
        k = np.full(N, 7, np.int64)
    elif kind == "zero":
        k = np.zeros(N, np.int64)
    elif kind == "half":
        k = (i > N // 2).astype(np.int64)                                  # N // 2 zeros: the lower median is 0 for even N, 1 for odd N
    elif kind == "middle-third":
        a = N // 3
        k = np.where(i <= a, i, np.where(i <= N - a, a + 5, 3 * i + 5))
    elif kind == "outliers":
        k = 100 + i
        if N >= 11:
            med = int(np.sort(k)[(N - 1) // 2])
            k[-5:] = 100 * med
    else:
        raise ValueError(kind)
    return rng.permutation(k)


def planted_batch(kind, N, seed=0):
    """depth, gt_depth (residual exact, sign alternating), var, rgb, gt_color with exact per-ray loss terms: sqrt(var + 1e-10) is 1, 0.5 or
    0.25 in fp32 (1e-10 is below half an ulp of each var), colour residuals are eighths, w_color = 0.5"""
    k = planted_residuals(kind, N, seed)
    rng = np.random.default_rng(1000 + seed + N)
    depth = np.full(N, BASE_DEPTH, np.float32)
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    big = k * RES_UNIT >= BASE_DEPTH - 1
    gt = (BASE_DEPTH + np.where(big, 1.0, sign) * k * RES_UNIT).astype(np.float32)
    if kind == "outliers" and N >= 16:
        gt[rng.permutation(N)[:2]] = 0.0                                   # no reading: residual = depth, in the median, never in the loss
    var = rng.choice(np.array([1.0, 0.25, 0.0625], np.float32), N)
    rgb = (rng.integers(0, 9, (N, 3)) / 8.0).astype(np.float32)
    gt_c = (rng.integers(0, 9, (N, 3)) / 8.0).astype(np.float32)
    assert np.array_equal(np.abs(gt.astype(np.float64) - depth), np.where(gt == 0, BASE_DEPTH, k * RES_UNIT))
    return dict(depth=depth, gt_depth=gt, var=var, rgb=rgb, gt_color=gt_c, w_color=0.5)


def track_terms64(B, keep=None, handle_dynamic=True, use_color=True, detach_var=False):
    """the Tracker loss of one batch from its definition: per-ray terms in float64, the counted set, the seed gradients"""
    d, gt, var = (B[k].astype(np.float64) for k in ("depth", "gt_depth", "var"))
    r32 = np.abs(B["gt_depth"] - B["depth"]).astype(np.float32)
    thr = lower_median_x10(r32, keep) if handle_dynamic else np.float32(np.inf)
    counted = (B["gt_depth"] > 0) & ((r32 < thr) if handle_dynamic else True)
    u = np.sqrt(var + 1e-10)
    res = gt - d
    rc = B["gt_color"].astype(np.float64) - B["rgb"].astype(np.float64)
    w = B["w_color"] if use_color else 0.0
    terms = np.where(counted, np.abs(res) / u + w * np.abs(rc).sum(1), 0.0)
    g_d = np.where(counted, -np.sign(res) / u, 0.0)
    g_v = np.where(counted & (not detach_var), -np.abs(res) / (2 * u ** 3), 0.0)
    g_c = np.where(counted[:, None], -w * np.sign(rc), 0.0)
    return dict(thr=thr, counted=counted, terms=terms, loss=float(terms.sum()), g_depth=g_d, g_var=g_v, g_rgb=g_c)


def check_track(loss, g_d, g_c, g_v, ref, label):
    n = len(ref["terms"])
    nonzero = ref["counted"] & (ref["g_depth"] != 0)            # a counted ray with a residual of exactly 0 has the gradient sign(0) = 0
    assert np.array_equal(np.asarray(g_d) != 0, nonzero), (label, int((np.asarray(g_d) != 0).sum()), int(nonzero.sum()))
    assert scenes.rel_l2(g_d, ref["g_depth"]) < 1e-6 and np.array_equal(np.asarray(g_c, np.float64), ref["g_rgb"]), label
    assert scenes.rel_l2(g_v, ref["g_var"]) < 1e-5, label
    assert abs(float(loss) - ref["loss"]) <= n * U32 * np.abs(ref["terms"]).sum(), (label, float(loss), ref["loss"])


def ray_mask(N):
    return (np.arange(N) % 3 != 0).astype(np.uint8)


_FUSED = {}


def fused_case(N, oracle, seed=33):
    """track_step batch with exact ties: N // 2 (even N) or N // 5 (odd N) distinct rays, each repeated.  The ground truth of a ray is the depth
    the scene renders for it (one fixed-point step with `oracle`, so that the residuals are centimetres, as in a tracked frame), zero depths
    stay zero, and five of the distinct rays have a ground truth off by 3 m so that the median really drops rays"""
    if N in _FUSED:
        return _FUSED[N]
    D = N // 2 if N % 2 == 0 else N // 5
    sc = scenes.make_scene(seed, scenes.SMALL_GRID_SHAPES, grid_std=0.3, bias_std=0.1)
    r = scenes.make_rays(seed + 1, D, sc["bound"], n_frames=1, zero_frac=0.1)
    fw = oracle.render_forward(oracle.opts(sc["bound"]), sc["grids"], sc["decoders"], "color", r["rays_o"], r["rays_d"], r["gt_depth"])
    gt = np.where(r["gt_depth"] > 0, fw["depth"], 0).astype(np.float32)
    off = np.flatnonzero(gt > 0)[3:8]
    gt[off] = gt[off] + np.float32(3.0)
    idx = np.arange(N) % D
    rays = dict(rays_o=np.ascontiguousarray(r["rays_o"][idx]), rays_d=np.ascontiguousarray(r["rays_d"][idx]), gt_depth=np.ascontiguousarray(gt[idx]),
                gt_color=np.ascontiguousarray(r["gt_color"][idx]))
    _FUSED[N] = (sc, rays, idx, off)
    return _FUSED[N]


def dropped_by_median(gt_depth, depth, keep=None):
    """(expected zero-gradient rows, rays within a relative 1e-5 of the threshold) from a rendered depth, in float32"""
    r = np.abs(np.asarray(gt_depth, np.float32) - np.asarray(depth, np.float32)).astype(np.float32)
    thr = lower_median_x10(r, keep)
    dropped = ~(r < thr) | (np.asarray(gt_depth) <= 0)
    near = np.abs(r.astype(np.float64) - float(thr)) <= 1e-5 * float(thr)
    return dropped, near, thr


# ---- 6. losses at exact zeros -----------------------------------------------------------------------------------------------------------------
LOSS_COUNTS = [1, 255, 256, 257, 1000]


def zero_batch(N, seed=0):
    """depth / colour residuals exactly zero on some rays, gt_depth = 0 on some, var = 0 and 1e-12 on some"""
    rng = np.random.default_rng(seed + N)
    depth, var = rng.uniform(0.5, 4, N).astype(np.float32), rng.uniform(1e-3, 0.5, N).astype(np.float32)
    rgb, gt_c = rng.uniform(0, 1, (N, 3)).astype(np.float32), rng.uniform(0, 1, (N, 3)).astype(np.float32)
    gt_d = (depth + rng.standard_normal(N) * 0.2).astype(np.float32)
    k = np.arange(N)
    gt_d[k % 5 == 0] = depth[k % 5 == 0]                                   # |.|'s gradient at 0 is 0
    gt_d[k % 7 == 3] = 0.0
    gt_c[k % 4 == 0] = rgb[k % 4 == 0]
    gt_c[k % 4 == 1, 1] = rgb[k % 4 == 1, 1]
    var[k % 6 == 0] = 0.0
    var[k % 6 == 1] = 1e-12
    return dict(depth=depth, var=var, rgb=rgb, gt_color=gt_c, gt_depth=gt_d)


# ---- ATen (torch on the CPU) where the operation is an ATen expression upstream --------------------------------------------------------------
def aten_filter(bound, ro, rd, gt):
    """src/Mapper.cpp:416-427, src/Tracker.cpp:48-58"""
    import torch
    b = torch.tensor(np.asarray(bound, np.float32))
    t_ = (b.unsqueeze(0) - torch.tensor(ro).unsqueeze(-1)) / torch.tensor(rd).unsqueeze(-1)
    t = torch.min(torch.max(t_, 2)[0], 1)[0]
    return (t >= torch.tensor(gt)).numpy()


def aten_median_x10(r, keep=None):
    import torch
    r = torch.tensor(np.asarray(r, np.float32))
    if keep is not None:
        r = r[torch.tensor(np.asarray(keep, bool))]
    return np.float32(np.inf) if r.numel() == 0 else (10 * r.median()).numpy()


def aten_loss_map(B, w_color, use_color):
    """src/Mapper.cpp:435-442 with autograd -> loss, d loss / d depth, d loss / d rgb"""
    import torch
    depth, rgb = torch.tensor(B["depth"], requires_grad=True), torch.tensor(B["rgb"], requires_grad=True)
    gt_d, gt_c = torch.tensor(B["gt_depth"]), torch.tensor(B["gt_color"])
    m = gt_d > 0
    loss = torch.abs(gt_d[m] - depth[m]).sum()
    if use_color:
        loss = loss + w_color * torch.abs(gt_c - rgb).sum()
    g_d, g_c = torch.autograd.grad(loss, (depth, rgb), allow_unused=True)
    z = lambda g, like: np.zeros(like.shape, np.float32) if g is None else g.numpy()
    return float(loss), z(g_d, depth), z(g_c, rgb)


def aten_loss_track(B, w_color, use_color, handle_dynamic, detach_var):
    """src/Tracker.cpp:67-82 with autograd -> loss, d loss / d depth, d loss / d rgb, d loss / d var"""
    import torch
    depth, rgb = torch.tensor(B["depth"], requires_grad=True), torch.tensor(B["rgb"], requires_grad=True)
    var = torch.tensor(B["var"], requires_grad=not detach_var)
    gt_d, gt_c = torch.tensor(B["gt_depth"]), torch.tensor(B["gt_color"])
    if handle_dynamic:
        tmp = torch.abs(gt_d - depth).detach()
        m = (tmp < 10 * tmp.median()) & (gt_d > 0)
    else:
        m = gt_d > 0
    loss = (torch.abs(gt_d - depth) / torch.sqrt(var + 1e-10))[m].sum()
    if use_color:
        loss = loss + w_color * torch.abs(gt_c - rgb)[m].sum()
    if not m.any():
        return 0.0, np.zeros(depth.shape, np.float32), np.zeros(rgb.shape, np.float32), np.zeros(var.shape, np.float32)
    gs = torch.autograd.grad(loss, (depth, rgb) + (() if detach_var else (var,)), allow_unused=True)
    z = lambda g, like: np.zeros(like.shape, np.float32) if g is None else g.numpy()
    return float(loss), z(gs[0], depth), z(gs[1], rgb), (np.zeros(var.shape, np.float32) if detach_var else z(gs[2], var))


def check_loss_grads(got, ref, label):
    """elementwise, to the tolerances tests/test_gpu_parity.py::test_losses_and_pose_kernels uses for the vectors; signs exact"""
    g_d, g_c, g_v = (np.asarray(a, np.float64) for a in got)
    r_d, r_c, r_v = (np.asarray(a, np.float64) for a in ref)
    assert np.array_equal(np.sign(g_d), np.sign(r_d)) and np.array_equal(g_c, r_c), label
    assert (np.abs(g_d - r_d) <= 1e-6 * np.abs(r_d)).all(), label
    if g_v is not None and r_v is not None and g_v.shape == r_v.shape:
        assert np.array_equal(np.sign(g_v), np.sign(r_v)) and (np.abs(g_v - r_v) <= 1e-5 * np.abs(r_v)).all(), label

"""ctypes binding of the C-ABI in include/nsk.h (libnsk.so, built from csrc/ for gfx950).

There is no CPU fallback: if the HIP library is missing or no MI355X is present, creating a context raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("NSK_LIB", os.path.join(_HERE, "csrc", "libnsk.so"))

STAGES = {"coarse": 0, "middle": 1, "fine": 2, "color": 3}
LEVELS = ("coarse", "middle", "fine", "color")
GRAD_GRIDS, GRAD_DECODERS, GRAD_RAYS = 1, 2, 4
GROUP_DECODERS, GROUP_COARSE, GROUP_MIDDLE, GROUP_FINE, GROUP_COLOR, GROUP_CAMERA = range(6)

# every symbol include/nsk.h declares
SYMBOLS = (
    "nsk_last_error", "nsk_version", "nsk_ctx_create", "nsk_ctx_destroy", "nsk_sync", "nsk_stream", "nsk_set_bound",
    "nsk_set_render_opts", "nsk_set_matmul_mode", "nsk_set_sort_mode", "nsk_set_tuning", "nsk_set_ray_mask", "nsk_grid_upload", "nsk_grid_download", "nsk_grid_grad_download", "nsk_set_mask", "nsk_frustum_mask", "nsk_keyframe_overlap", "nsk_sample_pixels", "nsk_gather_pixels", "nsk_rays_from_camera", "nsk_pose_step",
    "nsk_decoder_param_count", "nsk_decoder_upload", "nsk_decoder_download", "nsk_decoder_grad_download",
    "nsk_decoder_set_trainable", "nsk_render_forward", "nsk_eval_points", "nsk_raw2outputs", "nsk_render_backward", "nsk_map_step",
    "nsk_track_step", "nsk_loss_map", "nsk_loss_track", "nsk_rays_from_pixels", "nsk_rays_backward",
    "nsk_camera_from_tensor", "nsk_camera_backward", "nsk_inside_filter", "nsk_adam_vector", "nsk_adam_step",
    "nsk_adam_reset", "nsk_graph_begin", "nsk_graph_end", "nsk_graph_launch", "nsk_graph_destroy", "nsk_zero_grads", "nsk_prepare_rays", "nsk_map_prepare", "nsk_grad_slab", "nsk_grad_pack", "nsk_grad_unpack", "nsk_allreduce_grads", "nsk_last_call_stats",
    "nsk_profile_begin", "nsk_profile_end", "nsk_debug_relu_bits", "nsk_debug_preact", "nsk_debug_fetch", "nsk_debug_live_tiles", "nsk_debug_last_split",
    "nsk_debug_decoder_images", "nsk_decoder_image_table",
    "nsk_pose_step_multi", "nsk_set_depth_max_batch", "nsk_grad_extra", "nsk_set_backward_mode",
    "nsk_eval_lattice", "nsk_eval_lattice_masked", "nsk_mesh_extract", "nsk_mesh_buffers", "nsk_mesh_download", "nsk_mesh_table",
    "nsk_lattice_seen", "nsk_mesh_filter",
    "nsk_image_rays", "nsk_render_image", "nsk_image_metrics", "nsk_image_ssim",
    "nsk_mesh_sample", "nsk_cloud_nearest", "nsk_cloud_stats", "nsk_mesh_nearest", "nsk_normal_stats",
    "nsk_cloud_pair_sums", "nsk_rigid_from_sums", "nsk_cloud_icp", "nsk_cloud_transform",
    "nsk_mesh_depth", "nsk_depth_pair_stats", "nsk_depth_views", "nsk_depth_views_range",
    "nsk_points_seen", "nsk_mesh_select", "nsk_points_view_counts",
    "nsk_tsdf_integrate", "nsk_tsdf_volume",
    "nsk_mesh_vertex_normals", "nsk_normal_rays", "nsk_mesh_vertex_colors",
    "nsk_frame_plan", "nsk_frame_prepare",
    "nsk_set_importance", "nsk_get_importance", "nsk_importance_resample",
    "nsk_points_hull", "nsk_hull_download", "nsk_hull_upload", "nsk_lattice_in_hull",
    "nsk_mesh_simplify", "nsk_mesh_simplify_list_threshold",
)

FRAME_U8, FRAME_U16, FRAME_F32 = 0, 1, 2


class FrameOpts(C.Structure):
    """nsk_frame_opts of include/nsk.h"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("n_dist", C.c_int), ("dist", C.c_float * 8),
                ("crop_H", C.c_int), ("crop_W", C.c_int), ("crop_edge", C.c_int), ("png_depth_scale", C.c_float), ("scale", C.c_float),
                ("swap_rb", C.c_int)]


def frame_opts(intr, distortion=None, crop_size=None, crop_edge=0, png_depth_scale=1.0, scale=1.0, swap_rb=False):
    """the options of frame_plan / Context.prepare_frames as an nsk_frame_opts; intr = (fx, fy, cx, cy) for the depth size"""
    o = FrameOpts()
    o.fx, o.fy, o.cx, o.cy = (float(v) for v in intr)
    dist = [] if distortion is None else [float(v) for v in distortion]
    o.n_dist = len(dist)
    for i, v in enumerate(dist[:8]):
        o.dist[i] = v
    o.crop_H, o.crop_W = (0, 0) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    o.crop_edge = int(crop_edge)
    o.png_depth_scale, o.scale, o.swap_rb = float(png_depth_scale), float(scale), int(bool(swap_rb))
    return o


SSIM_TILE = (8, 32)          # windows per workgroup of nsk_image_ssim's tile kernel, rows x columns (csrc/nsk_ssim.h: SSIM_TILE_H, SSIM_TILE_W)


class NskError(RuntimeError):
    pass


def build(force=False):
    """compile csrc/ for gfx950 (hipcc cross-compiles without a GPU)"""
    # staleness is make's business: csrc/Makefile lists every source and header of the library
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")] + (["-B"] if force else []) + ["all"])
    return _LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NskError("libnsk.so is not built (%s); run __graft_entry__.build() -- there is no fallback path" % _LIB_PATH)
        try:
            import torch  # noqa: F401  -- first: torch ships its own HIP runtime; when libnsk.so is loaded before it, two runtimes end up in the process and
        except Exception:             # nsk_ctx_create sees no device although torch.cuda does (build() followed by smoke() in one process showed it)
            pass
        L = C.CDLL(_LIB_PATH)
        L.nsk_last_error.restype = C.c_char_p
        L.nsk_decoder_param_count.restype = C.c_size_t
        L.nsk_decoder_param_count.argtypes = [C.c_int]
        L.nsk_stream.restype = C.c_void_p
        L.nsk_stream.argtypes = [C.c_void_p]
        L.nsk_eval_lattice_masked.restype = C.c_int
        L.nsk_eval_lattice_masked.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                              C.c_void_p, C.POINTER(C.c_longlong)]
        L.nsk_mesh_sample.restype = C.c_int
        L.nsk_mesh_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.nsk_cloud_nearest.restype = C.c_int
        L.nsk_cloud_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.nsk_cloud_stats.restype = C.c_int
        L.nsk_cloud_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_double)]
        L.nsk_mesh_nearest.restype = C.c_int
        L.nsk_mesh_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_int)]
        L.nsk_normal_stats.restype = C.c_int
        L.nsk_normal_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        PD = C.POINTER(C.c_double)
        L.nsk_cloud_pair_sums.restype = C.c_int
        L.nsk_cloud_pair_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, PD, C.c_float, PD, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int)]
        L.nsk_rigid_from_sums.restype = C.c_int
        L.nsk_rigid_from_sums.argtypes = [PD, PD, C.POINTER(C.c_int)]
        L.nsk_cloud_icp.restype = C.c_int
        L.nsk_cloud_icp.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_double, C.c_double, PD, PD, PD]
        L.nsk_cloud_transform.restype = C.c_int
        L.nsk_cloud_transform.argtypes = [C.c_void_p, PD, C.c_void_p, C.c_int, C.c_void_p]
        L.nsk_mesh_depth.restype = C.c_int
        L.nsk_mesh_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                     C.c_float, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int)]
        L.nsk_depth_pair_stats.restype = C.c_int
        L.nsk_depth_pair_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.nsk_depth_views.restype = C.c_int
        L.nsk_depth_views.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_ulonglong, C.c_double, C.c_int, C.c_void_p]
        L.nsk_depth_views_range.restype = C.c_int
        L.nsk_depth_views_range.argtypes = [C.c_void_p, C.c_ulonglong, C.c_double, C.c_longlong, C.c_int, C.c_void_p]
        L.nsk_points_seen.restype = C.c_int
        L.nsk_points_seen.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
        L.nsk_mesh_select.restype = C.c_int
        L.nsk_mesh_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.nsk_points_view_counts.restype = C.c_int
        L.nsk_points_view_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                             C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.nsk_tsdf_integrate.restype = C.c_int
        L.nsk_tsdf_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
        L.nsk_tsdf_volume.restype = C.c_int
        L.nsk_tsdf_volume.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
        L.nsk_frame_plan.restype = C.c_int
        L.nsk_frame_plan.argtypes = [C.POINTER(FrameOpts), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
        L.nsk_frame_prepare.restype = C.c_int
        L.nsk_frame_prepare.argtypes = [C.c_void_p, C.POINTER(FrameOpts), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.nsk_mesh_vertex_normals.restype = C.c_int
        L.nsk_mesh_vertex_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.nsk_normal_rays.restype = C.c_int
        L.nsk_normal_rays.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nsk_mesh_vertex_colors.restype = C.c_int
        L.nsk_mesh_vertex_colors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.nsk_image_ssim.restype = C.c_int
        L.nsk_image_ssim.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.c_int, PD, C.c_void_p, PD, PD]
        L.nsk_set_importance.restype = C.c_int
        L.nsk_set_importance.argtypes = [C.c_void_p, C.c_int]
        L.nsk_get_importance.restype = C.c_int
        L.nsk_get_importance.argtypes = [C.c_void_p]
        L.nsk_importance_resample.restype = C.c_int
        L.nsk_importance_resample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_void_p]
        L.nsk_points_hull.restype = C.c_int
        L.nsk_points_hull.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
        L.nsk_hull_download.restype = C.c_int
        L.nsk_hull_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nsk_hull_upload.restype = C.c_int
        L.nsk_hull_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.nsk_lattice_in_hull.restype = C.c_int
        L.nsk_lattice_in_hull.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_longlong)]
        L.nsk_mesh_simplify.restype = C.c_int
        L.nsk_mesh_simplify.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        L.nsk_mesh_simplify_list_threshold.restype = C.c_int
        L.nsk_mesh_simplify_list_threshold.argtypes = []
        L.nsk_decoder_image_table.restype = C.c_int
        L.nsk_decoder_image_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise NskError(lib().nsk_last_error().decode())


def _ptr(t):
    """device pointer of a contiguous torch CUDA tensor (or None)"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous CUDA tensor"
    return C.c_void_p(t.data_ptr())


def simplify_list_threshold():
    """the longest smallest-corner list one thread of nsk_mesh_simplify searches (a longer one takes a workgroup); needs no GPU"""
    return int(lib().nsk_mesh_simplify_list_threshold())


def mesh_table(case):
    """the triangles of one of the 256 corner-sign cases as a list of edge triples (numbering: include/nsk.h); needs no GPU"""
    buf = (C.c_int8 * 64)()
    n = lib().nsk_mesh_table(int(case), buf, 64)
    if n < 0:
        raise NskError(lib().nsk_last_error().decode())
    return [(int(buf[3 * t]), int(buf[3 * t + 1]), int(buf[3 * t + 2])) for t in range(n)]


def decoder_image_table(which, what, pieces=2):
    """int32 array: the index table of image `what` (a name of Context.DECODER_IMAGES or its index) of decoder `which` (include/nsk.h: how the
    image follows from it); empty for an image the decoder does not have; needs no GPU"""
    import numpy as np
    w = STAGES[which] if isinstance(which, str) else int(which)
    code = Context.DECODER_IMAGES.index(what) if isinstance(what, str) else int(what)
    n = lib().nsk_decoder_image_table(w, code, int(pieces), None, 0)
    out = np.zeros(max(n, 0), np.int32)
    if n < 0 or lib().nsk_decoder_image_table(w, code, int(pieces), out.ctypes.data_as(C.c_void_p), out.size) != n:
        raise NskError(lib().nsk_last_error().decode())
    return out


def frame_plan(color_size, depth_size, intr, distortion=None, crop_size=None, crop_edge=0, png_depth_scale=1.0, scale=1.0, swap_rb=False):
    """nsk_frame_plan: what Context.prepare_frames will give for raw colour images of color_size (H, W) and depth images of depth_size,
    intr = (fx, fy, cx, cy) for the depth size -> (H', W', intr_out [4] float32); an invalid option set raises NskError; needs no GPU"""
    import numpy as np
    o = frame_opts(intr, distortion, crop_size, crop_edge, png_depth_scale, scale, swap_rb)
    H, W, out = C.c_int(0), C.c_int(0), (C.c_float * 4)()
    _chk(lib().nsk_frame_plan(C.byref(o), int(color_size[0]), int(color_size[1]), int(depth_size[0]), int(depth_size[1]), C.byref(H), C.byref(W), out))
    return int(H.value), int(W.value), np.array(list(out), np.float32)


def depth_views_from_box(box, n_views, seed=0, shrink=0.7):
    """nsk_depth_views on a given box (lo x y z, hi x y z): the world-to-camera matrices [n_views, 4, 4] float32; needs no GPU"""
    import numpy as np
    b = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(6))
    w = np.zeros((int(n_views), 4, 4), np.float32)
    _chk(lib().nsk_depth_views(None, None, 0, b.ctypes.data_as(C.c_void_p), int(seed) & 0xFFFFFFFFFFFFFFFF, float(shrink), int(n_views),
                               w.ctypes.data_as(C.c_void_p)))
    return w


def depth_views_range(box, first, n_views, seed=0, shrink=0.7):
    """nsk_depth_views_range: views first .. first + n_views - 1 of the stream depth_views draws from the box (lo x y z, hi x y z) -> w2c
    [n_views, 4, 4] float32; needs no GPU"""
    import numpy as np
    b = np.ascontiguousarray(np.asarray(box, dtype=np.float32).reshape(6))
    w = np.zeros((int(n_views), 4, 4), np.float32)
    _chk(lib().nsk_depth_views_range(b.ctypes.data_as(C.c_void_p), int(seed) & 0xFFFFFFFFFFFFFFFF, float(shrink), int(first), int(n_views),
                                     w.ctypes.data_as(C.c_void_p)))
    return w


def rigid_from_sums(sums):
    """nsk_rigid_from_sums: the rigid update [4, 4] float64 that best maps s' onto t from the 17 pair sums, and the numerical rank of the
    covariance (include/nsk.h: the rigid solve); needs no GPU"""
    import numpy as np
    h = (C.c_double * 17)(*[float(x) for x in np.asarray(sums, np.float64).reshape(17)])
    U = (C.c_double * 16)()
    rank = C.c_int(0)
    _chk(lib().nsk_rigid_from_sums(h, U, C.byref(rank)))
    return np.array(U[:], np.float64).reshape(4, 4), int(rank.value)


def _mat16(M):
    """a 4x4 (anything numpy reads) as the 16 doubles of the C ABI, or None"""
    if M is None:
        return None
    import numpy as np
    return (C.c_double * 16)(*[float(x) for x in np.asarray(M, np.float64).reshape(16)])


def _w2c16(w2c, K=-1):
    """world-to-camera matrices (anything numpy reads) as contiguous float32 [K, 16] and its pointer for the C ABI (None without a frame)"""
    import numpy as np
    w = np.ascontiguousarray(np.asarray(w2c, dtype=np.float32).reshape(K, 16))
    return w, (w.ctypes.data_as(C.c_void_p) if w.shape[0] else None)


def _intr4(intr):
    """(fx, fy, cx, cy) as the four floats of the C ABI (c_float: right with and without declared argument types)"""
    fx, fy, cx, cy = [C.c_float(float(x)) for x in intr]
    return fx, fy, cx, cy


def _vec3(v):
    """origin / step as contiguous float32 [3] and its pointer for the C ABI"""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(v, np.float32).reshape(3))
    return a, a.ctypes.data_as(C.c_void_p)


def _stage(s):
    return STAGES[s] if isinstance(s, str) else int(s)


class _CudaArray:
    """__cuda_array_interface__ view of a raw device pointer so that torch can wrap context-owned memory"""

    def __init__(self, ptr, n, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _ordered(fn):
    """order the context stream against torch's current stream around a launching call"""
    import functools

    @functools.wraps(fn)
    def wrap(self, *a, **k):
        import torch
        cur = torch.cuda.current_stream(self.device)
        same = cur == self.tstream
        if not same:
            self.tstream.wait_stream(cur)
        try:
            return fn(self, *a, **k)
        finally:
            if not same:
                cur.wait_stream(self.tstream)
    return wrap


class Context:
    """one nsk_ctx (one GPU, one HIP stream)"""

    def __init__(self, device=0, stream=None):
        """stream: a torch.cuda.Stream to launch on (default: a new one).  Every launching method orders the
        context's stream after torch's current stream and the current stream after the launch, so results are
        safe to consume with ordinary torch ops; run under `with torch.cuda.stream(ctx.tstream)` to avoid the
        two event waits per call."""
        import torch
        self.h = C.c_void_p()
        self.device = int(device)
        self.last_evaluated = None              # nodes the last eval_lattice with a mask decoded
        lib()
        if torch.cuda.is_available():
            self.tstream = stream if stream is not None else torch.cuda.Stream(self.device)
            handle = C.c_void_p(self.tstream.cuda_stream)
        else:
            self.tstream, handle = None, None
        _chk(lib().nsk_ctx_create(self.device, handle, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().nsk_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------------------------------
    def set_bound(self, bound):
        import numpy as np
        b = np.ascontiguousarray(np.asarray(bound, dtype=np.float32).reshape(6))
        _chk(lib().nsk_set_bound(self.h, b.ctypes.data_as(C.c_void_p)))

    def set_render_opts(self, n_samples=32, n_surface=16, lindisp=False, perturb=0.0, occupancy=False, seed=0):
        _chk(lib().nsk_set_render_opts(self.h, n_samples, n_surface, int(lindisp), C.c_float(perturb), int(occupancy),
                                       C.c_uint64(seed)))
        self.n_samples, self.n_surface = n_samples, n_surface

    def set_matmul_mode(self, mode):
        _chk(lib().nsk_set_matmul_mode(self.h, int(mode)))

    def set_importance(self, n):
        """nsk_set_importance: n extra depths per ray drawn from the compositing weights of a first pass (rendering.N_importance; 0: one
        pass).  Every renderer of the context then returns the second pass over n_samples (+ n_surface) + n samples per ray."""
        _chk(lib().nsk_set_importance(self.h, int(n)))
        self.n_importance = int(n)

    def get_importance(self):
        """nsk_get_importance: the installed n_importance"""
        return int(lib().nsk_get_importance(self.h))

    def set_ray_mask(self, keep):
        """uint8 cuda tensor [N] (or None): rays with keep == 0 take no part in the loss, its gradients and the batch statistics"""
        self._ray_mask = keep                     # keep the tensor alive while the context points at it
        _chk(lib().nsk_set_ray_mask(self.h, _ptr(keep) if keep is not None else None))

    def set_backward_mode(self, mode):
        """0: every backward chain on the fp32 MFMA (full-width operands; a measuring stick), 2 (default): two fp16 pieces"""
        _chk(lib().nsk_set_backward_mode(self.h, int(mode)))

    def set_sort_mode(self, mode):
        """-1 automatic, 0 ray order, 1 cell-sorted (include/nsk.h)"""
        _chk(lib().nsk_set_sort_mode(self.h, int(mode)))

    def set_tuning(self, key, value):
        _chk(lib().nsk_set_tuning(self.h, key.encode(), int(value)))

    def sync(self):
        _chk(lib().nsk_sync(self.h))

    # -- grids / decoders (host numpy in the reference layouts) ------------------------------------------
    def grid_upload(self, level, arr):
        import numpy as np
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        if a.ndim == 5:
            a = a[0]
        Cc, Z, Y, X = a.shape
        _chk(lib().nsk_grid_upload(self.h, _stage(level), a.ctypes.data_as(C.c_void_p), Cc, Z, Y, X))
        if not hasattr(self, "_gshape"):
            self._gshape = {}
        self._gshape[_stage(level)] = (Cc, Z, Y, X)

    def grid_download(self, level, grad=False):
        import numpy as np
        out = np.zeros(self._gshape[_stage(level)], np.float32)
        f = lib().nsk_grid_grad_download if grad else lib().nsk_grid_download
        _chk(f(self.h, _stage(level), out.ctypes.data_as(C.c_void_p)))
        return out

    def set_mask(self, level, mask):
        import numpy as np
        if mask is None:
            _chk(lib().nsk_set_mask(self.h, _stage(level), None))
            return
        m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        _chk(lib().nsk_set_mask(self.h, _stage(level), m.ctypes.data_as(C.c_void_p)))

    @_ordered
    def frustum_mask(self, level, depth_img, intr, c2w):
        """Mapper::get_mask_from_c2w on the device; installs the mask and returns it as bool [Z,Y,X]"""
        import numpy as np
        H, W = depth_img.shape
        Cc, Z, Y, X = self._gshape[_stage(level)]
        m = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(4, 4))
        out = np.zeros(Z * Y * X, np.uint8)
        fx, fy, cx, cy = intr
        _chk(lib().nsk_frustum_mask(self.h, _stage(level), _ptr(depth_img), H, W, C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                    C.c_float(cy), m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out.reshape(Z, Y, X).astype(bool)

    @_ordered
    def sample_pixels(self, seed, n, H0, H1, W0, W1):
        """raySampler's pixel draw on the device -> (pix_i cols, pix_j rows) int32 cuda tensors"""
        import torch
        pi = torch.empty(n, dtype=torch.int32, device="cuda:%d" % self.device)
        pj = torch.empty_like(pi)
        _chk(lib().nsk_sample_pixels(self.h, C.c_ulonglong(seed), n, H0, H1, W0, W1, _ptr(pi), _ptr(pj)))
        return pi, pj

    @_ordered
    def prepare_rays(self, frames, rays_per_frame, window, intr, mode=0, want_keep=True):
        """nsk_prepare_rays: pixel draw + ground-truth gather + ray generation + inside filter for a list of frames in one launch.
        frames: list of dicts {depth [H,W] cuda, color [H,W,3] cuda or None, pose cuda (12 floats c2w or 7 floats), seed};
        window = (H0, H1, W0, W1); returns dict of cuda tensors (pix_i, pix_j, gt_depth, gt_color, rays_o, rays_d, keep)"""
        import torch

        class FrameRays(C.Structure):
            _fields_ = [("d_depth", C.c_void_p), ("d_color", C.c_void_p), ("d_pose", C.c_void_p), ("pose_is_cam7", C.c_int), ("seed", C.c_ulonglong)]
        nf = len(frames)
        tab = (FrameRays * nf)()
        H, W = frames[0]["depth"].shape
        for k, f in enumerate(frames):
            tab[k].d_depth = f["depth"].data_ptr()
            tab[k].d_color = f["color"].data_ptr() if f.get("color") is not None else None
            tab[k].d_pose = f["pose"].data_ptr()
            tab[k].pose_is_cam7 = 1 if f["pose"].numel() == 7 else 0
            tab[k].seed = int(f["seed"])
        n = nf * rays_per_frame
        dev = frames[0]["depth"].device
        out = dict(pix_i=torch.empty(n, dtype=torch.int32, device=dev), pix_j=torch.empty(n, dtype=torch.int32, device=dev),
                   gt_depth=torch.empty(n, dtype=torch.float32, device=dev), gt_color=torch.empty((n, 3), dtype=torch.float32, device=dev),
                   rays_o=torch.empty((n, 3), dtype=torch.float32, device=dev), rays_d=torch.empty((n, 3), dtype=torch.float32, device=dev),
                   keep=torch.empty(n, dtype=torch.uint8, device=dev) if want_keep else None)
        has_color = all(f.get("color") is not None for f in frames)
        H0, H1, W0, W1 = window
        fx, fy, cx, cy = intr
        _chk(lib().nsk_prepare_rays(self.h, nf, tab, rays_per_frame, H0, H1, W0, W1, H, W, C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), mode,
                                    _ptr(out["pix_i"]), _ptr(out["pix_j"]), _ptr(out["gt_depth"]), _ptr(out["gt_color"]) if has_color else None,
                                    _ptr(out["rays_o"]), _ptr(out["rays_d"]), _ptr(out["keep"]) if want_keep else None))
        return out

    @_ordered
    def gather_pixels(self, pix_i, pix_j, depth_img, color_img=None):
        import torch
        n = pix_i.shape[0]
        H, W = depth_img.shape
        gd = torch.empty(n, dtype=torch.float32, device=depth_img.device)
        gc = torch.empty((n, 3), dtype=torch.float32, device=depth_img.device) if color_img is not None else None
        _chk(lib().nsk_gather_pixels(self.h, n, _ptr(pix_i), _ptr(pix_j), H, W, _ptr(depth_img), _ptr(color_img) if color_img is not None else None,
                                     _ptr(gd), _ptr(gc) if gc is not None else None))
        return gd, gc

    @_ordered
    def keyframe_overlap(self, rays_o, rays_d, gt_depth, intr, HW, c2w_list, n_samples=16):
        """Mapper::keyframe_selection_overlap: fraction of the frame's sample points seen by each keyframe -> float32 [K]"""
        import numpy as np
        m = np.ascontiguousarray(np.asarray(c2w_list, dtype=np.float32).reshape(-1, 16))
        out = np.zeros(m.shape[0], np.float32)
        fx, fy, cx, cy = intr
        _chk(lib().nsk_keyframe_overlap(self.h, rays_o.shape[0], _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth), n_samples, int(HW[0]), int(HW[1]),
                                        C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), m.shape[0], m.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def decoder_upload(self, which, packed):
        import numpy as np
        p = np.ascontiguousarray(np.asarray(packed, dtype=np.float32).reshape(-1))
        _chk(lib().nsk_decoder_upload(self.h, _stage(which), p.ctypes.data_as(C.c_void_p), C.c_size_t(p.size)))

    def decoder_download(self, which, grad=False):
        import numpy as np
        n = lib().nsk_decoder_param_count(_stage(which))
        out = np.zeros(n, np.float32)
        f = lib().nsk_decoder_grad_download if grad else lib().nsk_decoder_download
        _chk(f(self.h, _stage(which), out.ctypes.data_as(C.c_void_p), C.c_size_t(n)))
        return out

    def decoder_set_trainable(self, which, flag):
        _chk(lib().nsk_decoder_set_trainable(self.h, _stage(which), int(flag)))

    def load_scene(self, bound, grids, decoders):
        self.set_bound(bound)
        for k in LEVELS:
            if k in grids and grids[k] is not None:
                self.grid_upload(k, grids[k])
            if k in decoders and decoders[k] is not None:
                self.decoder_upload(k, decoders[k])

    # -- rendering (torch CUDA tensors in, torch CUDA tensors out) ------------------------------------------
    def _S(self, gt_depth):
        return getattr(self, "n_samples", 32) + (getattr(self, "n_surface", 16) if gt_depth is not None else 0) + getattr(self, "n_importance", 0)

    @_ordered
    def render_forward(self, stage, rays_o, rays_d, gt_depth=None, gt_depth_max=-1.0, want_weights=True):
        import torch
        N = rays_o.shape[0]
        dev = rays_o.device
        rgb = torch.empty(N, 3, device=dev); depth = torch.empty(N, device=dev); var = torch.empty(N, device=dev)
        w = torch.empty(N, self._S(gt_depth), device=dev) if want_weights else None
        _chk(lib().nsk_render_forward(self.h, _stage(stage), N, _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth),
                                      C.c_float(gt_depth_max), _ptr(rgb), _ptr(depth), _ptr(var), _ptr(w)))
        return rgb, depth, var, w

    # -- whole frames ----------------------------------------------------------------------------------------
    # Python default of render_image's chunk_rays: the smallest chunk within 3 % of the best frame time at 680 x 1200
    CHUNK_RAYS = 25600

    @staticmethod
    def view_shape(HW, window=None, stride=1):
        """(Hv, Wv) of the view: window = (H0, H1, W0, W1) (default: the whole image), every stride-th pixel"""
        H0, H1, W0, W1 = window if window is not None else (0, int(HW[0]), 0, int(HW[1]))
        return (H1 - H0 + stride - 1) // stride, (W1 - W0 + stride - 1) // stride

    @_ordered
    def image_rays(self, HW, intr, pose, depth_img=None, window=None, stride=1, first=0, n=None, mode=0):
        """nsk_image_rays: rays (and gathered depth) of view pixels [first, first + n) from pose (cuda tensor: 12 floats c2w or the
        7-vector) + intrinsics + image size -> (rays_o [n, 3], rays_d [n, 3], gt_depth [n] or None)"""
        import torch
        H, W = int(HW[0]), int(HW[1])
        H0, H1, W0, W1 = window if window is not None else (0, H, 0, W)
        if n is None:
            Hv, Wv = self.view_shape(HW, window, max(int(stride), 1))
            n = Hv * Wv - first
        dev = pose.device
        ro = torch.empty(max(n, 0), 3, device=dev); rd = torch.empty(max(n, 0), 3, device=dev)
        gd = torch.empty(max(n, 0), device=dev) if depth_img is not None else None
        fx, fy, cx, cy = intr
        _chk(lib().nsk_image_rays(self.h, int(first), int(n), int(H0), int(H1), int(W0), int(W1), int(stride), H, W, C.c_float(fx), C.c_float(fy),
                                  C.c_float(cx), C.c_float(cy), _ptr(pose), 1 if pose.numel() == 7 else 0, int(mode), _ptr(depth_img),
                                  _ptr(ro), _ptr(rd), _ptr(gd)))
        return ro, rd, gd

    @_ordered
    def render_image(self, stage, HW, intr, pose, depth_img=None, window=None, stride=1, gt_depth_max=-1.0, chunk_rays=None, mode=0):
        """nsk_render_image: the view rendered from the map -> (rgb [Hv, Wv, 3], depth [Hv, Wv], var [Hv, Wv]) cuda tensors.
        gt_depth_max < 0: every chunk of chunk_rays pixels is a batch of its own with its own max(gt_depth), as upstream's render_img
        (the frame then depends on chunk_rays); >= 0: that value for every chunk.  depth_img None: no ground truth."""
        import torch
        H, W = int(HW[0]), int(HW[1])
        H0, H1, W0, W1 = window if window is not None else (0, H, 0, W)
        Hv, Wv = self.view_shape(HW, window, max(int(stride), 1))
        dev = pose.device
        rgb = torch.empty(max(Hv, 0), max(Wv, 0), 3, device=dev); depth = torch.empty(max(Hv, 0), max(Wv, 0), device=dev); var = torch.empty_like(depth)
        fx, fy, cx, cy = intr
        _chk(lib().nsk_render_image(self.h, _stage(stage), int(H0), int(H1), int(W0), int(W1), int(stride), H, W, C.c_float(fx), C.c_float(fy),
                                    C.c_float(cx), C.c_float(cy), _ptr(pose), 1 if pose.numel() == 7 else 0, int(mode), _ptr(depth_img),
                                    C.c_float(gt_depth_max), int(self.CHUNK_RAYS if chunk_rays is None else chunk_rays), _ptr(rgb), _ptr(depth), _ptr(var)))
        return rgb, depth, var

    @_ordered
    def image_metrics(self, rgb, depth, gt_depth=None, gt_color=None, want_residuals=False):
        """nsk_image_metrics: residual sums of a rendered frame against the input frame -> dict with the counts and sums of include/nsk.h
        (pixels, depth_pixels, depth_sum, color_terms, color_sum, nonfinite), h_out (the eight doubles), depth_l1 = depth_sum / depth_pixels
        and psnr = -10 log10(color_sum / color_terms) formed on the host in double (None without the ground truth or without a term),
        and with want_residuals res_depth [Hv, Wv] / res_color [Hv, Wv, 3] (cuda tensors; None without the ground truth).  Synchronises."""
        import math
        import torch
        Hv, Wv = depth.shape
        res_d = torch.empty_like(depth) if want_residuals and gt_depth is not None else None
        res_c = torch.empty_like(rgb) if want_residuals and gt_color is not None else None
        h = (C.c_double * 8)()
        _chk(lib().nsk_image_metrics(self.h, int(Hv), int(Wv), _ptr(rgb), _ptr(depth), _ptr(gt_depth), _ptr(gt_color), _ptr(res_d), _ptr(res_c), h))
        h = [float(x) for x in h]
        out = dict(h_out=h, pixels=int(h[0]), depth_pixels=int(h[1]), depth_sum=h[2], color_terms=int(h[3]), color_sum=h[4], nonfinite=int(h[5]))
        out["depth_l1"] = h[2] / h[1] if h[1] > 0 else None
        out["psnr"] = (-10.0 * math.log10(h[4] / h[3]) if h[4] > 0 else math.inf) if h[3] > 0 else None
        if want_residuals:
            out["res_depth"], out["res_color"] = res_d, res_c
        return out

    def image_ssim(self, a, b, data_range=1.0, win=11, sigma=1.5, k1=0.01, k2=0.03, levels=1, weights=None, want_map=False):
        """nsk_image_ssim: structural similarity of two images ([H, W] or [H, W, C], C <= 4; tensors anywhere or numpy arrays) -> dict with
        ssim (the level-0 SSIM), ms_ssim (None when levels = 1), per_level (numpy [levels, C, 4]: the sum of ssim, the sum of cs, the windows
        counted, the value the level contributes), left_out (windows with a non-finite value), map (with want_map the level-0 ssim of every
        window, a float32 cuda tensor [Hm, Wm] or [Hm, Wm, C]; else None) and h_out (the eight doubles of include/nsk.h).  weights: one per
        level; None only for levels = 1, or 5 with the standard weights.  Synchronises."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        # (moved and converted on torch's current stream, before the context's stream is ordered behind it)
        a, b = ((t if torch.is_tensor(t) else torch.tensor(np.asarray(t, dtype=np.float32))).to(device=dev, dtype=torch.float32).contiguous() for t in (a, b))
        if a.shape != b.shape or a.dim() not in (2, 3):
            raise NskError("image_ssim: a and b must have one shape, [H, W] or [H, W, C] (got %s and %s)" % (tuple(a.shape), tuple(b.shape)))
        if weights is not None and len(weights) != int(levels):
            raise NskError("image_ssim: weights has %d entries for levels = %d" % (len(weights), int(levels)))
        return self._image_ssim(a, b, float(data_range), int(win), float(sigma), float(k1), float(k2), int(levels), weights, want_map)

    @_ordered
    def _image_ssim(self, a, b, data_range, win, sigma, k1, k2, levels, weights, want_map):
        import numpy as np
        import torch
        Hv, Wv = int(a.shape[0]), int(a.shape[1])
        Cn = int(a.shape[2]) if a.dim() == 3 else 1
        w = None if weights is None else (C.c_double * len(weights))(*[float(v) for v in weights])
        m = torch.empty((max(Hv - win + 1, 0), max(Wv - win + 1, 0)) + ((Cn,) if a.dim() == 3 else ()), dtype=torch.float32, device=a.device) if want_map else None
        h = (C.c_double * 8)()
        hl = (C.c_double * (max(levels, 1) * max(Cn, 1) * 4))()
        _chk(lib().nsk_image_ssim(self.h, Hv, Wv, Cn, _ptr(a), _ptr(b), win, sigma, data_range, k1, k2, levels, w, _ptr(m), h, hl))
        h = [float(x) for x in h]
        return dict(ssim=h[1], ms_ssim=h[0] if levels > 1 else None, per_level=np.array(hl[:levels * Cn * 4], np.float64).reshape(levels, Cn, 4),
                    left_out=int(h[3]), map=m, h_out=h)

    @_ordered
    def sample_mesh(self, verts, tris, n, seed, want_tri=False):
        """nsk_mesh_sample: n area-weighted surface samples of the mesh (verts [nv, 3] float32, tris [nt, 3] int32, cuda tensors) ->
        points [n, 3] float32 (and with want_tri the chosen triangles [n] int32).  The total area and the number of degenerate triangles
        are left in self.last_area / self.last_degenerate.  Synchronises."""
        import torch
        assert verts.dtype == torch.float32 and tris.dtype == torch.int32 and verts.shape[-1] == 3 and tris.shape[-1] == 3
        n = int(n)
        pts = torch.empty((n, 3), dtype=torch.float32, device=verts.device)
        tri = torch.empty((n,), dtype=torch.int32, device=verts.device) if want_tri else None
        area, deg = C.c_double(0.0), C.c_int(0)
        self.last_area = self.last_degenerate = None
        _chk(lib().nsk_mesh_sample(self.h, _ptr(verts), int(verts.shape[0]), _ptr(tris), int(tris.shape[0]), int(seed) & 0xFFFFFFFFFFFFFFFF, n,
                                   _ptr(pts) if n else None, _ptr(tri) if n else None, C.byref(area), C.byref(deg)))
        self.last_area, self.last_degenerate = float(area.value), int(deg.value)
        return (pts, tri) if want_tri else pts

    @_ordered
    def cloud_nearest(self, query, target, want_index=False):
        """nsk_cloud_nearest: the exact fp32 distance from every query point [nq, 3] to its nearest target point [nt, 3] -> dist [nq]
        (and with want_index the lowest nearest target's index [nq] int32).  The number of non-finite targets left out is in
        self.last_skipped.  Synchronises."""
        import torch
        assert query.dtype == torch.float32 and target.dtype == torch.float32 and query.shape[-1] == 3 and target.shape[-1] == 3
        nq = int(query.shape[0])
        dist = torch.empty((nq,), dtype=torch.float32, device=query.device)
        idx = torch.empty((nq,), dtype=torch.int32, device=query.device) if want_index else None
        sk = C.c_int(0)
        _chk(lib().nsk_cloud_nearest(self.h, _ptr(query) if nq else None, nq, _ptr(target), int(target.shape[0]), _ptr(dist) if nq else None,
                                     _ptr(idx) if nq else None, C.byref(sk)))
        self.last_skipped = int(sk.value)
        return (dist, idx) if want_index else dist

    @_ordered
    def cloud_stats(self, dist, threshold):
        """nsk_cloud_stats -> dict(sum, count, below, max) over the finite entries of dist (below: d < threshold, strict).  Synchronises."""
        h = (C.c_double * 4)()
        n = int(dist.numel())
        _chk(lib().nsk_cloud_stats(self.h, _ptr(dist) if n else None, n, C.c_float(threshold), h))
        return dict(sum=float(h[0]), count=int(h[1]), below=int(h[2]), max=float(h[3]))

    @_ordered
    def mesh_nearest(self, query, verts, tris, want_tri=False, want_point=False):
        """nsk_mesh_nearest: the exact fp32 distance from every query point [nq, 3] to the mesh (verts [nv, 3] float32, tris [nt, 3] int32)
        -> dist [nq] (with want_tri the triangle that holds the nearest point [nq] int32, with want_point that point [nq, 3]; a tuple in
        that order when either is asked for).  The number of triangles left out is in self.last_skipped.  Synchronises."""
        import torch
        assert query.dtype == torch.float32 and verts.dtype == torch.float32 and tris.dtype == torch.int32
        assert query.shape[-1] == 3 and verts.shape[-1] == 3 and tris.shape[-1] == 3
        nq = int(query.shape[0])
        dist = torch.empty((nq,), dtype=torch.float32, device=query.device)
        tri = torch.empty((nq,), dtype=torch.int32, device=query.device) if want_tri else None
        point = torch.empty((nq, 3), dtype=torch.float32, device=query.device) if want_point else None
        sk = C.c_int(0)
        nv = int(verts.shape[0])
        _chk(lib().nsk_mesh_nearest(self.h, _ptr(query) if nq else None, nq, _ptr(verts) if nv else None, nv, _ptr(tris), int(tris.shape[0]),
                                    _ptr(dist) if nq else None, _ptr(tri) if nq else None, _ptr(point) if nq else None, C.byref(sk)))
        self.last_skipped = int(sk.value)
        out = (dist,) + ((tri,) if want_tri else ()) + ((point,) if want_point else ())
        return out if len(out) > 1 else dist

    @_ordered
    def mesh_vertex_normals(self, verts, tris, want_info=False):
        """nsk_mesh_vertex_normals: the area-weighted unit normals [nv, 3] float32 of a mesh (verts [nv, 3] float32, tris [nt, 3] int32, cuda
        tensors); a vertex without a normal gets zeros.  With want_info also dict(left_out, zero, max_valence), which synchronises."""
        import torch
        assert verts.dtype == torch.float32 and tris.dtype == torch.int32 and verts.shape[-1] == 3 and tris.shape[-1] == 3
        nv, nt = int(verts.shape[0]), int(tris.shape[0])
        normals = torch.empty((nv, 3), dtype=torch.float32, device=verts.device)
        info = (C.c_int * 4)()
        _chk(lib().nsk_mesh_vertex_normals(self.h, _ptr(verts) if nv else None, nv, _ptr(tris) if nt else None, nt, _ptr(normals) if nv else None,
                                           info if want_info else None))
        if want_info:
            return normals, dict(left_out=int(info[0]), zero=int(info[1]), max_valence=int(info[2]))
        return normals

    @_ordered
    def normal_rays(self, verts, normals, length=0.1):
        """nsk_normal_rays: the rays that look at the vertices from `length` out along their normals -> (rays_o [n, 3], rays_d [n, 3],
        gt_depth [n], has_ray [n] uint8); a vertex without a normal, or with a non-finite component, gets a ray whose result is not used"""
        import torch
        assert verts.dtype == torch.float32 and normals.dtype == torch.float32 and verts.shape[-1] == 3 and normals.shape == verts.shape
        n = int(verts.shape[0])
        dev = verts.device
        ro = torch.empty((n, 3), dtype=torch.float32, device=dev); rd = torch.empty((n, 3), dtype=torch.float32, device=dev)
        gd = torch.empty((n,), dtype=torch.float32, device=dev); has = torch.empty((n,), dtype=torch.uint8, device=dev)
        opt = lambda t: _ptr(t) if n else None
        _chk(lib().nsk_normal_rays(self.h, n, opt(verts), opt(normals), C.c_float(length), opt(ro), opt(rd), opt(gd), opt(has)))
        return ro, rd, gd, has

    @_ordered
    def mesh_vertex_colors(self, verts, normals=None, length=0.1, chunk_rays=None, want_fallback=False):
        """nsk_mesh_vertex_colors: the colours [nv, 3] float32 (not clamped) of the vertices: with normals the colour stage rendered along
        the ray of normal_rays(verts, normals, length), the point query where a vertex has no ray; without normals the point query
        everywhere.  chunk_rays None: the library's default.  With want_fallback also the number of point queries, which synchronises."""
        import torch
        assert verts.dtype == torch.float32 and verts.shape[-1] == 3
        assert normals is None or (normals.dtype == torch.float32 and normals.shape == verts.shape)
        nv = int(verts.shape[0])
        rgb = torch.empty((nv, 3), dtype=torch.float32, device=verts.device)
        fb = C.c_int(0)
        _chk(lib().nsk_mesh_vertex_colors(self.h, _ptr(verts) if nv else None, nv, _ptr(normals) if (normals is not None and nv) else None,
                                          C.c_float(length), int(chunk_rays or 0), _ptr(rgb) if nv else None, C.byref(fb) if want_fallback else None))
        return (rgb, int(fb.value)) if want_fallback else rgb

    @_ordered
    def prepare_frames(self, color, depth, intr, distortion=None, crop_size=None, crop_edge=0, png_depth_scale=1.0, scale=1.0, swap_rb=False,
                       depth_size=None):
        """nsk_frame_prepare: raw frames made ready on the device.  color [n, Hc, Wc, 3] uint8 or float32, depth [n, Hd, Wd] uint16 (or
        int16 holding the same bits) or float32, cuda tensors; either may be None (depth_size then names the absent depth image's size,
        default: the colour's).  intr = (fx, fy, cx, cy) for the depth size; distortion: 4, 5 or 8 coefficients in OpenCV's order.
        -> (color [n, H', W', 3] float32 or None, depth [n, H', W'] float32 or None, intr_out [4] float32 numpy, n_border).
        Synchronises when it undistorts (the border count)."""
        import torch
        assert color is not None or depth is not None
        ref = color if color is not None else depth
        n = int(ref.shape[0])
        if color is not None:
            assert color.dim() == 4 and color.shape[-1] == 3 and color.dtype in (torch.uint8, torch.float32), "color: [n, H, W, 3] uint8 / float32"
        if depth is not None:
            assert depth.dim() == 3 and int(depth.shape[0]) == n and depth.dtype in (torch.uint16, torch.int16, torch.float32), "depth: [n, H, W] uint16 / float32"
            Hd, Wd = int(depth.shape[1]), int(depth.shape[2])
        else:
            Hd, Wd = (int(depth_size[0]), int(depth_size[1])) if depth_size is not None else (int(color.shape[1]), int(color.shape[2]))
        Hc, Wc = (int(color.shape[1]), int(color.shape[2])) if color is not None else (Hd, Wd)
        o = frame_opts(intr, distortion, crop_size, crop_edge, png_depth_scale, scale, swap_rb)
        H, W, intr_out = frame_plan((Hc, Wc), (Hd, Wd), intr, distortion, crop_size, crop_edge, png_depth_scale, scale, swap_rb)
        c_out = torch.empty((n, H, W, 3), dtype=torch.float32, device=ref.device) if color is not None else None
        d_out = torch.empty((n, H, W), dtype=torch.float32, device=ref.device) if depth is not None else None
        nb = C.c_int(0)
        ct = FRAME_U8 if color is not None and color.dtype == torch.uint8 else FRAME_F32
        dt = FRAME_F32 if depth is not None and depth.dtype == torch.float32 else FRAME_U16
        _chk(lib().nsk_frame_prepare(self.h, C.byref(o), n, _ptr(color) if n else None, ct, Hc, Wc, _ptr(depth) if n else None, dt, Hd, Wd,
                                     _ptr(c_out) if n else None, _ptr(d_out) if n else None, C.byref(nb)))
        return c_out, d_out, intr_out, int(nb.value)

    @_ordered
    def normal_stats(self, va, ta, ia, vb, tb, ib):
        """nsk_normal_stats: the agreement |n_A . n_B| / (|n_A| |n_B|) of the normals of triangle ia[i] of mesh A (va, ta) and triangle
        ib[i] of mesh B (vb, tb), cuda tensors (float32 [nv, 3], int32 [nt, 3], int32 [n]) -> dict(sum, count, skipped).  Synchronises."""
        import torch
        assert va.dtype == torch.float32 and vb.dtype == torch.float32 and all(t.dtype == torch.int32 for t in (ta, ia, tb, ib))
        n = int(ia.numel())
        assert int(ib.numel()) == n
        h = (C.c_double * 3)()
        opt = lambda t: _ptr(t) if t.numel() else None
        _chk(lib().nsk_normal_stats(self.h, n, opt(va), int(va.shape[0]), opt(ta), int(ta.shape[0]), opt(ia), opt(vb), int(vb.shape[0]),
                                    opt(tb), int(tb.shape[0]), opt(ib), h))
        return dict(sum=float(h[0]), count=int(h[1]), skipped=int(h[2]))

    @_ordered
    def cloud_pair_sums(self, source, target, M=None, threshold=0.1, want_pairs=False):
        """nsk_cloud_pair_sums: the 17 pair sums (numpy float64) of source [ns, 3] under the 4x4 M (None: the identity) against target
        [nt, 3]; with want_pairs also the correspondences (dist [ns] float32, index [ns] int32) by source index.  The number of non-finite
        targets left out is in self.last_skipped.  Synchronises."""
        import numpy as np
        import torch
        assert source.dtype == torch.float32 and target.dtype == torch.float32 and source.shape[-1] == 3 and target.shape[-1] == 3
        ns = int(source.shape[0])
        dist = torch.empty((ns,), dtype=torch.float32, device=source.device) if want_pairs else None
        idx = torch.empty((ns,), dtype=torch.int32, device=source.device) if want_pairs else None
        h = (C.c_double * 17)()
        sk = C.c_int(0)
        _chk(lib().nsk_cloud_pair_sums(self.h, _ptr(source) if ns else None, ns, _ptr(target), int(target.shape[0]), _mat16(M),
                                       C.c_float(threshold), h, _ptr(dist) if ns else None, _ptr(idx) if ns else None, C.byref(sk)))
        self.last_skipped = int(sk.value)
        sums = np.array(h[:], np.float64)
        return (sums, dist, idx) if want_pairs else sums

    @_ordered
    def cloud_icp(self, source, target, threshold=0.1, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, init=None):
        """nsk_cloud_icp: point-to-point ICP of source [ns, 3] onto target [nt, 3] (cuda float32) -> (M [4, 4] float64 numpy, info dict:
        iterations, fitness, rmse, correspondences, converged, target_skipped, source_nonfinite, degenerate).  Synchronises."""
        import numpy as np
        import torch
        assert source.dtype == torch.float32 and target.dtype == torch.float32 and source.shape[-1] == 3 and target.shape[-1] == 3
        ns = int(source.shape[0])
        M = (C.c_double * 16)()
        info = (C.c_double * 8)()
        _chk(lib().nsk_cloud_icp(self.h, _ptr(source) if ns else None, ns, _ptr(target), int(target.shape[0]), C.c_float(threshold), int(max_iter),
                                 float(rel_fitness), float(rel_rmse), _mat16(init), M, info))
        return np.array(M[:], np.float64).reshape(4, 4), dict(
            iterations=int(info[0]), fitness=float(info[1]), rmse=float(info[2]), correspondences=int(info[3]), converged=bool(info[4]),
            target_skipped=int(info[5]), source_nonfinite=int(info[6]), degenerate=bool(info[7]))

    @_ordered
    def cloud_transform(self, M, points, out=None):
        """nsk_cloud_transform: points [n, 3] (cuda float32) under the 4x4 M -> a new tensor, or into out (out may be points itself)"""
        import torch
        assert points.dtype == torch.float32 and points.shape[-1] == 3
        if out is None:
            out = torch.empty_like(points)
        assert out.dtype == torch.float32 and out.shape == points.shape
        n = int(points.shape[0])
        _chk(lib().nsk_cloud_transform(self.h, _mat16(M), _ptr(points) if n else None, n, _ptr(out) if n else None))
        return out

    def align_mesh(self, rec_verts, gt_verts, threshold=0.1, max_iter=30, n_points=0, rec_tris=None, gt_tris=None, seed=0):
        """upstream's get_align_transformation: the rigid transform (M [4, 4] float64, info as cloud_icp) that registers the reconstruction
        to the ground truth by point-to-point ICP from the identity.  n_points = 0 aligns the vertices, as upstream does; n_points > 0
        aligns that many surface samples of each mesh (seed, seed + 1), for which the triangles must be given."""
        if n_points > 0:
            assert rec_tris is not None and gt_tris is not None, "align_mesh: surface samples need the triangles"
            rec_verts = self.sample_mesh(rec_verts, rec_tris, n_points, seed)
            gt_verts = self.sample_mesh(gt_verts, gt_tris, n_points, seed + 1)
        return self.cloud_icp(rec_verts, gt_verts, threshold, max_iter)

    def _aligned(self, rec_verts, gt_verts, threshold, max_iter):
        M, info = self.align_mesh(rec_verts, gt_verts, threshold, max_iter)
        return self.cloud_transform(M, rec_verts), dict(transform=M, icp_fitness=info["fitness"], icp_rmse=info["rmse"],
                                                        icp_iterations=info["iterations"])

    def recon_metrics(self, rec_verts, rec_tris, gt_verts, gt_tris, n=200000, threshold=0.05, seed=0, align=False, align_threshold=0.1,
                      align_max_iter=30, surface=False):
        """upstream's three 3D numbers of a reconstruction (rec) against a ground-truth mesh (gt), both as cuda tensors (what extract_mesh /
        filter_mesh return goes in directly): n samples of each surface (seed, seed + 1), nearest distances both ways, the means in cm and
        the share of gt samples with a rec sample closer than threshold in %.  Coordinates are taken to be metres.  With align the
        reconstruction's vertices are first registered to the ground truth's (align_mesh) and the transformed mesh is measured; the
        result then also holds transform, icp_fitness, icp_rmse and icp_iterations.
        With surface the rec samples are measured against the gt MESH and the gt samples against the rec mesh (mesh_nearest), which takes
        the sampling of the other surface out of every distance; rec_skipped / gt_skipped then count the triangles left out.  The
        result also holds surface=True, precision_pct (rec samples with d < threshold), recall_pct (= completion_ratio_pct), fscore_pct
        = 2 P R / (P + R) (0 when P + R is 0), normal_accuracy / normal_completion (the mean |cos| between each sample's own triangle
        and the nearest triangle of the other mesh, in [0, 1]), their mean normal_consistency, and normal_skipped."""
        extra = {}
        if align:
            rec_verts, extra = self._aligned(rec_verts, gt_verts, align_threshold, align_max_iter)
        if surface:
            return self._recon_metrics_surface(rec_verts, rec_tris, gt_verts, gt_tris, n, threshold, seed, extra)
        rec = self.sample_mesh(rec_verts, rec_tris, n, seed)
        rec_area, rec_deg = self.last_area, self.last_degenerate
        gt = self.sample_mesh(gt_verts, gt_tris, n, seed + 1)
        gt_area, gt_deg = self.last_area, self.last_degenerate
        acc = self.cloud_stats(self.cloud_nearest(rec, gt), threshold)
        gt_skipped = self.last_skipped
        comp = self.cloud_stats(self.cloud_nearest(gt, rec), threshold)
        rec_skipped = self.last_skipped
        nan = float("nan")
        return dict(accuracy_cm=100.0 * acc["sum"] / acc["count"] if acc["count"] else nan,
                    completion_cm=100.0 * comp["sum"] / comp["count"] if comp["count"] else nan,
                    completion_ratio_pct=100.0 * comp["below"] / comp["count"] if comp["count"] else nan,
                    accuracy_max_cm=100.0 * acc["max"], completion_max_cm=100.0 * comp["max"],
                    rec_area=rec_area, gt_area=gt_area, rec_degenerate=rec_deg, gt_degenerate=gt_deg,
                    rec_skipped=rec_skipped, gt_skipped=gt_skipped, n=int(n), threshold=float(threshold), **extra)

    def _recon_metrics_surface(self, rec_verts, rec_tris, gt_verts, gt_tris, n, threshold, seed, extra):
        rec, rec_own = self.sample_mesh(rec_verts, rec_tris, n, seed, want_tri=True)
        rec_area, rec_deg = self.last_area, self.last_degenerate
        gt, gt_own = self.sample_mesh(gt_verts, gt_tris, n, seed + 1, want_tri=True)
        gt_area, gt_deg = self.last_area, self.last_degenerate
        d, hit = self.mesh_nearest(rec, gt_verts, gt_tris, want_tri=True)
        gt_skipped = self.last_skipped
        acc = self.cloud_stats(d, threshold)
        n_acc = self.normal_stats(rec_verts, rec_tris, rec_own, gt_verts, gt_tris, hit)
        d, hit = self.mesh_nearest(gt, rec_verts, rec_tris, want_tri=True)
        rec_skipped = self.last_skipped
        comp = self.cloud_stats(d, threshold)
        n_comp = self.normal_stats(gt_verts, gt_tris, gt_own, rec_verts, rec_tris, hit)
        nan = float("nan")
        prec = 100.0 * acc["below"] / acc["count"] if acc["count"] else nan
        rcl = 100.0 * comp["below"] / comp["count"] if comp["count"] else nan
        na = n_acc["sum"] / n_acc["count"] if n_acc["count"] else nan
        nc = n_comp["sum"] / n_comp["count"] if n_comp["count"] else nan
        return dict(accuracy_cm=100.0 * acc["sum"] / acc["count"] if acc["count"] else nan,
                    completion_cm=100.0 * comp["sum"] / comp["count"] if comp["count"] else nan,
                    completion_ratio_pct=rcl,
                    accuracy_max_cm=100.0 * acc["max"], completion_max_cm=100.0 * comp["max"],
                    rec_area=rec_area, gt_area=gt_area, rec_degenerate=rec_deg, gt_degenerate=gt_deg,
                    rec_skipped=rec_skipped, gt_skipped=gt_skipped, n=int(n), threshold=float(threshold), surface=True,
                    precision_pct=prec, recall_pct=rcl, fscore_pct=2.0 * prec * rcl / (prec + rcl) if prec + rcl > 0 else (0.0 if prec + rcl == 0 else nan),
                    normal_accuracy=na, normal_completion=nc, normal_consistency=0.5 * (na + nc),
                    normal_skipped=n_acc["skipped"] + n_comp["skipped"], **extra)

    @_ordered
    def mesh_depth(self, verts, tris, w2c, H, W, fx, fy, cx, cy, want_skipped=False):
        """nsk_mesh_depth: depth images [V, H, W] float32 (cuda) of the mesh (verts [nv, 3] float32, tris [nt, 3] int32, cuda tensors) from
        the views w2c [V, 4, 4] (host, world-to-camera, camera looking along -z); 0 where nothing is hit.  Asynchronous unless want_skipped,
        which leaves the number of triangles with an index out of range in self.last_skipped."""
        import numpy as np
        import torch
        assert verts.dtype == torch.float32 and tris.dtype == torch.int32 and verts.shape[-1] == 3 and tris.shape[-1] == 3
        w, wp = _w2c16(w2c)
        V, nv, nt = int(w.shape[0]), int(verts.shape[0]), int(tris.shape[0])
        depth = torch.empty((V, int(H), int(W)), dtype=torch.float32, device=verts.device)
        sk = C.c_int(0)
        _chk(lib().nsk_mesh_depth(self.h, _ptr(verts) if nv else None, nv, _ptr(tris) if nt else None, nt, V, wp, int(H), int(W), C.c_float(fx),
                                  C.c_float(fy), C.c_float(cx), C.c_float(cy), _ptr(depth) if V else None, C.byref(sk) if want_skipped else None))
        if want_skipped:
            self.last_skipped = int(sk.value)
        return depth

    @_ordered
    def depth_pair_stats(self, a, b):
        """nsk_depth_pair_stats of two depth stacks [V, H, W] (or [V, n_pix]) -> numpy [V, 4] float64: sum |a - b|, pixels with a > 0 and
        b > 0, sum |a - b| over those, pixels with a > 0.  Synchronises."""
        import numpy as np
        import torch
        assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and a.dim() >= 2
        V = int(a.shape[0])
        out = np.zeros((V, 4), np.float64)
        if V:
            _chk(lib().nsk_depth_pair_stats(self.h, _ptr(a), _ptr(b), V, int(a[0].numel()), out.ctypes.data_as(C.c_void_p)))
        return out

    @_ordered
    def depth_views(self, verts, n_views, seed=0, shrink=0.7):
        """nsk_depth_views: n_views random views inside the box of the mesh's vertices -> w2c [n_views, 4, 4] float32 (host); the box is left
        in self.last_box.  Synchronises."""
        import numpy as np
        import torch
        assert verts.dtype == torch.float32 and verts.shape[-1] == 3
        box = np.zeros(6, np.float32)
        w = np.zeros((int(n_views), 4, 4), np.float32)
        _chk(lib().nsk_depth_views(self.h, _ptr(verts), int(verts.shape[0]), box.ctypes.data_as(C.c_void_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   float(shrink), int(n_views), w.ctypes.data_as(C.c_void_p)))
        self.last_box = box
        return w

    # -- culling a mesh to what a trajectory saw; depth views clear of the unseen (nsk_cull.h) ----------------------------------------
    @_ordered
    def points_seen(self, points, w2c, intr, HW, depths=None, edge=0, eps=0.03, zero_sees=False, seen=None):
        """nsk_points_seen: the points [n, 3] (float32 cuda) that one of the K frames saw.  w2c [K, 4, 4] world-to-camera on the host;
        intr = (fx, fy, cx, cy); HW = (H, W); depths: float32 cuda tensor [K, H, W], or None for the frustum alone; zero_sees: the depth was
        rendered from the mesh itself (a pixel with depth 0 hides nothing).  seen: uint8 cuda tensor [n] to OR into (default: a new one).
        -> (seen, n_seen).  Synchronises (the count)."""
        import numpy as np
        import torch
        assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[-1] == 3
        w, wp = _w2c16(w2c)
        K, n, H, W = int(w.shape[0]), int(points.shape[0]), int(HW[0]), int(HW[1])
        if depths is not None:
            assert depths.dtype == torch.float32 and tuple(depths.shape) == (K, H, W)
        acc = seen is not None
        if acc:
            assert seen.dtype == torch.uint8 and seen.numel() == n
        else:
            seen = torch.empty((n,), dtype=torch.uint8, device=points.device)
        cnt = C.c_longlong(0)
        _chk(lib().nsk_points_seen(self.h, _ptr(points) if n else None, n, K, _ptr(depths) if depths is not None and K else None, H, W,
                                   *_intr4(intr), wp, int(edge), float(eps), int(bool(zero_sees)), int(acc), _ptr(seen) if n else None,
                                   C.byref(cnt)))
        return seen, int(cnt.value)

    @_ordered
    def mesh_select(self, verts, tris, seen, part=0):
        """nsk_mesh_select: the sub-mesh of (verts [nv, 3] float32, tris [nt, 3] int32, cuda) whose triangles have all three vertices set in
        seen [nv] uint8 (part 0), or every other valid triangle (part 1: the unseen complement); unreferenced vertices dropped, order kept,
        triangles re-indexed -> (verts, tris, vertex_src [int32: the input index of every output vertex], skipped [triangles with an index
        out of range]).  Synchronises."""
        import torch
        assert verts.dtype == torch.float32 and tris.dtype == torch.int32 and verts.shape[-1] == 3 and tris.shape[-1] == 3
        nv, nt = int(verts.shape[0]), int(tris.shape[0])
        assert seen.dtype in (torch.uint8, torch.bool) and seen.numel() == nv
        ov = torch.empty((nv, 3), dtype=torch.float32, device=verts.device)
        ot = torch.empty((nt, 3), dtype=torch.int32, device=verts.device)
        src = torch.empty((nv,), dtype=torch.int32, device=verts.device)
        a, b, sk = C.c_int(0), C.c_int(0), C.c_int(0)
        _chk(lib().nsk_mesh_select(self.h, _ptr(verts) if nv else None, nv, _ptr(tris) if nt else None, nt, _ptr(seen) if nv else None, int(part),
                                   _ptr(ov) if nv else None, _ptr(ot) if nt else None, _ptr(src) if nv else None, C.byref(a), C.byref(b),
                                   C.byref(sk)))
        return ov[:a.value].clone(), ot[:b.value].clone(), src[:a.value].clone(), int(sk.value)

    @_ordered
    def simplify_mesh(self, verts, tris, cell, keep_duplicates=False, want_map=False, want_info=False):
        """nsk_mesh_simplify: (verts [nv, 3] float32, tris [nt, 3] int32, cuda) clustered on a uniform grid of edge `cell`: every occupied
        cell's vertices collapse to their fixed-point mean, collapsed triangles and (unless keep_duplicates) same-orientation duplicates
        go, unreferenced vertices go -> (verts, tris[, vertex_map int32 [nv]: the output vertex of every input vertex or -1][, info: numpy
        int64 [8], include/nsk.h]).  Synchronises."""
        import numpy as np
        import torch
        assert verts.dtype == torch.float32 and tris.dtype == torch.int32 and verts.shape[-1] == 3 and tris.shape[-1] == 3
        nv, nt = int(verts.shape[0]), int(tris.shape[0])
        dev = "cuda:%d" % self.device
        ov = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        ot = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        vmap = torch.empty((nv,), dtype=torch.int32, device=dev) if want_map else None
        a, b = C.c_int(0), C.c_int(0)
        info = (C.c_longlong * 8)()
        _chk(lib().nsk_mesh_simplify(self.h, _ptr(verts) if nv else None, nv, _ptr(tris) if nt else None, nt, C.c_float(cell),
                                     1 if keep_duplicates else 0, _ptr(ov) if nv else None, _ptr(ot) if nt else None,
                                     _ptr(vmap) if want_map and nv else None, C.byref(a), C.byref(b), info))
        out = [ov[:a.value].clone(), ot[:b.value].clone()]
        if want_map:
            out.append(vmap)
        if want_info:
            out.append(np.array(list(info), np.int64))
        return tuple(out)

    @_ordered
    def points_view_counts(self, points, w2c, HW, intr, edge=0):
        """nsk_points_view_counts: how many of the points [n, 3] (float32 cuda) each view of w2c [V, 4, 4] (host) has in its image (the frustum
        alone: a hidden point counts) -> numpy int64 [V].  Synchronises."""
        import numpy as np
        import torch
        assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[-1] == 3
        w, wp = _w2c16(w2c)
        V, n = int(w.shape[0]), int(points.shape[0])
        out = np.zeros(V, np.int64)
        _chk(lib().nsk_points_view_counts(self.h, _ptr(points) if n else None, n, V, wp, int(HW[0]), int(HW[1]), *_intr4(intr), int(edge),
                                          out.ctypes.data_as(C.c_void_p) if V else None))
        return out

    depth_views_range = staticmethod(depth_views_range)

    def cull_mesh(self, verts, tris, w2c, intr, HW, depths=None, occlusion="none", edge=0, eps=0.03, frames_per_batch=32):
        """upstream's cull_mesh.py on the device: the part of the mesh (verts [nv, 3] float32, tris [nt, 3] int32, cuda) that the trajectory
        w2c [K, 4, 4] (host, world-to-camera, camera looking along -z) saw, by the per-vertex rule of points_seen.
          occlusion "none": the view frusta alone;
          "depth": against the caller's sensor depth images depths [K, H, W] float32 (a tensor anywhere, or numpy), streamed to the device
                   frames_per_batch at a time (a pixel without a measurement sees nothing);
          "self": every batch of frames is first rendered from the mesh itself (mesh_depth at HW / intr) and tested against that (a pixel
                  that hits nothing hides nothing).
        The trajectory is never resident as a whole.  eps (m): how far behind the depth a vertex still counts as seen; 0.03 is this
        project's first choice, not upstream's number.  -> dict(verts, tris, seen [nv] uint8, vertex_src, n_seen, skipped); the result
        does not depend on frames_per_batch."""
        import numpy as np
        import torch
        assert occlusion in ("none", "depth", "self"), occlusion
        w = np.ascontiguousarray(np.asarray(w2c, np.float32).reshape(-1, 4, 4))
        K, H, W = int(w.shape[0]), int(HW[0]), int(HW[1])
        fx, fy, cx, cy = [float(x) for x in intr]
        if occlusion == "depth":
            assert depths is not None and tuple(depths.shape) == (K, H, W), "cull_mesh: occlusion 'depth' needs depths [K, H, W]"
        step = max(1, int(frames_per_batch))
        seen, n_seen = self.points_seen(verts, w[:0], intr, HW)              # (cleared)
        for k0 in range(0, K, step):
            wb = w[k0:k0 + step]
            if occlusion == "none":
                d = None
            elif occlusion == "depth":
                d = torch.as_tensor(np.ascontiguousarray(depths[k0:k0 + step]) if isinstance(depths, np.ndarray) else depths[k0:k0 + step])
                d = d.to(device=verts.device, dtype=torch.float32).contiguous()
            else:
                d = self.mesh_depth(verts, tris, wb, H, W, fx, fy, cx, cy)
            seen, n_seen = self.points_seen(verts, wb, intr, HW, d, edge, eps, occlusion == "self", seen)
        ov, ot, src, skipped = self.mesh_select(verts, tris, seen, 0)
        return dict(verts=ov, tris=ot, seen=seen, vertex_src=src, n_seen=n_seen, skipped=skipped)

    def unseen_points(self, verts, tris, seen, n, seed=0):
        """n area-weighted samples [n, 3] of the part of the mesh the trajectory did not see (mesh_select part 1, then sample_mesh): the
        points depth_views_clear rejects views with.  n = 0, or an empty complement, gives an empty tensor."""
        import torch
        empty = torch.empty((0, 3), dtype=torch.float32, device=verts.device)
        if int(n) == 0:
            return empty
        cv, ct, _, _ = self.mesh_select(verts, tris, seen, 1)
        if ct.shape[0] == 0:
            return empty
        return self.sample_mesh(cv, ct, int(n), seed)

    def depth_views_clear(self, gt_verts, unseen, n_views, HW, focal, seed=0, shrink=0.7, edge=0, max_factor=16):
        """upstream's redraw of Depth L1 views: the first n_views candidates, in index order, of the stream depth_views draws (seed, shrink,
        the box of gt_verts) that have none of the unseen points [P, 3] in their H x W image (fx = fy = focal, cx = W / 2 - 0.5,
        cy = H / 2 - 0.5; points_view_counts: no depth test).  Candidates are drawn and counted in rounds; at most max_factor * n_views are
        tried, so fewer than n_views may come back.  -> (w2c [m, 4, 4] float32, index [m] int64, tried): tried is the index of the last
        accepted candidate + 1 when n_views were found, max_factor * n_views otherwise."""
        import numpy as np
        n_views, H, W = int(n_views), int(HW[0]), int(HW[1])
        cap = int(max_factor) * n_views
        self.depth_views(gt_verts, 0, seed, shrink)                         # (the box)
        box = self.last_box
        intr = (focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5)
        ws, idx, first = [], [], 0
        while len(idx) < n_views and first < cap:
            need = n_views - len(idx)
            m = min(cap - first, max(32, (need + 31) // 32 * 32))
            w = depth_views_range(box, first, m, seed, shrink)
            cnt = self.points_view_counts(unseen, w, (H, W), intr, edge)
            for k in np.nonzero(cnt == 0)[0][:need]:
                ws.append(w[k]); idx.append(first + int(k))
            first += m
        tried = idx[-1] + 1 if len(idx) == n_views and idx else (0 if n_views == 0 else cap)
        w2c = np.stack(ws).astype(np.float32) if ws else np.zeros((0, 4, 4), np.float32)
        return w2c, np.array(idx, np.int64), tried

    def recon_depth_l1(self, rec_verts, rec_tris, gt_verts, gt_tris, n_views=1000, HW=(500, 500), focal=300.0, seed=0, shrink=0.7,
                       min_cover=0.0, align=False, align_threshold=0.1, align_max_iter=30, unseen=None, max_factor=16):
        """upstream's Depth L1 of a reconstruction (rec) against a ground-truth mesh (gt), both as cuda tensors: both meshes rendered as
        depth images from the same n_views random views inside the ground truth's box (depth_views), cx = W / 2 - 0.5, cy = H / 2 - 0.5;
        depth_l1_cm = 100 x the mean over the used views of sum |gt - rec| / n_pix.  A view is used when the ground truth covers at least
        min_cover of its pixels (0: every view, upstream's plain mean).  Also: n_used, restricted_l1_cm (the mean over the pixels of the
        used views where both meshes are hit) and the per-view arrays view_l1 (m), view_cover, stats [n_views, 4], w2c.  With align the
        reconstruction's vertices are first registered to the ground truth's (align_mesh) and the transformed mesh is rendered; the result
        then also holds transform, icp_fitness, icp_rmse and icp_iterations.  With unseen (points [P, 3] float32 cuda: the never-observed
        ground truth, unseen_points) the views are depth_views_clear's: the first n_views candidates of the same stream that have none of
        those points in their image, at most max_factor * n_views candidates tried (upstream redraws such views); the per-view arrays then
        have one entry per accepted view (possibly fewer than n_views), and the result also holds candidates_tried and view_index (the
        accepted candidates' indices in the stream).  With None nothing changes."""
        import numpy as np
        extra = {}
        if align:
            rec_verts, extra = self._aligned(rec_verts, gt_verts, align_threshold, align_max_iter)
        H, W = int(HW[0]), int(HW[1])
        n_pix = H * W
        n_drawn = int(n_views)
        if unseen is None:
            w2c = self.depth_views(gt_verts, n_views, seed, shrink)
        else:
            w2c, view_index, tried = self.depth_views_clear(gt_verts, unseen, n_views, (H, W), focal, seed, shrink, 0, max_factor)
            extra = dict(extra, candidates_tried=tried, view_index=view_index)
            n_drawn = int(w2c.shape[0])
        stats = np.zeros((n_drawn, 4), np.float64)
        batch = max(1, (1 << 27) // n_pix)                 # both stacks together stay below about 1 GB
        if batch > 32:
            batch -= batch % 32
        for k0 in range(0, n_drawn, batch):
            w = w2c[k0:k0 + batch]
            gt = self.mesh_depth(gt_verts, gt_tris, w, H, W, focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5)
            rec = self.mesh_depth(rec_verts, rec_tris, w, H, W, focal, focal, W / 2.0 - 0.5, H / 2.0 - 0.5)
            stats[k0:k0 + batch] = self.depth_pair_stats(gt, rec)
        view_l1 = stats[:, 0] / n_pix
        cover = stats[:, 3] / n_pix
        used = cover >= min_cover
        n_used, l1, both, both_sum = 0, 0.0, 0.0, 0.0
        for k in range(n_drawn):                            # (in view order, as Mesher::eval_recon_depth adds them)
            if used[k]:
                n_used += 1; l1 += view_l1[k]; both += stats[k, 1]; both_sum += stats[k, 2]
        nan = float("nan")
        return dict(depth_l1_cm=100.0 * l1 / n_used if n_used else nan, n_used=n_used,
                    restricted_l1_cm=100.0 * both_sum / both if both else nan, view_l1=view_l1, view_cover=cover, stats=stats, w2c=w2c,
                    n_views=int(n_views), H=H, W=W, focal=float(focal), seed=int(seed), shrink=float(shrink), min_cover=float(min_cover),
                    **extra)

    @_ordered
    def eval_points(self, stage, pts):
        import torch
        M = pts.shape[0]
        raw = torch.empty(M, 4, device=pts.device)
        _chk(lib().nsk_eval_points(self.h, _stage(stage), M, _ptr(pts), _ptr(raw)))
        return raw

    @_ordered
    def eval_lattice(self, stage, origin, step, nx, ny, nz, valid=None, fill=100.0, out=None):
        """occupancy at the nodes origin + (i, j, k) * step -> float32 cuda tensor [nz, ny, nx] (nsk_eval_lattice).
        valid: uint8 / bool cuda tensor of nz * ny * nx elements: only the nodes with a non-zero byte are decoded, the others receive the bits
        of `fill` (a numpy float32 keeps its NaN payload) (nsk_eval_lattice_masked); the number of decoded nodes is left in
        self.last_evaluated (None after a call without a mask).  out: a contiguous float32 cuda tensor of nz * ny * nx elements to write into
        instead of a new one."""
        import numpy as np
        import torch
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3)); s = np.ascontiguousarray(np.asarray(step, np.float32).reshape(3))
        nodes = int(nx) * int(ny) * int(nz)
        if out is None:
            vol = torch.empty((int(nz), int(ny), int(nx)), dtype=torch.float32, device="cuda:%d" % self.device)
        else:
            assert out.dtype == torch.float32 and out.numel() == nodes
            vol = out
        if valid is None:
            self.last_evaluated = None
            _chk(lib().nsk_eval_lattice(self.h, _stage(stage), o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), int(nx), int(ny), int(nz), _ptr(vol)))
            return vol
        assert valid.dtype in (torch.uint8, torch.bool) and valid.numel() == nodes
        n = C.c_longlong(0)
        f = C.c_float.from_buffer_copy(np.float32(fill).tobytes())            # (the bits as they are: a conversion may quieten or drop a NaN's payload)
        _chk(lib().nsk_eval_lattice_masked(self.h, _stage(stage), o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), int(nx), int(ny), int(nz),
                                           _ptr(valid), f, _ptr(vol), C.byref(n)))
        self.last_evaluated = int(n.value)
        return vol

    @_ordered
    def extract_mesh(self, volume, origin, step, level=0.0, valid=None):
        """marching cubes over a float32 cuda volume [nz, ny, nx] (valid: uint8 cuda tensor of the same shape or None) ->
        (vertices [nv, 3] float32, triangles [nt, 3] int32) as cuda tensors of their own (nsk_mesh_extract)"""
        import numpy as np
        import torch
        assert volume.dim() == 3 and volume.dtype == torch.float32
        if valid is not None:
            assert valid.dtype == torch.uint8 and valid.numel() == volume.numel()
        nz, ny, nx = volume.shape
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3)); s = np.ascontiguousarray(np.asarray(step, np.float32).reshape(3))
        nv, nt = C.c_int(0), C.c_int(0)
        _chk(lib().nsk_mesh_extract(self.h, _ptr(volume), _ptr(valid), nx, ny, nz, o.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                                    C.c_float(level), C.byref(nv), C.byref(nt)))
        pv, pt = C.c_void_p(), C.c_void_p()
        _chk(lib().nsk_mesh_buffers(self.h, C.byref(pv), C.byref(pt)))
        dev = volume.device
        verts = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((nt.value, 3), dtype=torch.int32, device=dev)
        if nv.value:      # (nsk_mesh_extract has synchronised; the copies run on torch's current stream)
            verts.view(-1).copy_(torch.as_tensor(_CudaArray(pv.value, 3 * nv.value), device=dev))
        if nt.value:
            tris.view(-1).copy_(torch.as_tensor(_CudaArray(pt.value, 3 * nt.value, "<i4"), device=dev))
        return verts, tris

    def _mesh_tensors(self, nv, nt):
        """the context's mesh buffers copied into cuda tensors of their own"""
        import torch
        pv, pt = C.c_void_p(), C.c_void_p()
        _chk(lib().nsk_mesh_buffers(self.h, C.byref(pv), C.byref(pt)))
        dev = "cuda:%d" % self.device
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        if nv:
            verts.view(-1).copy_(torch.as_tensor(_CudaArray(pv.value, 3 * nv), device=dev))
        if nt:
            tris.view(-1).copy_(torch.as_tensor(_CudaArray(pt.value, 3 * nt, "<i4"), device=dev))
        return verts, tris

    @_ordered
    def lattice_seen(self, origin, step, nx, ny, nz, depths, intr, w2c, edge=0, trunc=0.5, valid=None):
        """the lattice nodes that one of the keyframes saw (nsk_lattice_seen).  depths: float32 cuda tensor [K, H, W] (K may be 0);
        intr = (fx, fy, cx, cy); w2c: [K, 4, 4] world-to-camera on the host.  valid: uint8 cuda tensor [nz, ny, nx] to OR into
        (default: a new one).  -> (valid, n_seen)"""
        import numpy as np
        import torch
        assert depths.dim() == 3 and depths.dtype == torch.float32
        K, H, W = depths.shape
        (w, wp), (o, op), (s, sp) = _w2c16(w2c, K), _vec3(origin), _vec3(step)
        acc = valid is not None
        if acc:
            assert valid.dtype == torch.uint8 and valid.numel() == int(nx) * int(ny) * int(nz)
        else:
            valid = torch.empty((int(nz), int(ny), int(nx)), dtype=torch.uint8, device="cuda:%d" % self.device)
        n = C.c_longlong(0)
        _chk(lib().nsk_lattice_seen(self.h, op, sp, int(nx), int(ny), int(nz), int(K), _ptr(depths) if K else None, int(H), int(W), *_intr4(intr), wp,
                                    int(edge), C.c_float(trunc), int(acc), _ptr(valid), C.byref(n)))
        return valid, int(n.value)

    @_ordered
    def filter_mesh(self, min_area=0.0, largest_only=False):
        """connected components of the mesh of the last extract_mesh, small ones (area <= min_area) or all but the largest dropped in
        place (nsk_mesh_filter) -> (vertices, triangles, n_components, n_kept), the arrays as cuda tensors of their own"""
        nv, nt, nc, nk = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _chk(lib().nsk_mesh_filter(self.h, C.c_float(min_area), int(bool(largest_only)), C.byref(nv), C.byref(nt), C.byref(nc), C.byref(nk)))
        verts, tris = self._mesh_tensors(nv.value, nt.value)
        return verts, tris, nc.value, nk.value

    # -- depth frames fused into a TSDF on a lattice, meshed by the extractor (nsk_tsdf.h) ---------------------------------------------
    @_ordered
    def tsdf_integrate(self, origin, step, nx, ny, nz, depths, intr, w2c, edge=0, trunc=0.5, max_weight=64, state=None):
        """nsk_tsdf_integrate: the K frames depths [K, H, W] (float32 cuda, K may be 0) at w2c [K, 4, 4] (host, world-to-camera) integrated
        into a truncated signed distance volume on the lattice origin + (i, j, k) * step.  intr = (fx, fy, cx, cy); edge, trunc and the
        projection as in lattice_seen.  state: (tsdf, weight), float32 cuda tensors of nz * ny * nx elements, to continue from (updated in
        place); default: new ones, started from zero.  -> (tsdf [nz, ny, nx], weight [nz, ny, nx], n_observed).  Synchronises (the count)."""
        import numpy as np
        import torch
        assert depths.dim() == 3 and depths.dtype == torch.float32
        K, H, W = depths.shape
        (w, wp), (o, op), (s, sp) = _w2c16(w2c, K), _vec3(origin), _vec3(step)
        nodes = int(nx) * int(ny) * int(nz)
        acc = state is not None
        if acc:
            tsdf, weight = state
            for t in (tsdf, weight):
                assert t.dtype == torch.float32 and t.numel() == nodes
        else:
            tsdf = torch.empty((int(nz), int(ny), int(nx)), dtype=torch.float32, device="cuda:%d" % self.device)
            weight = torch.empty_like(tsdf)
        n = C.c_longlong(0)
        _chk(lib().nsk_tsdf_integrate(self.h, op, sp, int(nx), int(ny), int(nz), int(K), _ptr(depths) if K else None, int(H), int(W), *_intr4(intr),
                                      wp, int(edge), float(trunc), float(max_weight), int(acc), _ptr(tsdf), _ptr(weight), C.byref(n)))
        return tsdf, weight, int(n.value)

    @_ordered
    def tsdf_volume(self, tsdf, weight, min_weight=1):
        """nsk_tsdf_volume: (volume, valid, n_valid) for extract_mesh at level 0: volume = -tsdf and valid = 1 where weight >= min_weight,
        a quiet NaN and 0 elsewhere.  Shapes follow tsdf.  Synchronises (the count)."""
        import torch
        assert tsdf.dtype == torch.float32 and weight.dtype == torch.float32 and tsdf.numel() == weight.numel()
        vol = torch.empty_like(tsdf)
        valid = torch.empty(tsdf.shape, dtype=torch.uint8, device=tsdf.device)
        n = C.c_longlong(0)
        m = int(tsdf.numel())
        _chk(lib().nsk_tsdf_volume(self.h, m, _ptr(tsdf) if m else None, _ptr(weight) if m else None, float(min_weight), _ptr(vol) if m else None,
                                   _ptr(valid) if m else None, C.byref(n)))
        return vol, valid, int(n.value)

    @staticmethod
    def _lattice_shape(n):
        return (int(n),) * 3 if isinstance(n, int) else tuple(int(x) for x in n)

    def _fused_mesh(self, origin, step, tsdf, weight, n_observed, min_weight, min_area, largest_only):
        """tsdf_volume -> extract_mesh at level 0 -> (asked for) filter_mesh"""
        vol, valid, n_valid = self.tsdf_volume(tsdf, weight, min_weight)
        verts, tris = self.extract_mesh(vol, origin, step, 0.0, valid)
        info = dict(n_observed=n_observed, n_valid=n_valid, n_vertices=int(verts.shape[0]), n_triangles=int(tris.shape[0]))
        if min_area > 0 or largest_only:
            verts, tris, nc, nk = self.filter_mesh(min_area, largest_only)
            info.update(n_components=nc, n_kept=nk, n_vertices=int(verts.shape[0]), n_triangles=int(tris.shape[0]))
        return verts, tris, info

    def fuse_depth_mesh(self, origin, step, n, depths, w2c, intr, HW, trunc=None, min_weight=1, frames_per_batch=32, min_area=0,
                        largest_only=False, edge=0, max_weight=64):
        """The mesh of what the sensor measured: the depth frames depths [K, H, W] (a tensor anywhere, or numpy; streamed to the device
        frames_per_batch at a time, so the trajectory is never resident as a whole) at w2c [K, 4, 4] (host, world-to-camera) fused by
        tsdf_integrate on the lattice origin + (i, j, k) * step, n = nodes per axis (an int, or (nx, ny, nz)); tsdf_volume with min_weight;
        extract_mesh at level 0; filter_mesh only when min_area > 0 or largest_only.  trunc None: three times the largest step -- this
        project's first choice; upstream's ratio of truncation to voxel is about five, but on the sphere scene of tests/tsdf_checks.py
        three gives the tighter surface.  -> (vertices [nv, 3] float32, triangles [nt, 3] int32, dict of counts); the result does not
        depend on frames_per_batch."""
        import numpy as np
        import torch
        nx, ny, nz = self._lattice_shape(n)
        w = np.ascontiguousarray(np.asarray(w2c, np.float32).reshape(-1, 4, 4))
        K, H, W = int(w.shape[0]), int(HW[0]), int(HW[1])
        assert tuple(depths.shape) == (K, H, W), "fuse_depth_mesh: depths must be [K, H, W]"
        if trunc is None:
            trunc = np.float32(3.0) * np.asarray(step, np.float32).max()
        dev = "cuda:%d" % self.device
        batch = max(1, int(frames_per_batch))
        tsdf, weight, n_obs = self.tsdf_integrate(origin, step, nx, ny, nz, torch.empty((0, H, W), dtype=torch.float32, device=dev), intr, w[:0],
                                                  edge, trunc, max_weight)              # (cleared)
        for k0 in range(0, K, batch):
            d = torch.as_tensor(np.ascontiguousarray(depths[k0:k0 + batch]) if isinstance(depths, np.ndarray) else depths[k0:k0 + batch])
            d = d.to(device=dev, dtype=torch.float32).contiguous()
            tsdf, weight, n_obs = self.tsdf_integrate(origin, step, nx, ny, nz, d, intr, w[k0:k0 + batch], edge, trunc, max_weight, (tsdf, weight))
        verts, tris, info = self._fused_mesh(origin, step, tsdf, weight, n_obs, min_weight, min_area, largest_only)
        info.update(trunc=float(trunc), frames=K)
        return verts, tris, info

    def fuse_rendered_mesh(self, stage, origin, step, n, poses, depth_imgs, intr, HW, trunc=None, min_weight=1, chunk_rays=None,
                           gt_depth_max=-1.0, min_area=0, largest_only=False, edge=0, max_weight=64):
        """The mesh of what the map renders: every frame is rendered by render_image at poses[k] ([4, 4] or [3, 4] camera-to-world, host)
        with the sensor depth depth_imgs[k] ([H, W], a tensor anywhere or numpy; None: no guidance) as upstream's render_img does, and the
        rendered depth is integrated at that pose (w2c: the pose inverted in float64, rounded once); the rendered frame never visits the
        host.  Then as fuse_depth_mesh.  -> (vertices, triangles, dict of counts)."""
        import numpy as np
        import torch
        nx, ny, nz = self._lattice_shape(n)
        H, W = int(HW[0]), int(HW[1])
        K = len(poses)
        if trunc is None:
            trunc = np.float32(3.0) * np.asarray(step, np.float32).max()
        dev = "cuda:%d" % self.device
        tsdf, weight, n_obs = self.tsdf_integrate(origin, step, nx, ny, nz, torch.empty((0, H, W), dtype=torch.float32, device=dev), intr,
                                                  np.zeros((0, 4, 4), np.float32), edge, trunc, max_weight)         # (cleared)
        for k in range(K):
            c2w = np.eye(4)
            c2w[:3, :4] = np.asarray(poses[k], np.float64).reshape(-1, 4)[:3]
            pose = torch.as_tensor(np.ascontiguousarray(c2w[:3, :4].astype(np.float32)), device=dev)
            g = None
            if depth_imgs is not None:
                g = torch.as_tensor(depth_imgs[k]).to(device=dev, dtype=torch.float32).contiguous()
            _, depth, _ = self.render_image(stage, HW, intr, pose, g, gt_depth_max=gt_depth_max, chunk_rays=chunk_rays)
            w2c = np.linalg.inv(c2w).astype(np.float32)
            tsdf, weight, n_obs = self.tsdf_integrate(origin, step, nx, ny, nz, depth.view(1, H, W), intr, w2c[None], edge, trunc, max_weight,
                                                      (tsdf, weight))
        verts, tris, info = self._fused_mesh(origin, step, tsdf, weight, n_obs, min_weight, min_area, largest_only)
        info.update(trunc=float(trunc), frames=K)
        return verts, tris, info

    # -- the convex hull of a cloud, the lattice nodes inside it (nsk_hull.h) -------------------------------------------------------------
    @_ordered
    def points_hull(self, points, extra=None):
        """nsk_points_hull: the convex hull of points [n, 3] (float32 cuda tensor, n may be 0) followed by extra [m, 3] (host: anything numpy
        reads, e.g. the camera centres).  -> (vertices int32 [nv] ascending indices into the concatenation, faces int32 [nf, 3] wound
        outwards, info int64 [8]: finite points, left out, rank (3 = a hull), vertices, faces, insertions, the quantum as the bits of a
        double, re-compactions), the arrays numpy.  Without a hull (rank < 3) both arrays are empty.  The hull stays in the context for
        lattice_in_hull.  Synchronises once per hull vertex."""
        import numpy as np
        import torch
        n = 0 if points is None else int(points.shape[0])
        if n:
            assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] == 3
        e = np.zeros((0, 3), np.float32) if extra is None else np.ascontiguousarray(np.asarray(extra, np.float32).reshape(-1, 3))
        info = (C.c_longlong * 8)()
        _chk(lib().nsk_points_hull(self.h, _ptr(points) if n else None, n, e.ctypes.data_as(C.c_void_p) if e.shape[0] else None, int(e.shape[0]), info))
        info = np.array(info[:], np.int64)
        verts, faces = np.zeros(int(info[3]), np.int32), np.zeros((int(info[4]), 3), np.int32)
        _chk(lib().nsk_hull_download(self.h, verts.ctypes.data_as(C.c_void_p), faces.ctypes.data_as(C.c_void_p)))
        return verts, faces, info

    def hull_upload(self, xyz, faces):
        """nsk_hull_upload: a convex mesh of the caller's (xyz [nv, 3], faces [nf, 3] wound outwards, host) as the hull lattice_in_hull uses"""
        import numpy as np
        v = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3)); f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
        _chk(lib().nsk_hull_upload(self.h, v.ctypes.data_as(C.c_void_p), int(v.shape[0]), f.ctypes.data_as(C.c_void_p), int(f.shape[0])))

    @_ordered
    def lattice_in_hull(self, origin, step, nx, ny, nz, scale=1.02, valid=None):
        """nsk_lattice_in_hull: the lattice nodes inside the last hull scaled about its centre (upstream's clean_mesh_bound_scale).  valid:
        uint8 cuda tensor [nz, ny, nx] to OR into (default: a new one).  -> (valid, n_inside)"""
        import torch
        (o, op), (s, sp) = _vec3(origin), _vec3(step)
        acc = valid is not None
        if acc:
            assert valid.dtype == torch.uint8 and valid.numel() == int(nx) * int(ny) * int(nz)
        else:
            valid = torch.empty((int(nz), int(ny), int(nx)), dtype=torch.uint8, device="cuda:%d" % self.device)
        n = C.c_longlong(0)
        _chk(lib().nsk_lattice_in_hull(self.h, op, sp, int(nx), int(ny), int(nz), float(scale), int(acc), _ptr(valid), C.byref(n)))
        return valid, int(n.value)

    def hull_mesh(self, stage, origin, step, n, depths, w2c, intr, HW, centres=None, scale=1.02, level=0.0, trunc=None, min_weight=1,
                  frames_per_batch=32, edge=0, max_weight=64):
        """Upstream's Mesher.get_mesh bound: the depth frames fused as in fuse_depth_mesh; the hull of the fused vertices and the camera
        centres (centres [K, 3] host; None: the translations of the inverted w2c); the lattice nodes inside the hull scaled by `scale`;
        the map's occupancy (eval_lattice of `stage`, fill 100) at those nodes only; extract_mesh at `level` WITH the mask, so no shell is
        drawn along the hull (upstream sets the outside to 100 and meshes the wall that makes).
        -> (vertices, triangles, dict: the fusion's counts, hull info, n_inside, valid)"""
        import numpy as np
        nx, ny, nz = self._lattice_shape(n)
        fv, ft, info = self.fuse_depth_mesh(origin, step, (nx, ny, nz), depths, w2c, intr, HW, trunc, min_weight, frames_per_batch, 0, False, edge,
                                            max_weight)
        if centres is None:
            w = np.asarray(w2c, np.float64).reshape(-1, 4, 4)
            centres = np.stack([np.linalg.inv(m)[:3, 3] for m in w]).astype(np.float32) if w.shape[0] else np.zeros((0, 3), np.float32)
        hv, hf, hinfo = self.points_hull(fv, centres)
        valid, n_inside = self.lattice_in_hull(origin, step, nx, ny, nz, scale)
        vol = self.eval_lattice(stage, origin, step, nx, ny, nz, valid=valid, fill=100.0)
        verts, tris = self.extract_mesh(vol, origin, step, level, valid)
        info = dict(fused=info, hull_vertices=hv, hull_faces=hf, hull_info=hinfo, n_inside=n_inside, valid=valid, fused_vertices=fv)
        return verts, tris, info

    @_ordered
    def raw2outputs(self, raw, z, rays_d, occupancy=False):
        import torch
        N, S = z.shape
        dev = z.device
        rgb = torch.empty(N, 3, device=dev); depth = torch.empty(N, device=dev); var = torch.empty(N, device=dev)
        w = torch.empty(N, S, device=dev)
        _chk(lib().nsk_raw2outputs(self.h, N, S, _ptr(raw), _ptr(z), _ptr(rays_d), int(occupancy), _ptr(rgb), _ptr(depth),
                                   _ptr(var), _ptr(w)))
        return rgb, depth, var, w

    @_ordered
    def importance_resample(self, z, weights, n, det=True, seed=0):
        """nsk_importance_resample: z, weights [N, S] cuda tensors (sorted depths and their compositing weights) -> the [N, S + n] sorted
        depths of the second pass; det: the evenly spaced u, else the hash of (seed, ray, 64 + j) (include/nsk.h)"""
        import torch
        assert z.dtype == torch.float32 and weights.dtype == torch.float32 and z.dim() == 2 and weights.shape == z.shape
        assert z.is_cuda and weights.device == z.device
        N, S = z.shape
        out = torch.empty(N, S + int(n), device=z.device)
        _chk(lib().nsk_importance_resample(self.h, N, S, _ptr(z), _ptr(weights), int(n), int(bool(det)), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                           _ptr(out)))
        return out

    @_ordered
    def render_backward(self, stage, rays_o, rays_d, gt_depth, gt_depth_max, g_rgb, g_depth, g_var=None, flags=GRAD_GRIDS):
        import torch
        N = rays_o.shape[0]
        g_ro = g_rd = None
        if flags & GRAD_RAYS:
            g_ro = torch.empty(N, 3, device=rays_o.device); g_rd = torch.empty(N, 3, device=rays_o.device)
        _chk(lib().nsk_render_backward(self.h, _stage(stage), N, _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth),
                                       C.c_float(gt_depth_max), _ptr(g_rgb), _ptr(g_depth), _ptr(g_var), C.c_uint(flags),
                                       _ptr(g_ro), _ptr(g_rd)))
        return g_ro, g_rd

    @_ordered
    def map_step(self, stage, rays_o, rays_d, gt_depth, gt_color, gt_depth_max=-1.0, w_color=0.2, use_color=True,
                 flags=GRAD_GRIDS | GRAD_DECODERS, loss=None, outputs=None, g_rays=None):
        N = rays_o.shape[0]
        rgb, depth, var = outputs if outputs is not None else (None, None, None)
        g_ro, g_rd = g_rays if g_rays is not None else (None, None)
        _chk(lib().nsk_map_step(self.h, _stage(stage), N, _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth), _ptr(gt_color),
                                C.c_float(gt_depth_max), C.c_float(w_color), int(use_color), C.c_uint(flags), _ptr(loss),
                                _ptr(rgb), _ptr(depth), _ptr(var), _ptr(g_ro), _ptr(g_rd)))

    @_ordered
    def map_prepare(self, stage, rays_o, rays_d, gt_depth, gt_depth_max=-1.0, flags=GRAD_GRIDS | GRAD_DECODERS):
        """nsk_map_prepare: register the NEXT batch before the current batch's map_step; its sampling and cell sort then ride in that step's
        composite / backward / Adam launches (include/nsk.h).  The ray mask remembered for the batch is the BUFFER installed by set_ray_mask
        when this is called; it is read later (inside the current step, or at the batch's own step), so it must not be the buffer the current
        step's mask lives in and must stay unchanged until the batch's step has run."""
        self._prep_keep = (getattr(self, "_ray_mask", None), rays_o, rays_d, gt_depth)      # alive until the next registration
        _chk(lib().nsk_map_prepare(self.h, _stage(stage), rays_o.shape[0], _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth), C.c_float(gt_depth_max), C.c_uint(flags)))

    @_ordered
    def track_step(self, stage, rays_o, rays_d, gt_depth, gt_color, gt_depth_max=-1.0, w_color=0.5, use_color=True,
                   handle_dynamic=True, detach_var=True, flags=GRAD_RAYS, loss=None, g_rays=None):
        N = rays_o.shape[0]
        g_ro, g_rd = g_rays if g_rays is not None else (None, None)
        _chk(lib().nsk_track_step(self.h, _stage(stage), N, _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth), _ptr(gt_color),
                                  C.c_float(gt_depth_max), C.c_float(w_color), int(use_color), int(handle_dynamic),
                                  int(detach_var), C.c_uint(flags), _ptr(loss), _ptr(g_ro), _ptr(g_rd)))

    @_ordered
    def loss_map(self, depth, rgb, gt_depth, gt_color, w_color, use_color):
        import torch
        N = depth.shape[0]
        g_d = torch.empty(N, device=depth.device); g_c = torch.empty(N, 3, device=depth.device)
        loss = torch.zeros(1, device=depth.device)
        _chk(lib().nsk_loss_map(self.h, N, _ptr(depth), _ptr(rgb), _ptr(gt_depth), _ptr(gt_color), C.c_float(w_color),
                                int(use_color), _ptr(g_d), _ptr(g_c), _ptr(loss)))
        return loss, g_d, g_c

    @_ordered
    def loss_track(self, depth, rgb, var, gt_depth, gt_color, w_color, use_color, handle_dynamic, detach_var=True):
        import torch
        N = depth.shape[0]
        dev = depth.device
        g_d = torch.empty(N, device=dev); g_c = torch.empty(N, 3, device=dev); g_v = torch.empty(N, device=dev)
        loss = torch.zeros(1, device=dev)
        _chk(lib().nsk_loss_track(self.h, N, _ptr(depth), _ptr(rgb), _ptr(var), _ptr(gt_depth), _ptr(gt_color),
                                  C.c_float(w_color), int(use_color), int(handle_dynamic), int(detach_var), _ptr(g_d),
                                  _ptr(g_c), _ptr(g_v), _ptr(loss)))
        return loss, g_d, g_c, g_v

    # -- rays / pose ------------------------------------------------------------------------------------------
    @_ordered
    def rays_from_pixels(self, pix_i, pix_j, intr, c2w, mode=0):
        import torch
        n = pix_i.shape[0]
        ro = torch.empty(n, 3, device=c2w.device); rd = torch.empty(n, 3, device=c2w.device)
        fx, fy, cx, cy = intr
        _chk(lib().nsk_rays_from_pixels(self.h, n, _ptr(pix_i), _ptr(pix_j), C.c_float(fx), C.c_float(fy), C.c_float(cx),
                                        C.c_float(cy), _ptr(c2w), mode, _ptr(ro), _ptr(rd)))
        return ro, rd

    @_ordered
    def rays_from_camera(self, pix_i, pix_j, intr, cam, mode=0, want_c2w=False):
        """camera_from_tensor + rays_from_pixels in one launch -> (rays_o, rays_d); want_c2w: -> (rays_o, rays_d, c2w [3, 4]), the matrix the
        launch formed from the pose"""
        import torch
        n = pix_i.shape[0]
        ro = torch.empty(n, 3, device=cam.device); rd = torch.empty(n, 3, device=cam.device)
        c2w = torch.empty(3, 4, device=cam.device) if want_c2w else None
        fx, fy, cx, cy = intr
        _chk(lib().nsk_rays_from_camera(self.h, n, _ptr(pix_i), _ptr(pix_j), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                        _ptr(cam), mode, _ptr(ro), _ptr(rd), _ptr(c2w)))
        return (ro, rd, c2w) if want_c2w else (ro, rd)

    @_ordered
    def pose_step(self, pix_i, pix_j, intr, g_ro, g_rd, cam, m, v, lr, step, mode=0, b1=0.9, b2=0.999, eps=1e-8, g_cam_out=None):
        """rays_backward + camera_backward + adam_vector on the pose in one launch (cam, m, v updated in place)"""
        fx, fy, cx, cy = intr
        _chk(lib().nsk_pose_step(self.h, pix_i.shape[0], _ptr(pix_i), _ptr(pix_j), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                 mode, _ptr(g_ro), _ptr(g_rd), _ptr(cam), _ptr(m), _ptr(v), C.c_float(lr), C.c_float(b1), C.c_float(b2),
                                 C.c_float(eps), int(step), _ptr(g_cam_out)))

    @_ordered
    def pose_step_multi(self, first, count, active, pix_i, pix_j, intr, g_ro, g_rd, cams, m=None, v=None, lr=0.0, step=0, mode=0, b1=0.9, b2=0.999,
                        eps=1e-8, g_cams=None, keep=None):
        """nsk_pose_step_multi: the pose kernels of every frame of a window in one launch.  first / count / active: per-frame ray ranges of the
        batch arrays and "this pose is optimised" flags (host lists); cams [nf, 8] cuda; step >= 1: gradient + Adam (m, v [nf, 8]);
        step == 0: gradients only into g_cams [8 nf + 8] (the N > 1 form; g_cams[8 nf + 1] = kept rays of `keep`)"""
        import numpy as np
        nf = len(first)
        f = np.ascontiguousarray(first, np.int32); c = np.ascontiguousarray(count, np.int32); a = np.ascontiguousarray(active, np.uint8)
        fx, fy, cx, cy = intr
        _chk(lib().nsk_pose_step_multi(self.h, nf, f.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p),
                                       _ptr(pix_i), _ptr(pix_j), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy), mode, _ptr(g_ro), _ptr(g_rd),
                                       _ptr(cams), _ptr(m), _ptr(v), C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps), int(step), _ptr(g_cams),
                                       _ptr(keep), int(keep.shape[0]) if keep is not None else 0))

    def set_depth_max_batch(self, gt_depth=None, keep=None):
        """nsk_set_depth_max_batch: steps given gt_depth_max < 0 take max(gt_depth) over THIS batch (the whole batch a shard belongs to)"""
        self._dmax = (gt_depth, keep)
        _chk(lib().nsk_set_depth_max_batch(self.h, _ptr(gt_depth), _ptr(keep), int(gt_depth.shape[0]) if gt_depth is not None else 0))

    def grad_extra(self, buf=None):
        """nsk_grad_extra: a float32 cuda vector (multiple of 4 floats) that travels with grad_pack / grad_unpack / allreduce_grads_rccl"""
        self._xextra = buf
        _chk(lib().nsk_grad_extra(self.h, _ptr(buf), C.c_size_t(buf.numel() if buf is not None else 0)))

    @_ordered
    def rays_backward(self, pix_i, pix_j, intr, g_ro, g_rd, mode=0):
        import torch
        g = torch.empty(3, 4, device=g_ro.device)
        fx, fy, cx, cy = intr
        _chk(lib().nsk_rays_backward(self.h, pix_i.shape[0], _ptr(pix_i), _ptr(pix_j), C.c_float(fx), C.c_float(fy),
                                     C.c_float(cx), C.c_float(cy), mode, _ptr(g_ro), _ptr(g_rd), _ptr(g)))
        return g

    @_ordered
    def camera_from_tensor(self, cam):
        import torch
        c2w = torch.empty(3, 4, device=cam.device)
        _chk(lib().nsk_camera_from_tensor(self.h, _ptr(cam), _ptr(c2w)))
        return c2w

    @_ordered
    def camera_backward(self, cam, g_c2w):
        import torch
        g = torch.empty(7, device=cam.device)
        _chk(lib().nsk_camera_backward(self.h, _ptr(cam), _ptr(g_c2w), _ptr(g)))
        return g

    def inside_filter(self, rays_o, rays_d, gt_depth):
        return self._inside_filter_u8(rays_o, rays_d, gt_depth).bool()       # (the conversion is a torch op: after the streams were ordered)

    @_ordered
    def _inside_filter_u8(self, rays_o, rays_d, gt_depth):
        import torch
        keep = torch.empty(rays_o.shape[0], dtype=torch.uint8, device=rays_o.device)
        _chk(lib().nsk_inside_filter(self.h, rays_o.shape[0], _ptr(rays_o), _ptr(rays_d), _ptr(gt_depth), _ptr(keep)))
        return keep

    @_ordered
    def adam_vector(self, p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-8):
        _chk(lib().nsk_adam_vector(self.h, p.numel(), _ptr(p), _ptr(g), _ptr(m), _ptr(v), C.c_float(lr), C.c_float(b1),
                                   C.c_float(b2), C.c_float(eps), int(step)))

    # -- optimiser / multi-GPU ----------------------------------------------------------------------------------
    @_ordered
    def adam_step(self, lr, b1=0.9, b2=0.999, eps=1e-8):
        arr = (C.c_float * 6)(*[float(x) for x in lr])
        _chk(lib().nsk_adam_step(self.h, arr, C.c_float(b1), C.c_float(b2), C.c_float(eps)))

    @_ordered
    def graph_begin(self):
        """record (instead of run) the kernels of the following calls; call from inside `with torch.cuda.stream(ctx.tstream)`"""
        _chk(lib().nsk_graph_begin(self.h))

    def graph_end(self):
        gid = C.c_int(-1)
        _chk(lib().nsk_graph_end(self.h, C.byref(gid)))
        return gid.value

    def graph_launch(self, gid):
        _chk(lib().nsk_graph_launch(self.h, gid))

    def graph_destroy(self, gid):
        _chk(lib().nsk_graph_destroy(self.h, gid))

    def adam_reset(self):
        _chk(lib().nsk_adam_reset(self.h))

    @_ordered
    def zero_grads(self):
        _chk(lib().nsk_zero_grads(self.h))

    @_ordered
    def grad_slab(self):
        """the contiguous gradient slab as a torch tensor aliasing context memory (for torch.distributed all-reduce).
        nsk_grad_slab launches the pending decoder-gradient reduction on the context's stream, so the call is stream-ordered
        like every other launching method: the caller's stream waits for it before the exchange reads the slab.  The wrapping
        tensor is cached per (pointer, size): no per-step host work beyond the C call."""
        import torch
        p, n = C.c_void_p(), C.c_size_t()
        _chk(lib().nsk_grad_slab(self.h, C.byref(p), C.byref(n)))
        key = (p.value, n.value)
        if getattr(self, "_slab_key", None) != key:
            self._slab_t = torch.as_tensor(_CudaArray(p.value, n.value), device="cuda:%d" % self.device)
            self._slab_key = key
        return self._slab_t

    @_ordered
    def grad_pack(self):
        """the step's exchange buffer (marked voxels of the touched levels + trainable decoders + loss) as a torch tensor aliasing
        context memory: all-reduce it, then call grad_unpack()"""
        import torch
        p, n = C.c_void_p(), C.c_size_t()
        _chk(lib().nsk_grad_pack(self.h, C.byref(p), C.byref(n)))
        key = (p.value, n.value)
        if getattr(self, "_pack_key", None) != key:
            self._pack_t = torch.as_tensor(_CudaArray(p.value, n.value), device="cuda:%d" % self.device)
            self._pack_key = key
        return self._pack_t

    @_ordered
    def grad_unpack(self):
        _chk(lib().nsk_grad_unpack(self.h))

    def allreduce_grads_rccl(self, comm):
        """nsk_allreduce_grads with a raw ncclComm_t (ctypes pointer)"""
        _chk(lib().nsk_allreduce_grads(self.h, comm))

    def profile_begin(self):
        _chk(lib().nsk_profile_begin(self.h))

    def profile_end(self):
        """{kernel name: (launches, total ms)} measured with HIP events on the context's stream"""
        buf = C.create_string_buffer(8192)
        _chk(lib().nsk_profile_end(self.h, buf, C.c_size_t(8192)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            out[name] = (int(cnt), float(ms))
        return out

    # -- test aids -------------------------------------------------------------------------------------
    def debug_relu_bits(self, which, M):
        """[M, 5, 32] bool: the ReLU "input > 0" bits the last step's forward saved for decoder `which`, by sample"""
        import numpy as np
        out = np.zeros((M, 5, 32), np.uint8)
        _chk(lib().nsk_debug_relu_bits(self.h, STAGES[which] if isinstance(which, str) else int(which), int(M), out.ctypes.data_as(C.c_void_p)))
        return out.astype(bool)

    def debug_fetch(self, what, M):
        """per-sample array of the last step's workspace: "occ0".."occ2" [M], "rgb4" [M, 4], "g_raw" [M, 4], "z" [M],
        "median_thr" [1] (the Tracker's 10 x median threshold)"""
        import numpy as np
        code = {"occ0": 0, "occ1": 1, "occ2": 2, "rgb4": 3, "g_raw": 4, "z": 5, "median_thr": 6}[what]
        out = np.zeros((M, 4) if code in (3, 4) else ((1,) if code == 6 else (M,)), np.float32)
        _chk(lib().nsk_debug_fetch(self.h, code, int(M), out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_live_tiles(self, M):
        """the dead-tile skip of the last step's backward (include/nsk.h): (counts [8] int32, perm [M] int32, bytes [M] uint8)"""
        import numpy as np
        counts, perm, lb = np.zeros(8, np.int32), np.zeros(M, np.int32), np.zeros(M, np.uint8)
        _chk(lib().nsk_debug_live_tiles(self.h, int(M), counts.ctypes.data_as(C.c_void_p), perm.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p)))
        return counts, perm, lb

    FWD_FORMS = (None, "single", "multi", "multi_split", "merged")
    BWD_FORMS = (None, "separate", "multi", "multi_full", "frozen", "track")

    def debug_last_split(self, backward=False):
        """the workgroup split of the last forward decoder launch (or the last backward), as recorded on the host (include/nsk.h): dict with
        form (a name of FWD_FORMS / BWD_FORMS; None: no launch), n, which, train, wgs (tuples of n), scan_wgs, loss_wg, tiles, grid, median_wg"""
        h = (C.c_int * 16)()
        _chk(lib().nsk_debug_last_split(self.h, 1 if backward else 0, h))
        n = int(h[1])
        return dict(form=(self.BWD_FORMS if backward else self.FWD_FORMS)[h[0]], n=n, which=tuple(h[2:2 + n]), train=tuple(h[5:5 + n]),
                    wgs=tuple(h[8:8 + n]), scan_wgs=int(h[11]), loss_wg=int(h[12]), tiles=int(h[13]), grid=int(h[14]), median_wg=int(h[15]))

    DECODER_IMAGES = ("fwd32", "bwd32", "fwd16", "bwd16")

    def debug_decoder_images(self, which, what):
        """uint8 array: the bytes of one device image of decoder `which` (include/nsk.h) -- what = a name of DECODER_IMAGES or its index:
        the fp32 forward / backward image, the forward image in 16-bit pieces + fp32 tail, the fp16 backward image + fp32 tail
        (empty for an image the decoder does not have)"""
        import numpy as np
        w = STAGES[which] if isinstance(which, str) else int(which)
        code = self.DECODER_IMAGES.index(what) if isinstance(what, str) else int(what)
        n = lib().nsk_debug_decoder_images(self.h, w, code, None, C.c_size_t(0))
        if n < 0:
            _chk(n)
        out = np.zeros(n, np.uint8)
        if n:
            got = lib().nsk_debug_decoder_images(self.h, w, code, out.ctypes.data_as(C.c_void_p), C.c_size_t(n))
            if got != n:
                _chk(-1 if got < 0 else 0)
                raise NskError("nsk_debug_decoder_images: the image changed size between two calls (%d, %d bytes)" % (n, got))
        return out

    @_ordered
    def debug_preact(self, which, rays_o, rays_d, M):
        """[M, 5, 32] float32: the ReLU inputs of decoder `which` over the samples of the last step (current matmul mode)"""
        import torch
        out = torch.zeros((M, 5, 32), dtype=torch.float32, device=rays_o.device)
        _chk(lib().nsk_debug_preact(self.h, STAGES[which] if isinstance(which, str) else int(which), int(rays_o.shape[0]), _ptr(rays_o), _ptr(rays_d), _ptr(out)))
        self.sync()
        return out.cpu().numpy()

    def last_call_stats(self):
        b, f, s = C.c_double(), C.c_double(), C.c_int()
        _chk(lib().nsk_last_call_stats(self.h, C.byref(b), C.byref(f), C.byref(s)))
        return b.value, f.value, s.value

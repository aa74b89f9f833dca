// nsk_view.h -- does frame k see the point p, and through which pixel?  The one statement of that rule on the device: the seen mask of a
// lattice (k_lattice_seen, nsk_mesh.h), the cull to a trajectory (k_points_seen / k_points_view_counts, nsk_cull.h) and the depth fusion
// (k_tsdf_integrate, nsk_tsdf.h) all decide it through the functions below, so `weight > 0` of a fusion is the seen mask bit for bit.
// (The rasteriser's projection, nsk_raster.h, is another rule: per triangle, continuous pixel boxes.)
//
// The rule, word for word (include/nsk.h; tests/mesh_cull_checks.py project_f32 / seen_f32 restate it one numpy operation per fp32
// operation).  Frame k sees the point p when, every operation an fp32 operation of its own (no FMA):
//   c_a = ((w[4a] p0 + w[4a+1] p1) + w[4a+2] p2) + w[4a+3], a = 0..2;   d = -c_2 > 0;
//   u = cx + (fx c_0) / d,  v = cy - (fy c_1) / d;   i = floor(u + 0.5), j = floor(v + 0.5)   (the nearest pixel);
//   edge <= i < W - edge and edge <= j < H - edge, decided on the floats (a NaN fails);
//   D = d_depth[k][j][i] is finite and > 0;   d <= D + reach   (reach: the callers' trunc / eps).
#pragma once
#include <hip/hip_runtime.h>
#include "nsk_device.h"

#define VIEW_MAX_K 32               // frames (views) per launch: 12 floats each in the kernel arguments
#define VIEW_FLT_MAX 3.402823466e38f
struct ViewArgs {
    float w[VIEW_MAX_K][12];        // rows 0..2 of the row-major world-to-camera matrices
    int K, H, W;
    float fx, fy, cx, cy;
    float ilo, ihi, jlo, jhi;       // edge <= i < W - edge, edge <= j < H - edge, as floats (exact: H, W <= 2^24)
    float reach;
    int accumulate;
};

// camera space and the nearest pixel of p under the frame's matrix; false: behind the camera or outside the edge bounds
__device__ __forceinline__ bool view_project(const ViewArgs& A, const float* __restrict__ w, const float p[3], float& d, float& fi, float& fj)
{
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        c[a] = __fadd_rn(__fadd_rn(__fadd_rn(mul_rn(w[4 * a], p[0]), mul_rn(w[4 * a + 1], p[1])), mul_rn(w[4 * a + 2], p[2])), w[4 * a + 3]);
    d = -c[2];
    if (!(d > 0.f)) return false;
    const float u = __fadd_rn(A.cx, __fdiv_rn(mul_rn(A.fx, c[0]), d));
    const float v = __fsub_rn(A.cy, __fdiv_rn(mul_rn(A.fy, c[1]), d));
    fi = floorf(__fadd_rn(u, 0.5f)); fj = floorf(__fadd_rn(v, 0.5f));
    return fi >= A.ilo && fi < A.ihi && fj >= A.jlo && fj < A.jhi;                      // (NaN fails; decided before any conversion to int)
}
// frame kf's depth at the pixel view_project found (depth: the launch's first frame)
__device__ __forceinline__ float view_pixel(const ViewArgs& A, const float* __restrict__ depth, int kf, float fi, float fj)
{
    return depth[(size_t)kf * ((size_t)A.H * A.W) + (size_t)(int)fj * A.W + (int)fi];
}
// a measurement; not one: 0, negative, NaN, inf
__device__ __forceinline__ bool view_measured(float D) { return D > 0.f && D <= VIEW_FLT_MAX; }

// *counter += the lanes of the wave with `on`: one add per wave (an integer count: any order, the same number).  Every lane calls it.
template <typename T>
__device__ __forceinline__ void wave_count(bool on, T* __restrict__ counter)
{
    const unsigned long long b = __ballot(on);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (T)__popcll(b));
}

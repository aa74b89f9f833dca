// nsk_icp.h -- point-to-point ICP between two clouds on the grid of nsk_cloud.h: the query that transforms the source on load, the pair
// sums behind the rigid solve (csrc/nsk_rigid.h, on the host) and the transform of a cloud.  (Upstream NICE-SLAM: src/tools/eval_recon.py
// get_align_transformation -- Open3D's registration_icp; include/nsk.h states the contract.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_cloud.h"

#define ICP_COLS 18                          // the 17 pair sums and the number of sources whose transformed point is not finite

// the first three rows of the row-major 4x4 M; a kernel argument, so its twelve doubles arrive by scalar loads
struct CloudXform { double m[12]; };

// s'_a = ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3] in double from the float32 point, every product and sum an operation of its own,
// rounded once to float32.  A point with a component that is not finite is passed on as it is (0 inf would make its other components NaN
// with a sign and payload of the machine's choosing).
__device__ __forceinline__ void cloud_xform(const CloudXform& X, float x, float y, float z, float (&out)[3])
{
#pragma clang fp contract(off)
    if (!(finite_f32(x) && finite_f32(y) && finite_f32(z))) { out[0] = x; out[1] = y; out[2] = z; return; }
    const double dx = (double)x, dy = (double)y, dz = (double)z;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p0 = X.m[4 * a] * dx, p1 = X.m[4 * a + 1] * dy, p2 = X.m[4 * a + 2] * dz;
        out[a] = (float)(((p0 + p1) + p2) + X.m[4 * a + 3]);
    }
}

__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_transform(CloudXform X, int n, const float* in, float* out)      // (in == out is allowed)
{
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (p >= n) return;
    float s[3];
    cloud_xform(X, in[3 * (size_t)p], in[3 * (size_t)p + 1], in[3 * (size_t)p + 2], s);
    out[3 * (size_t)p] = s[0]; out[3 * (size_t)p + 1] = s[1]; out[3 * (size_t)p + 2] = s[2];
}

// k_cloud_cells for the transformed sources (every source gets a cell: the ordering only decides who runs beside whom)
__global__ __launch_bounds__(CLOUD_BLOCK) void k_icp_cells(CloudGrid G, CloudXform X, int n, const float* __restrict__ src,
                                                          unsigned* __restrict__ cell, unsigned* __restrict__ hist)
{
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (p >= n) return;
    float s[3];
    cloud_xform(X, src[3 * (size_t)p], src[3 * (size_t)p + 1], src[3 * (size_t)p + 2], s);
    const int cx = cloud_cell_axis(s[0], G.lo[0], G.h, G.inv_h, G.dim[0]), cy = cloud_cell_axis(s[1], G.lo[1], G.h, G.inv_h, G.dim[1]),
              cz = cloud_cell_axis(s[2], G.lo[2], G.h, G.inv_h, G.dim[2]);
    const unsigned id = ((unsigned)cz * G.dim[1] + cy) * G.dim[0] + cx;
    cell[p] = id;
    atomicAdd(hist + id, 1u);
}

// k_cloud_query with the query formed on load: no transformed copy of the source exists anywhere.  dist / index are written by source index
template <int LANES>
__global__ __launch_bounds__(CLOUD_BLOCK) void k_icp_query(CloudGrid G, CloudXform X, int nq, const float* __restrict__ src,
                                                          const unsigned* __restrict__ qperm, const unsigned* __restrict__ start,
                                                          const float4* __restrict__ sorted4, float* __restrict__ dist, int* __restrict__ index)
{
    const long long slot = ((long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x) / LANES;
    const int lane = threadIdx.x % LANES;
    if (slot >= nq) return;                                     // (LANES = 64: the whole wave leaves)
    const size_t qi = qperm ? qperm[slot] : (size_t)slot;
    float q[3];
    cloud_xform(X, src[3 * qi], src[3 * qi + 1], src[3 * qi + 2], q);
    cloud_answer<LANES>(G, q, lane, start, sorted4, qi, dist, index);
}

// The pair sums: source p counts when its transformed point s' is finite and d <= threshold (inclusive, on the fp32 distance; NaN and the
// +inf of "no finite target" fail it).  Columns: [0] the count, [1] sum d d (the fp32 d widened, squared in double), [2..4] sum s',
// [5..7] sum t, [8..16] sum s'_a t_b (fp32 values widened, products in double), [17] the sources with s' not finite.  The association is
// that of nsk_reduce.h
__global__ __launch_bounds__(CLOUD_BLOCK) void k_icp_sums(CloudXform X, int n, const float* __restrict__ src, const float* __restrict__ dist,
                                                         const int* __restrict__ index, const float* __restrict__ target, float threshold,
                                                         double* __restrict__ rows)
{
#pragma clang fp contract(off)
    double acc[ICP_COLS];
#pragma unroll
    for (int k = 0; k < ICP_COLS; ++k) acc[k] = 0.0;
    for (long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x; p < n; p += (long long)gridDim.x * CLOUD_BLOCK) {
        float s[3];
        cloud_xform(X, src[3 * (size_t)p], src[3 * (size_t)p + 1], src[3 * (size_t)p + 2], s);
        if (!(finite_f32(s[0]) && finite_f32(s[1]) && finite_f32(s[2]))) { acc[17] += 1.0; continue; }
        const float d = dist[p];
        const int j = index[p];
        if (j < 0 || !(d <= threshold)) continue;
        const double dd = (double)d;
        double sv[3], tv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { sv[a] = (double)s[a]; tv[a] = (double)target[3 * (size_t)j + a]; }
        acc[0] += 1.0;
        acc[1] += dd * dd;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[2 + a] += sv[a]; acc[5 + a] += tv[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += sv[a] * tv[b];
        }
    }
    rows_store<RowSums<ICP_COLS>>(acc, rows + (size_t)blockIdx.x * ICP_COLS);
}

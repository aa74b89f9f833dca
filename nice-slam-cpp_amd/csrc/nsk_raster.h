// nsk_raster.h -- depth images of a triangle mesh (nsk_mesh_depth) and the per-view sums of two depth stacks (nsk_depth_pair_stats): what
// upstream NICE-SLAM's 2D reconstruction number, Depth L1, is made of.  (Upstream: src/tools/eval_recon.py calc_2d_metric, which renders
// both meshes in an Open3D window; include/nsk.h states the rule, tests/raster_checks.py restates it in numpy float32.)
// Every operation of the rule is an fp32 operation of its own (mul_rn / add_rn / sub_rn / div_rn: no FMA), and the inline walk and the
// queued walk go through the same three functions, so which of them visits a pixel changes no bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_device.h"
#include "nsk_reduce.h"

#define RASTER_MAX_V 32                     // views per launch: 12 floats each in the kernel arguments
#define RASTER_BLOCK 256
#define RASTER_QUEUE_WG 1024                // workgroups of the queue kernel (4 waves each)
#define RASTER_INF_BITS 0x7f800000u         // +inf: "nothing hit yet"; positive floats order as their bits
#define RASTER_STAT_ROWS 64                 // partial rows per view of nsk_depth_pair_stats

struct RasterArgs {
    float w[RASTER_MAX_V][12];              // rows 0..2 of the row-major world-to-camera matrices
    int K, H, W;
    float fx, fy, cx, cy;
    int nv, nt;
    int inline_max;                         // a box of more pixels goes to the queue
    unsigned queue_cap;
    int load_first;                         // a plain load in front of the atomic
};
struct RasterJob { int view, tri, x0, x1, y0, y1; };
// what a pixel needs of a (triangle, view) pair
struct RasterSetup { float nbc[3], nca[3], nab[3], n[3], num; };

__device__ __forceinline__ void raster_cross(const float* p, const float* q, float* n)
{
    n[0] = sub_rn(mul_rn(p[1], q[2]), mul_rn(p[2], q[1]));
    n[1] = sub_rn(mul_rn(p[2], q[0]), mul_rn(p[0], q[2]));
    n[2] = sub_rn(mul_rn(p[0], q[1]), mul_rn(p[1], q[0]));
}
// (x n_x + y n_y) - n_z: the ray (x, y, -1) against a normal
__device__ __forceinline__ float raster_edge(float x, float y, const float* n) { return sub_rn(add_rn(mul_rn(x, n[0]), mul_rn(y, n[1])), n[2]); }

// camera space of the three vertices; false when a component is not finite (the triangle is left out of this view)
__device__ __forceinline__ bool raster_camera(const float* w, const float v[3][3], float c[3][3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[k][a] = add_rn(add_rn(add_rn(mul_rn(w[4 * a], v[k][0]), mul_rn(w[4 * a + 1], v[k][1])), mul_rn(w[4 * a + 2], v[k][2])), w[4 * a + 3]);
            ok = ok && finite_f32(c[k][a]);
        }
    return ok;
}

// the pixel box of the rule; false when the triangle has no pixel in this view
__device__ __forceinline__ bool raster_box(const RasterArgs& A, const float c[3][3], int& x0, int& x1, int& y0, int& y1)
{
    const float d0 = -c[0][2], d1 = -c[1][2], d2 = -c[2][2];
    if (d0 <= 0.f && d1 <= 0.f && d2 <= 0.f) return false;                  // behind the camera
    x0 = 0; x1 = A.W - 1; y0 = 0; y1 = A.H - 1;                             // crossing the camera plane, or a projection out of range
    if (d0 > 0.f && d1 > 0.f && d2 > 0.f) {
        const float u0 = add_rn(A.cx, div_rn(mul_rn(A.fx, c[0][0]), d0)), v0 = sub_rn(A.cy, div_rn(mul_rn(A.fy, c[0][1]), d0));
        const float u1 = add_rn(A.cx, div_rn(mul_rn(A.fx, c[1][0]), d1)), v1 = sub_rn(A.cy, div_rn(mul_rn(A.fy, c[1][1]), d1));
        const float u2 = add_rn(A.cx, div_rn(mul_rn(A.fx, c[2][0]), d2)), v2 = sub_rn(A.cy, div_rn(mul_rn(A.fy, c[2][1]), d2));
        const float lim = 1048576.f;                                         // 2^20 (a NaN fails the comparison)
        if (fabsf(u0) < lim && fabsf(u1) < lim && fabsf(u2) < lim && fabsf(v0) < lim && fabsf(v1) < lim && fabsf(v2) < lim) {
            const float ulo = floorf(fminf(u0, fminf(u1, u2))) - 1.f, uhi = floorf(fmaxf(u0, fmaxf(u1, u2))) + 2.f;     // (exact below 2^20)
            const float vlo = floorf(fminf(v0, fminf(v1, v2))) - 1.f, vhi = floorf(fmaxf(v0, fmaxf(v1, v2))) + 2.f;
            x0 = (int)fmaxf(ulo, 0.f); x1 = (int)fminf(uhi, (float)(A.W - 1));
            y0 = (int)fmaxf(vlo, 0.f); y1 = (int)fminf(vhi, (float)(A.H - 1));
            if (x0 > x1 || y0 > y1) return false;
        }
    }
    return true;
}

__device__ __forceinline__ void raster_setup(const float c[3][3], RasterSetup& S)
{
    raster_cross(c[1], c[2], S.nbc); raster_cross(c[2], c[0], S.nca); raster_cross(c[0], c[1], S.nab);
    float e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { e1[a] = sub_rn(c[1][a], c[0][a]); e2[a] = sub_rn(c[2][a], c[0][a]); }
    raster_cross(e1, e2, S.n);
    S.num = add_rn(add_rn(mul_rn(c[0][0], S.n[0]), mul_rn(c[0][1], S.n[1])), mul_rn(c[0][2], S.n[2]));
}

// one pixel of the box: inside by the three edge values, depth from the plane, the minimum kept in the image (uint32 bits of t; i < W and
// j < H are the caller's business: the box is clamped to the image)
__device__ __forceinline__ void raster_pixel(const RasterArgs& A, const RasterSetup& S, int i, int j, unsigned* __restrict__ img)
{
    const float x = div_rn(sub_rn((float)i, A.cx), A.fx), y = -div_rn(sub_rn((float)j, A.cy), A.fy);
    const float U = raster_edge(x, y, S.nbc), V = raster_edge(x, y, S.nca), Wv = raster_edge(x, y, S.nab);
    if (!((U >= 0.f && V >= 0.f && Wv >= 0.f) || (U <= 0.f && V <= 0.f && Wv <= 0.f))) return;
    const float t = div_rn(S.num, raster_edge(x, y, S.n));
    if (!(t > 0.f && t < __builtin_inff())) return;
    const unsigned bits = __float_as_uint(t);
    unsigned* p = img + (size_t)j * A.W + i;
    if (A.load_first && __atomic_load_n(p, __ATOMIC_RELAXED) <= bits) return;       // (a stale value is safe: values only fall)
    atomicMin(p, bits);
}

__device__ __forceinline__ bool raster_load_tri(const RasterArgs& A, const int* __restrict__ tris, const float* __restrict__ verts, long long t,
                                                float v[3][3])
{
    const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
    if (i0 < 0 || i0 >= A.nv || i1 < 0 || i1 >= A.nv || i2 < 0 || i2 >= A.nv) return false;
    const int ix[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) v[k][a] = verts[3 * (size_t)ix[k] + a];
    return true;
}

// One thread per triangle: its vertices are loaded once, the views of the launch looped over.  A small box is walked here; a large one
// goes to the queue (one atomic cursor; order irrelevant), and when the queue is full it is walked here after all.
// depth: [K][H][W] uint32, the views of this launch.  skipped (or NULL): triangles with an index outside [0, nv).
__global__ __launch_bounds__(RASTER_BLOCK) void k_raster_tris(RasterArgs A, const float* __restrict__ verts, const int* __restrict__ tris,
                                                             unsigned* __restrict__ depth, RasterJob* __restrict__ queue,
                                                             unsigned* __restrict__ cursor, unsigned* __restrict__ skipped)
{
    const long long t = (long long)blockIdx.x * RASTER_BLOCK + threadIdx.x;
    const bool live = t < A.nt;
    float v[3][3];
    const bool good = live && raster_load_tri(A, tris, verts, t, v);
    if (skipped) {
        const unsigned long long b = __ballot(live && !good);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(skipped, (unsigned)__popcll(b));       // (an integer count: any order, the same number)
    }
    if (!good) return;
    const size_t img = (size_t)A.H * A.W;
    for (int k = 0; k < A.K; ++k) {
        float c[3][3];
        if (!raster_camera(A.w[k], v, c)) continue;
        int x0, x1, y0, y1;
        if (!raster_box(A, c, x0, x1, y0, y1)) continue;
        const int npix = (x1 - x0 + 1) * (y1 - y0 + 1);                     // (at most H W <= 2^24)
        if (npix > A.inline_max) {
            const unsigned slot = atomicAdd(cursor, 1u);                    // (at most nt K < 2^32 increments)
            if (slot < A.queue_cap) {
                RasterJob J; J.view = k; J.tri = (int)t; J.x0 = x0; J.x1 = x1; J.y0 = y0; J.y1 = y1;
                queue[slot] = J;
                continue;
            }
        }
        RasterSetup S;
        raster_setup(c, S);
        unsigned* out = depth + (size_t)k * img;
        for (int j = y0; j <= y1; ++j)
            for (int i = x0; i <= x1; ++i) raster_pixel(A, S, i, j, out);
    }
}

// The queue: a wave per entry strides over the entry's box 64 pixels at a time.  With fewer entries than waves an entry is shared by
// floor(waves / entries) waves, each taking every share-th group of 64 pixels (a box room's 12 walls would otherwise keep 12 waves busy).
__global__ __launch_bounds__(RASTER_BLOCK) void k_raster_queue(RasterArgs A, const float* __restrict__ verts, const int* __restrict__ tris,
                                                              unsigned* __restrict__ depth, const RasterJob* __restrict__ queue,
                                                              const unsigned* __restrict__ cursor)
{
    const unsigned filled = *cursor;
    const unsigned count = filled < A.queue_cap ? filled : A.queue_cap;
    if (!count) return;
    const unsigned nw = gridDim.x * (RASTER_BLOCK / 64), wave = blockIdx.x * (RASTER_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned share = nw / count > 1 ? nw / count : 1;
    const size_t img = (size_t)A.H * A.W;
    for (unsigned long long item = wave; item < (unsigned long long)count * share; item += nw) {
        const unsigned e = (unsigned)(item / share), sub = (unsigned)(item % share);
        const RasterJob J = queue[e];
        float v[3][3], c[3][3];
        if (!raster_load_tri(A, tris, verts, J.tri, v) || !raster_camera(A.w[J.view], v, c)) continue;     // (k_raster_tris queued neither)
        RasterSetup S;
        raster_setup(c, S);
        unsigned* out = depth + (size_t)J.view * img;
        const int bw = J.x1 - J.x0 + 1, npix = bw * (J.y1 - J.y0 + 1);
        for (long long p = (long long)sub * 64 + lane; p < npix; p += 64ll * share) {
            const int r = (int)(p / bw);
            raster_pixel(A, S, J.x0 + (int)(p - (long long)r * bw), J.y0 + r, out);
        }
    }
}

// +inf (nothing hit) becomes 0, the background value of upstream's renderer and the "no measurement" of nsk_image_metrics
__global__ __launch_bounds__(RASTER_BLOCK) void k_raster_finish(size_t n, unsigned* __restrict__ depth)
{
    for (size_t p = (size_t)blockIdx.x * RASTER_BLOCK + threadIdx.x; p < n; p += (size_t)gridDim.x * RASTER_BLOCK)
        if (depth[p] == RASTER_INF_BITS) depth[p] = 0u;
}

// ---- per-view sums of two depth stacks (nsk_depth_pair_stats) ---------------------------------------------------------------------------
// Workgroup (view, r) of R per view writes one row {sum |a - b|, pixels with a > 0 and b > 0, sum |a - b| over those, pixels with a > 0}
// in the association of nsk_reduce.h, a view being a group of R rows.  R is a function of n_pix alone.
__global__ __launch_bounds__(RASTER_BLOCK) void k_depth_pair_stats(int n_pix, int R, const float* __restrict__ a, const float* __restrict__ b,
                                                                  double* __restrict__ rows)
{
    const size_t view = blockIdx.x / R;
    const int r = blockIdx.x % R;
    const float* pa = a + view * (size_t)n_pix;
    const float* pb = b + view * (size_t)n_pix;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = r * RASTER_BLOCK + threadIdx.x; p < n_pix; p += R * RASTER_BLOCK) {
        const float x = pa[p], y = pb[p];
        const float d = fabsf(sub_rn(x, y));
        const bool fin = finite_f32(d), both = x > 0.f && y > 0.f;
        if (fin) acc[0] += (double)d;
        if (both) acc[1] += 1.0;
        if (both && fin) acc[2] += (double)d;
        if (x > 0.f) acc[3] += 1.0;
    }
    rows_store<RowSums<4>>(acc, rows + (size_t)blockIdx.x * 4);
}

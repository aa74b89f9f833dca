// nsk_cloud.h -- reconstruction metrics: area-weighted surface samples of a triangle mesh, exact nearest-point distances between two
// point clouds through a uniform grid, and the reductions behind accuracy / completion / completion ratio.
// (Upstream NICE-SLAM: src/tools/eval_recon.py -- trimesh's sample_surface and a KD-tree; include/nsk.h states the contract.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_reduce.h"

#define CLOUD_BLOCK 256
#define CLOUD_MAX_CELLS (1 << 22)
#define CLOUD_MAX_ROWS 1024
#define CLOUD_ORDER_MIN (1 << 19)            // queries from which on they are visited in cell order
#define CLOUD_CELL_CLAMP 268435456.f        // 2^28: an unclamped query cell plus a shell radius stays inside an int

// the correctly rounded fp32 square root: the fp64 root is correctly rounded, and rounding it again to 24 bits cannot differ from rounding
// the exact root (53 >= 2 * 24 + 2).  (__fsqrt_rn is the native instruction here, 1 ulp.)
__device__ __forceinline__ float cloud_sqrt_rn(float x) { return (float)sqrt((double)x); }

// ---- mesh sampling ----------------------------------------------------------------------------------------------------------------
// A_t = 0.5 |(b - a) x (c - a)| in double from the float32 vertices; not finite, not positive or an index outside [0, nv): area 0, counted.
// cum[t] = the inclusive sum inside the workgroup, bsum[workgroup] = its total
__global__ __launch_bounds__(CLOUD_BLOCK) void k_tri_area(int nv, int nt, const float* __restrict__ verts, const int* __restrict__ tris,
                                                         double* __restrict__ cum, double* __restrict__ bsum, unsigned* __restrict__ degenerate)
{
    const long long t = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    double area = 0.0;
    bool bad = false;
    if (t < nt) {
        const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) bad = true;
        else {
            double e[3], f[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double a = (double)verts[3 * (size_t)i0 + q];
                e[q] = (double)verts[3 * (size_t)i1 + q] - a; f[q] = (double)verts[3 * (size_t)i2 + q] - a;
            }
            const double x = e[1] * f[2] - e[2] * f[1], y = e[2] * f[0] - e[0] * f[2], z = e[0] * f[1] - e[1] * f[0];
            area = 0.5 * sqrt(x * x + y * y + z * z);
            if (!(area > 0.0 && area < __builtin_inf())) { area = 0.0; bad = true; }      // (NaN fails the comparison)
        }
    }
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(degenerate, (unsigned)__popcll(b));         // (an integer count: any order, the same number)
    double total;
    const double inc = block_scan(area, &total);
    if (t < nt) cum[t] = inc;
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// one workgroup: the exclusive scan of the workgroup totals in place.  Thread k owns the k-th run of `per` totals and adds them in index
// order, thread 0 adds the 256 run sums in index order: one fixed association
__global__ __launch_bounds__(CLOUD_BLOCK) void k_tri_area_sums(int nb, double* __restrict__ bsum)
{
    __shared__ double run[CLOUD_BLOCK];
    const int per = (nb + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
    const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
    double s = 0.0;
    for (int b = b0; b < b1; ++b) s += bsum[b];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int k = 0; k < CLOUD_BLOCK; ++k) { const double v = run[k]; run[k] = acc; acc += v; }
    }
    __syncthreads();
    double acc = run[threadIdx.x];
    for (int b = b0; b < b1; ++b) { const double v = bsum[b]; bsum[b] = acc; acc += v; }
}
__global__ __launch_bounds__(CLOUD_BLOCK) void k_tri_area_add(int nt, double* __restrict__ cum, const double* __restrict__ bsum)
{
    const long long t = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (t < nt) cum[t] = bsum[blockIdx.x] + cum[t];
}

// sample s: u_k = (hash_u32(seed, s, k) >> 8) 2^-24; the first triangle with cum[t] > u_0 cum[last]; r = sqrt(u_1),
// p = ((1 - r) a + r (1 - u_2) b) + r u_2 c, every product and sum rounded on its own
__global__ __launch_bounds__(CLOUD_BLOCK) void k_mesh_sample(unsigned long long seed, int n, int nt, const double* __restrict__ cum,
                                                            const float* __restrict__ verts, const int* __restrict__ tris,
                                                            float* __restrict__ points, int* __restrict__ tri_out)
{
    const int s = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (s >= n) return;
    float u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = (float)(hash_u32(seed, (uint32_t)s, (uint32_t)k) >> 8) * (1.0f / 16777216.0f);
    const double x = (double)u[0] * cum[nt - 1];
    int lo = 0, hi = nt - 1;                                 // cum[nt - 1] > x: u_0 < 1 and the total is positive
    while (lo < hi) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if (cum[mid] > x) hi = mid; else lo = mid + 1;
    }
    // (the chosen triangle has a positive area, so its indices are inside the vertex array)
    const int i0 = tris[3 * (size_t)lo], i1 = tris[3 * (size_t)lo + 1], i2 = tris[3 * (size_t)lo + 2];
    const float r = cloud_sqrt_rn(u[1]);
    const float wa = sub_rn(1.f, r), wb = mul_rn(r, sub_rn(1.f, u[2])), wc = mul_rn(r, u[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q)
        points[3 * (size_t)s + q] = add_rn(add_rn(mul_rn(wa, verts[3 * (size_t)i0 + q]), mul_rn(wb, verts[3 * (size_t)i1 + q])),
                                           mul_rn(wc, verts[3 * (size_t)i2 + q]));
    if (tri_out) tri_out[s] = lo;
}

// ---- the grid -------------------------------------------------------------------------------------------------------------------------
// Cubic cells of edge h over the box of the finite targets; an axis with dim 1 has one cell whatever the coordinate.  The planes of an axis
// are the fp32 numbers P(k) = lo + k h (product and sum rounded on their own): monotone in k, and the host keeps h above 8 ulp of the box's
// largest coordinate, so they are distinct.  A target lies in the LARGEST cell k of [0, dim) with P(k) <= x (cell 0 when there is none).
// That makes the two facts the query's stopping bound rests on exact in fp32:  cell >= k (k >= 1) => x >= P(k);  cell < k (k <= dim - 1)
// => x < P(k).
struct CloudGrid {
    float lo[3];
    float h, inv_h;
    int dim[3];
    int nfinite;                    // finite targets (0: every query gets +inf, -1)
};
__device__ __forceinline__ float cloud_plane(float lo, float h, int k) { return add_rn(lo, mul_rn((float)k, h)); }
__device__ __forceinline__ int cloud_cell_axis(float x, float lo, float h, float inv_h, int dim)
{
    if (dim == 1) return 0;
    const float f = floorf(mul_rn(sub_rn(x, lo), inv_h));
    int g = (int)fminf(fmaxf(f, 0.f), (float)(dim - 1));     // (fmaxf / fminf drop a NaN: a non-finite query still gets a cell for the ordering)
    while (g + 1 < dim && cloud_plane(lo, h, g + 1) <= x) ++g;
    while (g > 0 && cloud_plane(lo, h, g) > x) --g;
    return g;
}

// pass 1: box of the finite points and their number.  rows[workgroup] = {min x y z, max x y z, count}: the extrema widen to double exactly
struct CloudBoxCols { static constexpr int N = 7; static constexpr RowOp op(int k) { return k < 3 ? ROW_MIN : (k < 6 ? ROW_MAX : ROW_SUM); } };
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_box(int n, const float* __restrict__ pts, double* __restrict__ rows)
{
    const float inf = __builtin_inff();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf}, cnt = 0.f;
    for (long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x; p < n; p += (long long)gridDim.x * CLOUD_BLOCK) {
        const float x = pts[3 * (size_t)p], y = pts[3 * (size_t)p + 1], z = pts[3 * (size_t)p + 2];
        if (!(finite_f32(x) && finite_f32(y) && finite_f32(z))) continue;
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        cnt += 1.f;                                             // (a lane sees at most n / 256 < 2^24 points: exact)
    }
    const double acc[7] = {(double)mn[0], (double)mn[1], (double)mn[2], (double)mx[0], (double)mx[1], (double)mx[2], (double)cnt};
    rows_store<CloudBoxCols>(acc, rows + (size_t)blockIdx.x * 7);
}

// pass 2: the cell of every point (x fastest) and the histogram.  A target with a non-finite component gets no cell
#define CLOUD_NO_CELL 0xffffffffu
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_cells(CloudGrid G, int n, const float* __restrict__ pts, int keep_nonfinite,
                                                            unsigned* __restrict__ cell, unsigned* __restrict__ hist)
{
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float x = pts[3 * (size_t)p], y = pts[3 * (size_t)p + 1], z = pts[3 * (size_t)p + 2];
    if (!keep_nonfinite && !(finite_f32(x) && finite_f32(y) && finite_f32(z))) { cell[p] = CLOUD_NO_CELL; return; }
    const int cx = cloud_cell_axis(x, G.lo[0], G.h, G.inv_h, G.dim[0]), cy = cloud_cell_axis(y, G.lo[1], G.h, G.inv_h, G.dim[1]),
              cz = cloud_cell_axis(z, G.lo[2], G.h, G.inv_h, G.dim[2]);
    const unsigned id = ((unsigned)cz * G.dim[1] + cy) * G.dim[0] + cx;
    cell[p] = id;
    atomicAdd(hist + id, 1u);
}
// pass 4: into cell order.  The order inside a cell follows the atomics and is not fixed; nothing read from it depends on it (the query
// compares original indices).  sorted4 (targets): x, y, z and the bits of the original index; perm (queries): the original index alone
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_place(int n, const float* __restrict__ pts, const unsigned* __restrict__ cell,
                                                            const unsigned* __restrict__ start, unsigned* __restrict__ cursor,
                                                            float4* __restrict__ sorted4, unsigned* __restrict__ perm)
{
    const long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (p >= n) return;
    const unsigned id = cell[p];
    if (id == CLOUD_NO_CELL) return;
    const unsigned dst = start[id] + atomicAdd(cursor + id, 1u);
    if (sorted4) sorted4[dst] = make_float4(pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2], __uint_as_float((unsigned)p));
    if (perm) perm[dst] = (unsigned)p;
}

// ---- the query ------------------------------------------------------------------------------------------------------------------------
// d2 = (dx dx + dy dy) + dz dz, every operation rounded on its own; the lowest original index among equal d2
struct CloudBest { float d2; int idx; };
__device__ __forceinline__ void cloud_try(CloudBest& B, float qx, float qy, float qz, const float4 t)
{
    const float dx = sub_rn(qx, t.x), dy = sub_rn(qy, t.y), dz = sub_rn(qz, t.z);
    const float d2 = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
    const int idx = (int)__float_as_uint(t.w);
    if (d2 < B.d2 || (d2 == B.d2 && idx < B.idx)) { B.d2 = d2; B.idx = idx; }
}

// LANES lanes per query (1: a thread, 64: a wave whose lanes stride over the points of a row of cells).  The query walks shells of growing
// Chebyshev radius r around its own (unclamped) cell c; shell r = the cells of block(r) = [c - r, c + r]^3 that are not in block(r - 1),
// clipped to the grid; the first r is the first whose block meets the grid.  Cells are stored x fastest, so the cells [x0, x1] of a row
// (y, z) are one run of the sorted targets.
// Stopping: a target that is not in block(r) lies, on some axis a, in a cell below c_a - r or above c_a + r, so by the grid's two facts
// t_a < P(c_a - r) or t_a >= P(c_a + r + 1).  With m = the smallest of max(0, q_a - P(c_a - r)) and max(0, P(c_a + r + 1) - q_a) over the
// faces that have cells behind them (subtractions in fp32), monotone rounding gives |q_a - t_a| (as the kernel rounds it) >= m for that
// axis, and d2 as evaluated >= fl(m m) because the other two squares are not negative and every rounding is monotone.  So the walk ends
// when best < fl(m m) -- strictly: at equality a lower index could still sit outside -- or when no face has cells behind it.
// The walk of one finite query q against a grid with at least one target; every lane of the query's LANES returns the same best.
template <int LANES>
__device__ __forceinline__ CloudBest cloud_walk(const CloudGrid& G, const float (&q)[3], int lane, const unsigned* __restrict__ start,
                                                const float4* __restrict__ sorted4)
{
    static_assert(LANES == 1 || LANES == 64, "a thread or a wave per query");
    int c[3], r = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = 0;
        if (G.dim[a] > 1) {
            const float f = floorf(mul_rn(sub_rn(q[a], G.lo[a]), G.inv_h));
            c[a] = (int)fminf(fmaxf(f, -CLOUD_CELL_CLAMP), CLOUD_CELL_CLAMP);
        }
        r = max(r, max(-c[a], c[a] - (G.dim[a] - 1)));          // the first shell that meets the grid
    }
    CloudBest B = {__builtin_inff(), 0x7fffffff};
    for (;; ++r) {
        const int x0 = max(0, c[0] - r), x1 = min(G.dim[0] - 1, c[0] + r);
        const int y0 = max(0, c[1] - r), y1 = min(G.dim[1] - 1, c[1] + r);
        const int z0 = max(0, c[2] - r), z1 = min(G.dim[2] - 1, c[2] + r);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const size_t row = ((size_t)z * G.dim[1] + y) * G.dim[0];
                const bool full = abs(z - c[2]) == r || abs(y - c[1]) == r;
                // a row on the shell's top / bottom / front / back is walked whole, any other one at its two ends
                for (int part = 0; part < 2; ++part) {
                    int xa, xb;
                    if (full) { if (part) break; xa = x0; xb = x1; }
                    else {
                        xa = xb = part ? c[0] + r : c[0] - r;
                        if (xa < 0 || xa >= G.dim[0]) continue;
                    }
                    const unsigned e = start[row + xb + 1];
                    for (unsigned p = start[row + xa] + lane; p < e; p += LANES) cloud_try(B, q[0], q[1], q[2], sorted4[p]);
                }
            }
        if (LANES > 1)
            B = wave_all(B, [](CloudBest a, CloudBest b) { return b.d2 < a.d2 || (b.d2 == a.d2 && b.idx < a.idx) ? b : a; });
        float m = __builtin_inff();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (G.dim[a] == 1) continue;
            const int klo = c[a] - r, khi = c[a] + r + 1;       // (klo <= dim - 1 and khi >= 1 from the first r on)
            if (klo >= 1) m = fminf(m, fmaxf(0.f, sub_rn(q[a], cloud_plane(G.lo[a], G.h, klo))));
            if (khi <= G.dim[a] - 1) m = fminf(m, fmaxf(0.f, sub_rn(cloud_plane(G.lo[a], G.h, khi), q[a])));
        }
        if (m == __builtin_inff() || B.d2 < mul_rn(m, m)) break;   // (m = inf: the block covers the grid)
    }
    return B;
}
// what a query leaves behind: NaN / -1 when it is not finite, +inf / -1 without a finite target, else the walk's best
template <int LANES>
__device__ __forceinline__ void cloud_answer(const CloudGrid& G, const float (&q)[3], int lane, const unsigned* __restrict__ start,
                                             const float4* __restrict__ sorted4, size_t qi, float* __restrict__ dist, int* __restrict__ index)
{
    if (!(finite_f32(q[0]) && finite_f32(q[1]) && finite_f32(q[2]))) {
        if (lane == 0) { dist[qi] = __builtin_nanf(""); if (index) index[qi] = -1; }
        return;
    }
    if (G.nfinite == 0) {
        if (lane == 0) { dist[qi] = __builtin_inff(); if (index) index[qi] = -1; }
        return;
    }
    const CloudBest B = cloud_walk<LANES>(G, q, lane, start, sorted4);
    if (lane == 0) { dist[qi] = cloud_sqrt_rn(B.d2); if (index) index[qi] = B.idx; }
}
template <int LANES>
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_query(CloudGrid G, int nq, const float* __restrict__ query, const unsigned* __restrict__ qperm,
                                                            const unsigned* __restrict__ start, const float4* __restrict__ sorted4,
                                                            float* __restrict__ dist, int* __restrict__ index)
{
    const long long slot = ((long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x) / LANES;
    const int lane = threadIdx.x % LANES;
    if (slot >= nq) return;                                     // (LANES = 64: the whole wave leaves)
    const size_t qi = qperm ? qperm[slot] : (size_t)slot;
    const float q[3] = {query[3 * qi], query[3 * qi + 1], query[3 * qi + 2]};
    cloud_answer<LANES>(G, q, lane, start, sorted4, qi, dist, index);
}

// ---- the reductions (nsk_cloud_stats) --------------------------------------------------------------------------------------------------
// per workgroup one row {sum of the finite distances, their number, those below the threshold, the largest}, in the association of nsk_reduce.h
struct CloudStatCols { static constexpr int N = 4; static constexpr RowOp op(int k) { return k == 3 ? ROW_MAX : ROW_SUM; } };
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_stats(int n, const float* __restrict__ dist, float threshold, double* __restrict__ rows)
{
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x; p < n; p += (long long)gridDim.x * CLOUD_BLOCK) {
        const float d = dist[p];
        if (!finite_f32(d)) continue;
        acc[0] += (double)d; acc[1] += 1.0;
        if (d < threshold) acc[2] += 1.0;
        acc[3] = fmax(acc[3], (double)d);
    }
    rows_store<CloudStatCols>(acc, rows + (size_t)blockIdx.x * 4);
}

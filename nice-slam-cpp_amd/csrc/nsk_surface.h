// nsk_surface.h -- reconstruction metrics against the surface itself: the exact fp32 distance from a point to a triangle mesh with the
// triangle and the point that attain it (nsk_mesh_nearest), and the normal agreement of triangle pairs (nsk_normal_stats).
// include/nsk.h states the rule word for word; tests/surface_checks.py restates it in numpy and tests/test_gpu_surface.py holds the device
// to that bytes for bytes.  The grid's sizing is host code: nsk_surface_plan.h.
//
// The search.  A uniform grid with CloudGrid's planes and cloud_cell_axis (nsk_cloud.h) over the box of the participating triangles'
// vertices.  A triangle is registered in every cell its box [lo, hi] overlaps: cells cloud_cell_axis(lo_a) .. cloud_cell_axis(hi_a) on
// each axis (count -> exclusive scan -> place; a reference is the triangle's index, and the index finds its packed 48-byte record).  A
// triangle whose range covers more than SURF_WIDE_CELLS cells goes to the wide list instead, which every query tests before its walk.
//
// The walk and why it may stop.  cloud_walk's shells around the query's own (unclamped) cell c and the same m.  A triangle that is not
// registered in any cell of block(r) = [c - r, c + r]^3 has, on some axis a, its whole [lo_a, hi_a] in cells below c_a - r or above
// c_a + r, so by the grid's two facts hi_a < P(c_a - r) or lo_a >= P(c_a + r + 1).  Every candidate point is clamped to [lo, hi] before its
// distance is taken -- an exact operation -- so p_a lies inside [lo_a, hi_a], |fl(q_a - p_a)| >= m by monotone rounding, and d2 as
// evaluated >= fl(m m): the other two squares are not negative and every rounding is monotone.  The walk ends when best < fl(m m),
// strictly (at equality a lower index could still sit outside), or when the block covers the grid.  Every loop is bounded by the grid's
// dimensions.  A triangle met in several cells is tried again: the minimum with the lowest index among equals does not care.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_cloud.h"
#include "nsk_surface_plan.h"

struct SurfTri { float4 a, b, c; };          // 48 bytes: the three vertices; a.w = 1 when the triangle takes part, else 0

// ---- the rule of one triangle -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float surf_dot(const float (&u)[3], const float (&v)[3])
{
    return add_rn(add_rn(mul_rn(u[0], v[0]), mul_rn(u[1], v[1])), mul_rn(u[2], v[2]));
}
__device__ __forceinline__ void surf_cross(const float (&u)[3], const float (&v)[3], float (&r)[3])
{
    r[0] = sub_rn(mul_rn(u[1], v[2]), mul_rn(u[2], v[1]));
    r[1] = sub_rn(mul_rn(u[2], v[0]), mul_rn(u[0], v[2]));
    r[2] = sub_rn(mul_rn(u[0], v[1]), mul_rn(u[1], v[0]));
}
__device__ __forceinline__ void surf_sub(const float (&u)[3], const float (&v)[3], float (&r)[3])
{
    r[0] = sub_rn(u[0], v[0]); r[1] = sub_rn(u[1], v[1]); r[2] = sub_rn(u[2], v[2]);
}
// (((v - u) x (p - u)) . n) >= 0: p is not outside the edge u -> v
__device__ __forceinline__ bool surf_side(const float (&u)[3], const float (&v)[3], const float (&p)[3], const float (&n)[3])
{
    float e[3], w[3], x[3];
    surf_sub(v, u, e); surf_sub(p, u, w); surf_cross(e, w, x);
    return surf_dot(x, n) >= 0.f;
}

struct SurfBest { float d2; int idx; float p[3]; };           // idx = -1: nothing taken yet

// one candidate point of a triangle: clamped to the triangle's box (comparisons, so a NaN stays one and is never taken), its d2 as cloud_try
// forms it, taken when strictly smaller than the triangle's best so far
__device__ __forceinline__ void surf_candidate(SurfBest& T, const float (&q)[3], float (&p)[3], const float (&lo)[3], const float (&hi)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = p[a] < lo[a] ? lo[a] : (p[a] > hi[a] ? hi[a] : p[a]);
    const float dx = sub_rn(q[0], p[0]), dy = sub_rn(q[1], p[1]), dz = sub_rn(q[2], p[2]);
    const float d2 = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
    if (d2 < T.d2) { T.d2 = d2; T.p[0] = p[0]; T.p[1] = p[1]; T.p[2] = p[2]; }
}
// the nearest point of the segment u -> v: t = clamp((w . e) / (e . e), 0, 1), 0 unless e . e > 0
__device__ __forceinline__ void surf_edge(SurfBest& T, const float (&q)[3], const float (&u)[3], const float (&v)[3], const float (&lo)[3],
                                          const float (&hi)[3])
{
    float e[3], w[3], p[3];
    surf_sub(v, u, e); surf_sub(q, u, w);
    const float ee = surf_dot(e, e);
    float t = 0.f;
    if (ee > 0.f) { t = div_rn(surf_dot(w, e), ee); t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t); }
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = add_rn(u[a], mul_rn(t, e[a]));
    surf_candidate(T, q, p, lo, hi);
}
// triangle t against the best so far: the plane candidate, then the edges ab, bc, ca; the lowest triangle among equal d2
__device__ __forceinline__ void surf_try(SurfBest& B, const float (&q)[3], int t, const SurfTri* __restrict__ rec)
{
    const float4 ra = rec[t].a, rb = rec[t].b, rc = rec[t].c;
    const float a[3] = {ra.x, ra.y, ra.z}, b[3] = {rb.x, rb.y, rb.z}, c[3] = {rc.x, rc.y, rc.z};
    float lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(fminf(a[k], b[k]), c[k]); hi[k] = fmaxf(fmaxf(a[k], b[k]), c[k]); }
    SurfBest T;
    T.d2 = __builtin_inff(); T.idx = t; T.p[0] = T.p[1] = T.p[2] = __builtin_nanf("");
    float e0[3], e1[3], n[3], w[3], p[3];
    surf_sub(b, a, e0); surf_sub(c, a, e1); surf_cross(e0, e1, n);
    const float nn = surf_dot(n, n);
    surf_sub(q, a, w);
    const float s = div_rn(surf_dot(w, n), nn);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = sub_rn(q[k], mul_rn(s, n[k]));
    if (nn > 0.f && surf_side(a, b, p, n) && surf_side(b, c, p, n) && surf_side(c, a, p, n)) surf_candidate(T, q, p, lo, hi);
    surf_edge(T, q, a, b, lo, hi);
    surf_edge(T, q, b, c, lo, hi);
    surf_edge(T, q, c, a, lo, hi);
    if (T.d2 < B.d2 || (T.d2 == B.d2 && t < B.idx)) B = T;   // (B.idx = -1 at the start: an untaken +inf never replaces it)
}

// ---- the records and the box ------------------------------------------------------------------------------------------------------------
// rec[t] for every triangle; a triangle takes part when its indices are inside [0, nv), its vertices are finite and its fp64 area (the
// expression of k_tri_area) is finite and positive.  rows[workgroup] = {min x y z, max x y z of the participating vertices, their triangles}
__global__ __launch_bounds__(CLOUD_BLOCK) void k_surf_records(int nv, int nt, const float* __restrict__ verts, const int* __restrict__ tris,
                                                             SurfTri* __restrict__ rec, double* __restrict__ rows)
{
    const float inf = __builtin_inff();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf}, cnt = 0.f;
    for (long long t = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x; t < nt; t += (long long)gridDim.x * CLOUD_BLOCK) {
        const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
        SurfTri R;
        R.a = R.b = R.c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!(i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv)) {
            float v[3][3];
            bool fin = true;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                v[0][q] = verts[3 * (size_t)i0 + q]; v[1][q] = verts[3 * (size_t)i1 + q]; v[2][q] = verts[3 * (size_t)i2 + q];
                fin = fin && finite_f32(v[0][q]) && finite_f32(v[1][q]) && finite_f32(v[2][q]);
            }
            double e[3], f[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double a = (double)v[0][q];
                e[q] = (double)v[1][q] - a; f[q] = (double)v[2][q] - a;
            }
            const double x = e[1] * f[2] - e[2] * f[1], y = e[2] * f[0] - e[0] * f[2], z = e[0] * f[1] - e[1] * f[0];
            const double area = 0.5 * sqrt(x * x + y * y + z * z);
            if (fin && area > 0.0 && area < __builtin_inf()) {
                R.a = make_float4(v[0][0], v[0][1], v[0][2], 1.f);
                R.b = make_float4(v[1][0], v[1][1], v[1][2], 0.f);
                R.c = make_float4(v[2][0], v[2][1], v[2][2], 0.f);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    mn[q] = fminf(mn[q], fminf(fminf(v[0][q], v[1][q]), v[2][q]));
                    mx[q] = fmaxf(mx[q], fmaxf(fmaxf(v[0][q], v[1][q]), v[2][q]));
                }
                cnt += 1.f;                                     // (a lane sees at most nt / 256 < 2^24 triangles: exact)
            }
        }
        rec[t] = R;
    }
    const double acc[7] = {(double)mn[0], (double)mn[1], (double)mn[2], (double)mx[0], (double)mx[1], (double)mx[2], (double)cnt};
    rows_store<CloudBoxCols>(acc, rows + (size_t)blockIdx.x * 7);
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
// the cells a participating triangle's box overlaps: [c0[a], c1[a]] per axis -> their number
__device__ __forceinline__ long long surf_range(const CloudGrid& G, const SurfTri& R, int (&c0)[3], int (&c1)[3])
{
    const float a[3] = {R.a.x, R.a.y, R.a.z}, b[3] = {R.b.x, R.b.y, R.b.z}, c[3] = {R.c.x, R.c.y, R.c.z};
    long long cells = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = cloud_cell_axis(fminf(fminf(a[k], b[k]), c[k]), G.lo[k], G.h, G.inv_h, G.dim[k]);
        c1[k] = cloud_cell_axis(fmaxf(fmaxf(a[k], b[k]), c[k]), G.lo[k], G.h, G.inv_h, G.dim[k]);
        cells *= (long long)(c1[k] - c0[k] + 1);               // (the planes are monotone: c1 >= c0)
    }
    return cells;
}
// pass 2: the histogram of the references, their total (counters[0]) and the wide list with its length (counters[1]); wide has room for
// every triangle
__global__ __launch_bounds__(CLOUD_BLOCK) void k_surf_count(CloudGrid G, int nt, const SurfTri* __restrict__ rec, unsigned* __restrict__ hist,
                                                           int* __restrict__ wide, unsigned long long* __restrict__ counters)
{
    const long long t = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    unsigned long long mine = 0;
    if (t < nt) {
        const SurfTri R = rec[t];
        if (R.a.w != 0.f) {
            int c0[3], c1[3];
            const long long cells = surf_range(G, R, c0, c1);
            if (cells > SURF_WIDE_CELLS) wide[atomicAdd(counters + 1, 1ull)] = (int)t;
            else {
                mine = (unsigned long long)cells;
                for (int z = c0[2]; z <= c1[2]; ++z)
                    for (int y = c0[1]; y <= c1[1]; ++y)
                        for (int x = c0[0]; x <= c1[0]; ++x) atomicAdd(hist + (((size_t)z * G.dim[1] + y) * G.dim[0] + x), 1u);
            }
        }
    }
    unsigned lo = (unsigned)mine;                               // (at most 64 per lane: the wave's sum fits 32 bits)
    lo = wave_all(lo, [](unsigned a, unsigned b) { return a + b; });
    if ((threadIdx.x & 63) == 0 && lo) atomicAdd(counters, (unsigned long long)lo);
}
// pass 4: the references into cell order.  The order inside a cell follows the atomics and is not fixed; nothing read from it depends on it
__global__ __launch_bounds__(CLOUD_BLOCK) void k_surf_place(CloudGrid G, int nt, const SurfTri* __restrict__ rec, const unsigned* __restrict__ start,
                                                           unsigned* __restrict__ cursor, int* __restrict__ refs)
{
    const long long t = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (t >= nt) return;
    const SurfTri R = rec[t];
    if (R.a.w == 0.f) return;
    int c0[3], c1[3];
    if (surf_range(G, R, c0, c1) > SURF_WIDE_CELLS) return;
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const size_t id = ((size_t)z * G.dim[1] + y) * G.dim[0] + x;
                refs[start[id] + atomicAdd(cursor + id, 1u)] = (int)t;
            }
}

// ---- the query --------------------------------------------------------------------------------------------------------------------------
// One thread per query: the wide list, then cloud_walk's shells (the loop of nsk_cloud.h over references instead of points).  G.nfinite is
// the number of participating triangles.
__global__ __launch_bounds__(CLOUD_BLOCK) void k_surf_query(CloudGrid G, int nq, const float* __restrict__ query, const unsigned* __restrict__ qperm,
                                                           const unsigned* __restrict__ start, const int* __restrict__ refs,
                                                           const SurfTri* __restrict__ rec, const int* __restrict__ wide, int nwide,
                                                           float* __restrict__ dist, int* __restrict__ tri, float* __restrict__ point)
{
    const long long slot = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (slot >= nq) return;
    const size_t qi = qperm ? qperm[slot] : (size_t)slot;
    const float q[3] = {query[3 * qi], query[3 * qi + 1], query[3 * qi + 2]};
    SurfBest B;
    B.d2 = __builtin_inff(); B.idx = -1; B.p[0] = B.p[1] = B.p[2] = __builtin_nanf("");
    const bool finite = finite_f32(q[0]) && finite_f32(q[1]) && finite_f32(q[2]);
    if (finite && G.nfinite > 0) {
        for (int w = 0; w < nwide; ++w) surf_try(B, q, wide[w], rec);
        int c[3], r = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c[a] = 0;
            if (G.dim[a] > 1) {
                const float f = floorf(mul_rn(sub_rn(q[a], G.lo[a]), G.inv_h));
                c[a] = (int)fminf(fmaxf(f, -CLOUD_CELL_CLAMP), CLOUD_CELL_CLAMP);
            }
            r = max(r, max(-c[a], c[a] - (G.dim[a] - 1)));      // the first shell that meets the grid
        }
        for (;; ++r) {
            const int x0 = max(0, c[0] - r), x1 = min(G.dim[0] - 1, c[0] + r);
            const int y0 = max(0, c[1] - r), y1 = min(G.dim[1] - 1, c[1] + r);
            const int z0 = max(0, c[2] - r), z1 = min(G.dim[2] - 1, c[2] + r);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const size_t row = ((size_t)z * G.dim[1] + y) * G.dim[0];
                    const bool full = abs(z - c[2]) == r || abs(y - c[1]) == r;
                    for (int part = 0; part < 2; ++part) {
                        int xa, xb;
                        if (full) { if (part) break; xa = x0; xb = x1; }
                        else {
                            xa = xb = part ? c[0] + r : c[0] - r;
                            if (xa < 0 || xa >= G.dim[0]) continue;
                        }
                        const unsigned e = start[row + xb + 1];
                        for (unsigned p = start[row + xa]; p < e; ++p) surf_try(B, q, refs[p], rec);
                    }
                }
            float m = __builtin_inff();
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (G.dim[a] == 1) continue;
                const int klo = c[a] - r, khi = c[a] + r + 1;
                if (klo >= 1) m = fminf(m, fmaxf(0.f, sub_rn(q[a], cloud_plane(G.lo[a], G.h, klo))));
                if (khi <= G.dim[a] - 1) m = fminf(m, fmaxf(0.f, sub_rn(cloud_plane(G.lo[a], G.h, khi), q[a])));
            }
            if (m == __builtin_inff() || B.d2 < mul_rn(m, m)) break;   // (m = inf: the block covers the grid)
        }
    }
    // NaN / -1 / NaN for a non-finite query; +inf / -1 / NaN when no triangle takes part (or none gave a comparable distance)
    dist[qi] = finite ? cloud_sqrt_rn(B.d2) : __builtin_nanf("");
    if (tri) tri[qi] = B.idx;
    if (point) { point[3 * qi] = B.p[0]; point[3 * qi + 1] = B.p[1]; point[3 * qi + 2] = B.p[2]; }
}

// ---- normal agreement (nsk_normal_stats) --------------------------------------------------------------------------------------------------
// n = (b - a) x (c - a) in double from the float32 vertices, every operation on its own; false when the index is outside [0, nt) or a vertex
// index outside [0, nv)
__device__ __forceinline__ bool surf_normal(const float* __restrict__ verts, int nv, const int* __restrict__ tris, int nt, int t, double (&n)[3])
{
    if (t < 0 || t >= nt) return false;
    const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return false;
    double e[3], f[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double a = (double)verts[3 * (size_t)i0 + q];
        e[q] = (double)verts[3 * (size_t)i1 + q] - a; f[q] = (double)verts[3 * (size_t)i2 + q] - a;
    }
    n[0] = dmul(e[1], f[2]) - dmul(e[2], f[1]); n[1] = dmul(e[2], f[0]) - dmul(e[0], f[2]); n[2] = dmul(e[0], f[1]) - dmul(e[1], f[0]);
    return true;
}
__device__ __forceinline__ double surf_ddot(const double (&u)[3], const double (&v)[3]) { return (dmul(u[0], v[0]) + dmul(u[1], v[1])) + dmul(u[2], v[2]); }
// per workgroup one row {sum of cos_i, pairs counted, pairs skipped}, cos_i = |n_A . n_B| / (|n_A| |n_B|), in the association of nsk_reduce.h
__global__ __launch_bounds__(CLOUD_BLOCK) void k_normal_stats(int n, const float* __restrict__ va, int nva, const int* __restrict__ ta, int nta,
                                                             const int* __restrict__ ia, const float* __restrict__ vb, int nvb,
                                                             const int* __restrict__ tb, int ntb, const int* __restrict__ ib, double* __restrict__ rows)
{
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long p = (long long)blockIdx.x * CLOUD_BLOCK + threadIdx.x; p < n; p += (long long)gridDim.x * CLOUD_BLOCK) {
        double na[3], nb[3];
        bool ok = surf_normal(va, nva, ta, nta, ia[p], na) && surf_normal(vb, nvb, tb, ntb, ib[p], nb);
        double cosv = 0.0;
        if (ok) {
            const double la = sqrt(surf_ddot(na, na)), lb = sqrt(surf_ddot(nb, nb));
            ok = la > 0.0 && la < __builtin_inf() && lb > 0.0 && lb < __builtin_inf();
            if (ok) cosv = fabs(surf_ddot(na, nb)) / dmul(la, lb);     // (float32 vertices: |n| < 2^260, the product of two lengths cannot overflow)
        }
        if (ok) { acc[0] += cosv; acc[1] += 1.0; } else acc[2] += 1.0;
    }
    rows_store<RowSums<3>>(acc, rows + (size_t)blockIdx.x * 3);
}

// nsk_cull.h -- a mesh culled to what a trajectory saw, and depth views clear of the unseen (upstream src/tools/cull_mesh.py and the unseen
// points of eval_recon.py's calc_2d_metric).  include/nsk.h states the contract; this file is included by nsk.hip behind the context, the
// buffer helpers and the multi-launch scan (mc_scan), which its entry points use.
//
// The rule: nsk_view.h, with reach = eps (include/nsk.h, nsk_points_seen; tests/cull_checks.py calls tests/mesh_cull_checks.py seen_f32 for it).
// zero_sees: D == 0 is read as FLT_MAX.  No depth: every pixel is read as FLT_MAX.  A point with a non-finite component is never seen.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "nsk_mesh.h"

__device__ __forceinline__ bool cull_finite(float x) { return fabsf(x) <= VIEW_FLT_MAX; }      // (a NaN fails)

// One thread per point.  depth NULL: the frustum alone.
__global__ __launch_bounds__(256) void k_points_seen(ViewArgs A, int n, int zero_sees, const float* __restrict__ pts, const float* __restrict__ depth,
                                                     uint8_t* __restrict__ out, unsigned long long* __restrict__ count)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = q < n;
    bool seen = false, idle = true;                         // idle: no point, or a point no frame can see
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        p[0] = pts[3 * (size_t)q]; p[1] = pts[3 * (size_t)q + 1]; p[2] = pts[3 * (size_t)q + 2];
        seen = A.accumulate && out[q] != 0;
        idle = !(cull_finite(p[0]) && cull_finite(p[1]) && cull_finite(p[2]));
    }
    for (int kf = 0; kf < A.K; ++kf) {
        if (__all(seen || idle)) break;                     // the whole wave is done
        if (seen || idle) continue;
        float d, fi, fj;
        if (!view_project(A, A.w[kf], p, d, fi, fj)) continue;
        float D = VIEW_FLT_MAX;
        if (depth) {
            D = view_pixel(A, depth, kf, fi, fj);
            if (zero_sees && D == 0.f) D = VIEW_FLT_MAX;    // rendered depth: nothing hit, nothing in the way
        }
        if (!view_measured(D)) continue;
        seen = d <= __fadd_rn(D, A.reach);
    }
    if (live) out[q] = seen ? 1 : 0;
    if (count) wave_count(live && seen, count);
}

// One thread per point; every lane of a wave walks every view (the ballot needs them all), one integer add per wave and view.
__global__ __launch_bounds__(256) void k_points_view_counts(ViewArgs A, int n, const float* __restrict__ pts, unsigned* __restrict__ counts)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    float p[3] = {0.f, 0.f, 0.f};
    if (q < n) {
        p[0] = pts[3 * (size_t)q]; p[1] = pts[3 * (size_t)q + 1]; p[2] = pts[3 * (size_t)q + 2];
        ok = cull_finite(p[0]) && cull_finite(p[1]) && cull_finite(p[2]);
    }
    for (int kf = 0; kf < A.K; ++kf) {
        float d, fi, fj;
        wave_count(ok && view_project(A, A.w[kf], p, d, fi, fj), counts + kf);
    }
}

// ---- sub-mesh selection (nsk_mesh_select) ----------------------------------------------------------------------------------------
// tflag[t] = 1 for a kept triangle, vflag[v] = 1 for a vertex a kept triangle names (every writer stores the same 1: no order matters);
// both zeroed before.  A triangle with an index out of range is in neither part and counted.
__global__ __launch_bounds__(256) void k_select_flags(int nv, int nt, const int* __restrict__ tris, const uint8_t* __restrict__ seen, int part,
                                                      unsigned* __restrict__ vflag, unsigned* __restrict__ tflag, unsigned* __restrict__ skipped)
{
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (tl < nt) {
        const size_t t = (size_t)tl;
        const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
        bad = a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv;
        if (!bad) {
            const bool all = seen[a] != 0 && seen[b] != 0 && seen[c] != 0;
            if (all == (part == 0)) { tflag[t] = 1u; vflag[a] = 1u; vflag[b] = 1u; vflag[c] = 1u; }
        }
    }
    wave_count(bad, skipped);
}
// (the compaction behind the scans of these flags: k_mesh_compact, nsk_mesh.h)

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int nsk_points_seen(nsk_ctx* c, const float* pts, int n, int K, const float* depth, int H, int W, float fx, float fy, float cx, float cy,
                               const float* w2c, int edge, float eps, int zero_sees, int accumulate, uint8_t* seen, long long* n_seen)
{
    if (!c) return fail("nsk_points_seen: null ctx");
    if (n < 0 || K < 0) return fail("nsk_points_seen: n = %d, K = %d", n, K);
    if (n > 0 && (!pts || !seen)) return fail("nsk_points_seen: d_points / d_seen is NULL with n = %d", n);
    if (K > 0 && !w2c) return fail("nsk_points_seen: h_w2c is NULL with K = %d", K);
    CHK(view_checks("nsk_points_seen", H, W, fx, fy, cx, cy, edge));
    if (std::isnan(eps)) return fail("nsk_points_seen: eps is NaN");
    if (c->capturing) return fail("nsk_points_seen: not while a graph is being captured");
    if (n_seen) *n_seen = 0;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    CHK(count_begin(c, n_seen, "the seen count"));
    const unsigned nb = (unsigned)(((long long)n + 255) / 256);
    CHK(view_batches(c, "points_seen", view_args(H, W, fx, fy, cx, cy, edge, eps), K, w2c, depth, accumulate,
                     [&](const ViewArgs& A, const float* dk, int, bool last) {
        k_points_seen<<<nb, 256, 0, c->stream>>>(A, n, zero_sees ? 1 : 0, pts, dk, seen, last && n_seen ? c->count.get() : nullptr); }));
    return count_end(c, n_seen);
}

extern "C" int nsk_points_view_counts(nsk_ctx* c, const float* pts, int n, int V, const float* w2c, int H, int W, float fx, float fy, float cx,
                                      float cy, int edge, long long* h_count)
{
    if (!c) return fail("nsk_points_view_counts: null ctx");
    if (n < 0 || V < 0) return fail("nsk_points_view_counts: n = %d, V = %d", n, V);
    if (V > 0 && (!w2c || !h_count)) return fail("nsk_points_view_counts: h_w2c / h_count is NULL with V = %d", V);
    if (n > 0 && !pts) return fail("nsk_points_view_counts: d_points is NULL with n = %d", n);
    CHK(view_checks("nsk_points_view_counts", H, W, fx, fy, cx, cy, edge));
    if (c->capturing) return fail("nsk_points_view_counts: not while a graph is being captured");
    for (int k = 0; k < V; ++k) h_count[k] = 0;
    if (V == 0 || n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Cull& U = c->cull;
    CHK(grow(c, U.view_counts, (size_t)V, "the view counts", GROW_NO_CAPTURE));
    HIPCHK(hipMemsetAsync(U.view_counts, 0, (size_t)V * 4, c->stream));
    const unsigned nb = (unsigned)(((long long)n + 255) / 256);
    CHK(view_batches(c, "points_view_counts", view_args(H, W, fx, fy, cx, cy, edge, 0.f), V, w2c, nullptr, 0,
                     [&](const ViewArgs& A, const float*, int k0, bool) {
        k_points_view_counts<<<nb, 256, 0, c->stream>>>(A, n, pts, U.view_counts.get() + k0); }));
    std::vector<unsigned> h((size_t)V);
    HIPCHK(hipMemcpyAsync(h.data(), U.view_counts, (size_t)V * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < V; ++k) h_count[k] = (long long)h[(size_t)k];
    return 0;
}

extern "C" int nsk_mesh_select(nsk_ctx* c, const float* verts, int nv, const int32_t* tris, int nt, const uint8_t* seen, int part, float* out_v,
                               int32_t* out_t, int32_t* vsrc, int* out_vertices, int* out_triangles, int* h_skipped)
{
    if (!c) return fail("nsk_mesh_select: null ctx");
    if (!out_vertices || !out_triangles) return fail("nsk_mesh_select: out_vertices / out_triangles is NULL");
    if (nv < 0 || nt < 0) return fail("nsk_mesh_select: negative count");
    if (nv > 0x7fffffff / 3 || nt > 0x7fffffff / 3) return fail("nsk_mesh_select: %d vertices, %d triangles, at most %d of each", nv, nt, 0x7fffffff / 3);
    if (part != 0 && part != 1) return fail("nsk_mesh_select: part = %d, must be 0 (seen) or 1 (the complement)", part);
    if (nt > 0 && (!tris || !out_t)) return fail("nsk_mesh_select: d_triangles / d_out_triangles is NULL");
    if (nt > 0 && nv > 0 && (!verts || !seen || !out_v)) return fail("nsk_mesh_select: d_vertices / d_seen / d_out_vertices is NULL");
    if ((out_v && out_v == verts) || (out_t && out_t == tris)) return fail("nsk_mesh_select: the output buffers must not alias the input");
    if (c->capturing) return fail("nsk_mesh_select: not while a graph is being captured");
    *out_vertices = *out_triangles = 0;
    if (h_skipped) *h_skipped = 0;
    if (nt == 0) return 0;                                  // (no triangle names a vertex: nothing stays)
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Cull& U = c->cull;
    const size_t wv = mc_scan_words((size_t)nv + 1), wt = mc_scan_words((size_t)nt + 1);
    CHK(grow(c, U.scan, wv + wt + 64, "the selection's scan scratch", GROW_NO_CAPTURE));
    unsigned* voff = U.scan; unsigned* toff = U.scan + wv; unsigned* skipped = U.scan + wv + wt;
    const unsigned nbt = (unsigned)(((long long)nt + MC_BLOCK - 1) / MC_BLOCK), nbm = (unsigned)(((long long)std::max(nv, nt) + MC_BLOCK - 1) / MC_BLOCK);
    HIPCHK(hipMemsetAsync(U.scan, 0, (wv + wt + 64) * 4, c->stream));   // (the slot behind the last flag turns into the total)
    { ProfScope ps(c, "select_flags"); k_select_flags<<<nbt, MC_BLOCK, 0, c->stream>>>(nv, nt, tris, seen, part, voff, toff, skipped); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "select_scan"); CHK(mc_scan(c, voff, nv + 1)); CHK(mc_scan(c, toff, nt + 1)); }
    { ProfScope ps(c, "select_compact"); k_mesh_compact<<<nbm, MC_BLOCK, 0, c->stream>>>(nv, nt, verts, tris, voff, toff, out_v, out_t, vsrc); }
    HIPCHK(hipGetLastError());
    unsigned tot[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(&tot[0], voff + nv, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tot[1], toff + nt, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tot[2], skipped, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out_vertices = (int)tot[0]; *out_triangles = (int)tot[1];
    if (h_skipped) *h_skipped = (int)tot[2];
    return 0;
}

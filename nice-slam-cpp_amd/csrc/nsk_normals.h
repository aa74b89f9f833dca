// nsk_normals.h -- vertex normals of an indexed mesh (nsk_mesh_vertex_normals), the short rays along them (nsk_normal_rays) and the vertex
// colours those rays composite (nsk_mesh_vertex_colors): upstream's color_mesh_extraction_method render_ray_along_normal.  include/nsk.h states
// the rule word for word; tests/normals_checks.py restates it in numpy and tests/test_gpu_normals.py holds the device to that bytes for bytes.
// This file is included by nsk.hip behind the context, the buffer helpers, the multi-launch scan (mc_scan) and the forward's launches.
//
// The adjacency.  A corner is the number 3 t + k of corner k of triangle t; a vertex's normal is the sum of the face normals of the corners
// that name it, in ascending corner number.  Face normals are formed once (k_vn_face, which also counts every vertex's namings), the counts
// are scanned (mc_scan), and every corner is placed into its vertex's segment of one list through an integer cursor (k_vn_place).  The cursor
// hands out slots in arrival order, so a segment is then SORTED (k_vn_sort: one thread per vertex, a fixed network on registers for segments
// of up to VN_REG corners, an insertion sort in place up to VN_SHORT; k_vn_sort_long: a workgroup per longer segment, a bitonic network in
// place in global memory).  Sorting afterwards instead of ranking at placement: a rank is the number of earlier corners with the same
// vertex, which no pass over corners knows without a sort of its own by vertex, and the segments are short (a marching-cubes vertex is named
// by 4 to 8 corners).  Corner numbers are distinct, so the sorted segment is one fixed sequence whatever the arrival order was, and the sum
// over it (k_vn_accumulate: one thread per vertex, one add per component and corner) has one value.  No floating-point atomic anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define VN_SHORT 32                 // segments up to this many corners are sorted by their vertex's own thread
#define VN_REG 8                    // ... and up to this many in its registers, by a fixed network
#define VN_LONG_BLOCKS 1024         // workgroups of k_vn_sort_long; each walks the queue of long segments with this stride

__device__ __forceinline__ bool vn_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // (a NaN fails)

// (A) the face normal of every triangle, NaN when an index is out of range; a triangle whose normal has a component that is not finite is
// left out: counted, and no vertex counts its corners
__global__ __launch_bounds__(256) void k_vn_face(int nv, int nt, const float* __restrict__ verts, const int* __restrict__ tris,
                                                 float* __restrict__ fn, unsigned* __restrict__ cnt, unsigned* __restrict__ left_out)
{
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    bool out = false;
    if (tl < nt) {
        const size_t t = (size_t)tl;
        const int ia = tris[3 * t], ib = tris[3 * t + 1], ic = tris[3 * t + 2];
        const float nan = __builtin_nanf("");
        float n[3] = {nan, nan, nan};
        if (ia >= 0 && ia < nv && ib >= 0 && ib < nv && ic >= 0 && ic < nv) {
            float a[3], b[3], c[3], e0[3], e1[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) { a[q] = verts[3 * (size_t)ia + q]; b[q] = verts[3 * (size_t)ib + q]; c[q] = verts[3 * (size_t)ic + q]; }
            surf_sub(b, a, e0); surf_sub(c, a, e1); surf_cross(e0, e1, n);
        }
        out = !(vn_finite(n[0]) && vn_finite(n[1]) && vn_finite(n[2]));
        fn[3 * t] = n[0]; fn[3 * t + 1] = n[1]; fn[3 * t + 2] = n[2];
        if (!out) { atomicAdd(cnt + ia, 1u); atomicAdd(cnt + ib, 1u); atomicAdd(cnt + ic, 1u); }
    }
    wave_count(out, left_out);
}

// (C) every corner of a participating triangle into its vertex's segment.  off[v] enters as the segment's first slot and leaves as the slot
// behind its last: afterwards vertex v owns [v ? off[v - 1] : 0, off[v])
__global__ __launch_bounds__(256) void k_vn_place(int nt, const int* __restrict__ tris, const float* __restrict__ fn, unsigned* __restrict__ off,
                                                  unsigned* __restrict__ list)
{
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tl >= nt) return;
    const size_t t = (size_t)tl;
    if (!(vn_finite(fn[3 * t]) && vn_finite(fn[3 * t + 1]) && vn_finite(fn[3 * t + 2]))) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) list[atomicAdd(off + tris[3 * t + k], 1u)] = (unsigned)(3 * t + k);
}

// (D) short segments sorted by their vertex's thread; the long ones queued (the queue's order does not matter: each is sorted on its own).
// counters[2] = the largest number of namings, [3] = the queue's length
__global__ __launch_bounds__(256) void k_vn_sort(int nv, const unsigned* __restrict__ off, unsigned* __restrict__ list, unsigned* __restrict__ longq,
                                                 unsigned* counters)
{
    const long long vl = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned k = 0;
    if (vl < nv) {
        const unsigned s = vl ? off[vl - 1] : 0u;
        k = off[vl] - s;
        if (k > VN_SHORT) longq[atomicAdd(counters + 3, 1u)] = (unsigned)vl;
        else if (k <= VN_REG) {
            // the common case (a marching-cubes vertex is named 4 to 8 times): all loads at once, Batcher's 19 comparators on registers,
            // all stores at once; the slots behind the segment's end hold the largest number and stay behind
            unsigned a[VN_REG];
#pragma unroll
            for (unsigned i = 0; i < VN_REG; ++i) a[i] = i < k ? list[s + i] : 0xffffffffu;
#define VN_CE(i, j) { const unsigned lo = min(a[i], a[j]), hi = max(a[i], a[j]); a[i] = lo; a[j] = hi; }
            VN_CE(0, 1) VN_CE(2, 3) VN_CE(4, 5) VN_CE(6, 7) VN_CE(0, 2) VN_CE(1, 3) VN_CE(4, 6) VN_CE(5, 7) VN_CE(1, 2) VN_CE(5, 6)
            VN_CE(0, 4) VN_CE(1, 5) VN_CE(2, 6) VN_CE(3, 7) VN_CE(2, 4) VN_CE(3, 5) VN_CE(1, 2) VN_CE(3, 4) VN_CE(5, 6)
#undef VN_CE
#pragma unroll
            for (unsigned i = 0; i < VN_REG; ++i) if (i < k) list[s + i] = a[i];
        } else
            for (unsigned i = 1; i < k; ++i) {
                const unsigned x = list[s + i];
                unsigned j = i;
                for (; j > 0; --j) {
                    const unsigned y = list[s + j - 1];
                    if (y < x) break;
                    list[s + j] = y;
                }
                list[s + j] = x;
            }
    }
    unsigned m = k;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    // (a plain load first: after the first few waves hardly any raises the maximum, and 160 000 atomics on one word cost more than the sort)
    if ((threadIdx.x & 63) == 0 && m > *(volatile unsigned*)(counters + 2)) atomicMax(counters + 2, m);
}

// (E) a long segment sorted by one workgroup: the bitonic network whose comparators all put the smaller value at the lower slot, over the
// next power of two; a comparator that reaches behind the segment's end would meet +inf there and is skipped.  k is the same for the whole
// workgroup, so every barrier is reached by all of it.
__device__ __forceinline__ void vn_compare(unsigned* seg, unsigned i, unsigned j, unsigned k)
{
    if (j >= k) return;
    const unsigned x = seg[i], y = seg[j];
    if (y < x) { seg[i] = y; seg[j] = x; }
}
__global__ __launch_bounds__(256) void k_vn_sort_long(const unsigned* __restrict__ off, unsigned* list, const unsigned* __restrict__ longq,
                                                      const unsigned* __restrict__ counters)
{
    const unsigned n_long = counters[3];
    for (unsigned q = blockIdx.x; q < n_long; q += gridDim.x) {
        const unsigned v = longq[q], s = v ? off[v - 1] : 0u, k = off[v] - s;
        unsigned* seg = list + s;
        unsigned P = 2;
        while (P < k) P <<= 1;                              // (k <= 2^30 corners)
        for (unsigned size = 2; size <= P; size <<= 1) {
            const unsigned half = size >> 1;
            for (unsigned p = threadIdx.x; p < (P >> 1); p += 256) {
                const unsigned base = (p / half) * size, w = p % half;
                vn_compare(seg, base + w, base + size - 1 - w, k);
            }
            __syncthreads();
            for (unsigned st = size >> 2; st > 0; st >>= 1) {
                for (unsigned p = threadIdx.x; p < (P >> 1); p += 256) {
                    const unsigned i = 2 * st * (p / st) + p % st;
                    vn_compare(seg, i, i + st, k);
                }
                __syncthreads();
            }
        }
    }
}

// (F) the sum over the sorted segment, then the normal
__global__ __launch_bounds__(256) void k_vn_accumulate(int nv, const unsigned* __restrict__ off, const unsigned* __restrict__ list,
                                                       const float* __restrict__ fn, float* __restrict__ normals, unsigned* __restrict__ n_zero)
{
    const long long vl = (long long)blockIdx.x * 256 + threadIdx.x;
    bool zero = false;
    if (vl < nv) {
        const unsigned s = vl ? off[vl - 1] : 0u, e = off[vl];
        float acc[3] = {0.f, 0.f, 0.f};
        for (unsigned p = s; p < e; ++p) {
            const size_t t = list[p] / 3u;
            acc[0] = add_rn(acc[0], fn[3 * t]); acc[1] = add_rn(acc[1], fn[3 * t + 1]); acc[2] = add_rn(acc[2], fn[3 * t + 2]);
        }
        const float nn = surf_dot(acc, acc);
        zero = !(vn_finite(nn) && nn > 0.f);
        const float L = cloud_sqrt_rn(nn);
#pragma unroll
        for (int q = 0; q < 3; ++q) normals[3 * (size_t)vl + q] = zero ? 0.f : div_rn(acc[q], L);
    }
    wave_count(zero, n_zero);
}

// ---- rays along the normals --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_normal_rays(int n, const float* __restrict__ verts, const float* __restrict__ normals, float length,
                                                     float* __restrict__ ro, float* __restrict__ rd, float* __restrict__ gd, uint8_t* __restrict__ has)
{
    const long long il = (long long)blockIdx.x * 256 + threadIdx.x;
    if (il >= n) return;
    const size_t i = (size_t)il;
    float v[3], m[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { v[q] = verts[3 * i + q]; m[q] = normals[3 * i + q]; }
    const bool ok = vn_finite(v[0]) && vn_finite(v[1]) && vn_finite(v[2]) && vn_finite(m[0]) && vn_finite(m[1]) && vn_finite(m[2]) &&
                    (m[0] != 0.f || m[1] != 0.f || m[2] != 0.f);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        ro[3 * i + q] = ok ? add_rn(v[q], mul_rn(length, m[q])) : v[q];
        rd[3 * i + q] = ok ? -m[q] : (q == 2 ? -1.f : 0.f);
    }
    gd[i] = length;
    if (has) has[i] = ok ? 1 : 0;
}

// ---- the merge of the two colour queries ---------------------------------------------------------------------------------------------------
// has NULL: every vertex takes the point query.  raw: [n][4] of nsk_eval_points
__global__ __launch_bounds__(256) void k_vc_select(int n, const uint8_t* __restrict__ has, const float* __restrict__ raw, float* __restrict__ rgb,
                                                   unsigned long long* __restrict__ n_fallback)
{
    const long long il = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool fb = il < n && (!has || has[il] == 0);
    if (fb) {
        const size_t i = (size_t)il;
        rgb[3 * i] = raw[4 * i]; rgb[3 * i + 1] = raw[4 * i + 1]; rgb[3 * i + 2] = raw[4 * i + 2];
    }
    if (n_fallback) wave_count(fb, n_fallback);
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
#define VN_MAX_CORNERS (1LL << 30)

extern "C" int nsk_mesh_vertex_normals(nsk_ctx* c, const float* verts, int nv, const int32_t* tris, int nt, float* normals, int h_info[4])
{
    if (!c) return fail("nsk_mesh_vertex_normals: null ctx");
    if (nv < 0 || nt < 0) return fail("nsk_mesh_vertex_normals: negative count");
    if (3LL * nt > VN_MAX_CORNERS) return fail("nsk_mesh_vertex_normals: %d triangles, at most 2^30 corners", nt);
    if (nv > 0x7fffffff / 3) return fail("nsk_mesh_vertex_normals: %d vertices, at most %d", nv, 0x7fffffff / 3);
    if (nv > 0 && (!verts || !normals)) return fail("nsk_mesh_vertex_normals: d_vertices / d_normals is NULL");
    if (nt > 0 && !tris) return fail("nsk_mesh_vertex_normals: d_triangles is NULL");
    if (c->capturing) return fail("nsk_mesh_vertex_normals: not while a graph is being captured");
    if (h_info) { h_info[0] = h_info[1] = h_info[2] = h_info[3] = 0; }
    if (nv == 0) { if (h_info) h_info[0] = nt; return 0; }              // (every index is out of range)
    HIPCHK(hipSetDevice(c->device));
    if (nt == 0) {                                                      // no triangle: every normal is zero
        HIPCHK(hipMemsetAsync(normals, 0, (size_t)nv * 3 * sizeof(float), c->stream));
        if (h_info) { h_info[1] = nv; HIPCHK(hipStreamSynchronize(c->stream)); }
        return 0;
    }
    nsk_ctx::Normals& N = c->normals;
    const size_t words = mc_scan_words((size_t)nv + 1);
    CHK(grow(c, N.fn, (size_t)nt * 3, "the face normals", GROW_NO_CAPTURE));
    CHK(grow(c, N.list, (size_t)nt * 3, "the vertices' corner lists", GROW_NO_CAPTURE));
    CHK(grow(c, N.off, words, "the corner lists' offsets", GROW_NO_CAPTURE));
    CHK(grow(c, N.longq, (size_t)nt * 3 / (VN_SHORT + 1) + 1, "the queue of long corner lists", GROW_NO_CAPTURE));
    CHK(grow(c, N.counters, 4, "the normals' counters", GROW_NO_CAPTURE));
    const unsigned nbt = (unsigned)(((long long)nt + 255) / 256), nbv = (unsigned)(((long long)nv + 255) / 256);
    HIPCHK(hipMemsetAsync(N.off, 0, words * 4, c->stream));             // (the slot behind the last count turns into the total)
    HIPCHK(hipMemsetAsync(N.counters, 0, 16, c->stream));
    { ProfScope ps(c, "vn_face"); k_vn_face<<<nbt, 256, 0, c->stream>>>(nv, nt, verts, tris, N.fn, N.off, N.counters); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "vn_scan"); CHK(mc_scan(c, N.off, nv + 1)); }
    { ProfScope ps(c, "vn_place"); k_vn_place<<<nbt, 256, 0, c->stream>>>(nt, tris, N.fn, N.off, N.list); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "vn_sort");
      k_vn_sort<<<nbv, 256, 0, c->stream>>>(nv, N.off, N.list, N.longq, N.counters);
      k_vn_sort_long<<<VN_LONG_BLOCKS, 256, 0, c->stream>>>(N.off, N.list, N.longq, N.counters); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "vn_accumulate"); k_vn_accumulate<<<nbv, 256, 0, c->stream>>>(nv, N.off, N.list, N.fn, normals, N.counters + 1); }
    HIPCHK(hipGetLastError());
    if (h_info) {
        unsigned h[3] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(h, N.counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        h_info[0] = (int)h[0]; h_info[1] = (int)h[1]; h_info[2] = (int)h[2]; h_info[3] = 0;
    }
    return 0;
}

static int normal_rays_checks(const char* fn, nsk_ctx* c, int n, const float* verts, float length)
{
    if (!c) return fail("%s: null ctx", fn);
    if (n < 0) return fail("%s: negative count", fn);
    if (n > 0x7fffffff / 3) return fail("%s: %d vertices, at most %d", fn, n, 0x7fffffff / 3);
    if (!(length > 0.f) || !std::isfinite(length)) return fail("%s: length = %g, must be positive and finite", fn, (double)length);
    if (n > 0 && !verts) return fail("%s: d_vertices is NULL", fn);
    return 0;
}

extern "C" int nsk_normal_rays(nsk_ctx* c, int n, const float* verts, const float* normals, float length, float* ro, float* rd, float* gd,
                               uint8_t* has)
{
    CHK(normal_rays_checks("nsk_normal_rays", c, n, verts, length));
    if (n > 0 && (!normals || !ro || !rd || !gd)) return fail("nsk_normal_rays: d_normals / d_rays_o / d_rays_d / d_gt_depth is NULL");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    { ProfScope ps(c, "normal_rays"); k_normal_rays<<<(unsigned)(((long long)n + 255) / 256), 256, 0, c->stream>>>(n, verts, normals, length, ro, rd, gd, has); }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_mesh_vertex_colors(nsk_ctx* c, const float* verts, int nv, const float* normals, float length, int chunk_rays, float* rgb,
                                      int* h_fallback)
{
    CHK(normal_rays_checks("nsk_mesh_vertex_colors", c, nv, verts, length));
    if (nv > 0 && !rgb) return fail("nsk_mesh_vertex_colors: d_rgb is NULL");
    CHK(check_stage(c, NSK_COLOR));
    const int S = c->R.n_samples + c->R.n_surface + c->n_importance;      // (every ray carries its depth)
    const int chunk_max = (int)(((1LL << 26) - 1) / S);
    if (chunk_rays == 0) chunk_rays = 25600;                // nsk_render_image's default
    if (chunk_rays < 1 || chunk_rays > chunk_max)
        return fail("nsk_mesh_vertex_colors: chunk_rays = %d, must be 0 (default) or 1..%d (%d samples per ray, fewer than 2^26 samples per chunk)", chunk_rays, chunk_max, S);
    if (c->capturing) return fail("nsk_mesh_vertex_colors: not while a graph is being captured");
    if (h_fallback) *h_fallback = 0;
    if (nv == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    // a chunk of rays and a chunk of points hold the same number of samples, so one workspace serves both queries
    const int chunk = normals ? std::min(chunk_rays, nv) : (int)std::min<long long>((long long)chunk_rays * S, nv);
    CHK(ensure_ws(c, normals ? chunk : 1, normals ? chunk * S : chunk));
    nsk_ctx::Normals& N = c->normals;
    nsk_ctx::Image& I = c->img;
    CHK(grow(c, N.raw, (size_t)chunk * 4, "the chunk's point colours", GROW_NO_CAPTURE));
    if (normals) {
        CHK(grow(c, N.has, (size_t)chunk, "the chunk's ray flags", GROW_NO_CAPTURE));
        if ((size_t)chunk > I.gd.cap()) {
            CHK(grow_begin(c, GROW_NO_CAPTURE));
            const int r = [&]() -> int {
                CHK(dev_alloc(I.ro, (size_t)chunk * 3, "the chunk's ray origins")); CHK(dev_alloc(I.rd, (size_t)chunk * 3, "the chunk's ray directions"));
                CHK(dev_alloc(I.gd, (size_t)chunk, "the chunk's depths"));
                return 0;
            }();
            if (r != 0) { reset_all(I.ro, I.rd, I.gd); return r; }
        }
    }
    long long cnt = 0;
    long long* const pcnt = h_fallback ? &cnt : nullptr;
    CHK(count_begin(c, pcnt, "the fallback count"));
    const nsk_ctx::DMax own;                                // the maximum depth is `length`, given explicitly: an installed depth-max batch describes another batch
    for (long long first = 0; first < nv; first += chunk) {
        const int n = (int)std::min<long long>(chunk, nv - first);
        const unsigned nb = (unsigned)((n + 255) / 256);
        const float* v = verts + 3 * (size_t)first;
        float* out = rgb + 3 * (size_t)first;
        if (normals) {
            { ProfScope ps(c, "normal_rays"); k_normal_rays<<<nb, 256, 0, c->stream>>>(n, v, normals + 3 * (size_t)first, length, I.ro, I.rd, I.gd, N.has); }
            HIPCHK(hipGetLastError());
            CHK(forward_core(c, NSK_COLOR, n, S, I.ro, I.rd, I.gd, length, false, false, &own));
            CompArgs A;
            comp_args(c, A, NSK_COLOR, n, S, I.ro, I.rd);
            A.keep = nullptr;                               // (mode 0 does not read it: a render shows every ray)
            A.rgb = out; A.depth = nullptr; A.var = nullptr; A.weights = nullptr; A.mode = 0;
            { ProfScope ps(c, "composite"); k_composite<<<(n + 3) / 4, 256, 0, c->stream>>>(A); }
            HIPCHK(hipGetLastError());
        }
        CHK(nsk_eval_points(c, NSK_COLOR, n, v, N.raw));
        { ProfScope ps(c, "vc_select"); k_vc_select<<<nb, 256, 0, c->stream>>>(n, normals ? N.has.get() : nullptr, N.raw, out, h_fallback ? c->count.get() : nullptr); }
        HIPCHK(hipGetLastError());
    }
    CHK(count_end(c, pcnt));
    if (h_fallback) *h_fallback = (int)cnt;
    return 0;
}

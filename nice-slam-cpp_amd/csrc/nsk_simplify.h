// nsk_simplify.h -- a triangle mesh simplified by uniform vertex clustering (Rossignac-Borrel): nsk_mesh_simplify.  include/nsk.h states the
// rule operation by operation; tests/simplify_checks.py restates it in numpy and tests/test_gpu_simplify.py holds the device to that bytes
// for bytes.  This file is included by nsk.hip behind the context, the buffer helpers, the multi-launch scan (mc_scan) and nsk_hull.h, whose
// bounds pass (k_hull_bounds: the finite points' box and their count) is the first pass here as it stands.
//
// The passes, none of which depends on the order its threads or atomics run in:
//   bounds      k_hull_bounds -> the host combines the partial boxes and plans the grid (nsk_simplify_plan.h)            [synchronises]
//   cells       per vertex: its cell (or none), occupancy flag of the cell = 1 (every writer stores the same 1)
//   scan        mc_scan over the flags: occupied cells ranked in ascending cell index; the host reads their number       [synchronises]
//   accumulate  per vertex: (1, q_x, q_y, q_z) for its cell's count and sums, by rank; a run of equal ranks inside a wave is summed by
//               shuffles and adds once per word with integer atomics (the form that stayed)
//   triangles   per triangle: corner ranks, invalid ones counted, survivors counted under their smallest corner
//   lists       mc_scan over those counts, then every survivor placed into its smallest corner's list through an integer cursor
//   duplicates  per list: a triangle is a duplicate iff the list holds an equal rotated triple with a lower input index -- a property of
//               the list as a set, so the cursor's order does not matter.  One thread per list of up to SIMP_LIST_SHORT triangles
//               (k_simp_dups), a workgroup per longer one (k_simp_dups_long); both compare every pair, k^2 key loads for a list of k
//   compact     referenced flags of the occupied cells, mc_scan over the kept flags and over the referenced flags
//   out         representatives of the referenced cells, re-indexed triangles, the vertex map; the host reads five counts  [synchronises]
// Three synchronisations: the bounds size the flags, the occupied count sizes the sums, the last one fetches the counts.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "nsk_simplify_plan.h"

#define SIMP_NONE 0xffffffffu               // a vertex without a cell; tkey[3 t] of a triangle that is not a survivor
#define SIMP_LONG_BLOCKS 1024               // workgroups of k_simp_dups_long; each walks the queue of long lists with this stride

struct SimpGrid { double lo[3]; double cell; int n[3]; };

__device__ __forceinline__ double simp_mul(double a, double b) { double r = a * b; asm("" : "+v"(r)); return r; }      // (never fused)
// g = (double(p) - lo) / cell -> c = floor(g), q = rint((g - c) 2^20): the subtraction and the product by a power of two are exact
__device__ __forceinline__ void simp_coord(float p, double lo, double cell, long long& c, long long& q)
{
    const double g = __ddiv_rn(__dsub_rn((double)p, lo), cell), f = floor(g);
    c = (long long)f;
    q = (long long)rint((g - f) * (double)(1 << SIMP_FRAC_BITS));
}

// cells: vcell[i] = the cell index of vertex i, SIMP_NONE with a non-finite coordinate.  (A finite vertex lies in the box the grid was
// planned for, so 0 <= c_a < n_a; the comparison only guards the stores against a buffer that changed between the passes.)
__global__ __launch_bounds__(256) void k_simp_cells(int nv, const float* __restrict__ verts, SimpGrid G, unsigned* __restrict__ vcell,
                                                    unsigned* __restrict__ occ)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const float p[3] = {verts[3 * (size_t)i], verts[3 * (size_t)i + 1], verts[3 * (size_t)i + 2]};
    unsigned cell = SIMP_NONE;
    if (hull_finite(p[0]) && hull_finite(p[1]) && hull_finite(p[2])) {
        long long c[3], q;
        bool in = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) { simp_coord(p[a], G.lo[a], G.cell, c[a], q); in = in && c[a] >= 0 && c[a] < G.n[a]; }
        if (in) cell = (unsigned)((c[2] * G.n[1] + c[1]) * G.n[0] + c[0]);
    }
    vcell[i] = cell;
    if (cell != SIMP_NONE) occ[cell] = 1u;
}

// accumulate: rank[] is the scanned occupancy.  cnt [occupied], sums [occupied][3], cellof [occupied] (every member stores the same cell).
// Marching-cubes vertices arrive x-fastest, so neighbouring lanes often share a cell: a run of equal ranks inside a wave is summed by
// shuffles first (a run of at most 64 members: count and sums of q <= 2^20 fit 32 bits) and its first lane adds once per word.  Integer
// sums: how the members are grouped changes no bit.
__global__ __launch_bounds__(256) void k_simp_accumulate(int nv, const float* __restrict__ verts, SimpGrid G, const unsigned* __restrict__ vcell,
                                                         const unsigned* __restrict__ rank, unsigned* __restrict__ cnt,
                                                         unsigned long long* __restrict__ sums, unsigned* __restrict__ cellof)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned cell = SIMP_NONE, r = SIMP_NONE, v[4] = {0u, 0u, 0u, 0u};
    if (i < nv) cell = vcell[i];
    if (cell != SIMP_NONE) {
        r = rank[cell];
        v[0] = 1u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            long long c, q;
            simp_coord(verts[3 * (size_t)i + a], G.lo[a], G.cell, c, q);
            v[1 + a] = (unsigned)q;
        }
    }
    // the first lane of this lane's run of equal ranks (a lane without a cell is a run of its own kind: nothing is added for it)
    const unsigned before = (unsigned)__shfl_up((int)r, 1, 64);
    int start = (lane == 0 || before != r) ? lane : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(start, d, 64); if (lane >= d) start = max(start, t); }
    // suffix sums inside the run: afterwards its first lane holds the run's totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int os = __shfl_down(start, d, 64);
        const bool same = lane + d < 64 && os == start;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const unsigned t = (unsigned)__shfl_down((int)v[k], d, 64); if (same) v[k] += t; }
    }
    if (r == SIMP_NONE || start != lane) return;
    atomicAdd(cnt + r, v[0]);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(sums + 3 * (size_t)r + a, (unsigned long long)v[1 + a]);
    cellof[r] = cell;
}

// the position of the smallest of three distinct ranks
__device__ __forceinline__ int simp_min3(unsigned a, unsigned b, unsigned c) { return a < b ? (a < c ? 0 : 2) : (b < c ? 1 : 2); }

// triangles: tkey[3 t + k] = the rank of corner k's cell (a survivor), or tkey[3 t] = SIMP_NONE; tflag[t] = 1 for a survivor; with lists,
// lcnt[smallest rank] counts it.  counters[0] invalid
__global__ __launch_bounds__(256) void k_simp_tris(int nv, int nt, const int* __restrict__ tris, const unsigned* __restrict__ vcell,
                                                   const unsigned* __restrict__ rank, int lists, unsigned* __restrict__ tkey,
                                                   unsigned* __restrict__ tflag, unsigned* __restrict__ lcnt, unsigned* __restrict__ counters)
{
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    bool invalid = false;
    if (tl < nt) {
        const size_t t = (size_t)tl;
        const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
        unsigned ca = 0, cb = 0, cc = 0;
        invalid = a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv;
        if (!invalid) {
            ca = vcell[a]; cb = vcell[b]; cc = vcell[c];
            invalid = ca == SIMP_NONE || cb == SIMP_NONE || cc == SIMP_NONE;
        }
        const bool collapsed = !invalid && (ca == cb || cb == cc || ca == cc);
        if (!invalid && !collapsed) {
            const unsigned r[3] = {rank[ca], rank[cb], rank[cc]};
            tkey[3 * t] = r[0]; tkey[3 * t + 1] = r[1]; tkey[3 * t + 2] = r[2];
            tflag[t] = 1u;
            if (lists) atomicAdd(lcnt + r[simp_min3(r[0], r[1], r[2])], 1u);
        } else {
            tkey[3 * t] = SIMP_NONE; tkey[3 * t + 1] = 0u; tkey[3 * t + 2] = 0u;
            tflag[t] = 0u;
        }
    }
    // (collapsed triangles are not counted here: nearly every wave of a marching-cubes mesh holds some, and one add per wave on one word
    // made this pass 3.72 ms instead of 0.16 at 20.9 M triangles; the host has them as n_triangles - invalid - duplicates - kept)
    wave_count(invalid, counters);
}

// lists: off[r] enters as list r's first slot and leaves as the slot behind its last: afterwards list r owns [r ? off[r - 1] : 0, off[r])
__global__ __launch_bounds__(256) void k_simp_place(int nt, const unsigned* __restrict__ tkey, unsigned* __restrict__ off, unsigned* __restrict__ list)
{
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tl >= nt) return;
    const size_t t = (size_t)tl;
    const unsigned r[3] = {tkey[3 * t], tkey[3 * t + 1], tkey[3 * t + 2]};
    if (r[0] == SIMP_NONE) return;
    list[atomicAdd(off + r[simp_min3(r[0], r[1], r[2])], 1u)] = (unsigned)t;
}

// the two corners behind the smallest one, in the triangle's cyclic order (the smallest is the list's own rank)
__device__ __forceinline__ void simp_rest(const unsigned* __restrict__ tkey, unsigned t, unsigned& x, unsigned& y)
{
    const unsigned r[3] = {tkey[3 * (size_t)t], tkey[3 * (size_t)t + 1], tkey[3 * (size_t)t + 2]};
    const int m = simp_min3(r[0], r[1], r[2]);
    x = r[(m + 1) % 3]; y = r[(m + 2) % 3];
}
// is list[i] a duplicate: does list [s, e) hold a triangle with a lower index and the same rotated triple
__device__ __forceinline__ bool simp_is_dup(const unsigned* __restrict__ tkey, const unsigned* __restrict__ list, unsigned s, unsigned e, unsigned i)
{
    const unsigned t = list[i];
    unsigned x, y;
    simp_rest(tkey, t, x, y);
    for (unsigned j = s; j < e; ++j) {
        const unsigned u = list[j];
        if (u >= t) continue;
        unsigned ux, uy;
        simp_rest(tkey, u, ux, uy);
        if (ux == x && uy == y) return true;
    }
    return false;
}
__device__ __forceinline__ void simp_add_wave(unsigned n, unsigned* __restrict__ counter)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (unsigned)__shfl_xor((int)n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, n);
}

// duplicates: one thread per occupied cell's list; longer lists queued (the queue's order does not matter: each is searched on its own).
// counters[2] duplicates, [3] the queue's length
__global__ __launch_bounds__(256) void k_simp_dups(int n_lists, const unsigned* __restrict__ off, const unsigned* __restrict__ list,
                                                   const unsigned* __restrict__ tkey, unsigned* __restrict__ tflag, unsigned* __restrict__ longq,
                                                   unsigned long_cap, unsigned* __restrict__ counters)
{
    const long long rl = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned ndup = 0;
    if (rl < n_lists) {
        const unsigned s = rl ? off[rl - 1] : 0u, e = off[rl];
        if (e - s > SIMP_LIST_SHORT) {
            const unsigned slot = atomicAdd(counters + 3, 1u);
            if (slot < long_cap) longq[slot] = (unsigned)rl;       // (always: a long list holds more than SIMP_LIST_SHORT triangles)
        } else
            for (unsigned i = s; i < e; ++i)
                if (simp_is_dup(tkey, list, s, e, i)) { tflag[list[i]] = 0u; ++ndup; }
    }
    simp_add_wave(ndup, counters + 2);
}
// a long list searched by one workgroup, a triangle per thread and round
__global__ __launch_bounds__(256) void k_simp_dups_long(const unsigned* __restrict__ off, const unsigned* __restrict__ list,
                                                        const unsigned* __restrict__ tkey, unsigned* __restrict__ tflag,
                                                        const unsigned* __restrict__ longq, unsigned long_cap, unsigned* __restrict__ counters)
{
    const unsigned n_long = min(counters[3], long_cap);
    unsigned ndup = 0;
    for (unsigned q = blockIdx.x; q < n_long; q += gridDim.x) {
        const unsigned r = longq[q], s = r ? off[r - 1] : 0u, e = off[r];
        for (unsigned i = s + threadIdx.x; i < e; i += 256)
            if (simp_is_dup(tkey, list, s, e, i)) { tflag[list[i]] = 0u; ++ndup; }
    }
    simp_add_wave(ndup, counters + 2);
}

// compact: the cells a kept triangle names (every writer stores the same 1)
__global__ __launch_bounds__(256) void k_simp_refs(int nt, const unsigned* __restrict__ tkey, const unsigned* __restrict__ tflag, unsigned* __restrict__ vflag)
{
    const long long tl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tl >= nt || !tflag[tl]) return;
    const size_t t = (size_t)tl;
    vflag[tkey[3 * t]] = 1u; vflag[tkey[3 * t + 1]] = 1u; vflag[tkey[3 * t + 2]] = 1u;
}

// out: voff [occupied + 1], toff [nt + 1]: the exclusive scans of the flags (the last slot is the total).  Thread q writes the
// representative of occupied cell q, triangle q and the map entry of input vertex q
__global__ __launch_bounds__(256) void k_simp_out(int nv, int nt, int occupied, SimpGrid G, const unsigned* __restrict__ vcell,
                                                  const unsigned* __restrict__ rank, const unsigned* __restrict__ cnt,
                                                  const unsigned long long* __restrict__ sums, const unsigned* __restrict__ cellof,
                                                  const unsigned* __restrict__ tkey, const unsigned* __restrict__ voff,
                                                  const unsigned* __restrict__ toff, float* __restrict__ out_v, int* __restrict__ out_t,
                                                  int* __restrict__ vmap)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q < occupied) {
        const unsigned d = voff[q];
        if (voff[q + 1] != d) {
            const unsigned cell = cellof[q], nxy = (unsigned)G.n[0] * (unsigned)G.n[1];
            const unsigned c[3] = {cell % (unsigned)G.n[0], (cell / (unsigned)G.n[0]) % (unsigned)G.n[1], cell / nxy};
            const double n = (double)cnt[q];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double m = __ddiv_rn((double)sums[3 * (size_t)q + a], n);
                const double g = __dadd_rn((double)c[a], m * (1.0 / (double)(1 << SIMP_FRAC_BITS)));      // (the product by 2^-20 is exact)
                out_v[3 * (size_t)d + a] = (float)__dadd_rn(G.lo[a], simp_mul(g, G.cell));
            }
        }
    }
    if (q < nt) {
        const unsigned d = toff[q];
        if (toff[q + 1] != d)
            for (int a = 0; a < 3; ++a) out_t[3 * (size_t)d + a] = (int)voff[tkey[3 * (size_t)q + a]];
    }
    if (vmap && q < nv) {
        const unsigned cell = vcell[q];
        int m = -1;
        if (cell != SIMP_NONE) {
            const unsigned r = rank[cell];
            if (voff[r + 1] != voff[r]) m = (int)voff[r];
        }
        vmap[q] = m;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int nsk_mesh_simplify_list_threshold(void) { return SIMP_LIST_SHORT; }

extern "C" int nsk_mesh_simplify(nsk_ctx* c, const float* verts, int nv, const int32_t* tris, int nt, float cell, int flags, float* out_v,
                                 int32_t* out_t, int32_t* vmap, int* out_vertices, int* out_triangles, long long* info)
{
    if (!c) return fail("nsk_mesh_simplify: null ctx");
    if (!out_vertices || !out_triangles || !info) return fail("nsk_mesh_simplify: out_vertices / out_triangles / h_info is NULL");
    if (nv < 0 || nt < 0) return fail("nsk_mesh_simplify: negative count");
    if (nv > SIMP_MAX_COUNT || nt > SIMP_MAX_COUNT)
        return fail("nsk_mesh_simplify: %d vertices, %d triangles, at most %d of each", nv, nt, SIMP_MAX_COUNT);
    if (flags & ~1) return fail("nsk_mesh_simplify: flags = %d, only bit 0 (keep duplicates) is known", flags);
    if (!(std::isfinite(cell) && cell > 0.f)) return fail("nsk_mesh_simplify: cell = %g, must be positive and finite", (double)cell);
    if (nv > 0 && (!verts || !out_v)) return fail("nsk_mesh_simplify: d_vertices / d_out_vertices is NULL with %d vertices", nv);
    if (nt > 0 && (!tris || !out_t)) return fail("nsk_mesh_simplify: d_triangles / d_out_triangles is NULL with %d triangles", nt);
    if ((out_v && out_v == verts) || (out_t && out_t == tris)) return fail("nsk_mesh_simplify: the output buffers must not alias the input");
    if (c->capturing) return fail("nsk_mesh_simplify: not while a graph is being captured");
    *out_vertices = *out_triangles = 0;
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[1] = nv; info[2] = nt;                             // (what holds when no vertex is finite)
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Simplify& U = c->simplify;
    // bounds
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    long long finite = 0;
    if (nv > 0) {
        const int nb = (int)std::min<long long>(((long long)nv + 255) / 256, HULL_PARTS);
        CHK(grow(c, U.part, 8 * HULL_PARTS, "the bounds' partial boxes", GROW_NO_CAPTURE));
        std::vector<float> h((size_t)nb * 8);
        { ProfScope ps(c, "simp_bounds"); k_hull_bounds<<<nb, 256, 0, c->stream>>>(nv, verts, U.part); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h.data(), U.part, h.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int b = 0; b < nb; ++b) {
            unsigned cnt;
            memcpy(&cnt, &h[8 * (size_t)b + 6], 4);
            finite += cnt;
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)h[8 * (size_t)b + a]); hi[a] = std::max(hi[a], (double)h[8 * (size_t)b + 3 + a]); }
        }
    }
    if (finite == 0) {
        if (vmap && nv > 0) HIPCHK(hipMemsetAsync(vmap, 0xff, (size_t)nv * 4, c->stream));
        return 0;
    }
    SimplifyPlan P;
    const int pr = simplify_plan(lo, hi, cell, finite, P);
    if (pr == SIMP_TOO_MANY_CELLS) {
        if (P.cells > 0) return fail("nsk_mesh_simplify: cell = %g asks for %lld x %lld x %lld = %lld cells, at most 2^28", (double)cell, P.n[0], P.n[1], P.n[2], P.cells);
        return fail("nsk_mesh_simplify: cell = %g asks for about %.6g cells, at most 2^28", (double)cell, P.cells_approx);
    }
    if (pr == SIMP_AXIS_TOO_LONG)
        return fail("nsk_mesh_simplify: cell = %g asks for %lld x %lld x %lld cells, at most 2^21 - 1 along an axis", (double)cell, P.n[0], P.n[1], P.n[2]);
    if (pr != SIMP_OK) return fail("nsk_mesh_simplify: cell = %g, must be positive and finite", (double)cell);
    const size_t cells = (size_t)P.cells;
    if (simplify_scan_words(cells + 1) != mc_scan_words(cells + 1)) return fail("nsk_mesh_simplify: the plan's scan levels are not mc_scan's");
    SimpGrid G;
    for (int a = 0; a < 3; ++a) { G.lo[a] = P.lo[a]; G.n[a] = (int)P.n[a]; }
    G.cell = P.cell;
    const int lists = (flags & 1) ? 0 : 1;
    const unsigned nbv = (unsigned)(((long long)nv + 255) / 256), nbt = (unsigned)(((long long)nt + 255) / 256);
    // cells and their ranks
    const size_t w_occ = mc_scan_words(cells + 1);
    CHK(grow(c, U.vcell, (size_t)nv, "the vertices' cells", GROW_NO_CAPTURE));
    CHK(grow(c, U.occ, w_occ, "the cells' occupancy flags", GROW_NO_CAPTURE));
    CHK(grow(c, U.counters, 8, "the simplification's counters", GROW_NO_CAPTURE));
    HIPCHK(hipMemsetAsync(U.occ, 0, w_occ * 4, c->stream));
    HIPCHK(hipMemsetAsync(U.counters, 0, 8 * 4, c->stream));
    { ProfScope ps(c, "simp_cells"); k_simp_cells<<<nbv, 256, 0, c->stream>>>(nv, verts, G, U.vcell, U.occ); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "simp_scan"); CHK(mc_scan(c, U.occ, (int)cells + 1)); }
    unsigned occupied_u = 0;
    HIPCHK(hipMemcpyAsync(&occupied_u, U.occ.get() + cells, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t occupied = occupied_u;
    if (occupied == 0 || occupied > cells || occupied > (size_t)nv) return fail("nsk_mesh_simplify: %zu occupied cells of %zu for %d vertices", occupied, cells, nv);
    // representatives' sums
    const size_t w_list = mc_scan_words(occupied + 1), w_tri = mc_scan_words((size_t)nt + 1);
    CHK(grow(c, U.cnt, occupied, "the cells' member counts", GROW_NO_CAPTURE));
    CHK(grow(c, U.sums, occupied * 3, "the cells' coordinate sums", GROW_NO_CAPTURE));
    CHK(grow(c, U.cellof, occupied, "the occupied cells' indices", GROW_NO_CAPTURE));
    CHK(grow(c, U.loff, w_list, "the smallest-corner lists' ends", GROW_NO_CAPTURE));
    CHK(grow(c, U.vflag, w_list, "the referenced cells' flags", GROW_NO_CAPTURE));
    CHK(grow(c, U.tkey, (size_t)std::max(nt, 1) * 3, "the triangles' corner cells", GROW_NO_CAPTURE));
    CHK(grow(c, U.tflag, w_tri, "the kept triangles' flags", GROW_NO_CAPTURE));
    CHK(grow(c, U.list, (size_t)std::max(nt, 1), "the smallest-corner lists", GROW_NO_CAPTURE));
    const size_t long_cap = simplify_long_cap((size_t)nt);
    CHK(grow(c, U.longq, long_cap, "the queue of long lists", GROW_NO_CAPTURE));
    HIPCHK(hipMemsetAsync(U.cnt, 0, occupied * 4, c->stream));
    HIPCHK(hipMemsetAsync(U.sums, 0, occupied * 24, c->stream));
    HIPCHK(hipMemsetAsync(U.loff, 0, w_list * 4, c->stream));
    HIPCHK(hipMemsetAsync(U.vflag, 0, w_list * 4, c->stream));
    HIPCHK(hipMemsetAsync(U.tflag, 0, w_tri * 4, c->stream));
    { ProfScope ps(c, "simp_accumulate"); k_simp_accumulate<<<nbv, 256, 0, c->stream>>>(nv, verts, G, U.vcell, U.occ, U.cnt, U.sums, U.cellof); }
    HIPCHK(hipGetLastError());
    if (nt > 0) {
        { ProfScope ps(c, "simp_tris"); k_simp_tris<<<nbt, 256, 0, c->stream>>>(nv, nt, tris, U.vcell, U.occ, lists, U.tkey, U.tflag, U.loff, U.counters); }
        HIPCHK(hipGetLastError());
        if (lists) {
            { ProfScope ps(c, "simp_lists");
              CHK(mc_scan(c, U.loff, (int)occupied + 1));
              k_simp_place<<<nbt, 256, 0, c->stream>>>(nt, U.tkey, U.loff, U.list); }
            HIPCHK(hipGetLastError());
            { ProfScope ps(c, "simp_dups");
              k_simp_dups<<<(unsigned)((occupied + 255) / 256), 256, 0, c->stream>>>((int)occupied, U.loff, U.list, U.tkey, U.tflag, U.longq, (unsigned)long_cap, U.counters);
              k_simp_dups_long<<<SIMP_LONG_BLOCKS, 256, 0, c->stream>>>(U.loff, U.list, U.tkey, U.tflag, U.longq, (unsigned)long_cap, U.counters); }
            HIPCHK(hipGetLastError());
        }
        { ProfScope ps(c, "simp_compact");
          k_simp_refs<<<nbt, 256, 0, c->stream>>>(nt, U.tkey, U.tflag, U.vflag);
          CHK(mc_scan(c, U.tflag, nt + 1));
          CHK(mc_scan(c, U.vflag, (int)occupied + 1)); }
        HIPCHK(hipGetLastError());
    }
    // (without a triangle the flags are all 0 and their scans too: nothing is referenced, every map entry is -1)
    const long long most = std::max<long long>(std::max<long long>(nv, nt), (long long)occupied);
    { ProfScope ps(c, "simp_out");
      k_simp_out<<<(unsigned)((most + 255) / 256), 256, 0, c->stream>>>(nv, nt, (int)occupied, G, U.vcell, U.occ, U.cnt, U.sums, U.cellof, U.tkey, U.vflag,
                                                                        U.tflag, out_v, out_t, vmap); }
    HIPCHK(hipGetLastError());
    unsigned tot[2] = {0, 0}, cnt[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(&tot[0], U.vflag.get() + occupied, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tot[1], U.tflag.get() + nt, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cnt, U.counters, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out_vertices = (int)tot[0]; *out_triangles = (int)tot[1];
    info[0] = finite; info[1] = (long long)nv - finite; info[2] = cnt[0]; info[4] = cnt[2];
    info[3] = (long long)nt - info[2] - info[4] - (long long)tot[1];
    info[5] = (long long)occupied; info[6] = P.cells; info[7] = P.packed();
    return 0;
}

// nsk_hull.h -- the convex hull of a point cloud on the device, and the lattice nodes inside the scaled hull (upstream's
// get_bound_from_frames takes the hull of a TSDF fusion's vertices and the camera centres with a CPU library; Mesher.get_mesh then evaluates
// the map only inside it).  include/nsk.h states the rule; this file is included by nsk.hip behind the context, the buffer helpers and
// the multi-launch scan (mc_scan).  tests/hull_checks.py restates the rule one numpy / Python integer operation per operation here.
//
// What grows with the number of points runs here: the bounds, the quantisation to int32 triples, the four selection passes of the first
// simplex, and per insertion one pass over the list of the points that are still outside (k_hull_rehome), which re-homes the points whose
// face died and finds every new face's count and largest det; k_hull_argmin then takes the smallest index among the points that reach it,
// k_hull_report writes the answers for the host.  The face table lives on the host (nsk_hull_plan.h): each insertion uploads the new
// faces' planes and downloads their reports -- one synchronisation per hull vertex.
//
// Nothing here depends on the order atomics run in: they are integer maxima, minima and counts.  A workgroup combines its points in LDS
// first (one slot per new face), so a face receives at most one global update per workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>
#include <cstring>
#include "nsk_hull_plan.h"
#include "nsk_mesh.h"

#define HULL_INVALID INT_MIN        // q_x of a point with a non-finite coordinate
#define HULL_SLOTS 256              // new faces a workgroup combines in LDS; faces beyond them go to the global words directly
#define HULL_PARTS 1024             // workgroups (and partial results) of a bounds or selection pass

__device__ __forceinline__ long long hull_dev_side(const HullFaceRec& r, const int p[3])
{
    return r.n[0] * ((long long)p[0] - r.a[0]) + r.n[1] * ((long long)p[1] - r.a[1]) + r.n[2] * ((long long)p[2] - r.a[2]);
}
__device__ __forceinline__ long long hull_shfl_xor(long long v, int d)
{
    const int lo = __shfl_xor((int)(v & 0xffffffffll), d, 64), hi = __shfl_xor((int)(v >> 32), d, 64);
    return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ bool hull_finite(float x) { return fabsf(x) <= 3.402823466e38f; }      // (a NaN fails)

// ---- bounds and quantisation (steps 1 and 2) -----------------------------------------------------------------------------------------
// part [HULL_PARTS][8]: the finite points' minimum and maximum per axis (+inf / -inf without one), their count (bits), one unused word
__global__ __launch_bounds__(256) void k_hull_bounds(int n, const float* __restrict__ pts, float* __restrict__ part)
{
    __shared__ float sm[4][6];
    __shared__ unsigned sc[4];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned cnt = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (!(hull_finite(x) && hull_finite(y) && hull_finite(z))) continue;
        lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
        hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        ++cnt;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64)); }
        cnt += (unsigned)__shfl_xor((int)cnt, d, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { for (int a = 0; a < 3; ++a) { sm[wave][a] = lo[a]; sm[wave][3 + a] = hi[a]; } sc[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = part + 8 * (size_t)blockIdx.x;
        for (int a = 0; a < 3; ++a) {
            o[a] = fminf(fminf(sm[0][a], sm[1][a]), fminf(sm[2][a], sm[3][a]));
            o[3 + a] = fmaxf(fmaxf(sm[0][3 + a], sm[1][3 + a]), fmaxf(sm[2][3 + a], sm[3][3 + a]));
        }
        o[6] = __uint_as_float(sc[0] + sc[1] + sc[2] + sc[3]); o[7] = 0.f;
    }
}

struct HullQuant { double lo[3]; double s; };
// point i of the concatenation (pts [n][3], then extra [n_extra][3]): q_a = rint((double(p_a) - lo_a) * s), each operation rounded on its own
__global__ __launch_bounds__(256) void k_hull_quantise(int n, const float* __restrict__ pts, int n_extra, const float* __restrict__ extra, HullQuant Q,
                                                       int* __restrict__ q)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n + n_extra) return;
    const float* p = i < n ? pts + 3 * (size_t)i : extra + 3 * (size_t)(i - n);
    const float x = p[0], y = p[1], z = p[2];
    int* o = q + 3 * (size_t)i;
    if (!(hull_finite(x) && hull_finite(y) && hull_finite(z))) { o[0] = HULL_INVALID; o[1] = 0; o[2] = 0; return; }
    o[0] = (int)rint(__dmul_rn(__dsub_rn((double)x, Q.lo[0]), Q.s));
    o[1] = (int)rint(__dmul_rn(__dsub_rn((double)y, Q.lo[1]), Q.s));
    o[2] = (int)rint(__dmul_rn(__dsub_rn((double)z, Q.lo[2]), Q.s));
}

// ---- the first simplex (step 4) --------------------------------------------------------------------------------------------------------
// One pass per corner: the point with the largest score, ties to the smallest index.  mode 0: the lexicographically smallest (q_x, q_y,
// q_z) (the score is the complement of the packed triple); 1: the squared distance from a; 2: the largest |component| of u x (q - a);
// 3: |n . (q - a)|.  part [HULL_PARTS][2]: score (-1: the workgroup saw no finite point), index.
struct HullSel { int mode; int a[3]; long long u[3]; };
__device__ __forceinline__ long long hull_abs(long long v) { return v < 0 ? -v : v; }
__global__ __launch_bounds__(256) void k_hull_select(int N, const int* __restrict__ q, HullSel S, long long* __restrict__ part)
{
    __shared__ long long ss[4], si[4];
    long long best = -1, bidx = 0x7fffffffll;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const int x = q[3 * (size_t)i];
        if (x == HULL_INVALID) continue;
        const int y = q[3 * (size_t)i + 1], z = q[3 * (size_t)i + 2];
        const long long dx = (long long)x - S.a[0], dy = (long long)y - S.a[1], dz = (long long)z - S.a[2];
        long long sc;
        if (S.mode == 0) sc = ((1ll << 60) - 1) - (((long long)x << 40) | ((long long)y << 20) | (long long)z);
        else if (S.mode == 1) sc = dx * dx + dy * dy + dz * dz;
        else if (S.mode == 2) {
            const long long cx = S.u[1] * dz - S.u[2] * dy, cy = S.u[2] * dx - S.u[0] * dz, cz = S.u[0] * dy - S.u[1] * dx;
            sc = max(max(hull_abs(cx), hull_abs(cy)), hull_abs(cz));
        } else sc = hull_abs(S.u[0] * dx + S.u[1] * dy + S.u[2] * dz);
        if (sc > best) { best = sc; bidx = i; }             // (a thread walks ascending indices: a tie keeps the smaller)
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long os = hull_shfl_xor(best, d), oi = hull_shfl_xor(bidx, d);
        if (os > best || (os == best && oi < bidx)) { best = os; bidx = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { ss[wave] = best; si[wave] = bidx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) if (ss[w] > best || (ss[w] == best && si[w] < bidx)) { best = ss[w]; bidx = si[w]; }
        part[2 * (size_t)blockIdx.x] = best; part[2 * (size_t)blockIdx.x + 1] = bidx;
    }
}

// ---- outside sets (steps 5 and 6.7) ----------------------------------------------------------------------------------------------------
// The points walked: list[0 .. n_list) (NULL: every point of the cloud).  initial: every finite point moves; else a point moves when the
// apex (index, quantised coordinates aq) sees its face, which is how the host decides that the face dies.  A moving point goes to the
// first of the faces [first_new, first_new + n_new) it is outside of, or becomes interior (face_of = -1), as the apex does.
struct HullArgs { const int* list; int n_list; int initial; int apex; int aq[3]; int first_new, n_new; };

__global__ __launch_bounds__(256) void k_hull_rehome(HullArgs A, const int* __restrict__ q, int* __restrict__ face_of, const HullFaceRec* __restrict__ faces,
                                                     unsigned long long* __restrict__ best, unsigned long long* __restrict__ cnt)
{
    __shared__ unsigned long long s_best[HULL_SLOTS];
    __shared__ unsigned s_cnt[HULL_SLOTS];
    const int nslot = min(A.n_new, HULL_SLOTS);
    for (int t = threadIdx.x; t < nslot; t += 256) { s_best[t] = 0ull; s_cnt[t] = 0u; }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < A.n_list) {
        const int p = A.list ? A.list[i] : (int)i;
        int qp[3];
        qp[0] = q[3 * (size_t)p];
        bool move;
        if (A.initial) {
            move = qp[0] != HULL_INVALID;
            if (!move) face_of[p] = -1;
        } else {
            const int f = face_of[p];
            move = f >= 0 && hull_dev_side(faces[f], A.aq) > 0;
        }
        if (move) {
            qp[1] = q[3 * (size_t)p + 1]; qp[2] = q[3 * (size_t)p + 2];
            int g = -1;
            long long det = 0;
            if (p != A.apex)
                for (int k = 0; k < A.n_new; ++k) {
                    const long long d = hull_dev_side(faces[A.first_new + k], qp);
                    if (d > 0) { g = k; det = d; break; }
                }
            face_of[p] = g < 0 ? -1 : A.first_new + g;
            if (g >= 0) {
                if (g < HULL_SLOTS) { atomicMax(&s_best[g], (unsigned long long)det); atomicAdd(&s_cnt[g], 1u); }
                else { atomicMax(&best[g], (unsigned long long)det); atomicAdd(&cnt[g], 1ull); }
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nslot; t += 256)
        if (s_cnt[t]) { atomicMax(&best[t], s_best[t]); atomicAdd(&cnt[t], (unsigned long long)s_cnt[t]); }
}

// the smallest index among the points of a new face that reach its largest det (the det is recomputed: the same integers)
__global__ __launch_bounds__(256) void k_hull_argmin(HullArgs A, const int* __restrict__ q, const int* __restrict__ face_of,
                                                     const HullFaceRec* __restrict__ faces, const unsigned long long* __restrict__ best,
                                                     unsigned* __restrict__ arg)
{
    __shared__ unsigned s_arg[HULL_SLOTS];
    const int nslot = min(A.n_new, HULL_SLOTS);
    for (int t = threadIdx.x; t < nslot; t += 256) s_arg[t] = 0xffffffffu;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < A.n_list) {
        const int p = A.list ? A.list[i] : (int)i;
        const int f = face_of[p];
        if (f >= A.first_new && f - A.first_new < A.n_new) {
            const int g = f - A.first_new;
            const int qp[3] = {q[3 * (size_t)p], q[3 * (size_t)p + 1], q[3 * (size_t)p + 2]};
            if ((unsigned long long)hull_dev_side(faces[f], qp) == best[g]) {
                if (g < HULL_SLOTS) atomicMin(&s_arg[g], (unsigned)p);
                else atomicMin(&arg[g], (unsigned)p);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nslot; t += 256)
        if (s_arg[t] != 0xffffffffu) atomicMin(&arg[t], s_arg[t]);
}

// the reports of the new faces; their words are left as the next insertion expects them (0, 0, no index)
__global__ __launch_bounds__(256) void k_hull_report(int n_new, unsigned long long* __restrict__ best, unsigned long long* __restrict__ cnt,
                                                     unsigned* __restrict__ arg, const int* __restrict__ q, HullReport* __restrict__ rep)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_new) return;
    HullReport r;
    r.count = (long long)cnt[j];
    r.apex = r.count > 0 ? (int)arg[j] : -1;
    r.q[0] = r.q[1] = r.q[2] = 0;
    if (r.apex >= 0) { r.q[0] = q[3 * (size_t)r.apex]; r.q[1] = q[3 * (size_t)r.apex + 1]; r.q[2] = q[3 * (size_t)r.apex + 2]; }
    rep[j] = r;
    best[j] = 0ull; cnt[j] = 0ull; arg[j] = 0xffffffffu;
}

// the list re-compacted to the points that still belong to a face: count per workgroup -> mc_scan -> rank inside the workgroup, so the
// list stays in ascending order of its first form whatever the scheduling
__global__ __launch_bounds__(256) void k_hull_flags(const int* __restrict__ list, int n_list, const int* __restrict__ face_of, unsigned* __restrict__ bsum)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (i < n_list) on = face_of[list ? list[i] : (int)i] >= 0;
    unsigned total;
    block_scan(on ? 1u : 0u, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_hull_compact(const int* __restrict__ list, int n_list, const int* __restrict__ face_of,
                                                      const unsigned* __restrict__ boff, unsigned cap, int* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    int p = 0;
    if (i < n_list) { p = list ? list[i] : (int)i; on = face_of[p] >= 0; }
    unsigned total;
    const unsigned one = on ? 1u : 0u, rank = boff[blockIdx.x] + (block_scan(one, &total) - one);
    if (on && rank < cap) out[rank] = p;
}

// the fp32 coordinates of the listed points of pts
__global__ __launch_bounds__(256) void k_hull_gather(int m, const int* __restrict__ idx, const float* __restrict__ pts, float* __restrict__ out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const size_t p = (size_t)idx[j];
    out[3 * (size_t)j] = pts[3 * p]; out[3 * (size_t)j + 1] = pts[3 * p + 1]; out[3 * (size_t)j + 2] = pts[3 * p + 2];
}

// ---- the lattice nodes inside the scaled hull (nsk_lattice_in_hull) ------------------------------------------------------------------
// One thread per node, x fastest.  planes [nf][6] = (n, A') from hull_mask_planes; a node is inside when it lies in the box of the scaled
// vertices and no face has s = (w_x n_x + w_y n_y) + w_z n_z > 0, w = P - A', every operation an fp64 operation of its own.
struct HullBox { double lo[3], hi[3]; };
__global__ __launch_bounds__(256) void k_lattice_in_hull(McGeom G, int nf, const double* __restrict__ planes, HullBox B, int accumulate,
                                                         uint8_t* __restrict__ valid, unsigned long long* __restrict__ count)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool live = n < G.nn;
    bool in = false, old = false;
    double P[3] = {0.0, 0.0, 0.0};
    if (live) {
        float p[3];
        lattice_node(G, n, p);
        old = accumulate && valid[n] != 0;
        in = nf > 0;
        for (int a = 0; a < 3; ++a) { P[a] = (double)p[a]; in = in && P[a] >= B.lo[a] && P[a] <= B.hi[a]; }
    }
    bool open = in && !old;                                 // still to be decided by the faces
    for (int f = 0; f < nf; ++f) {
        if (__all(!open)) break;                            // the whole wave is outside (or was set before)
        if (!open) continue;
        const double* pl = planes + 6 * (size_t)f;
        const double wx = __dsub_rn(P[0], pl[3]), wy = __dsub_rn(P[1], pl[4]), wz = __dsub_rn(P[2], pl[5]);
        const double s = __dadd_rn(__dadd_rn(__dmul_rn(wx, pl[0]), __dmul_rn(wy, pl[1])), __dmul_rn(wz, pl[2]));
        if (s > 0.0) { in = false; open = false; }
    }
    const bool set = old || in;
    if (live) valid[n] = set ? 1 : 0;
    if (count) wave_count(live && set, count);
}

// ---- the points' side of hull_plan_run ------------------------------------------------------------------------------------------------
struct HullDevice {
    nsk_ctx* c;
    int N;
    const int* list = nullptr;          // NULL: every point
    int n_list = 0, which = 0;
    long long compactions = 0;
    std::vector<HullFaceRec> all;       // every face's planes, as the device holds them (re-uploaded when its table grows)

    int compact(long long outside)
    {
        nsk_ctx::Hull& U = c->hull;
        const int nb = (n_list + MC_BLOCK - 1) / MC_BLOCK;
        const size_t words = mc_scan_words((size_t)nb + 1);
        CHK(grow(c, U.scan, words, "the hull's scan scratch", GROW_NO_CAPTURE));
        CHK(grow(c, U.list[which], (size_t)std::max<long long>(outside, 1), "the list of outside points", GROW_NO_CAPTURE));
        HIPCHK(hipMemsetAsync(U.scan, 0, words * 4, c->stream));
        { ProfScope ps(c, "hull_compact");
          k_hull_flags<<<nb, MC_BLOCK, 0, c->stream>>>(list, n_list, U.face_of, U.scan);
          HIPCHK(hipGetLastError());
          CHK(mc_scan(c, U.scan, nb + 1));
          k_hull_compact<<<nb, MC_BLOCK, 0, c->stream>>>(list, n_list, U.face_of, U.scan, (unsigned)outside, U.list[which]);
          HIPCHK(hipGetLastError()); }
        list = U.list[which]; n_list = (int)outside; which ^= 1;
        ++compactions;
        return 0;
    }

    int rehome(bool initial, int apex, const int* aq, int first_new, int n_new, const HullFaceRec* recs, long long outside, HullReport* out)
    {
        nsk_ctx::Hull& U = c->hull;
        if (!initial && n_list > MC_BLOCK && outside * 2 < (long long)n_list) CHK(compact(outside));
        if ((size_t)first_new != all.size()) return fail("nsk_points_hull: face %d follows %zu faces", first_new, all.size());
        all.insert(all.end(), recs, recs + n_new);
        if (all.size() > U.faces.cap()) {
            CHK(grow(c, U.faces, std::max<size_t>(2 * all.size(), 1024), "the hull's face planes", GROW_NO_CAPTURE));
            HIPCHK(hipMemcpyAsync(U.faces, all.data(), all.size() * sizeof(HullFaceRec), hipMemcpyHostToDevice, c->stream));
        } else
            HIPCHK(hipMemcpyAsync(U.faces.get() + first_new, recs, (size_t)n_new * sizeof(HullFaceRec), hipMemcpyHostToDevice, c->stream));
        if ((size_t)n_new > U.rep.cap()) {
            const size_t cap = std::max<size_t>(2 * (size_t)n_new, 1024);
            CHK(grow(c, U.best, cap, "the new faces' largest dets", GROW_NO_CAPTURE));
            CHK(grow(c, U.cnt, cap, "the new faces' counts", GROW_NO_CAPTURE));
            CHK(grow(c, U.arg, cap, "the new faces' apexes", GROW_NO_CAPTURE));
            CHK(grow(c, U.rep, cap, "the new faces' reports", GROW_NO_CAPTURE));
            HIPCHK(hipMemsetAsync(U.best, 0, cap * 8, c->stream));
            HIPCHK(hipMemsetAsync(U.cnt, 0, cap * 8, c->stream));
            HIPCHK(hipMemsetAsync(U.arg, 0xff, cap * 4, c->stream));
        }
        HullArgs A;
        A.list = list; A.n_list = n_list; A.initial = initial ? 1 : 0; A.apex = apex;
        A.aq[0] = aq[0]; A.aq[1] = aq[1]; A.aq[2] = aq[2]; A.first_new = first_new; A.n_new = n_new;
        const unsigned nb = (unsigned)((n_list + 255) / 256);
        if (nb) {
            ProfScope ps(c, "hull_rehome");
            k_hull_rehome<<<nb, 256, 0, c->stream>>>(A, U.q, U.face_of, U.faces, U.best, U.cnt);
            k_hull_argmin<<<nb, 256, 0, c->stream>>>(A, U.q, U.face_of, U.faces, U.best, U.arg);
        }
        k_hull_report<<<(n_new + 255) / 256, 256, 0, c->stream>>>(n_new, U.best, U.cnt, U.arg, U.q, U.rep);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, U.rep, (size_t)n_new * sizeof(HullReport), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
};

// one selection pass and its finish on the host; q_out: the quantised coordinates of the chosen point
static int hull_select(nsk_ctx* c, int N, const HullSel& S, long long* score, int* index, int q_out[3])
{
    nsk_ctx::Hull& U = c->hull;
    const int nb = (int)std::min<long long>(((long long)N + 255) / 256, HULL_PARTS);
    long long h[2 * HULL_PARTS];
    { ProfScope ps(c, "hull_select"); k_hull_select<<<nb, 256, 0, c->stream>>>(N, U.q, S, U.part); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, U.part, (size_t)nb * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long best = -1, bidx = 0x7fffffffll;
    for (int b = 0; b < nb; ++b) if (h[2 * b] > best || (h[2 * b] == best && h[2 * b + 1] < bidx)) { best = h[2 * b]; bidx = h[2 * b + 1]; }
    *score = best; *index = (int)bidx;
    if (best >= 0) {
        HIPCHK(hipMemcpyAsync(q_out, U.q.get() + 3 * (size_t)bidx, 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int nsk_points_hull(nsk_ctx* c, const float* pts, int n, const float* extra, int n_extra, long long* info)
{
    if (!c) return fail("nsk_points_hull: null ctx");
    if (!info) return fail("nsk_points_hull: h_info is NULL");
    if (n < 0 || n_extra < 0) return fail("nsk_points_hull: n = %d, n_extra = %d", n, n_extra);
    if ((long long)n + n_extra > 0x7fffffffll) return fail("nsk_points_hull: %lld points, at most 2^31 - 1", (long long)n + n_extra);
    if (n > 0 && !pts) return fail("nsk_points_hull: d_points is NULL with n = %d", n);
    if (n_extra > 0 && !extra) return fail("nsk_points_hull: h_extra is NULL with n_extra = %d", n_extra);
    if (c->capturing) return fail("nsk_points_hull: not while a graph is being captured");
    nsk_ctx::Hull& U = c->hull;
    U.clear();
    for (int k = 0; k < 8; ++k) info[k] = 0;
    const int N = n + n_extra;
    if (N == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    // steps 1 and 2: the finite points' box (the device's partial boxes and the host points, combined here: minima and maxima are exact)
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    long long finite = 0;
    CHK(grow(c, U.part, 4 * HULL_PARTS, "the hull's partial results", GROW_NO_CAPTURE));      // (8 floats or 2 int64 per workgroup)
    if (n > 0) {
        const int nb = (int)std::min<long long>(((long long)n + 255) / 256, HULL_PARTS);
        std::vector<float> h((size_t)nb * 8);
        float* part = reinterpret_cast<float*>(U.part.get());
        { ProfScope ps(c, "hull_bounds"); k_hull_bounds<<<nb, 256, 0, c->stream>>>(n, pts, part); }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h.data(), part, h.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int b = 0; b < nb; ++b) {
            unsigned cnt;
            memcpy(&cnt, &h[8 * (size_t)b + 6], 4);
            finite += cnt;
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)h[8 * (size_t)b + a]); hi[a] = std::max(hi[a], (double)h[8 * (size_t)b + 3 + a]); }
        }
    }
    for (int i = 0; i < n_extra; ++i) {
        const float* p = extra + 3 * (size_t)i;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
        ++finite;
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)p[a]); hi[a] = std::max(hi[a], (double)p[a]); }
    }
    info[0] = finite; info[1] = (long long)N - finite;
    if (finite == 0) return 0;
    const double E = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    if (!(E > 0.0)) return 0;                               // (rank 0: every finite point is the same point)
    const double quantum = E / (double)HULL_QMAX;
    memcpy(&info[6], &quantum, 8);
    HullQuant Q;
    for (int a = 0; a < 3; ++a) Q.lo[a] = lo[a];
    Q.s = hull_scale(E);
    CHK(grow(c, U.q, (size_t)N * 3, "the quantised points", GROW_NO_CAPTURE));
    CHK(grow(c, U.face_of, (size_t)N, "the points' faces", GROW_NO_CAPTURE));
    if (n_extra > 0) {
        CHK(grow(c, U.extra, (size_t)n_extra * 3, "the host points", GROW_NO_CAPTURE));
        HIPCHK(hipMemcpyAsync(U.extra, extra, (size_t)n_extra * 12, hipMemcpyHostToDevice, c->stream));
    }
    { ProfScope ps(c, "hull_quantise");
      k_hull_quantise<<<(unsigned)(((long long)N + 255) / 256), 256, 0, c->stream>>>(n, pts, n_extra, U.extra, Q, U.q); }
    HIPCHK(hipGetLastError());
    // step 4
    int idx[4], q[4][3];
    long long score;
    HullSel S;
    memset(&S, 0, sizeof(S));
    S.mode = 0;
    CHK(hull_select(c, N, S, &score, &idx[0], q[0]));
    S.mode = 1; memcpy(S.a, q[0], 12);
    CHK(hull_select(c, N, S, &score, &idx[1], q[1]));
    if (score == 0) return 0;
    info[2] = 1;
    S.mode = 2;
    for (int a = 0; a < 3; ++a) S.u[a] = (long long)q[1][a] - q[0][a];
    CHK(hull_select(c, N, S, &score, &idx[2], q[2]));
    if (score == 0) return 0;
    info[2] = 2;
    S.mode = 3;
    hull_normal(q[0], q[1], q[2], S.u);
    CHK(hull_select(c, N, S, &score, &idx[3], q[3]));
    if (score == 0) return 0;
    info[2] = 3;
    // steps 5 .. 7
    HullPlan P;
    P.start(idx, q);
    HullDevice D;
    D.c = c; D.N = N; D.list = nullptr; D.n_list = N;
    const int r = hull_plan_run(P, D);
    if (r == -2) return fail("nsk_points_hull: the face table lost an edge's twin");
    if (r != 0) return r;
    std::vector<int> verts, tris;
    P.result(verts, tris);
    // the hull vertices' own fp32 coordinates, for the mask
    const int nv = (int)verts.size();
    std::vector<float> xyz((size_t)nv * 3);
    const int nd = (int)(std::lower_bound(verts.begin(), verts.end(), n) - verts.begin());       // vertices among the device points
    if (nd > 0) {
        CHK(grow(c, U.gidx, (size_t)nd, "the hull vertices' indices", GROW_NO_CAPTURE));
        CHK(grow(c, U.gxyz, (size_t)nd * 3, "the hull vertices' coordinates", GROW_NO_CAPTURE));
        HIPCHK(hipMemcpyAsync(U.gidx, verts.data(), (size_t)nd * 4, hipMemcpyHostToDevice, c->stream));
        k_hull_gather<<<(nd + 255) / 256, 256, 0, c->stream>>>(nd, U.gidx, pts, U.gxyz);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(xyz.data(), U.gxyz, (size_t)nd * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    for (int k = nd; k < nv; ++k) memcpy(&xyz[3 * (size_t)k], extra + 3 * (size_t)(verts[(size_t)k] - n), 12);
    U.set(verts, tris, xyz);
    info[3] = nv; info[4] = (long long)tris.size() / 3; info[5] = P.insertions; info[7] = D.compactions;
    return 0;
}

extern "C" int nsk_hull_download(nsk_ctx* c, int32_t* h_vertices, int32_t* h_faces)
{
    if (!c) return fail("nsk_hull_download: null ctx");
    const nsk_ctx::Hull& U = c->hull;
    if (h_vertices && !U.verts.empty()) memcpy(h_vertices, U.verts.data(), U.verts.size() * 4);
    if (h_faces && !U.tris.empty()) memcpy(h_faces, U.tris.data(), U.tris.size() * 4);
    return 0;
}

extern "C" int nsk_hull_upload(nsk_ctx* c, const float* xyz, int nv, const int32_t* faces, int nf)
{
    if (!c) return fail("nsk_hull_upload: null ctx");
    if (nv < 4 || nf < 4) return fail("nsk_hull_upload: %d vertices, %d faces, a hull has at least 4 of each", nv, nf);
    if (nv > (1 << 24) || nf > (1 << 24)) return fail("nsk_hull_upload: %d vertices, %d faces, at most 2^24 of each", nv, nf);
    if (!xyz || !faces) return fail("nsk_hull_upload: h_xyz / h_faces is NULL");
    for (size_t k = 0; k < (size_t)nv * 3; ++k) if (!std::isfinite(xyz[k])) return fail("nsk_hull_upload: vertex %zu has a non-finite coordinate", k / 3);
    for (size_t k = 0; k < (size_t)nf * 3; ++k)
        if (faces[k] < 0 || faces[k] >= nv) return fail("nsk_hull_upload: face %zu names vertex %d of %d", k / 3, faces[k], nv);
    std::vector<int> verts((size_t)nv), tris(faces, faces + (size_t)nf * 3);
    for (int k = 0; k < nv; ++k) verts[(size_t)k] = k;
    std::vector<float> v(xyz, xyz + (size_t)nv * 3);
    c->hull.set(verts, tris, v);
    return 0;
}

extern "C" int nsk_lattice_in_hull(nsk_ctx* c, const float* o, const float* s, int nx, int ny, int nz, double scale, int accumulate, uint8_t* valid,
                                   long long* n_inside)
{
    CHK(lattice_checks("nsk_lattice_in_hull", c, o, s, nx, ny, nz, 1));      // (refuses a call while a graph is being captured)
    if (!valid) return fail("nsk_lattice_in_hull: d_valid is NULL");
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail("nsk_lattice_in_hull: scale = %g, must be positive and finite", scale);
    const long long total = (long long)nx * ny * nz;
    if (total > MC_MAX_NODES) return fail("nsk_lattice_in_hull: %lld nodes, at most %lld per call", total, (long long)MC_MAX_NODES);
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Hull& U = c->hull;
    const int nf = (int)(U.local.size() / 3);
    HullBox B;
    for (int a = 0; a < 3; ++a) { B.lo[a] = 0.0; B.hi[a] = 0.0; }
    if (nf > 0) {
        std::vector<double> planes;
        double box[6];
        hull_mask_planes((int)U.verts.size(), U.xyz.data(), nf, U.local.data(), scale, planes, box);
        for (int a = 0; a < 3; ++a) { B.lo[a] = box[a]; B.hi[a] = box[3 + a]; }
        CHK(grow(c, U.planes, planes.size(), "the hull's planes", GROW_NO_CAPTURE));
        HIPCHK(hipMemcpyAsync(U.planes, planes.data(), planes.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));            // (the planes' host copy ends with this scope)
    }
    CHK(count_begin(c, n_inside, "the inside count"));
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = (int)total; G.level = 0.f;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    const int nb = (G.nn + MC_BLOCK - 1) / MC_BLOCK;
    { ProfScope ps(c, "lattice_in_hull");
      k_lattice_in_hull<<<nb, MC_BLOCK, 0, c->stream>>>(G, nf, U.planes, B, accumulate ? 1 : 0, valid, n_inside ? c->count.get() : nullptr); }
    HIPCHK(hipGetLastError());
    return count_end(c, n_inside);
}

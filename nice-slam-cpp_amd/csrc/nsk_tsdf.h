// nsk_tsdf.h -- depth frames at known poses fused into a truncated signed distance volume on a lattice, and that volume handed to
// nsk_mesh_extract (upstream's get_bound_from_frames fuses with Open3D's ScalableTSDFVolume; here the volume is dense and on the device).
// include/nsk.h states the contract; this file is included by nsk.hip behind the context and the buffer helpers.
//
// The rule, word for word (include/nsk.h, nsk_tsdf_integrate; tests/tsdf_checks.py fuse_f32 restates it one numpy operation per fp32
// operation).  Frame k sees the node p when, every operation an fp32 operation of its own (no FMA):
//   c_a = ((w[4a] p0 + w[4a+1] p1) + w[4a+2] p2) + w[4a+3], a = 0..2;   d = -c_2 > 0;
//   u = cx + (fx c_0) / d,  v = cy - (fy c_1) / d;   i = floor(u + 0.5), j = floor(v + 0.5)   (the nearest pixel);
//   edge <= i < W - edge and edge <= j < H - edge, decided on the floats (a NaN fails);
//   D = d_depth[k][j][i] is finite and > 0;   d <= D + trunc.
// A frame that sees the node updates it, frames in ascending k, one rounding each:
//   sdf = D - d;   t = min(1, sdf / trunc);   T <- ((W T) + t) / (W + 1);   W <- min(W + 1, max_weight).
// The projection is restated here rather than shared with k_lattice_seen, whose code stays as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "nsk_mesh.h"

#define TSDF_MAX_K 32               // frames per launch: 12 floats each in the kernel arguments
#define TSDF_AHEAD 4                // frames whose projections and depth loads are issued before the first of their updates (a first choice)
#define TSDF_FLT_MAX 3.402823466e38f
struct TsdfArgs {
    float w[TSDF_MAX_K][12];        // rows 0..2 of the row-major world-to-camera matrices
    int K, H, W;
    float fx, fy, cx, cy;
    float ilo, ihi, jlo, jhi;       // edge <= i < W - edge, edge <= j < H - edge, as floats (exact: H, W <= 2^24)
    float trunc, max_weight;
    int accumulate;
};

// One thread per node, x fastest.  T and W stay in registers over the launch's frames and are stored once.  Every frame counts, so no wave
// leaves the loop early.  The frames go in groups of TSDF_AHEAD: a group's projections and gathers are issued first (they do not depend on
// T and W), then its updates run in frame order (each a dependent multiply, add and division).
__global__ __launch_bounds__(256) void k_tsdf_integrate(McGeom G, TsdfArgs A, const float* __restrict__ depth, float* __restrict__ tsdf,
                                                        float* __restrict__ weight, unsigned long long* __restrict__ count)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool live = n < G.nn;
    float T = 0.f, Wt = 0.f;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        const int i = n % G.nx, r = n / G.nx, j = r % G.ny, k = r / G.ny;
        p[0] = mc_coord(G.o[0], i, G.s[0]); p[1] = mc_coord(G.o[1], j, G.s[1]); p[2] = mc_coord(G.o[2], k, G.s[2]);
        if (A.accumulate) { T = tsdf[n]; Wt = weight[n]; }     // (accumulate == 0: the old values are never read, so no 0 * NaN)
    }
    const size_t img = (size_t)A.H * A.W;
    for (int k0 = 0; k0 < A.K; k0 += TSDF_AHEAD) {
        float d[TSDF_AHEAD], D[TSDF_AHEAD];
#pragma unroll
        for (int g = 0; g < TSDF_AHEAD; ++g) {
            const int kf = k0 + g;
            d[g] = 0.f; D[g] = 0.f;                             // (D = 0: no measurement, the frame does not see the node)
            if (kf >= A.K || !live) continue;
            const float* w = A.w[kf];
            float c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                c[a] = __fadd_rn(__fadd_rn(__fadd_rn(mc_mul(w[4 * a], p[0]), mc_mul(w[4 * a + 1], p[1])), mc_mul(w[4 * a + 2], p[2])), w[4 * a + 3]);
            d[g] = -c[2];
            if (!(d[g] > 0.f)) continue;
            const float u = __fadd_rn(A.cx, __fdiv_rn(mc_mul(A.fx, c[0]), d[g]));
            const float v = __fsub_rn(A.cy, __fdiv_rn(mc_mul(A.fy, c[1]), d[g]));
            const float fi = floorf(__fadd_rn(u, 0.5f)), fj = floorf(__fadd_rn(v, 0.5f));
            if (!(fi >= A.ilo && fi < A.ihi && fj >= A.jlo && fj < A.jhi)) continue;        // (NaN fails; decided before any conversion to int)
            D[g] = depth[(size_t)kf * img + (size_t)(int)fj * A.W + (int)fi];
        }
#pragma unroll
        for (int g = 0; g < TSDF_AHEAD; ++g) {
            if (!(D[g] > 0.f && D[g] <= TSDF_FLT_MAX)) continue;                            // no measurement: 0, negative, NaN, inf
            if (!(d[g] <= __fadd_rn(D[g], A.trunc))) continue;
            const float t = fminf(1.f, __fdiv_rn(__fsub_rn(D[g], d[g]), A.trunc));
            T = __fdiv_rn(__fadd_rn(mc_mul(Wt, T), t), __fadd_rn(Wt, 1.f));
            Wt = fminf(__fadd_rn(Wt, 1.f), A.max_weight);
        }
    }
    if (live) { tsdf[n] = T; weight[n] = Wt; }
    if (count) {
        const unsigned long long b = __ballot(live && Wt > 0.f);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
    }
}

// W >= min_weight: the volume is -T (the sign bit flipped: nsk_mesh_extract's inside is value > level, the solid lies behind the surface)
// and the node is valid; otherwise a quiet NaN and 0.  A workgroup walks its nodes with a uniform trip count, so the ballot is whole.
__global__ __launch_bounds__(256) void k_tsdf_volume(long long n, const float* __restrict__ tsdf, const float* __restrict__ weight, float min_weight,
                                                     float* __restrict__ vol, uint8_t* __restrict__ valid, unsigned long long* __restrict__ count)
{
    const long long stride = (long long)gridDim.x * 256;
    unsigned long long mine = 0;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += stride) {
        const long long q = base + threadIdx.x;
        bool ok = false;
        if (q < n) {
            ok = weight[q] >= min_weight;                       // (a NaN weight fails)
            vol[q] = ok ? __uint_as_float(__float_as_uint(tsdf[q]) ^ 0x80000000u) : __uint_as_float(0x7fc00000u);
            if (valid) valid[q] = ok ? 1 : 0;
        }
        if (count) mine += (unsigned long long)__popcll(__ballot(ok));
    }
    if (count && (threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int nsk_tsdf_integrate(nsk_ctx* c, const float* o, const float* s, int nx, int ny, int nz, int K, const float* depth, int H, int W,
                                  float fx, float fy, float cx, float cy, const float* w2c, int edge, float trunc, float max_weight, int accumulate,
                                  float* tsdf, float* weight, long long* n_observed)
{
    CHK(lattice_checks("nsk_tsdf_integrate", c, o, s, nx, ny, nz, 1));      // (refuses a call while a graph is being captured)
    if (!tsdf || !weight) return fail("nsk_tsdf_integrate: d_tsdf / d_weight is NULL");
    if (K < 0) return fail("nsk_tsdf_integrate: K = %d", K);
    if (K > 0 && (!depth || !w2c)) return fail("nsk_tsdf_integrate: d_depth / h_w2c is NULL with K = %d", K);
    if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return fail("nsk_tsdf_integrate: image %d x %d, need 1 .. 2^24 pixels per side", H, W);
    if (edge < 0) return fail("nsk_tsdf_integrate: edge = %d, must be >= 0", edge);
    if (!std::isfinite(trunc) || !(trunc > 0.f)) return fail("nsk_tsdf_integrate: trunc = %g, must be positive and finite", (double)trunc);
    if (!(max_weight >= 1.f) || !(max_weight <= 16777216.f)) return fail("nsk_tsdf_integrate: max_weight = %g, must be 1 .. 2^24", (double)max_weight);
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy)) return fail("nsk_tsdf_integrate: intrinsics are not finite");
    const long long total = (long long)nx * ny * nz;
    if (total > MC_MAX_NODES) return fail("nsk_tsdf_integrate: %lld nodes, at most %lld per call", total, (long long)MC_MAX_NODES);
    HIPCHK(hipSetDevice(c->device));
    if (n_observed) {
        CHK(grow(c, c->tsdf.count, 1, "the observed count", 0));
        HIPCHK(hipMemsetAsync(c->tsdf.count, 0, 8, c->stream));
    }
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = (int)total; G.level = 0.f;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    TsdfArgs A;
    memset(&A, 0, sizeof(A));
    A.H = H; A.W = W; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.trunc = trunc; A.max_weight = max_weight;
    A.ilo = A.jlo = (float)edge;                            // (edge beyond 2^24 rounds, and is beyond W and H either way)
    A.ihi = (float)((long long)W - edge); A.jhi = (float)((long long)H - edge);
    const int nb = (G.nn + MC_BLOCK - 1) / MC_BLOCK;
    int k0 = 0;
    do {                                                    // (K = 0 still launches once: it clears, or keeps, and counts)
        A.K = std::min(K - k0, TSDF_MAX_K);
        A.accumulate = (accumulate || k0 > 0) ? 1 : 0;
        for (int k = 0; k < A.K; ++k) memcpy(A.w[k], w2c + 16 * (size_t)(k0 + k), 12 * sizeof(float));
        const bool last = k0 + A.K >= K;
        { ProfScope ps(c, "tsdf_integrate");
          k_tsdf_integrate<<<nb, MC_BLOCK, 0, c->stream>>>(G, A, depth ? depth + (size_t)k0 * H * W : nullptr, tsdf, weight,
                                                           last && n_observed ? c->tsdf.count.get() : nullptr); }
        HIPCHK(hipGetLastError());
        k0 += A.K;
    } while (k0 < K);
    if (n_observed) {
        unsigned long long cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, c->tsdf.count, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *n_observed = (long long)cnt;
    }
    return 0;
}

extern "C" int nsk_tsdf_volume(nsk_ctx* c, long long n, const float* tsdf, const float* weight, float min_weight, float* vol, uint8_t* valid,
                               long long* n_valid)
{
    if (!c) return fail("nsk_tsdf_volume: null ctx");
    if (n < 0) return fail("nsk_tsdf_volume: n = %lld", n);
    if (n > 0 && (!tsdf || !weight || !vol)) return fail("nsk_tsdf_volume: d_tsdf / d_weight / d_volume is NULL with n = %lld", n);
    if (std::isnan(min_weight)) return fail("nsk_tsdf_volume: min_weight is NaN");
    if (c->capturing) return fail("nsk_tsdf_volume: not while a graph is being captured");
    if (n_valid) *n_valid = 0;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    if (n_valid) {
        CHK(grow(c, c->tsdf.count, 1, "the valid count", 0));
        HIPCHK(hipMemsetAsync(c->tsdf.count, 0, 8, c->stream));
    }
    const unsigned nb = (unsigned)std::min<long long>((n + 255) / 256, 1ll << 20);
    { ProfScope ps(c, "tsdf_volume");
      k_tsdf_volume<<<nb, 256, 0, c->stream>>>(n, tsdf, weight, min_weight, vol, valid, n_valid ? c->tsdf.count.get() : nullptr); }
    HIPCHK(hipGetLastError());
    if (n_valid) {
        unsigned long long cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, c->tsdf.count, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *n_valid = (long long)cnt;
    }
    return 0;
}

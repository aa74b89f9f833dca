// nsk_tsdf.h -- depth frames at known poses fused into a truncated signed distance volume on a lattice, and that volume handed to
// nsk_mesh_extract (upstream's get_bound_from_frames fuses with Open3D's ScalableTSDFVolume; here the volume is dense and on the device).
// include/nsk.h states the contract; this file is included by nsk.hip behind the context and the buffer helpers.
//
// Which frames see a node, and through which pixel: the rule of nsk_view.h, with reach = trunc (include/nsk.h, nsk_tsdf_integrate;
// tests/tsdf_checks.py fuse_f32 restates the update one numpy operation per fp32 operation).  A frame that sees the node updates it, frames
// in ascending k, one rounding each:
//   sdf = D - d;   t = min(1, sdf / trunc);   T <- ((W T) + t) / (W + 1);   W <- min(W + 1, max_weight).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "nsk_mesh.h"

#define TSDF_AHEAD 4                // frames whose projections and depth loads are issued before the first of their updates (a first choice)

// One thread per node, x fastest.  T and W stay in registers over the launch's frames and are stored once.  Every frame counts, so no wave
// leaves the loop early.  The frames go in groups of TSDF_AHEAD: a group's projections and gathers are issued first (they do not depend on
// T and W), then its updates run in frame order (each a dependent multiply, add and division).
__global__ __launch_bounds__(256) void k_tsdf_integrate(McGeom G, ViewArgs A, float max_weight, const float* __restrict__ depth,
                                                        float* __restrict__ tsdf, float* __restrict__ weight, unsigned long long* __restrict__ count)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool live = n < G.nn;
    float T = 0.f, Wt = 0.f;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        lattice_node(G, n, p);
        if (A.accumulate) { T = tsdf[n]; Wt = weight[n]; }     // (accumulate == 0: the old values are never read, so no 0 * NaN)
    }
    for (int k0 = 0; k0 < A.K; k0 += TSDF_AHEAD) {
        float d[TSDF_AHEAD], D[TSDF_AHEAD];
#pragma unroll
        for (int g = 0; g < TSDF_AHEAD; ++g) {
            const int kf = k0 + g;
            float fi, fj;
            d[g] = 0.f; D[g] = 0.f;                             // (D = 0: no measurement, the frame does not see the node)
            if (kf >= A.K || !live) continue;
            if (!view_project(A, A.w[kf], p, d[g], fi, fj)) continue;
            D[g] = view_pixel(A, depth, kf, fi, fj);
        }
#pragma unroll
        for (int g = 0; g < TSDF_AHEAD; ++g) {
            if (!view_measured(D[g])) continue;
            if (!(d[g] <= __fadd_rn(D[g], A.reach))) continue;
            const float t = fminf(1.f, __fdiv_rn(__fsub_rn(D[g], d[g]), A.reach));
            T = __fdiv_rn(__fadd_rn(mul_rn(Wt, T), t), __fadd_rn(Wt, 1.f));
            Wt = fminf(__fadd_rn(Wt, 1.f), max_weight);
        }
    }
    if (live) { tsdf[n] = T; weight[n] = Wt; }
    if (count) wave_count(live && Wt > 0.f, count);
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
    CHK(view_checks("nsk_tsdf_integrate", H, W, fx, fy, cx, cy, edge));
    if (!std::isfinite(trunc) || !(trunc > 0.f)) return fail("nsk_tsdf_integrate: trunc = %g, must be positive and finite", (double)trunc);
    if (!(max_weight >= 1.f) || !(max_weight <= 16777216.f)) return fail("nsk_tsdf_integrate: max_weight = %g, must be 1 .. 2^24", (double)max_weight);
    const long long total = (long long)nx * ny * nz;
    if (total > MC_MAX_NODES) return fail("nsk_tsdf_integrate: %lld nodes, at most %lld per call", total, (long long)MC_MAX_NODES);
    HIPCHK(hipSetDevice(c->device));
    CHK(count_begin(c, n_observed, "the observed count"));
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = (int)total; G.level = 0.f;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    const int nb = (G.nn + MC_BLOCK - 1) / MC_BLOCK;
    CHK(view_batches(c, "tsdf_integrate", view_args(H, W, fx, fy, cx, cy, edge, trunc), K, w2c, depth, accumulate,
                     [&](const ViewArgs& A, const float* dk, int, bool last) {
        k_tsdf_integrate<<<nb, MC_BLOCK, 0, c->stream>>>(G, A, max_weight, dk, tsdf, weight, last && n_observed ? c->count.get() : nullptr); }));
    return count_end(c, n_observed);
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
    CHK(count_begin(c, n_valid, "the valid count"));
    const unsigned nb = (unsigned)std::min<long long>((n + 255) / 256, 1ll << 20);
    { ProfScope ps(c, "tsdf_volume");
      k_tsdf_volume<<<nb, 256, 0, c->stream>>>(n, tsdf, weight, min_weight, vol, valid, n_valid ? c->count.get() : nullptr); }
    HIPCHK(hipGetLastError());
    return count_end(c, n_valid);
}

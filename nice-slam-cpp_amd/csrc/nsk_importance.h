// nsk_importance.h -- hierarchical importance sampling (upstream NICE-SLAM's sample_pdf behind rendering.N_importance): the depths of a second
// pass drawn from the compositing weights of a first one.  Included by nsk.hip behind nsk_device.h; the rule is stated in include/nsk.h.
#pragma once

// K1b: per-ray resampling.  One wave per ray, lane = sample slot, NSK_SAMPLE_RAYS rays per workgroup, as k_sample.
// z1 [N][S1] sorted first-pass depths, w [N][S1] their compositing weights -> P.z_out [N][S2], S2 = P.S = S1 + Ni, rank-sorted by k_sample's rule.
// Every operation of the rule is an fp32 operation of its own (the *_rn helpers: no contraction), and the two sums run left to right: each lane
// walks its own prefix from LDS (at most 62 dependent adds), so that the bits are those of the sequential statement (tests/importance_checks.py).
// With P.skey / P.L.out set the kernel goes on as k_sample does behind its z store (sample_keys): the second pass is cell-sortable and skips
// dead tiles like any batch.  P.rays_o / P.rays_d are read only then.
struct ResampArgs { SampArgs P; const float* z1; const float* w; int S1, Ni, det; };

__global__ __launch_bounds__(64 * NSK_SAMPLE_RAYS) void k_resample(ResampArgs A)
{
    const SampArgs& P = A.P;
    const int N = P.N, S2 = P.S, S1 = A.S1, Ni = A.Ni;
    __shared__ float sa[NSK_SAMPLE_RAYS][64];      // z, then the concatenation [z, zs]
    __shared__ float sb[NSK_SAMPLE_RAYS][64];      // w, then the rank keys (a NaN as +inf)
    __shared__ float sbin[NSK_SAMPLE_RAYS][64];    // bins, then the sorted depths
    __shared__ float spdf[NSK_SAMPLE_RAYS][64];    // q, then pdf
    __shared__ float scdf[NSK_SAMPLE_RAYS][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * NSK_SAMPLE_RAYS + wave;
    const bool active = n < N;                      // whole waves; inactive ones repeat the last ray and store nothing
    const int nc = active ? n : N - 1;
    const float zin = lane < S1 ? A.z1[(size_t)nc * S1 + lane] : 0.f;
    const float win = lane < S1 ? A.w[(size_t)nc * S1 + lane] : 0.f;
    float* za = sa[wave]; float* wb = sb[wave]; float* bins = sbin[wave]; float* pdf = spdf[wave]; float* cdf = scdf[wave];
    za[lane] = zin; wb[lane] = win;
    lds_fence();
    if (lane < S1 - 1) bins[lane] = mul_rn(0.5f, add_rn(za[lane + 1], za[lane]));       // 1
    if (lane < S1 - 2) pdf[lane] = add_rn(wb[lane + 1], 1e-5f);                         // 2: q
    lds_fence();
    float total = pdf[0];                                                               // 3
    for (int k = 1; k < S1 - 2; ++k) total = add_rn(total, pdf[k]);
    const float p = lane < S1 - 2 ? div_rn(pdf[lane], total) : 0.f;                     // 4
    lds_fence();                                    // (every lane has read q before any lane overwrites it)
    pdf[lane] = p;
    lds_fence();
    float c = 0.f;                                                                      // 5: cdf[lane] = pdf[0] + .. + pdf[lane - 1]
    for (int k = 0; k < S1 - 2; ++k) { const float v = pdf[k]; if (k < lane) c = add_rn(c, v); }
    if (lane < S1 - 1) cdf[lane] = c;
    lds_fence();
    if (lane < Ni) {
        const float u = A.det ? linspace01(lane, Ni)                                    // 6
                              : (float)(hash_u32(P.R.seed, (uint32_t)nc, (uint32_t)(64 + lane)) >> 8) * (1.0f / 16777216.0f);
        int inds = 0;                                                                   // 7
        for (int k = 0; k < S1 - 1; ++k) inds += cdf[k] <= u ? 1 : 0;
        const int below = max(inds - 1, 0), above = min(inds, S1 - 2);                  // 8
        const float cb = cdf[below];
        float denom = sub_rn(cdf[above], cb);                                           // 9
        if (denom < 1e-5f) denom = 1.f;
        const float t = div_rn(sub_rn(u, cb), denom);                                   // 10
        const float bb = bins[below];
        za[S1 + lane] = add_rn(bb, mul_rn(t, sub_rn(bins[above], bb)));                 // 11: zs, behind z
    }
    lds_fence();
    // 12: the rank sort of k_sample over the concatenation
    const float zc = lane < S2 ? za[lane] : NSK_INF;
    const float zr = zc != zc ? NSK_INF : zc;
    wb[lane] = zr;
    lds_fence();
    int rank = 0;
    for (int k = 0; k < S2; ++k) {
        const float zk = wb[k];
        rank += (zk < zr || (zk == zr && k < lane)) ? 1 : 0;
    }
    if (lane < S2) bins[rank] = zc;
    lds_fence();
    const float z = lane < S2 ? bins[lane] : NSK_INF;
    if (active && lane < S2) P.z_out[(size_t)n * S2 + lane] = z;
    if (!P.skey && !P.L.out) return;                                                    // uniform over the launch
    const float ox = P.rays_o[3 * nc], oy = P.rays_o[3 * nc + 1], oz = P.rays_o[3 * nc + 2];
    const float dx = P.rays_d[3 * nc], dy = P.rays_d[3 * nc + 1], dz = P.rays_d[3 * nc + 2];
    sample_keys(P, blockIdx.x, n, active, lane, z, ox, oy, oz, dx, dy, dz);
}

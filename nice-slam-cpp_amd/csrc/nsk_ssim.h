// nsk_ssim.h -- structural similarity of two images on the device (Wang et al. 2004; include/nsk.h states the rule): the windowed means,
// variances and covariance of a tile through LDS, the 2 x 2 average that builds the MS-SSIM pyramid, and the partial rows of the sums.
//
// Everything after the one widening of a pixel is fp64 and every multiply and add an operation of its own (dmul below keeps a product
// out of an FMA): E[x^2] - mu^2 cancels against C2 = 9e-4, in fp32 a flat bright frame is wrong by 6e-4 in single map values.
//
// The tile: SSIM_TILE_H x SSIM_TILE_W = 8 x 32 windows per 256-thread workgroup and channel.  A 32-lane half of a wave is then one row
// of 32 consecutive doubles in both filter passes, whatever the window: ds_read_b64 banks by (address / 4) mod 64 within a 32-lane half,
// and 32 consecutive doubles are the 64 banks once each.  LDS: the two images' tiles with their halo, (8 + 14) x (32 + 14)
// doubles each, the five row-filtered quantities, (8 + 14) x 32 doubles each, the weights: 16192 + 28160 + 120 = 44472 bytes, static, sized
// for win = 15; three workgroups share a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_reduce.h"
#include "nsk_ssim_plan.h"

#define SSIM_TILE_H 8
#define SSIM_TILE_W 32
#define SSIM_IN_H (SSIM_TILE_H + SSIM_MAX_WIN - 1)
#define SSIM_IN_W (SSIM_TILE_W + SSIM_MAX_WIN - 1)

__device__ __forceinline__ double dmul(double a, double b) { double r = a * b; asm("" : "+v"(r)); return r; }      // mul_rn of nsk_device.h, in double
__device__ __forceinline__ bool finite_f64(double x) { return fabs(x) < __builtin_inf(); }                        // false for NaN and +-inf

struct SsimArgs {
    int H, W, C;                    // the level's image [H][W][C]
    int win, Hm, Wm;                // the window, the map [Hm][Wm] = [H - win + 1][W - win + 1]
    int tiles_x;                    // tiles per row of tiles (blockIdx.x = tile, blockIdx.y = channel)
    double C1, C2;
    double g[SSIM_MAX_WIN];         // the window's weights (host, double)
};

// T: float (level 0, widened on load) or double (a pooled level).  terms [Hm Wm][C][2] = (ssim, cs) of every window; map [Hm][Wm][C] (or
// NULL) = the float32 rounding of ssim.  Lanes outside the map neither read nor write: the loads walk the tile's part of the image only, and
// no LDS word is read that was not written.
template <class T>
__global__ __launch_bounds__(256) void k_ssim_tile(SsimArgs A, const T* __restrict__ a, const T* __restrict__ b, double* __restrict__ terms,
                                                   float* __restrict__ map)
{
    __shared__ double sx[SSIM_IN_H * SSIM_IN_W], sy[SSIM_IN_H * SSIM_IN_W];
    __shared__ double rf[5][SSIM_IN_H * SSIM_TILE_W];
    __shared__ double g[SSIM_MAX_WIN];
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
    const int i0 = ty * SSIM_TILE_H, j0 = tx * SSIM_TILE_W;
    const int out_h = min(SSIM_TILE_H, A.Hm - i0), out_w = min(SSIM_TILE_W, A.Wm - j0);        // >= 1: the grid covers the map only
    const int in_h = out_h + A.win - 1, in_w = out_w + A.win - 1;                              // i0 + in_h <= H, j0 + in_w <= W
    if (tid < A.win) g[tid] = A.g[tid];
    for (int p = tid; p < in_h * in_w; p += 256) {
        const int r = p / in_w, c = p - r * in_w;
        const size_t at = ((size_t)(i0 + r) * A.W + (j0 + c)) * A.C + ch;
        sx[r * SSIM_IN_W + c] = (double)a[at];
        sy[r * SSIM_IN_W + c] = (double)b[at];
    }
    __syncthreads();
    // along W: taps in increasing index order, acc = g_0 v_0, then acc = acc + g_k v_k; the products x x, y y, x y are formed per pixel
    for (int p = tid; p < in_h * SSIM_TILE_W; p += 256) {
        const int r = p >> 5, j = p & 31;
        if (j >= out_w) continue;
        const double* px = sx + r * SSIM_IN_W + j;
        const double* py = sy + r * SSIM_IN_W + j;
        double acc[5];
        for (int k = 0; k < A.win; ++k) {
            const double x = px[k], y = py[k], w = g[k];
            const double v[5] = {x, y, dmul(x, x), dmul(y, y), dmul(x, y)};
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[q] = k == 0 ? dmul(w, v[q]) : acc[q] + dmul(w, v[q]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) rf[q][p] = acc[q];
    }
    __syncthreads();
    // along H, then the window's values
    const int i = tid >> 5, j = tid & 31;
    if (i >= out_h || j >= out_w) return;
    double f[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double* col = rf[q] + i * SSIM_TILE_W + j;
        double acc = dmul(g[0], col[0]);
        for (int k = 1; k < A.win; ++k) acc = acc + dmul(g[k], col[k * SSIM_TILE_W]);
        f[q] = acc;
    }
    const double mx = f[0], my = f[1];
    const double mxx = dmul(mx, mx), myy = dmul(my, my), mxy = dmul(mx, my);
    const double vx = f[2] - mxx, vy = f[3] - myy, vxy = f[4] - mxy;
    const double cs = (dmul(2.0, vxy) + A.C2) / ((vx + vy) + A.C2);
    const double ssim = dmul((dmul(2.0, mxy) + A.C1) / ((mxx + myy) + A.C1), cs);
    const size_t at = ((size_t)(i0 + i) * A.Wm + (j0 + j)) * A.C + ch;
    terms[2 * at] = ssim;
    terms[2 * at + 1] = cs;
    if (map) map[at] = (float)ssim;
}

// Level l + 1 of both images from level l ([H][W][C] -> [H2][W2][C] doubles): the 2 x 2 average with p = size mod 2 of zero padding on an
// axis, ((v00 + v01) + (v10 + v11)) 0.25 -- F.avg_pool2d(kernel_size = 2, padding = size % 2) bit for bit.  blockIdx.y: 0 image a, 1 image b.
template <class T>
__global__ __launch_bounds__(256) void k_ssim_pool(int H, int W, int C, int H2, int W2, const T* __restrict__ a, const T* __restrict__ b,
                                                   double* __restrict__ a2, double* __restrict__ b2)
{
    const size_t n = (size_t)H2 * W2 * C, e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const T* __restrict__ src = blockIdx.y ? b : a;
    double* __restrict__ dst = blockIdx.y ? b2 : a2;
    const int c = (int)(e % C);
    const size_t px = e / C;
    const int i = (int)(px / W2), j = (int)(px - (size_t)i * W2);
    const int r0 = 2 * i - H % 2, c0 = 2 * j - W % 2;
    auto at = [&](int r, int q) -> double { return r >= 0 && r < H && q >= 0 && q < W ? (double)src[((size_t)r * W + q) * C + c] : 0.0; };
    dst[e] = dmul((at(r0, c0) + at(r0, c0 + 1)) + (at(r0 + 1, c0) + at(r0 + 1, c0 + 1)), 0.25);
}

// The partial rows of a level's sums (nsk_reduce.h): the element is the window i Wm + j, the columns 3 c + {0 the sum of ssim, 1 the sum of
// cs, 2 the windows counted}; a window whose ssim or cs is not finite is left out of the channel's three columns.
template <int C>
__global__ __launch_bounds__(256) void k_ssim_sums(int n, const double* __restrict__ terms, double* __restrict__ rows)
{
    double acc[3 * C];
#pragma unroll
    for (int k = 0; k < 3 * C; ++k) acc[k] = 0.0;
    for (unsigned p = blockIdx.x * 256 + threadIdx.x; p < (unsigned)n; p += gridDim.x * 256) {      // (n <= 2^30: no wrap)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double s = terms[2 * ((size_t)p * C + c)], q = terms[2 * ((size_t)p * C + c) + 1];
            if (finite_f64(s) && finite_f64(q)) { acc[3 * c] += s; acc[3 * c + 1] += q; acc[3 * c + 2] += 1.0; }
        }
    }
    rows_store<RowSums<3 * C>>(acc, rows + (size_t)blockIdx.x * 3 * C);
}

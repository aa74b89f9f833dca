// nsk_image.h -- whole-frame rendering: the rays of a view (pose + intrinsics + image window, no pixel-index arrays) and the residual
// metrics of a rendered frame against the input frame (depth L1, the squared colour error behind PSNR).
// (Upstream NICE-SLAM: Renderer.render_img and the visualiser's residual panels; include/nsk.h states the contract.)
//
// A view is the pixel set i = W0 + stride * col, j = H0 + stride * row with col < Wv = ceil((W1 - W0) / stride), row < Hv = ceil((H1 - H0) /
// stride); view pixel n = row * Wv + col (row-major: upstream's get_rays(...).reshape(-1, 3) order).  i is the column, j the row.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_reduce.h"

// defined in nsk.hip (quad2rotation / get_camera_from_tensor); the same body serves k_rays_from_camera and k_prepare_rays
__device__ __forceinline__ void camera_matrix(const float* cam, float* c2w);

struct ImgView {
    int H0, W0, stride, Wv;         // the window's first row / column, the pixel step, view pixels per row
    int W;                          // row length of the depth image
    int first, n;                   // the view pixels [first, first + n) this launch writes
    int mode;                       // bit 0: D11 as written (see k_rays_from_pixels); the D10 truncation is applied to the intrinsics by the host
    float fx, fy, cx, cy;
};

// Rays and gathered ground-truth depth of view pixels [first, first + n): the arithmetic of k_rays_from_pixels / k_rays_from_camera and
// the read of k_gather_pixels on the pixel the thread derives from its own index, so the results carry the same bits.  One thread per
// pixel, consecutive threads = consecutive columns (the depth image is read along its rows; ro / rd / gd are written densely).  The pose
// matrix is formed once per workgroup (thread 0, 12 floats through LDS) instead of once per thread.
__global__ __launch_bounds__(256) void k_image_rays(ImgView V, const float* __restrict__ pose, int cam7, const float* __restrict__ depth_img,
                                                    float* __restrict__ ro, float* __restrict__ rd, float* __restrict__ gd)
{
    __shared__ float m[12];
    if (threadIdx.x == 0) {
        float c2w[12];
        if (cam7) camera_matrix(pose, c2w);
        else for (int k = 0; k < 12; ++k) c2w[k] = pose[k];
        for (int k = 0; k < 12; ++k) m[k] = c2w[k];
    }
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= V.n) return;
    const int p = V.first + r;
    const int row = p / V.Wv, col = p - row * V.Wv;
    const int pi = V.W0 + V.stride * col, pj = V.H0 + V.stride * row;
    if (gd) gd[r] = depth_img[(size_t)pj * V.W + pi];
    const float i = (float)pi, j = (float)pj;
    const float d0 = div_rn(sub_rn(i, V.cx), V.fx);
    const float d1 = (V.mode & 1) ? div_rn(sub_rn(i, V.cy), V.fy) : -div_rn(sub_rn(j, V.cy), V.fy);
    const float d2 = -1.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        rd[3 * (size_t)r + a] = add_rn(add_rn(mul_rn(d0, m[4 * a]), mul_rn(d1, m[4 * a + 1])), mul_rn(d2, m[4 * a + 2]));
        ro[3 * (size_t)r + a] = m[4 * a + 3];
    }
}

// ---- metrics ---------------------------------------------------------------------------------------------------------------------
// Per workgroup one row of IMG_COLS doubles: [0] pixels that take part in the depth sum, [1] their sum |gt - d|, [2] colour components
// that take part, [3] their sum (gt_c - c)^2, [4] pixels with a non-finite rendered value.  The association is that of nsk_reduce.h.
#define IMG_COLS 5
#define IMG_MAX_ROWS 1024

__global__ __launch_bounds__(256) void k_image_metrics(int n, const float* __restrict__ rgb, const float* __restrict__ depth,
                                                       const float* __restrict__ gt_d, const float* __restrict__ gt_c,
                                                       float* __restrict__ res_d, float* __restrict__ res_c, double* __restrict__ rows)
{
    double acc[IMG_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned p = blockIdx.x * 256 + threadIdx.x; p < (unsigned)n; p += gridDim.x * 256) {      // (n <= 2^30: no wrap)
        const float d = depth[p];
        const float c0 = rgb[3 * (size_t)p], c1 = rgb[3 * (size_t)p + 1], c2 = rgb[3 * (size_t)p + 2];
        const bool good = finite_f32(d) && finite_f32(c0) && finite_f32(c1) && finite_f32(c2);
        if (!good) acc[4] += 1.0;
        if (gt_d) {
            const float g = gt_d[p];
            const float r = g > 0.f ? fabsf(sub_rn(g, d)) : 0.f;          // the visualiser's rule: no measurement, no residual
            if (res_d) res_d[p] = r;
            if (good && g > 0.f && finite_f32(r)) { acc[0] += 1.0; acc[1] += (double)r; }
        }
        if (gt_c) {
            const float c[3] = {c0, c1, c2};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float r = fabsf(sub_rn(gt_c[3 * (size_t)p + a], c[a]));
                if (res_c) res_c[3 * (size_t)p + a] = r;
                if (good && finite_f32(r)) { acc[2] += 1.0; acc[3] += (double)r * (double)r; }
            }
        }
    }
    rows_store<RowSums<IMG_COLS>>(acc, rows + (size_t)blockIdx.x * IMG_COLS);
}

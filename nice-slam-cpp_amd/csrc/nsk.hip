// nsk.hip -- C-ABI (include/nsk.h) of the MI355X-native NICE-SLAM hot path: context, data layouts, launches.
// Built only for gfx950:  hipcc --offload-arch=gfx950 -O3 -shared -fPIC nsk.hip -o libnsk.so
#include "../../include/nsk.h"
#include "nsk_device.h"
#include "nsk_importance.h"
#include "nsk_train.h"
#include "nsk_bf16.h"
#include "nsk_mesh.h"
#include "nsk_image.h"
#include "nsk_ssim.h"
#include "nsk_cloud.h"
#include "nsk_surface.h"
#include "nsk_icp.h"
#include "nsk_rigid.h"
#include "nsk_raster.h"
#include "nsk_reduce.h"
#include "nsk_buf.h"
#include "nsk_split.h"
#include "nsk_images.h"
#include "nsk_hull_plan.h"

#include <dlfcn.h>
#include <cstdarg>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define NSK_VERSION 101

static thread_local std::string g_err;
static int fail(const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_err = buf;
    return -1;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define CHK(x) do { int r_ = (x); if (r_ != 0) return r_; } while (0)

// ---------------------------------------------------------------------------------------------------------
// small kernels that only the host file needs
// ---------------------------------------------------------------------------------------------------------
__global__ void k_pack(float* __restrict__ img, const int* __restrict__ idx, const float* __restrict__ P, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { int k = idx[i]; img[i] = k >= 0 ? P[k] : 0.f; }
}

struct AdamSeg { float* p; float* g; float* m; float* v; const int* idx; int nidx; int n; float step_size, bc2s; int blk_end;      // idx: the marked voxels (nullptr = all)
                 const int* inv_f; const int* inv_b; float* fimg; float* bimg;      // decoders: image position of each parameter (-1 none)
                 const int* inv16; unsigned short* img16; float* img16_tail; int tail_off; int np16;      // forward image in np16 pieces (MlpFwdImgB), its fp32 tail
                 const int* invh; unsigned short* imgh; float* imgh_tail; int btail_off;      // fp16 backward image (MlpBwdImgH) and its fp32 tail
                 const float* slabs; int nslabs, slab_stride; };                      // pending per-workgroup gradient slabs (k_decode_bwd_multi)
struct AdamArgs { AdamSeg s[8]; int n; float b1, b2, eps;
                  PlaceArgs place; int adam_blocks; };       // optional (place.nblocks > 0): the NEXT batch's cell-sort placement rides behind the segments (nsk_map_prepare)
// all parameter groups of one optimiser step in one launch (3 grid levels + trainable decoders)
__global__ void k_adam_multi(AdamArgs A)
{
    if (A.place.nblocks > 0 && (int)blockIdx.x >= A.adam_blocks) { sort_place_body(A.place, (int)blockIdx.x - A.adam_blocks); return; }
    int r = 0;
    while (r < A.n - 1 && (int)blockIdx.x >= A.s[r].blk_end) ++r;
    const AdamSeg& S = A.s[r];
    const int b0 = r == 0 ? 0 : A.s[r - 1].blk_end;
    int i = (blockIdx.x - b0) * blockDim.x + threadIdx.x;
    f4 extra = (f4)(0.f);
    // a trainable decoder's parameters are walked 8 float4 per block; the thread that will update float4 `i` fetches everything that does not
    // depend on the gradient -- moments, parameter, the image positions of its four parameters -- TOGETHER with the slab loads below: the launch was
    // three dependent round trips (slabs -> moments / parameter -> index tables -> image stores), and its time is latency, not traffic
    f4 pre_m = (f4)(0.f), pre_v = (f4)(0.f), pre_p = (f4)(0.f);
    int pf[4] = {-1, -1, -1, -1}, pb[4] = {-1, -1, -1, -1}, p16[4] = {-1, -1, -1, -1}, ph[4] = {-1, -1, -1, -1};
    bool pre = false;
    if (S.slabs) {      // decoder whose gradient still sits in per-workgroup slabs: 8 float4 per block, 32 thread groups sum 1/32 of the slabs each
        // (all of a thread's ~6 slab reads are in flight at once: this sum, not the grids' Adam traffic, was most of the launch's time --
        // 18 us with 8 groups reading ~24 slabs one after the other, 14 us with four reads in flight, see profiles/)
        __shared__ f4 red[32][8];
        const int pi = threadIdx.x & 7, sg = threadIdx.x >> 3;
        i = (blockIdx.x - b0) * 8 + pi;
        f4 part = (f4)(0.f);
        if (4 * i < S.n) {
            if (sg == 0) {
                pre = true;
                pre_m = reinterpret_cast<const f4*>(S.m)[i]; pre_v = reinterpret_cast<const f4*>(S.v)[i]; pre_p = reinterpret_cast<const f4*>(S.p)[i];
                if (S.inv_f) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        pf[k] = S.inv_f[4 * i + k]; pb[k] = S.inv_b[4 * i + k];
                        if (S.inv16) p16[k] = S.inv16[4 * i + k];
                        if (S.invh) ph[k] = S.invh[4 * i + k];
                    }
                }
            }
            const float* base = S.slabs + 4 * i;
#pragma unroll 8
            for (int sl = sg; sl < S.nslabs; sl += 32) part += *reinterpret_cast<const f4*>(base + (size_t)sl * S.slab_stride);
        }
        red[sg][pi] = part;
        __syncthreads();
        if (sg != 0) return;
#pragma unroll
        for (int k = 0; k < 32; ++k) extra += red[k][pi];
    }
    if (S.idx) {                  // a masked level: the launch covers the marked voxels only (8 float4 each); unmarked ones are never touched
        if (i >= S.nidx * 8) return;
        i = S.idx[i >> 3] * 8 + (i & 7);
    }
    if (4 * i >= S.n) return;
    f4* g4 = reinterpret_cast<f4*>(S.g) + i;
    const f4 g0 = *g4;
    f4 gg = g0 + extra, mm = pre ? pre_m : reinterpret_cast<f4*>(S.m)[i], vv = pre ? pre_v : reinterpret_cast<f4*>(S.v)[i];
    // a parameter that never received a gradient (g = m = v = 0) does not move under Adam: skip its five memory operations
    if (!S.inv_f && gg[0] == 0.f && gg[1] == 0.f && gg[2] == 0.f && gg[3] == 0.f && mm[0] == 0.f && mm[1] == 0.f && mm[2] == 0.f && mm[3] == 0.f &&
        vv[0] == 0.f && vv[1] == 0.f && vv[2] == 0.f && vv[3] == 0.f) return;
    f4 pp = pre ? pre_p : reinterpret_cast<f4*>(S.p)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mm[k] = A.b1 * mm[k] + (1.f - A.b1) * gg[k];
        vv[k] = A.b2 * vv[k] + (1.f - A.b2) * gg[k] * gg[k];
        float denom = sqrtf(vv[k]) / S.bc2s + A.eps;
        pp[k] -= S.step_size * (mm[k] / denom);
    }
    reinterpret_cast<f4*>(S.p)[i] = pp; reinterpret_cast<f4*>(S.m)[i] = mm; reinterpret_cast<f4*>(S.v)[i] = vv;
    if (g0[0] != 0.f || g0[1] != 0.f || g0[2] != 0.f || g0[3] != 0.f) *g4 = (f4)(0.f);
    if (S.inv_f) {      // keep the MFMA fragment images of a trainable decoder in step with its parameters
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int fi = pre ? pf[k] : S.inv_f[4 * i + k], bi = pre ? pb[k] : S.inv_b[4 * i + k];
            if (fi >= 0) S.fimg[fi] = pp[k];
            if (bi >= 0) S.bimg[bi] = pp[k];
            if (S.inv16) {
                const int t = pre ? p16[k] : S.inv16[4 * i + k];
                if (t >= 0) store_pieces(S.img16, t, pp[k], S.np16);
                if (fi >= S.tail_off) S.img16_tail[fi - S.tail_off] = pp[k];
            }
            if (S.invh) {
                const int t = pre ? ph[k] : S.invh[4 * i + k];
                if (t >= 0) store_pieces(S.imgh, t, pp[k], 2);
                if (bi >= S.btail_off) S.imgh_tail[bi - S.btail_off] = pp[k];
            }
        }
    }
}

// Mask-compacted gradient exchange (multi-GPU): every rank holds the same optimiser mask, so only the marked voxels' gradients need to
// travel.  k_mask_index lists them in ascending order (one workgroup, deterministic: every rank must build the same list).
__global__ __launch_bounds__(1024) void k_mask_index(int nvox, const uint8_t* __restrict__ mask, int* __restrict__ idx, int* __restrict__ count)
{
    __shared__ int wsum[16];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int v0 = 0; v0 < nvox; v0 += 1024) {
        const int v = v0 + threadIdx.x;
        const bool on = v < nvox && mask[v];
        const unsigned long long b = __builtin_amdgcn_ballot_w64(on);
        if (lane == 0) wsum[wave] = __builtin_popcountll(b);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (on) idx[off + __builtin_popcountll(b & ((1ull << lane) - 1ull))] = v;
        __syncthreads();
        if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; base += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// Per-cell liveness of a masked level, once per mask: a cell (named by its lower corner voxel, as tri_setup's i0) is live when any of its eight
// corner voxels is marked.  The corners are tri_setup's: the neighbour along an axis clamped into the grid, so a cell on an upper face sees only
// the voxels a sample in it can reach.  The backward skips tiles of samples whose cells are all dead (decode_bwd_body<.., SKIP>).
__global__ __launch_bounds__(256) void k_cell_live(int X, int Y, int Z, const uint8_t* __restrict__ mask, uint8_t* __restrict__ live)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= X * Y * Z) return;
    const int ix = v % X, iy = (v / X) % Y, iz = v / (X * Y);
    unsigned on = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int jx = min(ix + (c & 1), X - 1), jy = min(iy + ((c >> 1) & 1), Y - 1), jz = min(iz + (c >> 2), Z - 1);
        on |= mask[(jz * Y + jy) * X + jx];
    }
    live[v] = on ? 1 : 0;
}

// the whole packed exchange buffer in ONE launch each way (it was one launch per level plus two copies: eleven small operations per
// step around the all-reduce): segments = grid levels (32 floats per listed voxel), trainable decoders and the loss scalars (plain runs)
struct XSeg { const int* idx; int n4; float* slab; float* buf; int blk_end;       // n4 = float4 count of the segment; idx != nullptr: voxel list, 8 float4 per voxel
              const float* slabs; int nslabs, slab_stride; };                     // gather only: a decoder whose gradient still sits in per-workgroup slabs
struct XArgs { XSeg s[10]; int n; int gather; };
__global__ __launch_bounds__(256) void k_xchg_multi(XArgs A)
{
    int r = 0;
    while (r < A.n - 1 && (int)blockIdx.x >= A.s[r].blk_end) ++r;
    const XSeg& S = A.s[r];
    const int b0 = r ? A.s[r - 1].blk_end : 0;
    if (S.slabs) {          // the pending decoder-gradient slabs are summed on the way into the buffer (the sum k_adam_multi does on one GPU):
        __shared__ f4 red[32][8];                 // 8 float4 per block, 32 thread groups sum 1/32 of the slabs each
        const int pi = threadIdx.x & 7, sg = threadIdx.x >> 3;
        const int i = (blockIdx.x - b0) * 8 + pi;
        f4 part = (f4)(0.f);
        if (i < S.n4) {
            const float* base = S.slabs + 4 * i;
#pragma unroll 8
            for (int sl = sg; sl < S.nslabs; sl += 32) part += *reinterpret_cast<const f4*>(base + (size_t)sl * S.slab_stride);
        }
        red[sg][pi] = part;
        __syncthreads();
        if (sg != 0 || i >= S.n4) return;
        f4 sum = reinterpret_cast<const f4*>(S.slab)[i];          // + what earlier calls accumulated
#pragma unroll
        for (int k = 0; k < 32; ++k) sum += red[k][pi];
        reinterpret_cast<f4*>(S.buf)[i] = sum;
        reinterpret_cast<f4*>(S.slab)[i] = sum;                 // the slab stays what nsk_grid/decoder gradient downloads and a second pack expect
        return;
    }
    const int t = (blockIdx.x - b0) * 256 + threadIdx.x;
    if (t >= S.n4) return;
    const size_t at = S.idx ? (size_t)S.idx[t >> 3] * 8 + (t & 7) : (size_t)t;
    f4* sl = reinterpret_cast<f4*>(S.slab) + at;
    f4* bf = reinterpret_cast<f4*>(S.buf) + t;
    if (A.gather) *bf = *sl; else *sl = *bf;
}

// Adam on one float: ONE body for k_adam_scalar, k_pose_step and k_pose_multi, which are asserted to agree bit for bit (tests/test_gpu_pose.py).
// Left to hipcc's default contraction the same three lines were compiled differently per kernel: rounded products and a sum for both moments in
// k_adam_scalar and k_pose_step, FMAs in k_pose_multi.  Here the moments are spelled as the first two had them (every product and the sum rounded on
// its own) and the one fused operation all three had, p - step_size * r, is written as the fmaf it was: their bits stay, k_pose_multi's follow.
__device__ __forceinline__ void adam_scalar_update(float gg, float& p, float& m, float& v, float step_size, float bc2s, float b1, float b2, float eps)
{
#pragma clang fp contract(off)
    const float mm = b1 * m + (1.f - b1) * gg;
    const float vv = b2 * v + (1.f - b2) * gg * gg;
    p = fmaf(-step_size, mm / (sqrtf(vv) / bc2s + eps), p);
    m = mm; v = vv;
}

__global__ void k_adam_scalar(int n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                              float* __restrict__ v, float step_size, float bc2s, float b1, float b2, float eps)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    adam_scalar_update(g[i], p[i], m[i], v[i], step_size, bc2s, b1, b2, eps);
}

__global__ void k_sum(int n, const float* __restrict__ x, float* __restrict__ out)
{
    __shared__ float sh[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += sh[w]; *out = s; }
}

// Mapper loss, reference src/Mapper.cpp:435-442
__global__ void k_loss_map(int N, const float* depth, const float* rgb, const float* gt_d, const float* gt_c, float w_color,
                           int use_color, float* g_depth, float* g_rgb, float* ray_loss)
{
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float l = 0.f, g = 0.f;
    if (gt_d[n] > 0.f) { float r = gt_d[n] - depth[n]; l += fabsf(r); g = -sgnf(r); }
    g_depth[n] = g;
    for (int k = 0; k < 3; ++k) {
        float r = gt_c[3 * n + k] - rgb[3 * n + k];
        if (use_color) { l += w_color * fabsf(r); g_rgb[3 * n + k] = -w_color * sgnf(r); }
        else g_rgb[3 * n + k] = 0.f;
    }
    ray_loss[n] = l;
}

// Tracker loss, reference src/Tracker.cpp:67-82
__global__ void k_loss_track(int N, const float* depth, const float* rgb, const float* var, const float* gt_d, const float* gt_c,
                             float w_color, int use_color, int handle_dynamic, int detach_var, const float* thr,
                             float* g_depth, float* g_rgb, float* g_var, float* ray_loss)
{
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float r = gt_d[n] - depth[n];
    bool mk = gt_d[n] > 0.f && (!handle_dynamic || fabsf(r) < *thr);
    float l = 0.f, gd = 0.f, gv = 0.f, gc[3] = {0.f, 0.f, 0.f};
    if (mk) {
        float u = sqrtf(var[n] + 1e-10f);
        l = fabsf(r) / u; gd = -sgnf(r) / u;
        if (!detach_var) gv = -fabsf(r) / (2.f * u * u * u);
        if (use_color) for (int k = 0; k < 3; ++k) { float rc = gt_c[3 * n + k] - rgb[3 * n + k]; l += w_color * fabsf(rc); gc[k] = -w_color * sgnf(rc); }
    }
    g_depth[n] = gd; if (g_var) g_var[n] = gv;
    for (int k = 0; k < 3; ++k) g_rgb[3 * n + k] = gc[k];
    ray_loss[n] = l;
}

// 10 * torch.median(|gt - depth|) (lower median) by a single-workgroup bitonic sort in LDS
__global__ __launch_bounds__(1024) void k_median_thr(int N, int P2, const float* gt_d, const float* depth, const uint8_t* keep, float* thr)
{
    extern __shared__ float shm[];
    __shared__ int nvalid;
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < P2; i += 1024) {
        const bool ok = i < N && (!keep || keep[i]);
        shm[i] = ok ? fabsf(gt_d[i] - depth[i]) : NSK_INF;       // masked rays sort to the end
        cnt += ok ? 1 : 0;
    }
    if (cnt) atomicAdd(&nvalid, cnt);
    __syncthreads();
    N = max(nvalid, 1);
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P2; i += 1024) {
                int ixj = i ^ j;
                if (ixj > i) {
                    float a = shm[i], b = shm[ixj];
                    bool up = (i & k) == 0;
                    if ((a > b) == up) { shm[i] = b; shm[ixj] = a; }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) *thr = 10.f * shm[(N - 1) / 2];
}

// raySampler direction part, reference include/torchlib/utils.h:44-52
__global__ void k_rays_from_pixels(int n, const int* pi, const int* pj, float fx, float fy, float cx, float cy, const float* c2w,
                                   int mode, float* ro, float* rd)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    float i = (float)pi[r], j = (float)pj[r];
    float d0 = div_rn(sub_rn(i, cx), fx);
    float d1 = (mode & 1) ? div_rn(sub_rn(i, cy), fy) : -div_rn(sub_rn(j, cy), fy);
    float d2 = -1.f;
    for (int a = 0; a < 3; ++a) {
        rd[3 * r + a] = add_rn(add_rn(mul_rn(d0, c2w[4 * a]), mul_rn(d1, c2w[4 * a + 1])), mul_rn(d2, c2w[4 * a + 2]));
        ro[3 * r + a] = c2w[4 * a + 3];
    }
}

// d loss / d c2w of the rays [r0, r0 + n) of a batch by one block of 256 threads: a partial per thread over r = r0 + t, r0 + t + 256, ..., the
// butterfly over a wave's 64 lanes, ((s0 + s1) + s2) + s3 over the four waves; threads 0..11 store the 12 sums to `out` (global or shared: the
// caller puts its own barrier behind it).  ONE body for k_rays_backward, k_pose_step and k_pose_multi, and no contraction in it: the three are
// asserted to agree bit for bit, and with hipcc's default (a * b + c fused per instantiation) they did not -- see camera_matrix below.
__device__ __forceinline__ void rays_backward_block(int r0, int n, const int* pi, const int* pj, float fx, float fy, float cx, float cy, int mode,
                                                    const float* g_ro, const float* g_rd, float (*sh)[12], float* out)
{
#pragma clang fp contract(off)
    float acc[12];
    for (int k = 0; k < 12; ++k) acc[k] = 0.f;
    for (int r = r0 + threadIdx.x; r < r0 + n; r += 256) {
        float i = (float)pi[r], j = (float)pj[r];
        float dir[3] = {(i - cx) / fx, (mode & 1) ? (i - cy) / fy : -(j - cy) / fy, -1.f};
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) acc[4 * a + b] += g_rd[3 * r + a] * dir[b];
            acc[4 * a + 3] += g_ro[3 * r + a];
        }
    }
    for (int k = 0; k < 12; ++k) { float s = wave_sum(acc[k]); if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = s; }
    __syncthreads();
    if (threadIdx.x < 12) out[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void k_rays_backward(int n, const int* pi, const int* pj, float fx, float fy, float cx, float cy,
                                                       int mode, const float* g_ro, const float* g_rd, float* g_c2w)
{
    __shared__ float sh[4][12];
    rays_backward_block(0, n, pi, pj, fx, fy, cx, cy, mode, g_ro, g_rd, sh, g_c2w);
}

// quad2rotation / get_camera_from_tensor, reference include/torchlib/utils.h:174-210
__device__ __forceinline__ void camera_matrix(const float* cam, float* c2w)
{
    // every product and sum rounded on its own, as the reference's tensor ops do.  The pragma matters: hipcc contracts a * b + c into an
    // FMA across statements by default (and HIP's __fmul_rn / __fadd_rn are plain operators), so without it the matrix depended on the
    // kernel this is inlined into -- k_rays_from_camera and k_prepare_rays differed in the last bit.
#pragma clang fp contract(off)
    const float qr = cam[0], qi = cam[1], qj = cam[2], qk = cam[3];
    const float rr = qr * qr, ii = qi * qi, jj = qj * qj, kk = qk * qk;
    const float ssum = ((rr + ii) + jj) + kk;
    const float two_s = 2.f / ssum;
    const float ij = qi * qj, ik = qi * qk, jk = qj * qk, ir = qi * qr, jr = qj * qr, kr = qk * qr;
    const float s0 = jj + kk, s1 = ii + kk, s2 = ii + jj;
    const float a01 = ij - kr, a02 = ik + jr, a10 = ij + kr, a12 = jk - ir, a20 = ik - jr, a21 = jk + ir;
    const float t0 = two_s * s0, t1 = two_s * s1, t2 = two_s * s2;
    float R[9] = {1.f - t0, two_s * a01, two_s * a02, two_s * a10, 1.f - t1, two_s * a12, two_s * a20, two_s * a21, 1.f - t2};
    for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) c2w[4 * a + b] = R[3 * a + b]; c2w[4 * a + 3] = cam[4 + a]; }
}
__global__ void k_camera_from_tensor(const float* cam, float* c2w) { camera_matrix(cam, c2w); }

__device__ __forceinline__ void camera_matrix_backward(const float* cam, const float* g_c2w, float* g_cam)
{
    // no contraction, for camera_matrix's reason: inlined into k_camera_backward, k_pose_step and k_pose_multi, which must give the same bits --
    // with the default the rotation gradients of the fused kernels differed from k_camera_backward's in the last bits (tests/test_gpu_pose.py)
#pragma clang fp contract(off)
    float q[4] = {cam[0], cam[1], cam[2], cam[3]};
    float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    float two_s = 2.f / n2;
    float qr = q[0], qi = q[1], qj = q[2], qk = q[3];
    float M[9] = {-(qj * qj + qk * qk), qi * qj - qk * qr, qi * qk + qj * qr, qi * qj + qk * qr, -(qi * qi + qk * qk),
                  qj * qk - qi * qr, qi * qk - qj * qr, qj * qk + qi * qr, -(qi * qi + qj * qj)};
    float dM[9][4] = {{0, 0, -2 * qj, -2 * qk}, {-qk, qj, qi, -qr}, {qj, qk, qr, qi}, {qk, qj, qi, qr}, {0, -2 * qi, 0, -2 * qk},
                      {-qi, -qr, qk, qj}, {-qj, qk, -qr, qi}, {qi, qr, qk, qj}, {0, -2 * qi, -2 * qj, 0}};
    for (int c = 0; c < 4; ++c) {
        float dts = -2.f * two_s * q[c] / n2;
        float s = 0.f;
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) s += g_c2w[4 * a + b] * (dts * M[3 * a + b] + two_s * dM[3 * a + b][c]);
        g_cam[c] = s;
    }
    for (int a = 0; a < 3; ++a) g_cam[4 + a] = g_c2w[4 * a + 3];
}
__global__ void k_camera_backward(const float* cam, const float* g_c2w, float* g_cam) { camera_matrix_backward(cam, g_c2w, g_cam); }

// Fused forms for a device-resident Tracker iteration (each removes launches of ~6 us from a ~70 us, launch-bound iteration):
// pose 7-vector -> c2w -> rays in one kernel; ray gradients -> d c2w -> d pose -> Adam on the pose in one single-block kernel.
__global__ void k_rays_from_camera(int n, const int* pi, const int* pj, float fx, float fy, float cx, float cy, const float* cam, int mode,
                                   float* ro, float* rd, float* c2w_out)
{
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    float c2w[12];
    camera_matrix(cam, c2w);
    if (r == 0 && c2w_out) for (int k = 0; k < 12; ++k) c2w_out[k] = c2w[k];
    if (r >= n) return;
    float i = (float)pi[r], j = (float)pj[r];
    float d0 = div_rn(sub_rn(i, cx), fx);
    float d1 = (mode & 1) ? div_rn(sub_rn(i, cy), fy) : -div_rn(sub_rn(j, cy), fy);
    float d2 = -1.f;
    for (int a = 0; a < 3; ++a) {
        rd[3 * r + a] = add_rn(add_rn(mul_rn(d0, c2w[4 * a]), mul_rn(d1, c2w[4 * a + 1])), mul_rn(d2, c2w[4 * a + 2]));
        ro[3 * r + a] = c2w[4 * a + 3];
    }
}
__global__ __launch_bounds__(256) void k_pose_step(int n, const int* pi, const int* pj, float fx, float fy, float cx, float cy, int mode,
                                                   const float* g_ro, const float* g_rd, float* cam, float* m, float* v, float step_size,
                                                   float bc2s, float b1, float b2, float eps, float* g_cam_out)
{
    __shared__ float sh[4][12];
    __shared__ float g_c2w[12];
    rays_backward_block(0, n, pi, pj, fx, fy, cx, cy, mode, g_ro, g_rd, sh, g_c2w);
    __syncthreads();
    if (threadIdx.x == 0) {
        float g[7];
        camera_matrix_backward(cam, g_c2w, g);
        for (int k = 0; k < 7; ++k) {              // k_adam_scalar's update
            adam_scalar_update(g[k], cam[k], m[k], v[k], step_size, bc2s, b1, b2, eps);
            if (g_cam_out) g_cam_out[k] = g[k];
        }
    }
}

// The pose kernels of a whole window in ONE launch (bundle adjustment, reference src/Mapper.cpp:305-329,467-489): block f reduces the ray
// gradients of frame f's rays [first, first + count) of the batch to d loss / d c2w, chains through quad2rotation to the 7-vector
// and either steps the pose (adam = 1: k_pose_step's arithmetic, frame by frame) or only stores the gradient (adam = 0: N > 1, the
// gradients of all frames are summed over the ranks first, then nsk_adam_vector steps every pose at once).  Inactive frames (not optimised,
// or no ray of theirs in this shard) get a zero gradient.  One more block counts the shard's kept rays into g_out[8 * nframes + 1].
struct PoseFrames { int first[NSK_MAX_POSE_FRAMES], count[NSK_MAX_POSE_FRAMES]; unsigned char active[NSK_MAX_POSE_FRAMES]; };
__global__ __launch_bounds__(256) void k_pose_multi(PoseFrames F, int nframes, const int* pi, const int* pj, float fx, float fy, float cx, float cy, int mode,
                                                    const float* g_ro, const float* g_rd, float* cams, float* ms, float* vs, float step_size, float bc2s,
                                                    float b1, float b2, float eps, int adam, float* g_out, const uint8_t* keep, int n_keep)
{
    __shared__ float sh[4][12];
    __shared__ float g_c2w[12];
    const int f = blockIdx.x;
    if (f == nframes) {                                  // the count of the rays that take part (keep == nullptr: all of them)
        float cnt = 0.f;
        for (int r = threadIdx.x; r < n_keep; r += 256) cnt += (!keep || keep[r]) ? 1.f : 0.f;
        cnt = wave_sum(cnt);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][0] = cnt;
        __syncthreads();
        if (threadIdx.x == 0 && g_out) g_out[8 * nframes + 1] = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
        return;
    }
    const int n = F.active[f] ? F.count[f] : 0, r0 = F.first[f];
    rays_backward_block(r0, n, pi, pj, fx, fy, cx, cy, mode, g_ro, g_rd, sh, g_c2w);
    __syncthreads();
    if (threadIdx.x == 0) {
        float* cam = cams + 8 * f;
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (n > 0) camera_matrix_backward(cam, g_c2w, g);
        if (g_out) for (int k = 0; k < 8; ++k) g_out[8 * f + k] = g[k];
        if (adam && F.active[f]) {
            float* m = ms + 8 * f; float* v = vs + 8 * f;
            for (int k = 0; k < 7; ++k) adam_scalar_update(g[k], cam[k], m[k], v[k], step_size, bc2s, b1, b2, eps);      // k_adam_scalar's update
        }
    }
}

__global__ void k_inside_filter(RParams R, int N, const float* ro, const float* rd, const float* gt, uint8_t* keep)
{
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    keep[n] = ray_inside(R.bound, ro[3 * n], ro[3 * n + 1], ro[3 * n + 2], rd[3 * n], rd[3 * n + 1], rd[3 * n + 2], gt[n]);
}

// the whole ray preparation of an iteration in one launch (nsk_prepare_rays): the bodies of k_sample_pixels, k_gather_pixels,
// k_rays_from_pixels / k_rays_from_camera and k_inside_filter, one thread per ray, frames from a table in the kernel arguments
struct PrepFrame { const float* depth; const float* color; const float* pose; int cam7; unsigned long long seed; };
struct PrepArgs {
    PrepFrame f[16];
    int nframes, per, H0, W0, Ww, W, mode;
    unsigned long long total;
    float fx, fy, cx, cy;
    int* pi; int* pj; float* gd; float* gc; float* ro; float* rd; uint8_t* keep;
    RParams R;
};
__global__ __launch_bounds__(256) void k_prepare_rays(PrepArgs A)
{
    const int fi = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;      // one frame per block row: the table index is wave-uniform
    if (r >= A.per) return;
    const int t = fi * A.per + r;
    const PrepFrame& F = A.f[fi];
    const unsigned long long ind = ((unsigned long long)hash_u32(F.seed, (uint32_t)r, 0x51u) * A.total) >> 32;      // k_sample_pixels
    const int pi = A.W0 + (int)(ind % (unsigned long long)A.Ww), pj = A.H0 + (int)(ind / (unsigned long long)A.Ww);
    A.pi[t] = pi; A.pj[t] = pj;
    const size_t p = (size_t)pj * A.W + pi;                                                                         // k_gather_pixels
    const float gd = F.depth[p];
    A.gd[t] = gd;
    if (F.color && A.gc) { A.gc[3 * t] = F.color[3 * p]; A.gc[3 * t + 1] = F.color[3 * p + 1]; A.gc[3 * t + 2] = F.color[3 * p + 2]; }
    float c2w[12];
    if (F.cam7) camera_matrix(F.pose, c2w);                                                                          // k_rays_from_camera
    else for (int k = 0; k < 12; ++k) c2w[k] = F.pose[k];                                                            // k_rays_from_pixels
    const float i = (float)pi, j = (float)pj;
    const float d0 = div_rn(sub_rn(i, A.cx), A.fx);
    const float d1 = (A.mode & 1) ? div_rn(sub_rn(i, A.cy), A.fy) : -div_rn(sub_rn(j, A.cy), A.fy);
    const float d2 = -1.f;
    float o[3], d[3];
    for (int a = 0; a < 3; ++a) {
        d[a] = add_rn(add_rn(mul_rn(d0, c2w[4 * a]), mul_rn(d1, c2w[4 * a + 1])), mul_rn(d2, c2w[4 * a + 2]));
        o[a] = c2w[4 * a + 3];
        A.rd[3 * t + a] = d[a]; A.ro[3 * t + a] = o[a];
    }
    if (A.keep) A.keep[t] = ray_inside(A.R.bound, o[0], o[1], o[2], d[0], d[1], d[2], gd);                           // k_inside_filter
}

// in-bound override for eval_points (reference src/Renderer.cpp:26-36)
__global__ void k_eval_finish(int M, int stage, const float* pts, const float* bound6, const float* occ_a, const float* occ_b,
                              const float* rgb4, float* raw)
{
    int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float px = pts[3 * m], py = pts[3 * m + 1], pz = pts[3 * m + 2];
    bool inb = px < bound6[1] && px > bound6[0] && py < bound6[3] && py > bound6[2] && pz < bound6[5] && pz > bound6[4];
    float occ = occ_a[m];
    if (occ_b) occ = occ_b[m] + occ;
    f4 c = (f4)(0.f);
    if (rgb4) c = *reinterpret_cast<const f4*>(rgb4 + (size_t)m * 4);
    *reinterpret_cast<f4*>(raw + (size_t)m * 4) = (f4){c[0], c[1], c[2], inb ? occ : 100.f};
}

// raw2outputs_nerf_color as a stand-alone op (reference include/torchlib/utils.h:148-172): one wave per ray
__global__ __launch_bounds__(256) void k_raw2outputs(int N, int S, int occupancy, const float* __restrict__ raw, const float* __restrict__ zv,
                                                     const float* __restrict__ rays_d, float* rgb, float* depth, float* var, float* weights)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const bool act = lane < S;
    const size_t m = (size_t)n * S + (act ? lane : S - 1);
    const float dx = rays_d[3 * n], dy = rays_d[3 * n + 1], dz = rays_d[3 * n + 2];
    const float z = zv[m];
    const f4 r4 = *reinterpret_cast<const f4*>(raw + m * 4);
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float znext = __shfl_down(z, 1);
    const float dist = ((lane + 1 < S) ? (znext - z) : 1e10f) * nrm;
    float alpha = occupancy ? 1.f / (1.f + expf(-10.f * r4[3])) : 1.f - expf(-relu_keep_nan(r4[3]) * dist);
    if (!act) alpha = 0.f;
    float incl = act ? (1.f - alpha + 1e-10f) : 1.f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { float up = __shfl_up(incl, o); if (lane >= o) incl *= up; }
    float T = __shfl_up(incl, 1);
    if (lane == 0) T = 1.f;
    const float w = act ? alpha * T : 0.f;
    const float D = wave_sum(w * z);
    const float cr = wave_sum(w * r4[0]), cg = wave_sum(w * r4[1]), cb = wave_sum(w * r4[2]);
    const float V = wave_sum(w * (z - D) * (z - D));
    if (weights && act) weights[m] = w;
    if (lane == 0) { depth[n] = D; var[n] = V; rgb[3 * n] = cr; rgb[3 * n + 1] = cg; rgb[3 * n + 2] = cb; }
}

// Frustum voxel mask (next row N2): Mapper::get_mask_from_c2w, reference src/Mapper.cpp:42-130 (intended semantics, D21/D22):
// pass 1 projects every voxel centre into the frame, samples the depth image bilinearly (cv::remap INTER_LINEAR, zero border)
// and takes the maximum sampled depth; pass 2 applies the in-image / depth / near-camera tests.
__device__ __forceinline__ void voxel_point(const float* b, int Z, int Y, int X, int v, float (&p)[3])
{
    int ix = v % X, iy = (v / X) % Y, iz = v / (X * Y);
    p[0] = add_rn(b[0], mul_rn(sub_rn(b[1], b[0]), linspace01(ix, X)));
    p[1] = add_rn(b[2], mul_rn(sub_rn(b[3], b[2]), linspace01(iy, Y)));
    p[2] = add_rn(b[4], mul_rn(sub_rn(b[5], b[4]), linspace01(iz, Z)));
}
struct FrustumArgs { float bound[6]; float w2c[16]; float cam[3]; int Z, Y, X, H, W; float fx, fy, cx, cy; };
__global__ void k_frustum_pass1(FrustumArgs A, const float* __restrict__ img, float* __restrict__ dep, float* __restrict__ zz,
                                uint8_t* __restrict__ inimg, unsigned int* __restrict__ dmax_bits)
{
    const int n = A.Z * A.Y * A.X;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    float d = 0.f;
    if (v < n) {
        float p[3], cam[3];
        voxel_point(A.bound, A.Z, A.Y, A.X, v, p);
        for (int a = 0; a < 3; ++a)
            cam[a] = add_rn(add_rn(add_rn(mul_rn(A.w2c[4 * a], p[0]), mul_rn(A.w2c[4 * a + 1], p[1])), mul_rn(A.w2c[4 * a + 2], p[2])), A.w2c[4 * a + 3]);
        cam[0] = -cam[0];
        const float z = add_rn(cam[2], 1e-5f);
        const float u = div_rn(add_rn(mul_rn(A.fx, cam[0]), mul_rn(A.cx, cam[2])), z);
        const float w = div_rn(add_rn(mul_rn(A.fy, cam[1]), mul_rn(A.cy, cam[2])), z);
        const float x0 = floorf(u), y0 = floorf(w);
        const float ax = sub_rn(u, x0), ay = sub_rn(w, y0);
        const int ix = (int)x0, iy = (int)y0;
        float s = 0.f;
        for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx) {
            int x = ix + dx, y = iy + dy;
            if (x < 0 || x >= A.W || y < 0 || y >= A.H) continue;
            s = add_rn(s, mul_rn(mul_rn(dx ? ax : sub_rn(1.f, ax), dy ? ay : sub_rn(1.f, ay)), img[(size_t)y * A.W + x]));
        }
        d = s;
        dep[v] = d; zz[v] = z;
        inimg[v] = (u < (float)A.W && u > 0.f && w < (float)A.H && w > 0.f) ? 1 : 0;
    }
    float m = wave_max(fmaxf(d, 0.f));
    if ((threadIdx.x & 63) == 0) atomicMax(dmax_bits, __float_as_uint(m));     // non-negative floats order like their bit patterns
}
__global__ void k_frustum_pass2(FrustumArgs A, const float* __restrict__ dep, const float* __restrict__ zz, const uint8_t* __restrict__ inimg,
                                const unsigned int* __restrict__ dmax_bits, uint8_t* __restrict__ mask)
{
    const int n = A.Z * A.Y * A.X;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const float dmax = __uint_as_float(*dmax_bits);
    const float d = dep[v] == 0.f ? dmax : dep[v];
    const float nz = -zz[v];
    int m = inimg[v] && (0.f <= nz) && (nz <= add_rn(d, 0.5f));
    float p[3];
    voxel_point(A.bound, A.Z, A.Y, A.X, v, p);
    const float dx = sub_rn(p[0], A.cam[0]), dy = sub_rn(p[1], A.cam[1]), dz = sub_rn(p[2], A.cam[2]);
    if (add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)) < 0.25f) m = 1;
    mask[v] = (uint8_t)m;
}

// Keyframe overlap (next row N3): Mapper::keyframe_selection_overlap, reference src/Mapper.cpp:132-196.  One workgroup per
// keyframe projects the N x ns sample points of the current frame into that keyframe and counts those inside its image.
struct OverlapArgs { int N, ns, H, W, K; float fx, fy, cx, cy; };
__global__ __launch_bounds__(256) void k_keyframe_overlap(OverlapArgs A, const float* __restrict__ ro, const float* __restrict__ rd,
                                                           const float* __restrict__ gd, const float* __restrict__ w2c_all,
                                                           float* __restrict__ percent)
{
    __shared__ int sh[4];
    const float* w2c = w2c_all + 16 * blockIdx.x;
    const int total = A.N * A.ns;
    int count = 0;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int n = i / A.ns, s = i - n * A.ns;
        const float nearv = mul_rn(gd[n], 0.8f), farv = add_rn(gd[n], 0.5f);
        const float t = linspace01(s, A.ns);
        const float z = add_rn(mul_rn(nearv, sub_rn(1.f, t)), mul_rn(farv, t));
        float p[3], cam[3];
        for (int a = 0; a < 3; ++a) p[a] = add_rn(ro[3 * n + a], mul_rn(rd[3 * n + a], z));
        for (int a = 0; a < 3; ++a)
            cam[a] = add_rn(add_rn(add_rn(mul_rn(w2c[4 * a], p[0]), mul_rn(w2c[4 * a + 1], p[1])), mul_rn(w2c[4 * a + 2], p[2])), w2c[4 * a + 3]);
        cam[0] = -cam[0];
        const float zc = add_rn(cam[2], 1e-5f);
        const float u = div_rn(add_rn(mul_rn(A.fx, cam[0]), mul_rn(A.cx, cam[2])), zc);
        const float v = div_rn(add_rn(mul_rn(A.fy, cam[1]), mul_rn(A.cy, cam[2])), zc);
        if (u < (float)(A.W - 20) && u > 20.f && v < (float)(A.H - 20) && v > 20.f && zc < 0.f) ++count;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) percent[blockIdx.x] = div_rn((float)(sh[0] + sh[1] + sh[2] + sh[3]), (float)total);
}

// Pixel draw and ground-truth gather of raySampler (next row N1): reference include/torchlib/utils.h:13-43.  torch::randint's
// stream cannot be reproduced; the draw uses a counter-based hash of (seed, ray index), the same the perturbation of k_sample uses.
__global__ void k_sample_pixels(unsigned long long seed, int n, int H0, int W0, int Ww, unsigned long long total, int* __restrict__ pi,
                                int* __restrict__ pj)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const unsigned long long ind = ((unsigned long long)hash_u32(seed, (uint32_t)r, 0x51u) * total) >> 32;
    pi[r] = W0 + (int)(ind % (unsigned long long)Ww);
    pj[r] = H0 + (int)(ind / (unsigned long long)Ww);
}
__global__ void k_gather_pixels(int n, const int* __restrict__ pi, const int* __restrict__ pj, int W, const float* __restrict__ depth,
                                const float* __restrict__ color, float* __restrict__ gd, float* __restrict__ gc)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const size_t p = (size_t)pj[r] * W + pi[r];
    gd[r] = depth[p];
    if (color && gc) { gc[3 * r] = color[3 * p]; gc[3 * r + 1] = color[3 * p + 1]; gc[3 * r + 2] = color[3 * p + 2]; }
}

// ---------------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------------
// Every device buffer of the context is a Buf: freed by its owner's destructor, empty (null, capacity 0) after a failed allocation.
struct HipAlloc {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
template <typename T> using Buf = DevBuf<T, HipAlloc>;

struct GridState {
    int C = 0, Z = 0, Y = 0, X = 0;
    size_t n = 0;                // floats = nvox*32 (0 = not uploaded)
    Buf<float> v, m, s;          // one group: allocated together or not at all
    Buf<uint8_t> mask;
    size_t g_off = 0;            // offset in the gradient slab
    Buf<int> midx; int nmask = 0; bool midx_dirty = true;      // ascending list of the marked voxels (packed gradient exchange)
    Buf<uint8_t> live; bool live_dirty = true;                 // per cell: any corner voxel marked (k_cell_live); rebuilt like midx when the mask changed
};
// One derived copy of a decoder's parameters (nsk_images.h): the image, the table an upload builds it through, the inverse table the optimiser
// launch rewrites it through.  dirty: the image lags behind the parameters and is rebuilt before use (image 3 alone is ever left so).
struct DecImage { Buf<float> data; Buf<int> idx, inv; ImageSpec spec; bool dirty = false; };
struct DecState {
    int n = 0;                                    // parameter count; set once the one-time setup is complete (0 = never uploaded)
    Buf<float> p, m, s;
    DecImage img[NSK_NUM_IMAGES];                 // by `what` of nsk_images.h; 2 and 3 of the coarse decoder stay empty
    int trainable = 0;
    bool loaded = false;
    size_t g_off = 0;
};
// One set of sampling outputs: what k_sample, k_sort_scan and k_sort_place leave of one batch for the decoders, the compositing and the backward.
struct SampleSet {
    Buf<float> z;                    // [m] sample depths
    // cell sort of the samples (k_sample keys -> k_sort_scan -> k_sort_place): perm lists the samples cell by cell
    Buf<int> perm, skey, srank;      // [m]
    // liveness bytes (LiveArgs): by sample as k_sample writes them, by slot as k_sort_place re-orders them (ray order: the samples' are the slots')
    Buf<uint8_t> lsamp, lslot;       // [m]
    Buf<int> offs;                   // [bins of the key level], sized apart from the six above (ensure_hist, ensure_next)
    size_t cap() const { return z.cap(); }      // m: the six are allocated and released together (alloc_samples)
    uint8_t* live_out(bool wanted) const { return wanted ? lsamp.get() : nullptr; }      // where a sampling writes liveness bytes, if it is to write any
    void swap(SampleSet& o) noexcept { z.swap(o.z); perm.swap(o.perm); skey.swap(o.skey); srank.swap(o.srank); lsamp.swap(o.lsamp); lslot.swap(o.lslot); offs.swap(o.offs); }
};
struct Workspace {
    int capM = 0, capN = 0;          // the batch (samples, rays) the group below was allocated for; 0 = not allocated
    // cur: the set the current step's launches read.  next: the set of the batch nsk_map_prepare registered, filled while the current step runs; a
    // step that finds its batch prepared swaps the two (forward_core).  Both are kept at the same capacities (ensure_next).
    SampleSet cur, next;
    Buf<float> occ[3], rgb4;
    Buf<float> imp_z, imp_w;         // importance sampling (forward_core): the first pass's depths and compositing weights [m], allocated with the first such step
    Buf<unsigned long long> masks[4];
    Buf<f4> hsave[4];                // block outputs of trainable decoders saved by the forward (save_h)
    int hsave_M[4] = {0, 0, 0, 0};   // sample count of the forward that filled hsave (0 = stale)
    Buf<float> g_raw, ray_loss;
    Buf<float> tmp_rgb, tmp_depth;
    Buf<float> dec_slabs;            // per-workgroup partial decoder gradients [num_cu][20920]
    Buf<int> hist_raw;               // the cell sort's histogram, one for both sets [bins of the key level] (cur.offs.cap() = bins); zero between steps
    int* hist() const { return hist_raw ? hist_raw.get() + 16 : nullptr; }      // behind one 64-byte line: hist()[-1] is k_sort_scan's cursor
};
// how much of a prepared batch's sampling has run (nsk_ctx::Prep): the samples, then -- cell-sorted batches only -- the offsets, then the placement
enum PrepDone { PREP_NOTHING, PREP_SAMPLED, PREP_SCANNED, PREP_PLACED };
struct nsk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    RParams R;
    int n_importance = 0;                   // nsk_set_importance: extra depths per ray drawn from a first pass's weights (0: one pass)
    Buf<float> d_bound;
    GridState grid[4];
    DecState dec[4];
    Buf<float> slab; size_t slab_n = 0;
    Buf<float> xbuf; size_t xbuf_n = 0;     // packed exchange buffer (nsk_grad_pack) and its current length
    bool x_identity = false;                                              // the last pack handed out the slab itself (no masks)
    bool xlevels[4] = {false, false, false, false}; bool xdecs[4] = {false, false, false, false};      // what the last pack holds
    Workspace ws;
    Buf<float> scal;             // [0] gt max, [1] median threshold, [2] loss, [4] frustum max depth (bits)
    Buf<uint8_t> fr_tmp;         // scratch of nsk_frustum_mask and nsk_keyframe_overlap, in bytes
    int adam_step[NSK_NUM_GROUPS] = {0, 0, 0, 0, 0, 0};
    // ---- hipGraph capture of a step (nsk_graph_*): the kernels of the calls made between begin and end are recorded once and
    // replayed with one launch; Adam's bias-correction constants are kernel arguments, so the recorded k_adam_multi node is
    // patched with the current step counts before every replay
    bool capturing = false;
    struct CapAdam { AdamArgs args; int group[8]; float lr[8]; };
    std::vector<CapAdam> cap_adams;             // Adam launches seen during the current capture
    struct CapVec { int n; float* p; const float* g; float* m; float* v; float lr, b1, b2, eps; int step; hipGraphNode_t node; float ss, bc2s; };
    std::vector<CapVec> cap_vecs;               // nsk_adam_vector launches seen during the current capture
    int cap_rollback[NSK_NUM_GROUPS] = {0, 0, 0, 0, 0, 0};
    int ws_flip = 0;                            // parity of the swaps between the workspace's two sampling sets (forward_core): a graph records the set that was primary at capture
    struct GraphRec { bool stale = false; int flip = 0; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; hipGraphNode_t adam_node = nullptr; bool has_adam = false; CapAdam adam; std::vector<CapVec> vecs; };
    std::vector<GraphRec> graphs;
    bool touched[NSK_NUM_GROUPS] = {false, false, false, false, false, false};
    bool deterministic = false;             // debug: bit-reproducible gradients (see nsk_set_tuning in include/nsk.h)
    bool roctx = false;                     // roctx ranges around every profiled launch group (libroctx64, loaded on demand)
    SplitTune tune;                         // the cost model of the workgroup splits (nsk_split.h)
    int tune_no_occ_role = 0;               // the merged middle + fine role of the forward: 1 = never merged, 2 = always
    bool median_fused_pending = false;
    int tune_no_deferred_median = 0;        // 1: the threshold inside the compositing launch (grid barrier) even where the backward could find it (round 3's form)
    int tune_no_fused_median = 0;           // 1: the Tracker's median threshold in its own launch even where the fused form applies (experiments, tests)
    int tune_no_frozen_kernel = 0;          // 1: launches without a trainable role also go through k_decode_bwd_multi (experiments, tests)
    // ---- dead-tile skip of the frozen roles under optimiser masks (decode_bwd_body<.., SKIP>)
    int tune_no_dead_skip = 0;              // 1: every tile runs (A/B runs, tests)
    int live_epoch = 0;                     // bumped whenever a mask or a masked level changes: liveness bytes written before are stale
    bool live_ok = false;                   // the primary sampling set holds liveness bytes for the current step (forward_core)
    Buf<int> live_cnt;                      // device: tiles run by [middle, fine, colour] + the publishing ticket
    int* live_host = nullptr; int* live_host_dev = nullptr;      // host memory the last counting workgroup writes [3 counts, tag]; never waited for
    // ---- queue dealing of the backward's skipping roles (decode_bwd_body: Dealing)
    Buf<int> deal_cur;                      // device: one cursor per level [middle, fine, colour], NSK_DEAL_STRIDE ints apart (a memory line each)
    bool deal_armed = false;                // the launch in front of the coming backward zeroes the cursors (k_composite); else backward_core does, with a memset
    int tune_static_deal = 0;               // 1: every role deals its tiles statically (tile_of), as before the cursors (A/B runs, tests)
    int tune_deal_head_pct = 75;            // share of a skipping frozen role's rounds that stay dealt statically
    int tune_deal_min_rounds = 24;          // a role whose waves have fewer rounds of tiles than this deals statically
    int tune_deal_chunk = 2;                // consecutive tiles per claim of the rest (1 .. 16)
    int live_tag = 1;                       // names the current (stage, batch size, flags, masks) of the counts: a step reads only counts of its own kind
    int live_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int dbg_wgs[3] = {0, 0, 0}, dbg_ntasks = 0;      // the last backward's split: workgroups of the role of each level (frozen or trainable), its tile count
    int dbg_live[3] = {-1, -1, -1}; bool dbg_counted[3] = {false, false, false};      // the last backward: tiles per level (-1 no frozen role), which of them the device counts
    const uint8_t* ray_mask = nullptr;      // nsk_set_ray_mask
    // nsk_set_depth_max_batch: the batch whose max(gt_depth) the sampling uses when gt_depth_max < 0 (a ray shard of a larger batch: N > 1)
    struct DMax { const float* gt = nullptr; const uint8_t* keep = nullptr; int n = 0; } dmax;
    float* xextra = nullptr; size_t xextra_n = 0;      // nsk_grad_extra: a caller-owned vector that travels with the packed exchange
    int sort_mode = -1;                     // -1 automatic (sort_pays), 0 never, 1 always (nsk_set_sort_mode; tests)
    bool sorted = false;                    // the current step's decoder launches walk the samples in cell-sorted order (ws.cur.perm)
    // nsk_map_prepare: the sampling (+ cell sort) of the NEXT batch rides in the launches of the current step (composite + sample, backward + scan,
    // Adam + place): `req` is a registered batch nothing has been launched for yet, `prep` the batch whose outputs sit (or are being built) in the
    // workspace's `next` set; done: how far its sampling has come (PrepDone: the stages run in this order and none is skipped)
    struct Prep { bool valid = false; int stage = 0, N = 0, S = 0; const float* ro = nullptr; const float* rd = nullptr; const float* gt = nullptr;
                  float gtmax = 0.f; const uint8_t* mask = nullptr; bool sorted = false; PrepDone done = PREP_NOTHING; RParams R; DMax dmax;
                  bool live = false; int live_epoch = 0; } prep, req;      // live: its sampling wrote liveness bytes, under the masks of live_epoch
    int tune_no_piggyback = 0;              // 1: a prepared batch is sampled by launches of its own at the start of its step (experiments, tests)
    int pend_w = -1, pend_nb = 0;           // decoder whose per-workgroup gradient slabs are not yet summed into the slab (flush_pending)
    int dbg_split[2][NSK_SPLIT_INTS] = {{0}, {0}};      // nsk_debug_last_split: the last forward decoder launch / the last backward, recorded where wg_end is filled
    int dbg_M = 0, dbg_S = 0;               // sample count / samples per ray of the last forward_core (nsk_debug_relu_bits, nsk_debug_preact)
    int bwd_mode = 2;                       // decoder backward chains: 2 fp16 2-piece split (default), 0 fp32 MFMA (nsk_set_backward_mode: a measuring stick)
    int matmul_mode = 2;                    // decoder forward: 0 fp32 MFMA, 1 bf16 3-piece split, 2 fp16 2-piece split (nsk_bf16.h)
    double last_bytes = 0, last_flops = 0; int last_samples = 0;
    // mesh extraction (nsk_eval_lattice / nsk_mesh_extract): slab points, per-node scratch, the table's device copy, the last mesh
    struct Mesh {
        Buf<float> lat_pts;                                  // [slab][3] points of the lattice slab being evaluated
        Buf<unsigned> lat_idx, lat_scan;                     // nsk_eval_lattice_masked: [set nodes] ascending node indices; the workgroup counts' scan words
        int slab = 0;                                        // nsk_set_tuning "lattice_slab": nodes per slab (0 = automatic)
        Buf<uint8_t> cellcase; Buf<int> emap;                // [nodes], [nodes][3]: one group
        Buf<unsigned> scan;
        Buf<int8_t> table; Buf<uint8_t> ntri;                // one group
        Buf<float> verts; Buf<int> tris;                     // [nv][3], [nt][3]
        int nv = 0, nt = 0;
        bool extracted = false;                              // a mesh (possibly empty) is there for nsk_mesh_filter
        // nsk_mesh_filter: per-vertex scratch (one group), the statistics, the compacted mesh (swapped with verts / tris)
        Buf<int> cc_label; Buf<double> cc_area; Buf<uint8_t> cc_used, cc_keep;
        Buf<CcStats> cc_stats;
        Buf<float> verts2; Buf<int> tris2;
    } mesh;
    // row reductions (rows_reduce): [groups][rows][columns] partial rows of the call in flight, then its [groups][columns] results
    Buf<double> rows;
    // whole-frame rendering (nsk_render_image): the rays of the chunk being rendered
    struct Image {
        Buf<float> ro, rd, gd;                               // [chunk][3], [chunk][3], [chunk]: one group
    } img;
    // structural similarity (nsk_image_ssim): the pooled levels of both images, and the windows' (ssim, cs) of the level being summed
    struct Ssim {
        Buf<double> pyr;                                     // levels 1 .. of a, then of b: [H_l][W_l][C] each
        Buf<double> terms;                                   // [Hm Wm][C][2] of level 0 (the largest)
    } ssim;
    // reconstruction metrics (nsk_mesh_sample / nsk_cloud_nearest / nsk_cloud_stats): scratch that grows to the largest call and stays
    struct Cloud {
        Buf<double> cum, bsum;                               // [triangles] cumulative areas, [workgroups] their totals
        Buf<unsigned> degenerate;
        Buf<unsigned> tcell, start, cursor; Buf<float4> sorted;      // targets: [n] cells, [cells + 1 + scan levels], [cells], [n] in cell order
        Buf<unsigned> qcell, qstart, qcursor, qperm;         // queries in cell order (the same grid)
        Buf<float> icp_dist; Buf<int> icp_index;             // [sources] the correspondences, when the caller keeps none
        int cells_x4 = 4;                                    // nsk_set_tuning "cloud_cells_x4": grid cells aimed at per finite target, in quarters
        int query_mode = 0;                                  // nsk_set_tuning "cloud_query_mode": bit 0 a wave per query; + 2 queries always in input order, + 4 always in cell order (neither: by size)
    } cloud;
    // distances to a mesh (nsk_mesh_nearest): the packed triangles and their grid; the queries' ordering reuses cloud.q*
    struct Surface {
        Buf<SurfTri> rec;                                    // [triangles] 48-byte records, a.w = 1: takes part
        Buf<unsigned> start, cursor;                         // [cells + 1 + scan levels] first reference of every cell, [cells] placement cursors
        Buf<int> refs, wide;                                 // [references] triangle indices in cell order, [triangles] the wide list
        Buf<unsigned long long> counters;                    // [0] references, [1] wide triangles
        int cells_x4 = SURF_CELLS_X4;                        // nsk_set_tuning "surface_cells_x4": grid cells aimed at per participating triangle, in quarters
        int query_mode = 0;                                  // nsk_set_tuning "surface_query_mode": bit 0 reserved; + 2 queries always in input order, + 4 always in cell order (neither: by size)
    } surface;
    // mesh depth views (nsk_mesh_depth): the queue of large pixel boxes, its cursor and the skipped count
    struct Raster {
        Buf<RasterJob> queue;                                // [queue_cap] (view, triangle, box) entries of the launch in flight
        Buf<unsigned> counters;                              // [0] the queue's cursor, [1] triangles with an index out of range
        int inline_max = 64;                                 // nsk_set_tuning "raster_inline_max": a box of more pixels is queued
        int queue_cap = 1 << 18;                             // nsk_set_tuning "raster_queue_cap": entries (24 B each)
        int load_first = 1;                                  // nsk_set_tuning "raster_load_first": a plain load in front of the atomic minimum
    } raster;
    // culling (nsk_cull.h): nsk_points_view_counts' counters, nsk_mesh_select's scan words
    struct Cull {
        Buf<unsigned> view_counts;                           // [V]
        Buf<unsigned> scan;                                  // vertex flags' scan | triangle flags' scan | the skipped count
    } cull;
    // vertex normals and colours along them (nsk_normals.h): scratch that grows to the largest call and stays
    struct Normals {
        Buf<float> fn;                                       // [triangles][3] face normals, NaN = the triangle is left out
        Buf<unsigned> off;                                   // [vertices + 1 + scan levels] namings -> first slot -> slot behind the last
        Buf<unsigned> list;                                  // [corners] corner numbers 3 t + k, by vertex, ascending inside a vertex
        Buf<unsigned> longq;                                 // vertices named by more than VN_SHORT corners
        Buf<unsigned> counters;                              // [0] triangles left out, [1] vertices without a normal, [2] most namings, [3] the queue's length
        Buf<float> raw; Buf<uint8_t> has;                    // nsk_mesh_vertex_colors: [chunk][4] point colours, [chunk] ray flags
    } normals;
    // convex hull of a cloud and the lattice nodes inside it (nsk_hull.h): the points' side of the insertion loop, and the last hull
    struct Hull {
        Buf<int> q, face_of;                                 // [points][3] quantised coordinates, [points] the face a point is outside of (-1: none)
        Buf<int> list[2];                                    // the points still outside, re-compacted from one into the other
        Buf<unsigned> scan;
        Buf<HullFaceRec> faces;                              // every face's plane, by face number
        Buf<unsigned long long> best, cnt; Buf<unsigned> arg; Buf<HullReport> rep;      // per new face of the insertion in flight: one group
        Buf<long long> part;                                 // partial results of the bounds and selection passes
        Buf<float> extra, gxyz; Buf<int> gidx;               // the host points; the hull vertices' coordinates and indices on their way to the host
        Buf<double> planes;                                  // nsk_lattice_in_hull: [faces][6]
        // the hull of the last nsk_points_hull / nsk_hull_upload: ascending vertex indices, faces as index triples, the vertices' fp32
        // coordinates, the faces as positions in `verts`
        std::vector<int> verts, tris, local;
        std::vector<float> xyz;
        void clear() { verts.clear(); tris.clear(); local.clear(); xyz.clear(); }
        void set(const std::vector<int>& v, const std::vector<int>& t, const std::vector<float>& x)
        {
            verts = v; tris = t; xyz = x;
            local.resize(t.size());
            for (size_t k = 0; k < t.size(); ++k) local[k] = (int)(std::lower_bound(verts.begin(), verts.end(), t[k]) - verts.begin());
        }
    } hull;
    // mesh simplification by vertex clustering (nsk_simplify.h): scratch that grows to the largest call and stays
    struct Simplify {
        Buf<float> part;                                     // the bounds pass's partial boxes
        Buf<unsigned> vcell;                                 // [vertices] the cell of every vertex
        Buf<unsigned> occ;                                   // [cells + 1 + scan levels] occupancy flag -> rank among the occupied cells
        Buf<unsigned> cnt, cellof; Buf<unsigned long long> sums;     // [occupied], [occupied], [occupied][3]: members, cell index, sums of q
        Buf<unsigned> loff, vflag;                           // [occupied + 1 + scan levels] each: the smallest-corner lists' ends; referenced flag -> output index
        Buf<unsigned> tkey, tflag, list, longq;              // [triangles][3] corner ranks, [triangles + 1 + scan levels] kept flag -> output index, [triangles] the lists, the long lists' queue
        Buf<unsigned> counters;                              // [0] invalid, [2] duplicates, [3] the queue's length
    } simplify;
    // the optional count of an entry point (count_begin / count_end): nsk_lattice_seen, nsk_points_seen, nsk_tsdf_integrate, nsk_tsdf_volume,
    // nsk_lattice_in_hull
    Buf<unsigned long long> count;
    // optional per-kernel timing with HIP events on the context's stream (nsk_profile_begin / _end)
    bool prof = false;
    struct ProfRec { const char* name; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    ~nsk_ctx();                 // graphs, profiling events, an owned stream; the buffers free themselves
};

// roctx ranges (rocprofv3 --marker-trace shows them around the kernels of each launch group); libroctx64 is loaded on first use
typedef int (*roctx_push_t)(const char*);
typedef int (*roctx_pop_t)(void);
static roctx_push_t g_roctx_push = nullptr;
static roctx_pop_t g_roctx_pop = nullptr;
static bool roctx_ready()
{
    static int state = 0;       // 0 untried, 1 ok, -1 unavailable
    if (state == 0) {
        void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (h) { g_roctx_push = (roctx_push_t)dlsym(h, "roctxRangePushA"); g_roctx_pop = (roctx_pop_t)dlsym(h, "roctxRangePop"); }
        state = (g_roctx_push && g_roctx_pop) ? 1 : -1;
    }
    return state == 1;
}

struct ProfScope {      // records start/stop events around the launches issued while it is alive
    nsk_ctx* c; hipEvent_t a = nullptr, b = nullptr; const char* name; bool ranged = false;
    ProfScope(nsk_ctx* c_, const char* n, bool on = true) : c(c_), name(n)
    {
        if (!on) return;                                    // launches on the side stream are not timed (the events sit on c->stream)
        if (c->roctx && roctx_ready()) { g_roctx_push(n); ranged = true; }
        if (!c->prof) return;
        hipEventCreate(&a); hipEventCreate(&b);
        hipEventRecord(a, c->stream);
    }
    ~ProfScope()
    {
        if (ranged) g_roctx_pop();
        if (!c->prof || !a) return;
        hipEventRecord(b, c->stream);
        c->prof_recs.push_back({name, a, b});
    }
};

// Captured graphs hold raw pointers into the workspace, the gradient slab and the grids: whenever one of those buffers is
// freed or reallocated every recorded graph becomes unusable and nsk_graph_launch must say so instead of replaying onto freed memory.
static void invalidate_graphs(nsk_ctx* c)
{
    for (auto& R : c->graphs) {
        if (R.stale) continue;
        if (R.exec) { hipGraphExecDestroy(R.exec); R.exec = nullptr; }
        if (R.graph) { hipGraphDestroy(R.graph); R.graph = nullptr; }
        R.stale = true;
    }
}

nsk_ctx::~nsk_ctx()
{
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    invalidate_graphs(this);
    for (auto& r : prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    if (own_stream && stream) hipStreamDestroy(stream);
    if (live_host) hipHostFree(live_host);
}

// ---- growing a buffer ---------------------------------------------------------------------------------------------
// dev_alloc: (re)allocate and report a failure with its size; the buffer is empty afterwards, never dangling.
template <typename T>
static int dev_alloc(Buf<T>& b, size_t n, const char* what)
{
    const int e = b.alloc(n);
    if (e == 0) return 0;
    (void)hipGetLastError();
    return fail("cannot allocate %zu bytes for %s (%s)", n * sizeof(T), what, hipGetErrorString((hipError_t)e));
}
// the six per-sample buffers of a sampling set, m elements each; after a failure the set is empty (its offsets are not touched).  what: one name
// for the whole set in the failure's text, else each buffer is named by its content
static int alloc_samples(SampleSet& s, size_t m, const char* what = nullptr)
{
    const int r = [&]() -> int {
        CHK(dev_alloc(s.z, m, what ? what : "the sample depths"));
        CHK(dev_alloc(s.perm, m, what ? what : "the cell sort")); CHK(dev_alloc(s.skey, m, what ? what : "the cell sort")); CHK(dev_alloc(s.srank, m, what ? what : "the cell sort"));
        CHK(dev_alloc(s.lsamp, m, what ? what : "the liveness bytes")); CHK(dev_alloc(s.lslot, m, what ? what : "the liveness bytes"));
        return 0;
    }();
    if (r != 0) reset_all(s.z, s.perm, s.skey, s.srank, s.lsamp, s.lslot);
    return r;
}
// what has to happen before a buffer that launches (and, per site, recorded graphs) may point into is replaced
enum { GROW_NO_CAPTURE = 1,         // refuse while a graph is being captured
       GROW_STALE_GRAPHS = 2 };     // the recorded graphs hold this buffer's address
static int grow_begin(nsk_ctx* c, unsigned flags)
{
    if ((flags & GROW_NO_CAPTURE) && c->capturing) return fail("graph capture: the workspace must grow (run the same step once before nsk_graph_begin)");
    HIPCHK(hipStreamSynchronize(c->stream));
    if (flags & GROW_STALE_GRAPHS) invalidate_graphs(c);
    return 0;
}
template <typename T>
static int grow(nsk_ctx* c, Buf<T>& b, size_t n, const char* what, unsigned flags)
{
    if (n <= b.cap()) return 0;
    CHK(grow_begin(c, flags));
    return dev_alloc(b, n, what);
}

// the rows of a row reduction (nsk_reduce.h) of n elements: a function of n alone
static int rows_count(long long n, int block, int cap) { return (int)std::min<long long>((n + block - 1) / block, cap); }
// the launches of a row reduction alone: launch(nrows, rows) the caller's partial-rows kernel, then the finisher's groups * Cols::N results
// into `out` (rows, out: device memory of the caller's choice; nsk_image_ssim queues one reduction per level and reads them back together)
template <class Cols, class Launch>
static int rows_launch(nsk_ctx* c, const char* name, int groups, int nrows, double* rows, double* out, Launch launch)
{
    const size_t nout = (size_t)groups * Cols::N;
    { ProfScope ps(c, name);
      launch(nrows, rows);
      k_rows_finish<Cols><<<(unsigned)((nout + 255) / 256), 256, 0, c->stream>>>(groups, nrows, rows, out); }
    HIPCHK(hipGetLastError());
    return 0;
}
// A row reduction (nsk_reduce.h) of `groups` sets of n elements each: min(ceil(n / block), cap) rows per group -- a function of n alone --
// in the context's one scratch, launch(nrows, rows) the caller's partial-rows kernel, the finisher, groups * Cols::N doubles back to the
// host.  Synchronises, so the scratch is free again when it returns.
template <class Cols, class Launch>
static int rows_reduce(nsk_ctx* c, const char* name, const char* what, int groups, long long n, int block, int cap, Launch launch, double* h_out)
{
    const int nrows = rows_count(n, block, cap);
    const size_t nout = (size_t)groups * Cols::N;
    CHK(grow(c, c->rows, (size_t)groups * (cap + 1) * Cols::N, what, GROW_NO_CAPTURE));
    double* rows = c->rows;
    double* out = rows + (size_t)nrows * nout;
    CHK(rows_launch<Cols>(c, name, groups, nrows, rows, out, launch));
    HIPCHK(hipMemcpyAsync(h_out, out, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" const char* nsk_last_error(void) { return g_err.c_str(); }
extern "C" int nsk_version(void) { return NSK_VERSION; }

static int which_ok(int w) { return w >= 0 && w < 4; }

template <typename K>
static int set_lds(K kern, size_t bytes)
{
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

static size_t fwd_img_floats(int w) { return w == 0 ? CoarseFwdImg::TOTAL : (w == 2 ? MlpFwdImg<4>::TOTAL : MlpFwdImg<2>::TOTAL); }
static size_t bwd_img_floats(int w) { return w == 0 ? CoarseBwdImg::TOTAL : MlpBwdImg::TOTAL; }
static size_t bwd_lds_bytes(int w, bool train)
{
    size_t scratch = 8 * 3840;                               // 8 waves x (NSK_SCRATCH_FLOATS <= 960) floats
    if (!train) return bwd_img_floats(w) * 4 + scratch;
    if (w == 1 || w == 3) return PM_LDS_BYTES;               // merged-phase body (nsk_train.h): 18 fragment groups + tail + 224 panel rows
    size_t img = w == 2 ? 0 : bwd_img_floats(w);          // saved-activation form: only the backward image sits in LDS
    return (img + PN_FLOATS(w == 2 ? 4 : 2)) * 4;            // the per-wave scatter scratch lives in panel rows 0..63
}
// dynamic LDS of a backward launch with roles (nsk_split.h: BwdKernel): the largest of its roles' needs in that kernel
static size_t bwd_form_lds_bytes(BwdKernel k, int n, const int* which, const int* train)
{
    size_t lds = 0;
    for (int r = 0; r < n; ++r) {
        // the full-width chains keep a trainable role's panel beside the image (CQ 2 for every decoder)
        if (k == BWD_MULTI_FULL || k == BWD_MULTI_FULL_RAYS) lds = std::max(lds, bwd_img_floats(which[r]) * 4 + (train[r] ? PN_FLOATS(2) * 4 : 8 * 3840));
        else lds = std::max(lds, bwd_lds_bytes(which[r], train[r] != 0));
    }
    if (k == BWD_TRACK) lds += NSK_DYN_LDS_BYTES;                                        // the residuals and the median's counters
    if (k == BWD_FROZEN) lds += (size_t)(NSK_FROZEN_NW - 8) * 3840;                      // image + one scatter scratch per wave
    return lds;
}
static_assert(BWD_FROZEN_WAVES == NSK_FROZEN_NW && BWD_MEDIAN_MAX_RAYS == NSK_MEDIAN_FUSED_MAX, "nsk_split.h mirrors nsk_device.h");
static_assert(NSK_SPLIT_BWD_SEPARATE == 1 && NSK_SPLIT_BWD_MULTI == 2 && NSK_SPLIT_BWD_MULTI_FULL == 3 && NSK_SPLIT_BWD_FROZEN == 4 && NSK_SPLIT_BWD_TRACK == 5,
              "bwd_split_form (nsk_split.h) returns the values of include/nsk.h");

extern "C" int nsk_ctx_create(int device, void* hip_stream, nsk_ctx** out)
{
    if (!out) return fail("nsk_ctx_create: out is NULL");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail("nsk_ctx_create: no HIP device (the MI355X kernels have no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("nsk_ctx_create: device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail("nsk_ctx_create: device arch %s, this library is built for gfx950 only", prop.gcnArchName);
    std::unique_ptr<nsk_ctx> owner(new nsk_ctx());       // every early return below releases what was made, the stream included
    nsk_ctx* c = owner.get();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
    else { HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    const float b[6] = {-4.5f, 3.82f, -1.5f, 2.02f, -3.0f, 2.76f};     // reference src/Renderer.cpp:15
    memcpy(c->R.bound, b, sizeof(b));
    c->R.n_samples = 32; c->R.n_surface = 16; c->R.lindisp = 0; c->R.occupancy = 0; c->R.perturb = 0.f; c->R.seed = 0;
    CHK(dev_alloc(c->d_bound, 6, "the bound"));
    HIPCHK(hipMemcpy(c->d_bound, b, sizeof(b), hipMemcpyHostToDevice));
    CHK(dev_alloc(c->scal, 16, "the scalars"));
    HIPCHK(hipMemset(c->scal, 0, 16 * sizeof(float)));
    CHK(dev_alloc(c->live_cnt, 4, "the live-tile counters"));
    HIPCHK(hipMemset(c->live_cnt, 0, 4 * sizeof(int)));
    CHK(dev_alloc(c->deal_cur, 3 * NSK_DEAL_STRIDE, "the dealing cursors"));
    HIPCHK(hipMemset(c->deal_cur, 0, 3 * NSK_DEAL_STRIDE * sizeof(int)));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->live_host), 16 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->live_host, 0, 16 * sizeof(int));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->live_host_dev), c->live_host, 0));
    // dynamic LDS limits
    CHK(set_lds(k_decode_fwd<0>, fwd_img_floats(0) * 4)); CHK(set_lds(k_decode_fwd<1>, fwd_img_floats(1) * 4));
    CHK(set_lds(k_decode_fwd<2>, fwd_img_floats(2) * 4)); CHK(set_lds(k_decode_fwd<3>, fwd_img_floats(3) * 4));
#define SETB(W) \
    CHK(set_lds(k_decode_bwd<W, false>, bwd_lds_bytes(W, false))); CHK(set_lds(k_decode_bwd<W, true>, bwd_lds_bytes(W, false))); \
    CHK(set_lds(k_decode_bwd_train<W, false>, bwd_lds_bytes(W, true))); CHK(set_lds(k_decode_bwd_train<W, true>, bwd_lds_bytes(W, true)));
    SETB(0) SETB(1) SETB(2) SETB(3)
#undef SETB
    CHK(set_lds(k_median_thr, 16384 * 4));
    CHK(set_lds(k_decode_fwd_multi, 160 * 1024)); CHK(set_lds(k_decode_fwd_multi_bf16<8>, 160 * 1024)); CHK(set_lds(k_decode_fwd_multi_bf16<8, 2>, 160 * 1024)); CHK(set_lds(k_decode_fwd_multi_occ<8>, 160 * 1024));
    CHK(set_lds(k_decode_bwd_multi<false>, 160 * 1024 - 256)); CHK(set_lds(k_decode_bwd_multi_deal, 160 * 1024 - 256)); CHK(set_lds(k_decode_bwd_multi<true>, 160 * 1024));      // (<false>, frozen: the scan role keeps a few words of static LDS)
    CHK(set_lds(k_decode_bwd_frozen, 160 * 1024 - 256));
    CHK(set_lds(k_decode_bwd_track, 160 * 1024)); CHK(set_lds(k_decode_bwd_multi_full<false>, 160 * 1024)); CHK(set_lds(k_decode_bwd_multi_full<true>, 160 * 1024));
    CHK(set_lds(k_decode_fwd_dump<0>, 160 * 1024)); CHK(set_lds(k_decode_fwd_dump<1>, 160 * 1024)); CHK(set_lds(k_decode_fwd_dump<2>, 160 * 1024));
    *out = owner.release();
    return 0;
}

extern "C" int nsk_ctx_destroy(nsk_ctx* c)
{
    delete c;
    return 0;
}

extern "C" int nsk_sync(nsk_ctx* c)
{
    if (!c) return fail("null ctx");
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->median_fused_pending) {          // k_composite mode 4 ran since the last sync: did its grid barrier time out?
        c->median_fused_pending = false;
        unsigned bar[3] = {0, 0, 0};
        HIPCHK(hipMemcpy(bar, c->scal + 5, sizeof(bar), hipMemcpyDeviceToHost));
        if (bar[2]) {
            HIPCHK(hipMemset(c->scal + 5, 0, sizeof(bar)));
            return fail("nsk_track_step: the grid barrier of the fused median timed out (threshold was infinite for that step); nsk_set_tuning(\"no_fused_median\", 1) selects the three-launch form");
        }
    }
    return 0;
}
extern "C" void* nsk_stream(nsk_ctx* c) { return c ? (void*)c->stream : nullptr; }

static int pack_image(nsk_ctx* c, DecState& D, int what);
extern "C" int nsk_set_matmul_mode(nsk_ctx* c, int mode)
{
    if (!c) return fail("null ctx");
    if (mode < 0 || mode > 2) return fail("nsk_set_matmul_mode: mode must be 0 (fp32 MFMA), 1 (bf16 3-piece split) or 2 (fp16 2-piece split)");
    if (c->capturing) return fail("nsk_set_matmul_mode: not while a graph is being captured");
    const bool relayout = (mode == 2) != (c->matmul_mode == 2);
    c->matmul_mode = mode;
    if (relayout) {              // the forward images change their piece format: rebuild those of the loaded decoders
        HIPCHK(hipSetDevice(c->device));
        for (int w = 1; w < 4; ++w) if (c->dec[w].loaded) CHK(pack_image(c, c->dec[w], 2));
        invalidate_graphs(c);
    }
    return 0;
}

extern "C" int nsk_set_backward_mode(nsk_ctx* c, int mode)
{
    if (!c) return fail("null ctx");
    if (mode != 0 && mode != 2) return fail("nsk_set_backward_mode: 0 (fp32 MFMA chains) or 2 (two fp16 pieces, default)");
    c->bwd_mode = mode;
    return 0;
}

extern "C" int nsk_set_tuning(nsk_ctx* c, const char* key, int value)
{
    if (!c || !key) return fail("nsk_set_tuning: null argument");
    if (!strcmp(key, "frozen_cost")) { if (value < 0 || value > 1000000) return fail("nsk_set_tuning: frozen_cost out of range"); c->tune.frozen_cost = value; return 0; }
    if (!strcmp(key, "frozen_cost_rays")) { if (value < 0 || value > 1000000) return fail("nsk_set_tuning: frozen_cost_rays out of range"); c->tune.frozen_cost_rays = value; return 0; }
    if (!strcmp(key, "no_frozen_kernel")) { c->tune_no_frozen_kernel = value; return 0; }
    if (!strcmp(key, "no_piggyback")) { c->tune_no_piggyback = value; return 0; }
    if (!strcmp(key, "frozen_mid_pct")) { if (value < 10 || value > 1000) return fail("nsk_set_tuning: frozen_mid_pct out of range"); c->tune.frozen_mid_pct = value; return 0; }
    if (!strcmp(key, "no_fused_median")) { c->tune_no_fused_median = value; return 0; }
    if (!strcmp(key, "no_deferred_median")) { c->tune_no_deferred_median = value; return 0; }
    if (!strcmp(key, "fwd_fine_cost")) { if (value < 0 || value > 1000000) return fail("nsk_set_tuning: fwd_fine_cost out of range"); c->tune.fwd_fine_cost = value; return 0; }
    if (!strcmp(key, "fwd_occ_cost")) { if (value < 0 || value > 1000000) return fail("nsk_set_tuning: fwd_occ_cost out of range"); c->tune.fwd_occ_cost = value; return 0; }
    if (!strcmp(key, "no_occ_role")) { c->tune_no_occ_role = value; return 0; }
    if (!strcmp(key, "fwd_color_cost")) { if (value < 0 || value > 1000000) return fail("nsk_set_tuning: fwd_color_cost out of range"); c->tune.fwd_color_cost = value; return 0; }
    if (!strcmp(key, "deterministic")) { c->deterministic = value != 0; return 0; }
    if (!strcmp(key, "no_dead_skip")) { c->tune_no_dead_skip = value; return 0; }
    if (!strcmp(key, "dead_tile_pct")) { if (value < 0 || value > 100) return fail("nsk_set_tuning: dead_tile_pct out of range"); c->tune.dead_tile_pct = value; return 0; }
    if (!strcmp(key, "static_deal")) { c->tune_static_deal = value; return 0; }
    if (!strcmp(key, "deal_head_pct")) { if (value < 0 || value > 100) return fail("nsk_set_tuning: deal_head_pct out of range"); c->tune_deal_head_pct = value; return 0; }
    if (!strcmp(key, "deal_min_rounds")) { if (value < 0) return fail("nsk_set_tuning: deal_min_rounds must be >= 0"); c->tune_deal_min_rounds = value; return 0; }
    if (!strcmp(key, "deal_chunk")) { if (value < 1 || value > 16) return fail("nsk_set_tuning: deal_chunk must be 1 .. 16"); c->tune_deal_chunk = value; return 0; }
    if (!strcmp(key, "roctx")) { c->roctx = value != 0; return 0; }
    if (!strcmp(key, "lattice_slab")) { if (value < 0 || value >= (1 << 26)) return fail("nsk_set_tuning: lattice_slab must be 0 (automatic) or a node count below 2^26"); c->mesh.slab = value; return 0; }
    if (!strcmp(key, "cloud_cells_x4")) { if (value < 1 || value > 256) return fail("nsk_set_tuning: cloud_cells_x4 must be 1 .. 256"); c->cloud.cells_x4 = value; return 0; }
    if (!strcmp(key, "cloud_query_mode")) { if (value < 0 || value > 5) return fail("nsk_set_tuning: cloud_query_mode must be 0 .. 5"); c->cloud.query_mode = value; return 0; }
    if (!strcmp(key, "surface_cells_x4")) { if (value < 1 || value > 256) return fail("nsk_set_tuning: surface_cells_x4 must be 1 .. 256"); c->surface.cells_x4 = value; return 0; }
    if (!strcmp(key, "surface_query_mode")) { if (value != 0 && value != 2 && value != 4) return fail("nsk_set_tuning: surface_query_mode must be 0, 2 or 4 (bit 0 is reserved)"); c->surface.query_mode = value; return 0; }
    if (!strcmp(key, "raster_inline_max")) { if (value < 0) return fail("nsk_set_tuning: raster_inline_max must be >= 0"); c->raster.inline_max = value; return 0; }
    if (!strcmp(key, "raster_queue_cap")) { if (value < 1 || value > (1 << 24)) return fail("nsk_set_tuning: raster_queue_cap must be 1 .. 2^24"); c->raster.queue_cap = value; return 0; }
    if (!strcmp(key, "raster_load_first")) { if (value < 0 || value > 1) return fail("nsk_set_tuning: raster_load_first must be 0 or 1"); c->raster.load_first = value; return 0; }
    return fail("nsk_set_tuning: unknown key '%s'", key);
}

extern "C" int nsk_set_ray_mask(nsk_ctx* c, const uint8_t* d_keep)
{
    if (!c) return fail("null ctx");
    c->ray_mask = d_keep;
    return 0;
}

extern "C" int nsk_set_sort_mode(nsk_ctx* c, int mode)
{
    if (!c) return fail("null ctx");
    if (mode < -1 || mode > 1) return fail("nsk_set_sort_mode: mode must be -1 (automatic), 0 (never) or 1 (always)");
    c->sort_mode = mode;
    return 0;
}

extern "C" int nsk_set_bound(nsk_ctx* c, const float h_bound[6])
{
    if (!c || !h_bound) return fail("nsk_set_bound: null argument");
    for (int k = 0; k < 3; ++k) if (!(h_bound[2 * k + 1] > h_bound[2 * k])) return fail("nsk_set_bound: empty axis %d", k);
    memcpy(c->R.bound, h_bound, 6 * sizeof(float));
    HIPCHK(hipMemcpyAsync(c->d_bound, c->R.bound, 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// the sample counts importance sampling can live with: both passes in one wave, and a first pass with an interior weight
static int importance_fits(const char* who, int n_samples, int n_surface, int n_importance)
{
    if (n_importance == 0) return 0;
    if (n_samples + n_surface + n_importance > 64) return fail("%s: need n_samples+n_surface+n_importance <= 64 (got %d+%d+%d)", who, n_samples, n_surface, n_importance);
    if (n_samples < 3) return fail("%s: n_importance > 0 needs n_samples >= 3 (got %d)", who, n_samples);
    return 0;
}

static int prep_drop(nsk_ctx* c);
extern "C" int nsk_set_importance(nsk_ctx* c, int n_importance)
{
    if (!c) return fail("null ctx");
    if (n_importance < 0) return fail("nsk_set_importance: n_importance must be >= 0 (got %d)", n_importance);
    if (c->capturing) return fail("nsk_set_importance: not while a graph is being captured");
    CHK(importance_fits("nsk_set_importance", c->R.n_samples, c->R.n_surface, n_importance));
    if (n_importance == c->n_importance) return 0;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    CHK(prep_drop(c));                          // a registered or prepared batch was sized for the other sample count
    c->n_importance = n_importance;
    invalidate_graphs(c);                       // the recorded steps have the other launch sequence
    return 0;
}

extern "C" int nsk_get_importance(nsk_ctx* c) { return c ? c->n_importance : -1; }

extern "C" int nsk_set_render_opts(nsk_ctx* c, int n_samples, int n_surface, int lindisp, float perturb, int occupancy, uint64_t seed)
{
    if (!c) return fail("null ctx");
    if (n_samples < 1 || n_surface < 0 || n_samples + n_surface > 64) return fail("nsk_set_render_opts: need 1 <= n_samples, n_samples+n_surface <= 64 (got %d+%d)", n_samples, n_surface);
    CHK(importance_fits("nsk_set_render_opts", n_samples, n_surface, c->n_importance));
    c->R.n_samples = n_samples; c->R.n_surface = n_surface; c->R.lindisp = lindisp ? 1 : 0; c->R.perturb = perturb;
    c->R.occupancy = occupancy ? 1 : 0; c->R.seed = seed;
    return 0;
}

// gradient slab = [grid0..3 | dec0..3 | 4 floats (loss)]
static int rebuild_slab(nsk_ctx* c)
{
    size_t n = 0;
    for (int i = 0; i < 4; ++i) { c->grid[i].g_off = n; n += c->grid[i].n; }
    for (int i = 0; i < 4; ++i) { c->dec[i].g_off = n; n += (size_t)((c->dec[i].n + 3) & ~3); }
    n += 4;
    if (n != c->slab_n) {                  // (a smaller slab is replaced too: every offset in it has moved)
        CHK(grow_begin(c, GROW_STALE_GRAPHS));
        c->slab_n = 0;
        CHK(dev_alloc(c->slab, n, "the gradient slab"));
        c->slab_n = n;
    }
    HIPCHK(hipMemsetAsync(c->slab, 0, n * sizeof(float), c->stream));
    return 0;
}

static int grid_upload(nsk_ctx* c, GridState& G, const float* h, int C, int Z, int Y, int X)
{
    size_t nvox = (size_t)Z * Y * X, n = nvox * 32;
    bool realloc_ = n != G.n;
    if (realloc_) {
        CHK(grow_begin(c, GROW_STALE_GRAPHS));
        G = GridState();
        CHK(dev_alloc(G.v, n, "a grid level")); CHK(dev_alloc(G.m, n, "a grid level's first moment")); CHK(dev_alloc(G.s, n, "a grid level's second moment"));
    }
    if (G.Z != Z || G.Y != Y || G.X != X) { if (G.mask) { CHK(grow_begin(c, GROW_STALE_GRAPHS)); G.mask.reset(); } }
    G.C = C; G.Z = Z; G.Y = Y; G.X = X; G.n = n; G.midx_dirty = true; G.live_dirty = true; ++c->live_epoch;
    std::vector<float> t(n);
    for (int ch = 0; ch < 32; ++ch)
        for (size_t v = 0; v < nvox; ++v) t[v * 32 + ch] = h[(size_t)ch * nvox + v];
    HIPCHK(hipMemcpyAsync(G.v, t.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(G.m, 0, n * 4, c->stream));
    HIPCHK(hipMemsetAsync(G.s, 0, n * 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (realloc_) CHK(rebuild_slab(c));
    return 0;
}
extern "C" int nsk_grid_upload(nsk_ctx* c, int level, const float* h, int C, int Z, int Y, int X)
{
    if (!c || !h) return fail("nsk_grid_upload: null argument");
    if (!which_ok(level)) return fail("nsk_grid_upload: bad level %d", level);
    if (C != 32) return fail("nsk_grid_upload: C must be 32 (got %d)", C);
    if (Z < 1 || Y < 1 || X < 1) return fail("nsk_grid_upload: bad shape");
    if ((size_t)Z * Y * X >= ((size_t)1 << 25)) return fail("nsk_grid_upload: at most 2^25 - 1 voxels per level (32-bit byte offsets in the forward's gather: 128 B per voxel)");
    HIPCHK(hipSetDevice(c->device));
    GridState& G = c->grid[level];
    const bool fresh = (size_t)Z * Y * X * 32 != G.n;
    const int r = grid_upload(c, G, h, C, Z, Y, X);
    // a level that was being (re)allocated when something failed is left unloaded: check_stage asks for it, a retry allocates again
    if (r != 0 && fresh) { invalidate_graphs(c); G = GridState(); }
    return r;
}

static int grid_fetch(nsk_ctx* c, int level, const float* src, float* h)
{
    GridState& G = c->grid[level];
    if (!G.n) return fail("grid level %d not uploaded", level);
    std::vector<float> t(G.n);
    HIPCHK(hipMemcpyAsync(t.data(), src, G.n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    size_t nvox = G.n / 32;
    for (int ch = 0; ch < 32; ++ch)
        for (size_t v = 0; v < nvox; ++v) h[(size_t)ch * nvox + v] = t[v * 32 + ch];
    return 0;
}
extern "C" int nsk_grid_download(nsk_ctx* c, int level, float* h)
{
    if (!c || !h || !which_ok(level)) return fail("nsk_grid_download: bad argument");
    return grid_fetch(c, level, c->grid[level].v, h);
}
extern "C" int nsk_grid_grad_download(nsk_ctx* c, int level, float* h)
{
    if (!c || !h || !which_ok(level)) return fail("nsk_grid_grad_download: bad argument");
    CHK(grid_fetch(c, level, c->slab + c->grid[level].g_off, h));
    GridState& G = c->grid[level];
    if (G.mask) {                                   // "gradients of unmarked voxels are discarded": what the scatter left there is not a gradient
        const size_t nvox = G.n / 32;
        std::vector<uint8_t> m(nvox);
        HIPCHK(hipMemcpy(m.data(), G.mask, nvox, hipMemcpyDeviceToHost));
        for (int ch = 0; ch < 32; ++ch)
            for (size_t v = 0; v < nvox; ++v) if (!m[v]) h[(size_t)ch * nvox + v] = 0.f;
    }
    return 0;
}

extern "C" int nsk_set_mask(nsk_ctx* c, int level, const uint8_t* h_mask)
{
    if (!c || !which_ok(level)) return fail("nsk_set_mask: bad argument");
    GridState& G = c->grid[level];
    if (!G.n) return fail("nsk_set_mask: grid level %d not uploaded", level);
    if (c->capturing) return fail("nsk_set_mask: not while a graph is being captured");
    HIPCHK(hipStreamSynchronize(c->stream));
    size_t nvox = G.n / 32;
    G.midx_dirty = true; G.live_dirty = true; ++c->live_epoch;
    // A captured step holds the level's voxel list as kernel arguments (its pointer, its length and the block ranges derived from it:
    // k_adam_multi, k_xchg_multi): new mask CONTENTS make every recorded graph wrong, not only a new allocation.
    invalidate_graphs(c);
    // Unmarked voxels are never visited by the optimiser, so whatever the scatter added to their gradient stays there: a voxel that
    // becomes marked now must not inherit it.  The level's gradient is cleared whenever its mask changes.
    if (c->slab) HIPCHK(hipMemsetAsync(c->slab + G.g_off, 0, G.n * 4, c->stream));
    if (!h_mask) { G.mask.reset(); return 0; }
    if (!G.mask) CHK(dev_alloc(G.mask, nvox, "the voxel mask"));
    HIPCHK(hipMemcpy(G.mask, h_mask, nvox, hipMemcpyHostToDevice));
    return 0;
}

// ---- decoder images -------------------------------------------------------------------------------------
// One image from the parameters (tables and sizes: nsk_images.h): the fragments through its table, the fp32 tail through the sibling's.  The
// forward image in pieces takes its piece count from the matmul mode: 2 fp16 under mode 2, 3 bf16 under modes 0 and 1 (mode 0 reads the fp32
// image; the 3-piece one is kept so that a switch to mode 1 changes no layout).
static int pack_image(nsk_ctx* c, DecState& D, int what)
{
    DecImage& I = D.img[what];
    if (!I.data) return 0;
    if (what == 2) I.spec = with_pieces(I.spec, c->matmul_mode == 2 ? 2 : 3);
    const ImageSpec& s = I.spec;
    if (s.pieces) k_pack_bf16<<<(s.entries + 255) / 256, 256, 0, c->stream>>>(reinterpret_cast<unsigned short*>(I.data.get()), I.idx, D.p, s.entries, s.pieces);
    else k_pack<<<(s.entries + 255) / 256, 256, 0, c->stream>>>(I.data, I.idx, D.p, s.entries);
    if (s.tail_n) k_pack<<<(s.tail_n + 255) / 256, 256, 0, c->stream>>>(I.data + s.tail_off, D.img[what - 2].idx + s.sib_off, D.p, s.tail_n);
    HIPCHK(hipGetLastError());
    I.dirty = false;
    return 0;
}

// the fp16 backward image follows the parameters lazily: marked stale by uploads, rebuilt before use (the optimiser launch rewrites it in place)
static int ensure_image(nsk_ctx* c, int w, int what)
{
    if (!c->dec[w].img[what].dirty) return 0;
    ProfScope ps(c, "pack_bwd_bf16");
    return pack_image(c, c->dec[w], what);
}

static int repack(nsk_ctx* c, int w)
{
    DecState& D = c->dec[w];
    ProfScope ps(c, "pack_images");
    for (int what = 0; what < 3; ++what) CHK(pack_image(c, D, what));
    D.img[3].dirty = (bool)D.img[3].data;
    return 0;
}

static int flush_pending(nsk_ctx* c);
static int ensure_midx(nsk_ctx* c, int l);
static void adam_consts(float lr, float b1, float b2, int step, float& step_size, float& bc2s);

extern "C" size_t nsk_decoder_param_count(int which) { return which_ok(which) ? (size_t)nsk_dec_layout(which).total : 0; }

// one-time setup of a decoder: parameters, moments, fragment images and their index tables, into a DecState of its own
static int dec_setup(int w, size_t n, DecState& D)
{
    const size_t n4 = (n + 3) & ~(size_t)3;
    auto table = [](Buf<int>& d, const std::vector<int>& h, const char* what) -> int {
        CHK(dev_alloc(d, h.size(), what));
        HIPCHK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        return 0;
    };
    CHK(dev_alloc(D.p, n4, "a decoder's parameters")); CHK(dev_alloc(D.m, n4, "a decoder's first moment")); CHK(dev_alloc(D.s, n4, "a decoder's second moment"));
    HIPCHK(hipMemset(D.p, 0, n4 * 4));
    static const char* const names[NSK_NUM_IMAGES] = {"forward", "backward", "forward in pieces", "fp16 backward"};
    std::vector<int> idx, inv;
    for (int what = 0; what < NSK_NUM_IMAGES; ++what) {
        DecImage& I = D.img[what];
        I.spec = image_spec(w, what, 3);          // the forward image in pieces is allocated for its larger (3-piece) form
        if (!I.spec.floats) continue;
        build_image_table(w, what, idx);
        CHK(dev_alloc(I.data, (size_t)I.spec.floats, "a decoder's image"));
        if (I.spec.pieces) HIPCHK(hipMemset(I.data, 0, (size_t)I.spec.floats * 4));
        CHK(table(I.idx, idx, "a decoder's index table"));
        const int twice = invert_table(idx, n4, inv);      // image position of each canonical parameter (-1 none)
        if (twice >= 0) return fail("decoder %d: parameter %d appears twice in the %s image", w, twice, names[what]);
        CHK(table(I.inv, inv, "a decoder's inverse index table"));
    }
    D.n = (int)n;
    return 0;
}

extern "C" int nsk_decoder_upload(nsk_ctx* c, int w, const float* h, size_t n)
{
    if (!c || !h || !which_ok(w)) return fail("nsk_decoder_upload: bad argument");
    if (n != nsk_decoder_param_count(w)) return fail("nsk_decoder_upload: decoder %d expects %zu parameters, got %zu", w, nsk_decoder_param_count(w), n);
    HIPCHK(hipSetDevice(c->device));
    DecState& D = c->dec[w];
    if (!D.n) {                 // never set up: the setup completes (and only then replaces D) or leaves the decoder as never uploaded
        DecState fresh;
        fresh.trainable = D.trainable;
        CHK(dec_setup(w, n, fresh));
        D = std::move(fresh);
        const int r = rebuild_slab(c);
        if (r != 0) { const int t = D.trainable; D = DecState(); D.trainable = t; return r; }
    }
    HIPCHK(hipMemcpyAsync(D.p, h, n * 4, hipMemcpyHostToDevice, c->stream));
    size_t n4 = (n + 3) & ~(size_t)3;
    HIPCHK(hipMemsetAsync(D.m, 0, n4 * 4, c->stream));
    HIPCHK(hipMemsetAsync(D.s, 0, n4 * 4, c->stream));
    CHK(repack(c, w));
    HIPCHK(hipStreamSynchronize(c->stream));
    D.loaded = true;
    return 0;
}

static int dec_fetch(nsk_ctx* c, int w, const float* src, float* h, size_t n)
{
    if (!c->dec[w].loaded) return fail("decoder %d not uploaded", w);
    if (n != (size_t)c->dec[w].n) return fail("decoder %d has %d parameters, buffer has %zu", w, c->dec[w].n, n);
    HIPCHK(hipMemcpyAsync(h, src, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int nsk_decoder_download(nsk_ctx* c, int w, float* h, size_t n)
{
    if (!c || !h || !which_ok(w)) return fail("nsk_decoder_download: bad argument");
    return dec_fetch(c, w, c->dec[w].p, h, n);
}
extern "C" int nsk_decoder_grad_download(nsk_ctx* c, int w, float* h, size_t n)
{
    if (!c || !h || !which_ok(w)) return fail("nsk_decoder_grad_download: bad argument");
    CHK(flush_pending(c));
    return dec_fetch(c, w, c->slab + c->dec[w].g_off, h, n);
}
extern "C" int nsk_decoder_set_trainable(nsk_ctx* c, int w, int t)
{
    if (!c || !which_ok(w)) return fail("nsk_decoder_set_trainable: bad argument");
    c->dec[w].trainable = t ? 1 : 0;
    return 0;
}

// ---- workspace --------------------------------------------------------------------------------------------
static int prep_drop(nsk_ctx* c);
static int ensure_ws(nsk_ctx* c, int N, int M)
{
    Workspace& w = c->ws;
    if (M <= w.capM && N <= w.capN) return 0;
    CHK(grow_begin(c, GROW_NO_CAPTURE | GROW_STALE_GRAPHS));
    CHK(prep_drop(c));
    const int capM = std::max(M, w.capM), capN = std::max(N, w.capN);
    w = Workspace();             // everything, the histogram, the saved block outputs and both sampling sets included
    const size_t m = (size_t)capM + 64, n = (size_t)capN + 64, slabs = (size_t)c->num_cu * 20920;
    const int r = [&]() -> int {
        CHK(alloc_samples(w.cur, m));
        for (int i = 0; i < 3; ++i) CHK(dev_alloc(w.occ[i], m, "the occupancies"));
        CHK(dev_alloc(w.rgb4, m * 4, "the colours"));
        for (int i = 0; i < 4; ++i) CHK(dev_alloc(w.masks[i], m * 4, "the ReLU bits"));
        CHK(dev_alloc(w.g_raw, m * 4, "the sample gradients"));
        CHK(dev_alloc(w.ray_loss, n, "the ray losses"));
        CHK(dev_alloc(w.tmp_rgb, n * 3, "the ray colours")); CHK(dev_alloc(w.tmp_depth, n, "the ray depths"));
        CHK(dev_alloc(w.dec_slabs, slabs, "the decoder gradient slabs"));
        HIPCHK(hipMemsetAsync(w.dec_slabs, 0, slabs * 4, c->stream));
        return 0;
    }();
    if (r != 0) { w = Workspace(); return r; }
    w.capM = capM; w.capN = capN;
    return 0;
}

// histogram / offsets of the cell sort: one bin per cell of the key level
static int ensure_hist(nsk_ctx* c, size_t bins)
{
    Workspace& w = c->ws;
    if (bins <= w.cur.offs.cap()) return 0;
    CHK(grow_begin(c, GROW_NO_CAPTURE | GROW_STALE_GRAPHS));
    c->prep.valid = false; c->req.valid = false;       // (the histogram is replaced: nothing to clean)
    const size_t slots = ((bins / 8 + 1) / 2) * 16 + 16;    // hist_slot() layout (bins = 8 keys per cell) + one 64-byte line in front (Workspace::hist)
    const int r = [&]() -> int {
        CHK(dev_alloc(w.hist_raw, slots, "the cell histogram")); CHK(dev_alloc(w.cur.offs, bins, "the cell offsets"));
        HIPCHK(hipMemsetAsync(w.hist_raw, 0, slots * 4, c->stream));
        return 0;
    }();
    if (r != 0) reset_all(w.hist_raw, w.cur.offs);
    return r;
}

// the forward of a trainable decoder (all but the fine one, see nsk_train.h) also stores its block outputs for the backward
static bool saves_h(nsk_ctx* c, int w, bool save_masks) { return save_masks && w != 2 && c->dec[w].trainable; }

static const int STAGE_DEC[4][3] = {{0, -1, -1}, {1, -1, -1}, {1, 2, -1}, {1, 2, 3}};

static GridD grid_dev(nsk_ctx* c, int level, bool with_grad)
{
    GridD g;
    GridState& G = c->grid[level];
    g.v = G.v; g.g = with_grad ? c->slab + G.g_off : nullptr; g.mask = G.mask; g.Z = G.Z; g.Y = G.Y; g.X = G.X;
    return g;
}

static int check_stage(nsk_ctx* c, int stage)
{
    if (stage < 0 || stage > 3) return fail("bad stage %d", stage);
    for (int q = 0; q < 3; ++q) {
        int w = STAGE_DEC[stage][q];
        if (w < 0) break;
        if (!c->grid[w].n) return fail("stage %d needs grid level %d (nsk_grid_upload)", stage, w);
        if (!c->dec[w].loaded) return fail("stage %d needs decoder %d (nsk_decoder_upload)", stage, w);
    }
    if (!c->slab) return fail("the gradient slab is not allocated (its last allocation failed: upload a grid level or a decoder again)");
    return 0;
}

static void fill_args(nsk_ctx* c, DecArgs& A, int w, int M, int S, const float* ro, const float* rd, const float* pts)
{
    memset(&A, 0, sizeof(A));
    A.rays_o = ro; A.rays_d = rd; A.z = c->ws.cur.z; A.pts = pts; A.M = M; A.S = S; A.S_magic = S > 1 ? (unsigned)((0x100000000ull + (unsigned)S - 1) / (unsigned)S) : 0u;
    A.perm = (c->sorted && !pts) ? c->ws.cur.perm : nullptr;
    memcpy(A.bound, c->R.bound, sizeof(A.bound));
    A.grid = grid_dev(c, w, false);
    if (w == 2) A.grid_mid = grid_dev(c, 1, false);
    const DecImage* I = c->dec[w].img;
    A.img = reinterpret_cast<const f4*>(I[0].data.get());
    A.bimg = reinterpret_cast<const f4*>(I[1].data.get());
    A.img_f4 = I[0].spec.floats / 4;
    A.img16 = I[2].data;
    A.bimg16 = I[3].data;
    A.out = w == 3 ? c->ws.rgb4 : c->ws.occ[w];
}

// one decoder of a forward launch: its arguments, the ReLU masks and (trainable, see saves_h) the block outputs kept for the backward
static int fill_fwd_role(nsk_ctx* c, DecArgs& A, int w, int M, int S, const float* ro, const float* rd, const float* pts, bool save_masks)
{
    fill_args(c, A, w, M, S, ro, rd, pts);
    A.masks = save_masks ? c->ws.masks[w] : nullptr;
    if (save_masks) c->ws.hsave_M[w] = 0;
    if (saves_h(c, w, save_masks)) {
        CHK(grow(c, c->ws.hsave[w], ((size_t)(M + 15) / 16 + 1) * 10 * 64, "the saved block outputs", GROW_NO_CAPTURE | GROW_STALE_GRAPHS));
        A.hsave = c->ws.hsave[w]; c->ws.hsave_M[w] = M;
    }
    return 0;
}

// nsk_debug_last_split: what the launch that is about to go out looks like (dir 0 forward, 1 backward; layout: include/nsk.h)
static void record_split(nsk_ctx* c, int dir, int form, int n, const int* which, const int* train, const int* wg_end, int scan_wgs, int loss_wg,
                         int ntasks, int grid)
{
    int* d = c->dbg_split[dir];
    memset(d, 0, sizeof(c->dbg_split[dir]));
    d[0] = form; d[1] = n;
    for (int r = 0; r < n && r < 3; ++r) { d[2 + r] = which[r]; d[5 + r] = train ? train[r] : 0; d[8 + r] = wg_end ? role_wgs(wg_end, r) : grid; }
    d[11] = scan_wgs; d[12] = loss_wg; d[13] = ntasks; d[14] = grid;
}

static int launch_decode_fwd(nsk_ctx* c, int w, int M, int S, const float* ro, const float* rd, const float* pts, bool save_masks)
{
    DecArgs A;
    CHK(fill_fwd_role(c, A, w, M, S, ro, rd, pts, save_masks));
    int ntasks = (M + 15) / 16;
    size_t lds = fwd_img_floats(w) * 4;
    int maxwg = c->num_cu;        // persistent: one workgroup per CU balances the 16-sample tasks over SIMDs
    int grid = std::max(1, std::min((ntasks + 7) / 8, maxwg));
    static const char* names[4] = {"decode_fwd_coarse", "decode_fwd_middle", "decode_fwd_fine", "decode_fwd_color"};
    record_split(c, 0, NSK_SPLIT_FWD_SINGLE, 1, &w, nullptr, nullptr, 0, 0, ntasks, grid);
    ProfScope ps(c, names[w]);
    switch (w) {
    case 0: k_decode_fwd<0><<<grid, 512, lds, c->stream>>>(A); break;
    case 1: k_decode_fwd<1><<<grid, 512, lds, c->stream>>>(A); break;
    case 2: k_decode_fwd<2><<<grid, 512, lds, c->stream>>>(A); break;
    default: k_decode_fwd<3><<<grid, 512, lds, c->stream>>>(A); break;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// one decoder of a backward launch: what every launch form gives it (flags and the Tracker's deferred mask stay with the callers)
static int fill_bwd_role(nsk_ctx* c, DecArgs& A, int w, int M, int S, const float* ro, const float* rd, bool train, bool grids, float* g_ro, float* g_rd)
{
    fill_args(c, A, w, M, S, ro, rd, nullptr);
    A.grid = grid_dev(c, w, grids);
    A.masks = c->ws.masks[w];
    A.g_raw = c->ws.g_raw;
    A.g_rays_o = g_ro; A.g_rays_d = g_rd;
    A.g_dec = train ? c->ws.dec_slabs : c->slab + c->dec[w].g_off;
    if (w != 0 && (!train || w != 2)) CHK(ensure_image(c, w, 3));      // the chains on fp16 pieces: every frozen MLP decoder, trainable middle / colour
    if (train && w != 2) {
        if (c->ws.hsave_M[w] != M) return fail("backward of trainable decoder %d: its forward must run with the decoder already trainable (block outputs not saved)", w);
        A.hsave = c->ws.hsave[w];
    }
    return 0;
}

static int launch_decode_bwd(nsk_ctx* c, int w, int M, int S, const float* ro, const float* rd, bool train, bool rays, unsigned flags,
                             float* g_ro, float* g_rd)
{
    DecArgs A;
    CHK(fill_bwd_role(c, A, w, M, S, ro, rd, train, (flags & NSK_GRAD_GRIDS) != 0, g_ro, g_rd));
    A.flags = flags;
    int ntasks = (M + 15) / 16;
    size_t lds = bwd_lds_bytes(w, train);
    const int grid = bwd_separate_grid(c->num_cu, ntasks, c->deterministic != 0);
    if (c->deterministic) A.flags |= 0x8000u;      // one workgroup, its waves scatter one after the other
    static const char* names[8] = {"decode_bwd_coarse", "decode_bwd_middle", "decode_bwd_fine", "decode_bwd_color",
                                   "decode_bwd_coarse_train", "decode_bwd_middle_train", "decode_bwd_fine_train", "decode_bwd_color_train"};
    {
    ProfScope ps(c, names[w + (train ? 4 : 0)]);
#define LB(W) \
    if (train) { if (rays) k_decode_bwd_train<W, true><<<grid, 512, lds, c->stream>>>(A); else k_decode_bwd_train<W, false><<<grid, 512, lds, c->stream>>>(A); } \
    else { if (rays) k_decode_bwd<W, true><<<grid, 512, lds, c->stream>>>(A); else k_decode_bwd<W, false><<<grid, 512, lds, c->stream>>>(A); }
    switch (w) {
    case 0: LB(0) break;
    case 1: LB(1) break;
    case 2: LB(2) break;
    default: LB(3) break;
    }
#undef LB
    }
    HIPCHK(hipGetLastError());
    if (train) {
        int n = c->dec[w].n, n4 = (n + 3) & ~3;
        ProfScope ps2(c, "dec_grad_reduce");
        k_dec_grad_reduce<<<dim3((n + 255) / 256, 8), 256, 0, c->stream>>>(n, n4, grid, c->ws.dec_slabs, c->slab + c->dec[w].g_off);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// all decoders of the stage in ONE launch (workgroup roles), or a plain launch when the stage has one decoder
static int launch_decode_fwd_stage(nsk_ctx* c, int stage, int M, int S, const float* ro, const float* rd, bool save_masks)
{
    int n = 0;
    for (int q = 0; q < 3; ++q) if (STAGE_DEC[stage][q] >= 0) ++n;
    if (n == 1) return launch_decode_fwd(c, STAGE_DEC[stage][0], M, S, ro, rd, nullptr, save_masks);
    const int ntasks = (M + 15) / 16;
    MultiArgs MA;
    memset(&MA, 0, sizeof(MA));
    size_t lds = 0;
    for (int r = 0; r < n; ++r) {
        const int w = STAGE_DEC[stage][r];
        CHK(fill_fwd_role(c, MA.a[r], w, M, S, ro, rd, nullptr, save_masks));
        MA.which[r] = w;
        lds = std::max(lds, fwd_img_floats(w) * 4);
    }
    // middle + fine as ONE role (decode_fwd_occ_body: the middle level looked up once): frozen occupancy decoders on two-piece operands, neither
    // keeping block outputs (the merged body stores none); which form runs, and its split: plan_fwd (nsk_split.h)
    const bool can_merge = c->matmul_mode == 2 && STAGE_DEC[stage][0] == 1 && STAGE_DEC[stage][1] == 2 && !saves_h(c, 1, save_masks) && !saves_h(c, 2, save_masks);
    const FwdPlan P = plan_fwd(c->num_cu, ntasks, STAGE_DEC[stage][2] == 3, c->tune, can_merge ? c->tune_no_occ_role : 1);
    MA.n = P.n;
    memcpy(MA.wg_end, P.wg_end, sizeof(P.wg_end));
    {
        const int merged_which[2] = {1, 3};      // the merged role reports as the middle decoder's
        record_split(c, 0, P.merged ? NSK_SPLIT_FWD_MERGED : (c->matmul_mode != 0 ? NSK_SPLIT_FWD_MULTI_SPLIT : NSK_SPLIT_FWD_MULTI), P.n,
                     P.merged ? merged_which : MA.which, nullptr, MA.wg_end, 0, 0, ntasks, MA.wg_end[P.n - 1]);
    }
    ProfScope ps(c, "decode_fwd_multi");
    if (P.merged) {
        size_t lds_occ = ((size_t)c->dec[1].img[2].spec.floats + (size_t)c->dec[2].img[2].spec.floats) * 4;
        if (n == 3) lds_occ = std::max(lds_occ, (size_t)c->dec[3].img[2].spec.floats * 4);
        k_decode_fwd_multi_occ<8><<<MA.wg_end[MA.n - 1], 512, lds_occ, c->stream>>>(MA);
    } else if (c->matmul_mode != 0) {
        size_t lds16 = 0;
        for (int r = 0; r < n; ++r) lds16 = std::max(lds16, MA.which[r] == 0 ? fwd_img_floats(0) * 4 : (size_t)c->dec[MA.which[r]].img[2].spec.floats * 4);
        if (c->matmul_mode == 2) k_decode_fwd_multi_bf16<8, 2><<<MA.wg_end[n - 1], 512, lds16, c->stream>>>(MA);
        else k_decode_fwd_multi_bf16<8><<<MA.wg_end[n - 1], 512, lds16, c->stream>>>(MA);       // 12 waves (168 VGPRs) spill: 59 -> 71 us (the two-piece form at 12 waves: 50 spilled registers, K3 forward 139 -> 202 us, round 4)
    } else
    k_decode_fwd_multi<<<MA.wg_end[n - 1], 512, lds, c->stream>>>(MA);
    HIPCHK(hipGetLastError());
    return 0;
}

// importance sampling: the samples of the first pass behind a batch of N rays with S samples each in the second (forward_core's M1); 0 without
static int first_pass_samples(const nsk_ctx* c, int N, int S) { return c->n_importance > 0 ? N * (S - c->n_importance) : 0; }

// algorithmic bytes / flops per sample; M1 > 0: a first pass of M1 samples, a forward, went before the M counted here
static void account(nsk_ctx* c, int stage, int M, int M1, bool bwd, unsigned flags)
{
    static const double fwd_b[4] = {1024, 1024, 2048, 3072}, fwd_f[4] = {12.4e3, 31.0e3, 72.2e3, 103.3e3};
    double b = fwd_b[stage] + 5.0, f = fwd_f[stage];
    if (bwd) {
        int lv = stage == 0 ? 1 : stage;      // levels receiving gradient
        if (flags & NSK_GRAD_GRIDS) b += 2048.0 * lv;
        f *= 2.0;
        if (flags & NSK_GRAD_DECODERS) for (int q = 0; q < 3; ++q) { int w = STAGE_DEC[stage][q]; if (w >= 0 && c->dec[w].trainable) f += 2.0 * (w == 0 ? 6176 : (w == 2 ? 20599 : 15500)); }
    }
    c->last_bytes = b * M; c->last_flops = f * M; c->last_samples = M;
    if (M1 > 0) { c->last_bytes += (fwd_b[stage] + 5.0) * M1; c->last_flops += fwd_f[stage] * M1; c->last_samples += M1; }
}

// sampling + decoders of the stage; leaves z / occ / rgb4 (and ReLU bits) in the workspace
// The cell sort pays when the step scatters into the grids and does not need per-ray gradient sums (those rely on a tile's 16
// samples sharing a ray: the Tracker and bundle adjustment keep the ray order)
static bool sort_pays(nsk_ctx* c, int stage, int M, unsigned flags)
{
    if (c->deterministic) return false;          // (the cell sort's ranks come from atomics in arrival order)
    if (c->sort_mode >= 0) return c->sort_mode == 1;
    if (!(flags & NSK_GRAD_GRIDS)) return false;             // (the Tracker: 200 rays, no scatter)
    // Bundle adjustment (grids + rays): in cell order a tile's 16 samples belong to 16 rays, so the ray-gradient sums go lane by lane instead of
    // one add per tile -- and the scatter still wins: per-role stamps at 1000 / 5000 rays 168 -> 136 us / 742 -> 432 us.
    // Measured (tools/exp_sort_threshold.py, host_test): on the reference's grids (41 k fine cells) the two extra launches pay from ~300
    // rays x 48 on (200 rays: 92 us in ray order, 97 us sorted; 1000 rays: 236 against 162 us); on a small grid (792 cells, 9600 samples)
    // many samples share the few cells, ray order serialises their atomics and sorting wins much earlier (118 against 102 us).
    int key_level = 0;
    for (int q = 0; q < 3; ++q) if (STAGE_DEC[stage][q] >= 0) key_level = std::max(key_level, STAGE_DEC[stage][q] == 3 ? 3 : STAGE_DEC[stage][q]);
    const long cells = (long)(c->grid[key_level].n / 32);
    return M >= 14336 || (cells > 0 && (long)M >= 4 * cells);
}

// sorted: the decoders of this step (forward and the backward that follows) walk the samples cell by cell (see k_sample)
static int stage_key_level(int stage)
{
    int key_level = 0;
    for (int q = 0; q < 3; ++q) if (STAGE_DEC[stage][q] >= 0) key_level = STAGE_DEC[stage][q];      // the finest level the stage reads
    return key_level;
}
// ---- liveness bytes for the backward's dead-tile skip -------------------------------------------------------------------------------------
// A step that forms a loss writes them with its sampling when a level its decoders read carries an optimiser mask; no mask, the deterministic
// mode or nsk_set_tuning("no_dead_skip", 1): none are written and the backward runs every tile through the body it always had.
static bool live_wanted(nsk_ctx* c, int stage, bool save_masks)
{
    if (!save_masks || c->tune_no_dead_skip || c->deterministic) return false;
    for (int q = 0; q < 3; ++q) { const int w = STAGE_DEC[stage][q]; if (w >= 1 && c->grid[w].mask) return true; }
    return false;
}
static int ensure_live(nsk_ctx* c, int l)
{
    GridState& G = c->grid[l];
    if (!G.mask || !G.live_dirty) return 0;
    if (c->capturing) return fail("graph capture: a mask changed since the last eager step (run the step once after installing masks, then capture)");
    const size_t nvox = G.n / 32;
    CHK(grow(c, G.live, nvox, "the live-cell table", GROW_STALE_GRAPHS));
    k_cell_live<<<(int)((nvox + 255) / 256), 256, 0, c->stream>>>(G.X, G.Y, G.Z, G.mask, G.live);
    HIPCHK(hipGetLastError());
    G.live_dirty = false;
    return 0;
}
static int ensure_live_stage(nsk_ctx* c, int stage)
{
    for (int q = 0; q < 3; ++q) { const int w = STAGE_DEC[stage][q]; if (w >= 1) CHK(ensure_live(c, w)); }
    return 0;
}
static void live_args(nsk_ctx* c, LiveArgs& L, int stage, uint8_t* out)
{
    memset(&L, 0, sizeof(L));
    L.out = out;
    if (!out) return;
    const int key = stage_key_level(stage);
    const GridState& KG = c->grid[key];
    for (int q = 0; q < 3; ++q) {
        const int w = STAGE_DEC[stage][q];
        if (w < 1) continue;
        const GridState& G = c->grid[w];
        if (!G.mask || G.live_dirty) continue;       // no mask on the level: its bit is always set
        const int k = w - 1;
        L.lv[k] = G.live; L.X[k] = G.X; L.Y[k] = G.Y; L.Z[k] = G.Z;
        L.src[k] = (w == key || (G.X == KG.X && G.Y == KG.Y && G.Z == KG.Z)) ? 0 : ((w == 1 && stage >= 2) ? 1 : 2);
    }
}

static void samp_args(nsk_ctx* c, SampArgs& A, const RParams& R, int stage, int N, int S, const float* ro, const float* rd, const float* gt, float gtmax,
                      const float* gmax_dev, const uint8_t* mask, bool sorted, const SampleSet& out, bool live, const nsk_ctx::DMax& dm)      // live: also the liveness bytes (live_wanted)
{
    const GridState& KG = c->grid[stage_key_level(stage)];
    const GridState* PG = stage >= 2 ? &c->grid[1] : nullptr;      // parent level whose cells order the samples inside a key cell (k_sample)
    const size_t bins = KG.n / 32 * 8;
    memset(&A, 0, sizeof(A));
    A.R = R; A.N = N; A.S = S; A.rays_o = ro; A.rays_d = rd; A.gt_depth = gt; A.gtmax_host = gtmax; A.gtmax_dev = gmax_dev; A.keep = mask; A.z_out = out.z;
    A.kX = KG.X; A.kY = KG.Y; A.kZ = KG.Z; A.pX = PG ? PG->X : 0; A.pY = PG ? PG->Y : 0; A.pZ = PG ? PG->Z : 0; A.ncell2 = (int)((bins / 8 + 1) / 2);
    A.skey = sorted ? out.skey.get() : nullptr; A.srank = out.srank; A.hist = c->ws.hist();
    if (dm.n > 0) { A.mx_gt = dm.gt; A.mx_keep = dm.keep; A.mx_n = dm.n; } else { A.mx_gt = gt; A.mx_keep = mask; A.mx_n = N; }
    live_args(c, A.L, stage, out.live_out(live));
}
// halves: 256-cell chunks per workgroup (1: k_sort_scan, 2: the role inside k_decode_bwd_multi)
static ScanArgs scan_args(nsk_ctx* c, int stage, const SampleSet& out, int halves)
{
    const size_t bins = c->grid[stage_key_level(stage)].n / 32 * 8;
    ScanArgs A; A.nkeys = (int)bins; A.ncell2 = (int)((bins / 8 + 1) / 2); A.hist = c->ws.hist(); A.offs = out.offs;
    A.nblocks = (int)((bins + 2048 * (size_t)halves - 1) / (2048 * (size_t)halves));
    return A;
}
static PlaceArgs place_args(int M, const SampleSet& out, bool live)      // live: the sampling wrote liveness bytes; they are re-ordered with the samples
{
    PlaceArgs A; A.M = M; A.skey = out.skey; A.srank = out.srank; A.offs = out.offs; A.perm = out.perm; A.nblocks = (M + 255) / 256;
    A.live_in = out.live_out(live); A.live_out = live ? out.lslot.get() : nullptr;
    return A;
}
// the batch maximum of gt_depth has to come from a launch of its own (k_sample's waves take it themselves for smaller batches)
static bool needs_depth_max(const float* gt, float gtmax, int N, const nsk_ctx::DMax& dm) { return gt && gtmax < 0.f && (dm.n > 0 ? dm.n : N) > 8192; }

// sampling (+ cell sort) of one batch into the set `out` by launches of its own; live: also the liveness bytes (live_wanted), by sample and,
// sorted, by slot; done: what has already run (a prepared batch's riders)
static int launch_sampling(nsk_ctx* c, const RParams& R, int stage, int N, int S, const float* ro, const float* rd, const float* gt, float gtmax,
                           const uint8_t* mask, bool sorted, const SampleSet& out, bool live, const nsk_ctx::DMax& dm, PrepDone done = PREP_NOTHING)
{
    const int M = N * S;
    hipStream_t st = c->stream;
    if (done < PREP_SAMPLED) {
        const float* gmax_dev = nullptr;
        if (needs_depth_max(gt, gtmax, N, dm)) {
            ProfScope ps(c, "depth_max");
            if (dm.n > 0) k_depth_max<<<1, 1024, 0, st>>>(dm.n, dm.gt, dm.keep, c->scal);      // the maximum of the batch this call's rays are a shard of
            else k_depth_max<<<1, 1024, 0, st>>>(N, gt, mask, c->scal);
            gmax_dev = c->scal;
        }
        ProfScope ps(c, "sample");
        SampArgs A;
        samp_args(c, A, R, stage, N, S, ro, rd, gt, gtmax, gmax_dev, mask, sorted, out, live, dm);
        k_sample<<<(N + NSK_SAMPLE_RAYS - 1) / NSK_SAMPLE_RAYS, 64 * NSK_SAMPLE_RAYS, 0, st>>>(A);
    }
    if (sorted && done < PREP_PLACED) {
        ProfScope ps(c, "cell_sort");
        if (done < PREP_SCANNED) { const ScanArgs A = scan_args(c, stage, out, 1); k_sort_scan<<<A.nblocks, 256, 0, st>>>(A); }
        const PlaceArgs A = place_args(M, out, live); k_sort_place<<<A.nblocks, 256, 0, st>>>(A);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static size_t stage_bins(nsk_ctx* c, int stage) { return c->grid[stage_key_level(stage)].n / 32 * 8; }

// ---- the life of a prepared batch (nsk_map_prepare) ---------------------------------------------------------------------------------------
// nsk_map_prepare registers the NEXT batch as c->req and launches nothing.  The nsk_map_step that follows promotes it to c->prep, the batch whose
// outputs are built in ws.next, and carries its sampling in the composite launch (prep_ride_sample); that step's backward launch carries the
// offsets of its cell sort (prep_ride_scan), the nsk_adam_step after it the placement (prep_ride_place).  Whatever no launch has carried when the
// batch's own step arrives -- or when something else needs the cell histogram or ws.next -- runs by launches of its own (prep_finish), or the
// batch is forgotten and sampled afresh by its step (prep_drop).  Its step then swaps ws.next for ws.cur (forward_core).  No rider goes into a
// graph capture, and none under nsk_set_tuning("no_piggyback", 1).

// ws.next at the capacities of ws.cur
static int ensure_next(nsk_ctx* c, bool need_offs)
{
    Workspace& w = c->ws;
    const size_t m = (size_t)w.capM + 64;
    if (m > w.next.cap()) { CHK(grow_begin(c, 0)); CHK(alloc_samples(w.next, m, "the second sampling set")); }
    if (need_offs) CHK(grow(c, w.next.offs, w.cur.offs.cap(), "the second sampling set's offsets", 0));
    return 0;
}

// a registered batch becomes the prepared one (ws.next is free: the step that was using it has swapped it out); ride: its sampling may go into
// this step's composite launch
static int prep_promote(nsk_ctx* c, bool* ride)
{
    *ride = false;
    if (!c->req.valid || c->capturing) return 0;
    if (c->prep.valid) { const nsk_ctx::Prep keep = c->req; CHK(prep_drop(c)); c->req = keep; }      // an unclaimed set makes room
    const nsk_ctx::Prep R = c->req;
    if (R.sorted) CHK(ensure_hist(c, stage_bins(c, R.stage)));
    CHK(ensure_next(c, R.sorted));
    c->prep = R; c->prep.done = PREP_NOTHING; c->req.valid = false;
    *ride = !c->tune_no_piggyback && !needs_depth_max(R.gt, R.gtmax, R.N, R.dmax);
    return 0;
}

// whether the prepared batch's sampling writes liveness bytes is decided when it is sampled: under the masks of then
static int prep_sample_live(nsk_ctx* c, nsk_ctx::Prep& P)
{
    P.live = live_wanted(c, P.stage, true); P.live_epoch = c->live_epoch;
    if (P.live) CHK(ensure_live_stage(c, P.stage));
    return 0;
}

// Rider 1, nsk_map_step's composite launch (k_composite_sample): the sampling.  Promotes a registered batch first.  Precondition: that batch was
// promoted by this very call, so nothing of it has run, and it needs no depth-max launch in front (prep_promote's `ride`).  *wgs: the workgroups
// to append for SA; 0 = nothing rides.
static int prep_ride_sample(nsk_ctx* c, SampArgs& SA, int* wgs)
{
    bool ride = false;
    *wgs = 0;
    CHK(prep_promote(c, &ride));
    if (!ride) return 0;
    nsk_ctx::Prep& P = c->prep;
    CHK(prep_sample_live(c, P));
    samp_args(c, SA, P.R, P.stage, P.N, P.S, P.ro, P.rd, P.gt, P.gtmax, nullptr, P.mask, P.sorted, c->ws.next, P.live, P.dmax);
    *wgs = (P.N + NSK_SAMPLE_RAYS - 1) / NSK_SAMPLE_RAYS;
    P.done = PREP_SAMPLED;
    return 0;
}

// Rider 2, the backward launch (k_decode_bwd_multi<false> / k_decode_bwd_frozen; may_ride: it is one of those): the cell sort's offsets, by short
// workgroups behind the roles that wait for nothing of the launch.  Precondition: sampled, not scanned.  Returns the workgroups to append for
// MA.scan; waves4: 256-cell chunks per workgroup.
static int prep_ride_scan(nsk_ctx* c, MultiArgs& MA, bool may_ride, int waves4)
{
    nsk_ctx::Prep& P = c->prep;
    if (!(P.valid && P.sorted && P.done == PREP_SAMPLED && may_ride && !c->capturing && !c->tune_no_piggyback)) return 0;
    MA.scan = scan_args(c, P.stage, c->ws.next, waves4);
    P.done = PREP_SCANNED;
    return MA.scan.nblocks;
}

// Rider 3, nsk_adam_step's launch (k_adam_multi, when it has a segment to update): the cell sort's placement behind the segments.
// Precondition: scanned, not placed.  Returns the workgroups to append for AA.place; adam_blocks: those of the segments.
static int prep_ride_place(nsk_ctx* c, AdamArgs& AA, int adam_blocks)
{
    nsk_ctx::Prep& P = c->prep;
    if (!(AA.n && P.valid && P.sorted && P.done == PREP_SCANNED && !c->capturing && !c->tune_no_piggyback)) return 0;
    AA.place = place_args(P.N * P.S, c->ws.next, P.live);
    AA.adam_blocks = adam_blocks;
    P.done = PREP_PLACED;
    return AA.place.nblocks;
}

// the stages of the prepared batch that have not run yet, by launches of their own (its step has come, or something else needs the histogram)
static int prep_finish(nsk_ctx* c)
{
    nsk_ctx::Prep& P = c->prep;
    if (!P.valid) return 0;
    const PrepDone all = P.sorted ? PREP_PLACED : PREP_SAMPLED;
    if (P.done >= all) return 0;
    if (P.done < PREP_SAMPLED) CHK(prep_sample_live(c, P));
    CHK(launch_sampling(c, P.R, P.stage, P.N, P.S, P.ro, P.rd, P.gt, P.gtmax, P.mask, P.sorted, c->ws.next, P.live, P.dmax, P.done));
    P.done = all;
    return 0;
}
// forget the prepared batch and any registered one; a histogram that holds its counts is cleared by the scan
static int prep_drop(nsk_ctx* c)
{
    nsk_ctx::Prep& P = c->prep;
    if (P.valid && P.sorted && P.done == PREP_SAMPLED) { const ScanArgs A = scan_args(c, P.stage, c->ws.next, 1); k_sort_scan<<<A.nblocks, 256, 0, c->stream>>>(A); HIPCHK(hipGetLastError()); }
    P.valid = false; c->req.valid = false;
    return 0;
}

static void comp_args(nsk_ctx* c, CompArgs& A, int stage, int N, int S, const float* ro, const float* rd);
static int forward_core(nsk_ctx* c, int stage, int N, int S, const float* ro, const float* rd, const float* gt, float gtmax, bool save_masks,
                        bool sorted = false, const nsk_ctx::DMax* dmax = nullptr)      // dmax: instead of the installed depth-max batch (nsk_render_image: none)
{
    const int M = N * S;
    const uint8_t* mask = save_masks ? c->ray_mask : nullptr;      // (only the steps that form a loss honour it; a plain render shows every ray)
    const bool want_live = live_wanted(c, stage, save_masks);
    auto is_this_batch = [&](const nsk_ctx::Prep& X) {
        return X.valid && save_masks && (X.done < PREP_SAMPLED || (X.live == want_live && (!X.live || X.live_epoch == c->live_epoch))) && !c->capturing && X.stage == stage && X.N == N && X.S == S && X.ro == ro && X.rd == rd && X.gt == gt && X.gtmax == gtmax &&
               X.mask == mask && X.sorted == sorted && memcmp(&X.R, &c->R, sizeof(RParams)) == 0 &&
               X.dmax.gt == c->dmax.gt && X.dmax.keep == c->dmax.keep && X.dmax.n == c->dmax.n;
    };
    nsk_ctx::Prep& P = c->prep;
    if (!c->capturing) CHK(prep_finish(c));                 // (also when the set is for another batch: the sampling below needs the cell histogram; nsk_graph_begin has settled it before a capture)
    if (c->n_importance > 0) {
        // Importance sampling (include/nsk.h): a first pass over the S1 stratified and surface samples in ray order, whose compositing weights
        // place n_importance further depths; the S samples of the merged set are then an ordinary batch for everything downstream.  The first
        // pass keeps nothing for a backward.  No batch is ever prepared for such a step (nsk_map_prepare).
        const int Ni = c->n_importance, S1 = S - Ni, M1 = N * S1;
        Workspace& w = c->ws;
        const size_t m = (size_t)w.capM + 64;
        CHK(grow(c, w.imp_z, m, "the first pass's depths", GROW_NO_CAPTURE | GROW_STALE_GRAPHS));
        CHK(grow(c, w.imp_w, m, "the first pass's weights", GROW_NO_CAPTURE | GROW_STALE_GRAPHS));
        const nsk_ctx::DMax& dm = dmax ? *dmax : c->dmax;
        c->sorted = false;
        w.cur.z.swap(w.imp_z);                              // the launches of the first pass read their depths where every launch does
        int r = launch_sampling(c, c->R, stage, N, S1, ro, rd, gt, gtmax, mask, false, w.cur, false, dm);
        if (r == 0) r = launch_decode_fwd_stage(c, stage, M1, S1, ro, rd, false);
        if (r == 0) {
            CompArgs A;
            comp_args(c, A, stage, N, S1, ro, rd);
            A.keep = nullptr; A.weights = w.imp_w; A.mode = 0;
            ProfScope ps(c, "composite_first"); k_composite<<<(N + 3) / 4, 256, 0, c->stream>>>(A);
        }
        w.cur.z.swap(w.imp_z);                              // back: imp_z holds the first pass's depths, cur.z takes the merged ones
        CHK(r);
        HIPCHK(hipGetLastError());
        c->sorted = sorted;
        if (sorted) CHK(ensure_hist(c, stage_bins(c, stage)));
        if (want_live) CHK(ensure_live_stage(c, stage));
        {
            ProfScope ps(c, "resample");
            ResampArgs A;
            samp_args(c, A.P, c->R, stage, N, S, ro, rd, gt, gtmax, nullptr, mask, sorted, w.cur, want_live, dm);
            A.z1 = w.imp_z; A.w = w.imp_w; A.S1 = S1; A.Ni = Ni; A.det = c->R.perturb > 0.f ? 0 : 1;
            k_resample<<<(N + NSK_SAMPLE_RAYS - 1) / NSK_SAMPLE_RAYS, 64 * NSK_SAMPLE_RAYS, 0, c->stream>>>(A);
        }
        CHK(launch_sampling(c, c->R, stage, N, S, ro, rd, gt, gtmax, mask, sorted, w.cur, want_live, dm, PREP_SAMPLED));      // the cell sort, if any
        c->live_ok = want_live;
    } else if (is_this_batch(P)) {
        // this batch was sampled during the previous step (nsk_map_prepare): take its outputs
        c->ws.cur.swap(c->ws.next);                         // (both sets are kept at the same capacities: ensure_next)
        c->ws_flip ^= 1;
        P.valid = false;
        c->sorted = sorted;
        c->live_ok = P.live;
    } else {
        if (is_this_batch(c->req)) c->req.valid = false;    // registered, but no step came by to carry its sampling: sampled here like any other batch
        c->sorted = sorted;
        if (sorted) CHK(ensure_hist(c, stage_bins(c, stage)));
        if (want_live) CHK(ensure_live_stage(c, stage));
        CHK(launch_sampling(c, c->R, stage, N, S, ro, rd, gt, gtmax, mask, sorted, c->ws.cur, want_live, dmax ? *dmax : c->dmax));
        c->live_ok = want_live;
    }
    CHK(launch_decode_fwd_stage(c, stage, M, S, ro, rd, save_masks));
    c->dbg_M = M; c->dbg_S = S;
    return 0;
}

static void comp_args(nsk_ctx* c, CompArgs& A, int stage, int N, int S, const float* ro, const float* rd)
{
    memset(&A, 0, sizeof(A));
    A.R = c->R; A.N = N; A.S = S; A.stage = stage; A.rays_o = ro; A.rays_d = rd; A.z = c->ws.cur.z;
    A.occ_a = stage == 0 ? c->ws.occ[0] : c->ws.occ[1];
    A.occ_b = stage >= 2 ? c->ws.occ[2] : nullptr;
    A.rgb4 = stage == 3 ? c->ws.rgb4 : nullptr;
    A.g_raw = c->ws.g_raw;
    A.keep = c->ray_mask;
}

static int common_checks(nsk_ctx* c, int stage, int N, const float* ro, const float* rd, int* S_out, const float* gt)
{
    if (!c) return fail("null ctx");
    if (N < 1) return fail("N must be >= 1 (got %d)", N);
    if (!ro || !rd) return fail("rays_o / rays_d is NULL");
    CHK(check_stage(c, stage));
    HIPCHK(hipSetDevice(c->device));
    int S = c->R.n_samples + (gt ? c->R.n_surface : 0) + c->n_importance;      // with importance sampling: the merged set of the second pass
    if ((long long)N * S >= (1LL << 26)) return fail("N*S too large (%lld samples; at most 2^26 - 1 per call)", (long long)N * S);      // (also the range of ray_of)
    CHK(ensure_ws(c, N, N * S));
    *S_out = S;
    return 0;
}

extern "C" int nsk_render_forward(nsk_ctx* c, int stage, int N, const float* ro, const float* rd, const float* gt, float gtmax,
                                  float* rgb, float* depth, float* var, float* weights)
{
    int S;
    CHK(common_checks(c, stage, N, ro, rd, &S, gt));
    CHK(forward_core(c, stage, N, S, ro, rd, gt, gtmax, false));
    CompArgs A;
    comp_args(c, A, stage, N, S, ro, rd);
    A.rgb = rgb; A.depth = depth; A.var = var; A.weights = weights; A.mode = 0;
    { ProfScope ps(c, "composite"); k_composite<<<(N + 3) / 4, 256, 0, c->stream>>>(A); }
    HIPCHK(hipGetLastError());
    account(c, stage, N * S, first_pass_samples(c, N, S), false, 0);
    return 0;
}

extern "C" int nsk_raw2outputs(nsk_ctx* c, int N, int S, const float* raw, const float* z, const float* rd, int occupancy,
                               float* rgb, float* depth, float* var, float* weights)
{
    if (!c || !raw || !z || !rd || !rgb || !depth || !var) return fail("nsk_raw2outputs: null argument");
    if (N < 1 || S < 1 || S > 64) return fail("nsk_raw2outputs: need N >= 1 and 1 <= S <= 64");
    HIPCHK(hipSetDevice(c->device));
    k_raw2outputs<<<(N + 3) / 4, 256, 0, c->stream>>>(N, S, occupancy, raw, z, rd, rgb, depth, var, weights);
    HIPCHK(hipGetLastError());
    return 0;
}

// the resampling launch on its own: no rays, no cell keys, no liveness bytes
extern "C" int nsk_importance_resample(nsk_ctx* c, int N, int S, const float* z, const float* weights, int n_importance, int det, uint64_t seed,
                                       float* z_out)
{
    if (!c || !z || !weights || !z_out) return fail("nsk_importance_resample: null argument");
    if (N < 1 || S < 3 || n_importance < 1 || S + n_importance > 64)
        return fail("nsk_importance_resample: need N >= 1, S >= 3, n_importance >= 1 and S + n_importance <= 64 (got N = %d, %d + %d)", N, S, n_importance);
    if ((long long)N * (S + n_importance) >= (1LL << 31)) return fail("nsk_importance_resample: N * (S + n_importance) must stay below 2^31");
    {   // rows are read with stride S and written with stride S + n_importance: never in place
        const uintptr_t o0 = (uintptr_t)z_out, o1 = o0 + (size_t)N * (S + n_importance) * sizeof(float), in_bytes = (size_t)N * S * sizeof(float);
        for (const float* in : {z, weights})
            if ((uintptr_t)in < o1 && o0 < (uintptr_t)in + in_bytes) return fail("nsk_importance_resample: d_z_out overlaps %s", in == z ? "d_z" : "d_weights");
    }
    HIPCHK(hipSetDevice(c->device));
    ResampArgs A;
    memset(&A, 0, sizeof(A));
    A.P.N = N; A.P.S = S + n_importance; A.P.R.seed = seed; A.P.z_out = z_out;
    A.z1 = z; A.w = weights; A.S1 = S; A.Ni = n_importance; A.det = det ? 1 : 0;
    { ProfScope ps(c, "resample"); k_resample<<<(N + NSK_SAMPLE_RAYS - 1) / NSK_SAMPLE_RAYS, 64 * NSK_SAMPLE_RAYS, 0, c->stream>>>(A); }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_eval_points(nsk_ctx* c, int stage, int M, const float* pts, float* raw)
{
    if (!c || !pts || !raw) return fail("nsk_eval_points: null argument");
    if (M < 1) return fail("nsk_eval_points: M must be >= 1");
    CHK(check_stage(c, stage));
    HIPCHK(hipSetDevice(c->device));
    CHK(ensure_ws(c, 1, M));
    for (int q = 0; q < 3; ++q) {
        int w = STAGE_DEC[stage][q];
        if (w < 0) break;
        CHK(launch_decode_fwd(c, w, M, 1, nullptr, nullptr, pts, false));
    }
    k_eval_finish<<<(M + 255) / 256, 256, 0, c->stream>>>(M, stage, pts, c->d_bound, stage == 0 ? c->ws.occ[0] : c->ws.occ[1],
                                                          stage >= 2 ? c->ws.occ[2] : nullptr, stage == 3 ? c->ws.rgb4 : nullptr, raw);
    HIPCHK(hipGetLastError());
    account(c, stage, M, 0, false, 0);
    return 0;
}

// ---- scene mesh: lattice evaluation + marching cubes (nsk_mesh.h) ------------------------------------------------
static int lattice_checks(const char* fn, nsk_ctx* c, const float* o, const float* s, int nx, int ny, int nz, int nmin)
{
    if (!c || !o || !s) return fail("%s: null argument", fn);
    if (nx < nmin || ny < nmin || nz < nmin) return fail("%s: need at least %d nodes per axis (got %d x %d x %d)", fn, nmin, nx, ny, nz);
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(o[a])) return fail("%s: origin[%d] is not finite", fn, a);
        if (!(s[a] > 0.f) || !std::isfinite(s[a])) return fail("%s: step[%d] = %g, must be positive and finite", fn, a, (double)s[a]);
    }
    if (c->capturing) return fail("%s: not while a graph is being captured", fn);
    return 0;
}

// ---- what the entry points that project points into frames share (the rule itself: nsk_view.h) ---------------------------------------
static int view_checks(const char* fn, int H, int W, float fx, float fy, float cx, float cy, int edge)
{
    if (H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return fail("%s: image %d x %d, need 1 .. 2^24 pixels per side", fn, H, W);
    if (edge < 0) return fail("%s: edge = %d, must be >= 0", fn, edge);
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy)) return fail("%s: intrinsics are not finite", fn);
    return 0;
}
static ViewArgs view_args(int H, int W, float fx, float fy, float cx, float cy, int edge, float reach)
{
    ViewArgs A;
    memset(&A, 0, sizeof(A));
    A.H = H; A.W = W; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.reach = reach;
    A.ilo = A.jlo = (float)edge;                            // (edge beyond 2^24 rounds, and is beyond W and H either way)
    A.ihi = (float)((long long)W - edge); A.jhi = (float)((long long)H - edge);
    return A;
}
// rows 0..2 of the n row-major 4 x 4 matrices from k0 on
static void view_matrices(float (*w)[12], const float* w2c, int k0, int n)
{
    for (int k = 0; k < n; ++k) memcpy(w[k], w2c + 16 * (size_t)(k0 + k), 12 * sizeof(float));
}
// K frames in launches of VIEW_MAX_K: launch(A, the batch's first depth image (or NULL), its first frame k0, whether it is the last).  Every
// launch but the first of a call that does not accumulate adds to what the ones before it left.  K = 0 still launches once: it clears, or
// keeps, and counts.
template <class Launch>
static int view_batches(nsk_ctx* c, const char* name, ViewArgs A, int K, const float* w2c, const float* depth, int accumulate, Launch launch)
{
    int k0 = 0;
    do {
        A.K = std::min(K - k0, VIEW_MAX_K);
        A.accumulate = (accumulate || k0 > 0) ? 1 : 0;
        view_matrices(A.w, w2c, k0, A.K);
        { ProfScope ps(c, name); launch(A, depth ? depth + (size_t)k0 * A.H * A.W : nullptr, k0, k0 + A.K >= K); }
        HIPCHK(hipGetLastError());
        k0 += A.K;
    } while (k0 < K);
    return 0;
}
// An entry point's optional count (h_count NULL: none): the context's one counter, zeroed in front of the launches that add to it, and
// read back behind them, which synchronises.  (Every caller has refused a graph capture before.)
static int count_begin(nsk_ctx* c, const long long* h_count, const char* what)
{
    if (!h_count) return 0;
    CHK(grow(c, c->count, 1, what, GROW_NO_CAPTURE));
    HIPCHK(hipMemsetAsync(c->count, 0, 8, c->stream));
    return 0;
}
static int count_end(nsk_ctx* c, long long* h_count)
{
    if (!h_count) return 0;
    unsigned long long cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, c->count, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *h_count = (long long)cnt;
    return 0;
}

extern "C" int nsk_eval_lattice(nsk_ctx* c, int stage, const float* o, const float* s, int nx, int ny, int nz, float* vol)
{
    CHK(lattice_checks("nsk_eval_lattice", c, o, s, nx, ny, nz, 1));
    if (!vol) return fail("nsk_eval_lattice: d_volume is NULL");
    if (stage < 0 || stage > 3) return fail("bad stage %d", stage);
    const int st = stage == NSK_COLOR ? NSK_FINE : stage;       // the colour stage's occupancy is the fine stage's (src/models/NICE.cpp:41-50)
    CHK(check_stage(c, st));
    HIPCHK(hipSetDevice(c->device));
    const long long total = (long long)nx * ny * nz;
    long long slab = c->mesh.slab > 0 ? c->mesh.slab : std::max(c->ws.capM, 1 << 21);
    slab = std::min(std::min(slab, total), (1LL << 26) - 1);
    CHK(ensure_ws(c, 1, (int)slab));
    CHK(grow(c, c->mesh.lat_pts, (size_t)slab * 3, "the lattice slab's points", 0));
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = 0; G.level = 0.f;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    float* pts = c->mesh.lat_pts;
    for (long long n0 = 0; n0 < total; n0 += slab) {
        const int cnt = (int)std::min(slab, total - n0);
        { ProfScope ps(c, "lattice_points"); k_lattice_points<<<(cnt + 255) / 256, 256, 0, c->stream>>>(G, n0, cnt, pts); }
        HIPCHK(hipGetLastError());
        for (int q = 0; q < 3; ++q) {
            const int w = STAGE_DEC[st][q];
            if (w < 0) break;
            CHK(launch_decode_fwd(c, w, cnt, 1, nullptr, nullptr, pts, false));
        }
        { ProfScope ps(c, "lattice_finish");
          k_lattice_finish<<<(cnt + 255) / 256, 256, 0, c->stream>>>(cnt, pts, c->d_bound, st == 0 ? c->ws.occ[0] : c->ws.occ[1], st >= 2 ? c->ws.occ[2] : nullptr, vol + n0); }
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// levels of the multi-launch scan over n values: [n | ceil(n / 256) | ...] until one workgroup covers a level, each level at a 64-word boundary
static size_t mc_scan_words(size_t n)
{
    size_t words = 0;
    for (;;) { words += (n + 63) & ~(size_t)63; if (n <= MC_BLOCK) return words; n = (n + MC_BLOCK - 1) / MC_BLOCK; }
}
static int mc_scan(nsk_ctx* c, unsigned* d, int n)
{
    const int nb = (n + MC_BLOCK - 1) / MC_BLOCK;
    unsigned* sums = d + ((n + 63) & ~63);
    k_mc_scan_block<<<nb, MC_BLOCK, 0, c->stream>>>(d, n, nb > 1 ? sums : nullptr);
    HIPCHK(hipGetLastError());
    if (nb == 1) return 0;
    CHK(mc_scan(c, sums, nb));
    k_mc_scan_add<<<nb, MC_BLOCK, 0, c->stream>>>(d, n, sums);
    HIPCHK(hipGetLastError());
    return 0;
}

// nsk_eval_lattice at the nodes a mask keeps: count, scan and compact the set nodes into an ascending index list (the other nodes receive
// `fill` in the compaction pass), then the slabs of nsk_eval_lattice walk that list instead of the lattice
extern "C" int nsk_eval_lattice_masked(nsk_ctx* c, int stage, const float* o, const float* s, int nx, int ny, int nz, const uint8_t* valid, float fill,
                                       float* vol, long long* n_evaluated)
{
    CHK(lattice_checks("nsk_eval_lattice_masked", c, o, s, nx, ny, nz, 1));
    if (!valid) return fail("nsk_eval_lattice_masked: d_valid is NULL (nsk_eval_lattice evaluates every node)");
    if (!vol) return fail("nsk_eval_lattice_masked: d_volume is NULL");
    if (stage < 0 || stage > 3) return fail("bad stage %d", stage);
    const int st = stage == NSK_COLOR ? NSK_FINE : stage;
    CHK(check_stage(c, st));
    const long long total = (long long)nx * ny * nz;
    if (total > MC_MAX_NODES) return fail("nsk_eval_lattice_masked: %lld nodes, at most %lld per call", total, (long long)MC_MAX_NODES);
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Mesh& M = c->mesh;
    if (n_evaluated) *n_evaluated = 0;
    const int nn = (int)total, nb = (nn + MC_BLOCK - 1) / MC_BLOCK;
    const size_t words = mc_scan_words((size_t)nb + 1);
    CHK(grow(c, M.lat_scan, words, "the lattice mask's scan scratch", 0));
    unsigned* boff = M.lat_scan;
    unsigned fill_bits;
    memcpy(&fill_bits, &fill, 4);
    unsigned n_set = 0;
    { ProfScope ps(c, "lattice_compact");
      HIPCHK(hipMemsetAsync(boff, 0, words * 4, c->stream));            // (the slot behind the last workgroup count turns into the total)
      k_lattice_flags<<<nb, MC_BLOCK, 0, c->stream>>>(nn, valid, boff);
      HIPCHK(hipGetLastError());
      CHK(mc_scan(c, boff, nb + 1));
      HIPCHK(hipMemcpyAsync(&n_set, boff + nb, 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      CHK(grow(c, M.lat_idx, (size_t)n_set, "the set nodes' indices", 0));
      k_lattice_compact<<<nb, MC_BLOCK, 0, c->stream>>>(nn, valid, boff, n_set, fill_bits, M.lat_idx, reinterpret_cast<unsigned*>(vol));
      HIPCHK(hipGetLastError()); }
    if (n_evaluated) *n_evaluated = (long long)n_set;
    if (n_set == 0) return 0;                                           // (no decoder launch, the workspace stays as it is)
    long long slab = M.slab > 0 ? M.slab : std::max(c->ws.capM, 1 << 21);
    slab = std::min(std::min(slab, (long long)n_set), (1LL << 26) - 1);
    CHK(ensure_ws(c, 1, (int)slab));
    CHK(grow(c, M.lat_pts, (size_t)slab * 3, "the lattice slab's points", 0));
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = nn; G.level = 0.f;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    float* pts = M.lat_pts;
    for (long long m0 = 0; m0 < (long long)n_set; m0 += slab) {
        const int cnt = (int)std::min(slab, (long long)n_set - m0);
        const unsigned* idx = M.lat_idx.get() + m0;
        { ProfScope ps(c, "lattice_points_idx"); k_lattice_points_idx<<<(cnt + 255) / 256, 256, 0, c->stream>>>(G, idx, cnt, pts); }
        HIPCHK(hipGetLastError());
        for (int q = 0; q < 3; ++q) {
            const int w = STAGE_DEC[st][q];
            if (w < 0) break;
            CHK(launch_decode_fwd(c, w, cnt, 1, nullptr, nullptr, pts, false));
        }
        { ProfScope ps(c, "lattice_finish_idx");
          k_lattice_finish_idx<<<(cnt + 255) / 256, 256, 0, c->stream>>>(cnt, pts, c->d_bound, st == 0 ? c->ws.occ[0] : c->ws.occ[1], st >= 2 ? c->ws.occ[2] : nullptr, idx, vol); }
        HIPCHK(hipGetLastError());
    }
    return 0;
}

extern "C" int nsk_mesh_extract(nsk_ctx* c, const float* vol, const uint8_t* valid, int nx, int ny, int nz, const float* o, const float* s,
                                float level, int* n_vertices, int* n_triangles)
{
    CHK(lattice_checks("nsk_mesh_extract", c, o, s, nx, ny, nz, 2));
    if (!vol) return fail("nsk_mesh_extract: d_volume is NULL");
    if (!n_vertices || !n_triangles) return fail("nsk_mesh_extract: n_vertices / n_triangles is NULL");
    if (std::isnan(level)) return fail("nsk_mesh_extract: level is NaN");
    const long long total = (long long)nx * ny * nz;
    if (total > MC_MAX_NODES) return fail("nsk_mesh_extract: %lld nodes, at most %lld per call", total, (long long)MC_MAX_NODES);
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Mesh& M = c->mesh;
    M.nv = M.nt = 0; M.extracted = false;
    *n_vertices = *n_triangles = 0;
    const int nn = (int)total, nb = (nn + MC_BLOCK - 1) / MC_BLOCK;
    if (!M.ntri) {
        const McTable& T = mc_table();
        const int r = [&]() -> int {
            CHK(dev_alloc(M.table, sizeof(T.edges), "the case table")); CHK(dev_alloc(M.ntri, sizeof(T.ntri), "the case table"));
            HIPCHK(hipMemcpy(M.table, T.edges, sizeof(T.edges), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(M.ntri, T.ntri, sizeof(T.ntri), hipMemcpyHostToDevice));
            return 0;
        }();
        if (r != 0) { reset_all(M.table, M.ntri); return r; }
    }
    int r = grow(c, M.cellcase, (size_t)nn, "the cell cases", 0);
    if (r == 0) r = grow(c, M.emap, (size_t)nn * 3, "the edge map", 0);
    if (r != 0) { reset_all(M.cellcase, M.emap); return r; }
    const size_t words = mc_scan_words((size_t)nb + 1);
    CHK(grow(c, M.scan, 2 * words, "the scan scratch", 0));
    unsigned* sv = M.scan; unsigned* stri = M.scan + words;
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = nn; G.level = level;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    HIPCHK(hipMemsetAsync(M.scan, 0, 2 * words * 4, c->stream));        // (the slot behind the last workgroup count turns into the total)
    { ProfScope ps(c, "mc_cells"); k_mc_cells<<<nb, MC_BLOCK, 0, c->stream>>>(G, vol, valid, M.ntri, M.cellcase, stri); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "mc_edge_count"); k_mc_edges<false><<<nb, MC_BLOCK, 0, c->stream>>>(G, vol, M.cellcase, sv, nullptr, nullptr, nullptr); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "mc_scan"); CHK(mc_scan(c, sv, nb + 1)); CHK(mc_scan(c, stri, nb + 1)); }
    unsigned tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&tot[0], sv + nb, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tot[1], stri + nb, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (tot[0] > 0x7fffffffu / 3 || tot[1] > 0x7fffffffu / 3) return fail("nsk_mesh_extract: %u vertices, %u triangles do not fit 32-bit indices", tot[0], tot[1]);
    CHK(grow(c, M.verts, (size_t)tot[0] * 3, "the vertices", 0));
    CHK(grow(c, M.tris, (size_t)tot[1] * 3, "the triangles", 0));
    if (tot[0]) {
        { ProfScope ps(c, "mc_vertices"); k_mc_edges<true><<<nb, MC_BLOCK, 0, c->stream>>>(G, vol, M.cellcase, nullptr, sv, M.emap, M.verts); }
        HIPCHK(hipGetLastError());
    }
    if (tot[1]) {
        { ProfScope ps(c, "mc_triangles"); k_mc_tris<<<nb, MC_BLOCK, 0, c->stream>>>(G, M.cellcase, M.ntri, M.table, stri, M.emap, M.tris); }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    M.nv = (int)tot[0]; M.nt = (int)tot[1]; M.extracted = true;
    *n_vertices = M.nv; *n_triangles = M.nt;
    return 0;
}

// the nodes of a lattice that at least one of K keyframes sees (k_lattice_seen); keyframe lists longer than a launch holds go in several
extern "C" int nsk_lattice_seen(nsk_ctx* c, const float* o, const float* s, int nx, int ny, int nz, int K, const float* depth, int H, int W,
                                float fx, float fy, float cx, float cy, const float* w2c, int edge, float trunc, int accumulate, uint8_t* valid,
                                long long* n_seen)
{
    CHK(lattice_checks("nsk_lattice_seen", c, o, s, nx, ny, nz, 1));
    if (!valid) return fail("nsk_lattice_seen: d_valid is NULL");
    if (K < 0) return fail("nsk_lattice_seen: K = %d", K);
    if (K > 0 && (!depth || !w2c)) return fail("nsk_lattice_seen: d_depth / h_w2c is NULL with K = %d", K);
    CHK(view_checks("nsk_lattice_seen", H, W, fx, fy, cx, cy, edge));
    if (std::isnan(trunc)) return fail("nsk_lattice_seen: trunc is NaN");
    const long long total = (long long)nx * ny * nz;
    if (total > MC_MAX_NODES) return fail("nsk_lattice_seen: %lld nodes, at most %lld per call", total, (long long)MC_MAX_NODES);
    HIPCHK(hipSetDevice(c->device));
    CHK(count_begin(c, n_seen, "the seen count"));
    McGeom G;
    G.nx = nx; G.ny = ny; G.nz = nz; G.nn = (int)total; G.level = 0.f;
    for (int a = 0; a < 3; ++a) { G.o[a] = o[a]; G.s[a] = s[a]; }
    const int nb = (G.nn + MC_BLOCK - 1) / MC_BLOCK;
    CHK(view_batches(c, "lattice_seen", view_args(H, W, fx, fy, cx, cy, edge, trunc), K, w2c, depth, accumulate,
                     [&](const ViewArgs& A, const float* dk, int, bool last) {
        k_lattice_seen<<<nb, MC_BLOCK, 0, c->stream>>>(G, A, dk, valid, last && n_seen ? c->count.get() : nullptr); }));
    return count_end(c, n_seen);
}

// connected components of the last extracted mesh, the keep rule, compaction by the multi-launch scans (nsk_mesh.h)
extern "C" int nsk_mesh_filter(nsk_ctx* c, float min_area, int largest_only, int* n_vertices, int* n_triangles, int* n_components, int* n_kept)
{
    if (!c) return fail("null ctx");
    if (!n_vertices || !n_triangles || !n_components || !n_kept) return fail("nsk_mesh_filter: n_vertices / n_triangles / n_components / n_kept is NULL");
    if (std::isnan(min_area)) return fail("nsk_mesh_filter: min_area is NaN");
    if (c->capturing) return fail("nsk_mesh_filter: not while a graph is being captured");
    nsk_ctx::Mesh& M = c->mesh;
    if (!M.extracted) return fail("nsk_mesh_filter: no mesh (call nsk_mesh_extract first)");
    HIPCHK(hipSetDevice(c->device));
    *n_vertices = M.nv; *n_triangles = M.nt; *n_components = *n_kept = 0;
    if (M.nv == 0 || M.nt == 0) { M.nv = M.nt = 0; *n_vertices = *n_triangles = 0; return 0; }
    const int nv = M.nv, nt = M.nt, nbv = (nv + MC_BLOCK - 1) / MC_BLOCK, nbt = (nt + MC_BLOCK - 1) / MC_BLOCK, nbm = std::max(nbv, nbt);
    int r = grow(c, M.cc_label, (size_t)nv, "the component labels", 0);
    if (r == 0) r = grow(c, M.cc_area, (size_t)nv, "the component areas", 0);
    if (r == 0) r = grow(c, M.cc_used, (size_t)nv, "the vertex flags", 0);
    if (r == 0) r = grow(c, M.cc_keep, (size_t)nv, "the keep flags", 0);
    if (r != 0) { reset_all(M.cc_label, M.cc_area, M.cc_used, M.cc_keep); return r; }
    CHK(grow(c, M.cc_stats, 1, "the component statistics", 0));
    const size_t wv = mc_scan_words((size_t)nv + 1), wt = mc_scan_words((size_t)nt + 1);
    CHK(grow(c, M.scan, wv + wt, "the scan scratch", 0));
    CHK(grow(c, M.verts2, (size_t)nv * 3, "the filtered vertices", 0));
    CHK(grow(c, M.tris2, (size_t)nt * 3, "the filtered triangles", 0));
    unsigned* voff = M.scan; unsigned* toff = M.scan + wv;
    const CcStats init = {0ull, 0x7fffffff, 0u, 0u};
    HIPCHK(hipMemcpyAsync(M.cc_stats, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(M.scan, 0, (wv + wt) * 4, c->stream));         // (the slot behind the last flag turns into the total)
    { ProfScope ps(c, "cc_label");
      k_cc_init<<<nbv, MC_BLOCK, 0, c->stream>>>(nv, M.cc_label, M.cc_area, M.cc_used);
      k_cc_hook<<<nbt, MC_BLOCK, 0, c->stream>>>(nt, M.tris, M.cc_label, M.cc_used);
      k_cc_flatten<<<nbv, MC_BLOCK, 0, c->stream>>>(nv, M.cc_label); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "cc_area"); k_cc_area<<<(nbt + CC_AREA_ITERS - 1) / CC_AREA_ITERS, MC_BLOCK, 0, c->stream>>>(nt, M.tris, M.verts, M.cc_label, M.cc_area); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "cc_keep");
      k_cc_roots<<<nbv, MC_BLOCK, 0, c->stream>>>(nv, M.cc_label, M.cc_used, M.cc_area, (double)min_area, largest_only, M.cc_keep, M.cc_stats);
      if (largest_only) {
          k_cc_pick<<<nbv, MC_BLOCK, 0, c->stream>>>(nv, M.cc_label, M.cc_used, M.cc_area, M.cc_stats);
          k_cc_pick_done<<<1, 1, 0, c->stream>>>(M.cc_keep, M.cc_stats);
      }
      k_cc_flags<<<nbm, MC_BLOCK, 0, c->stream>>>(nv, nt, M.tris, M.cc_label, M.cc_used, M.cc_keep, voff, toff); }
    HIPCHK(hipGetLastError());
    { ProfScope ps(c, "cc_scan"); CHK(mc_scan(c, voff, nv + 1)); CHK(mc_scan(c, toff, nt + 1)); }
    { ProfScope ps(c, "cc_compact"); k_mesh_compact<<<nbm, MC_BLOCK, 0, c->stream>>>(nv, nt, M.verts, M.tris, voff, toff, M.verts2, M.tris2, nullptr); }
    HIPCHK(hipGetLastError());
    CcStats st;
    unsigned tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&st, M.cc_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tot[0], voff + nv, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&tot[1], toff + nt, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    M.verts.swap(M.verts2); M.tris.swap(M.tris2);
    M.nv = (int)tot[0]; M.nt = (int)tot[1];
    *n_vertices = M.nv; *n_triangles = M.nt; *n_components = (int)st.n_components; *n_kept = (int)st.n_kept;
    return 0;
}

extern "C" int nsk_mesh_buffers(nsk_ctx* c, float** d_vertices, int32_t** d_triangles)
{
    if (!c) return fail("null ctx");
    if (d_vertices) *d_vertices = c->mesh.nv ? c->mesh.verts : nullptr;
    if (d_triangles) *d_triangles = c->mesh.nt ? c->mesh.tris : nullptr;
    return 0;
}

extern "C" int nsk_mesh_download(nsk_ctx* c, float* h_vertices, int32_t* h_triangles)
{
    if (!c) return fail("null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_vertices && c->mesh.nv) HIPCHK(hipMemcpy(h_vertices, c->mesh.verts, (size_t)c->mesh.nv * 12, hipMemcpyDeviceToHost));
    if (h_triangles && c->mesh.nt) HIPCHK(hipMemcpy(h_triangles, c->mesh.tris, (size_t)c->mesh.nt * 12, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nsk_mesh_table(int case_index, int8_t* h_edges, int capacity)
{
    if (case_index < 0 || case_index > 255) return fail("nsk_mesh_table: case %d out of range", case_index);
    const McTable& T = mc_table();
    const int n = 3 * T.ntri[case_index];
    if (h_edges) {
        if (capacity < n) return fail("nsk_mesh_table: case %d has %d entries, capacity %d", case_index, n, capacity);
        memcpy(h_edges, T.edges[case_index], (size_t)n);
    }
    return T.ntri[case_index];
}

// decoders' backward after k_composite wrote g_raw: ONE launch for every decoder of the stage that needs it
// sum the per-workgroup decoder-gradient slabs of the last backward into the gradient slab (normally done inside k_adam_multi)
static int flush_pending(nsk_ctx* c)
{
    if (c->pend_w < 0) return 0;
    const int w = c->pend_w, np = c->dec[w].n, n4 = (np + 3) & ~3;
    ProfScope ps(c, "dec_grad_reduce");
    k_dec_grad_reduce<<<dim3((np + 255) / 256, 8), 256, 0, c->stream>>>(np, n4, c->pend_nb, c->ws.dec_slabs, c->slab + c->dec[w].g_off);
    HIPCHK(hipGetLastError());
    c->pend_w = -1;
    return 0;
}

// The steps of backward_core.  BwdRoles: the launch's roles in launch order (colour, fine, middle) and their costs in the split
struct BwdRoles { int n = 0, cost[3] = {0, 0, 0}; };

// collect: every decoder of the stage that has a gradient to compute becomes a role of MA; marks the parameter groups the launch writes
static int collect_bwd_roles(nsk_ctx* c, MultiArgs& MA, BwdRoles& R, int stage, int N, int S, const float* ro, const float* rd, unsigned flags,
                             float* g_ro, float* g_rd, const float* dyn_resid)
{
    const bool rays = (flags & NSK_GRAD_RAYS) != 0, grids = (flags & NSK_GRAD_GRIDS) != 0;
    for (int q = 2; q >= 0; --q) {
        int w = STAGE_DEC[stage][q];
        if (w < 0) continue;
        bool train = (flags & NSK_GRAD_DECODERS) && c->dec[w].trainable;
        if (!train && !grids && !rays) continue;
        DecArgs& A = MA.a[R.n];
        CHK(fill_bwd_role(c, A, w, N * S, S, ro, rd, train, grids, g_ro, g_rd));
        A.dyn_resid = dyn_resid; A.dyn_n = N;
        A.flags = flags & 0xffu;
        MA.which[R.n] = w; MA.train[R.n] = train ? 1 : 0;
        R.cost[R.n] = bwd_role_cost(train, w, rays, c->tune);
        if (train) c->touched[NSK_GROUP_DECODERS] = true;
        if (grids) c->touched[NSK_GROUP_COARSE + w] = true;
        ++R.n;
    }
    return 0;
}

// Dead-tile skip: a frozen role whose level carries an optimiser mask walks the slots' liveness bytes (forward_core) and runs only the tiles
// with a sample that reaches a marked voxel, where the launch form allows it (BwdForm::skip_eligible).  The roles count what they ran (counted[]); the count of an EARLIER step of the same kind (whatever has arrived
// in live_host: nobody waits for it) tells the split how long the frozen roles really are (tasks[]) -- the first step of a kind assumes every
// tile runs.
static void bwd_liveness(nsk_ctx* c, MultiArgs& MA, const BwdRoles& R, const BwdForm& F, int stage, int M, unsigned flags, int* tasks, bool* counted)
{
    const int ntasks = (M + 15) / 16;
    for (int r = 0; r < 3; ++r) { tasks[r] = ntasks; counted[r] = false; }
    if (!c->live_ok || !F.skip_eligible) return;
    const int key[8] = {stage, M, (int)(flags & 0xffu), c->sorted ? 1 : 0, c->live_epoch, R.n, F.train_role, F.kernel == BWD_FROZEN ? 1 : 0};
    if (memcmp(key, c->live_key, sizeof(key)) != 0) { memcpy(c->live_key, key, sizeof(key)); ++c->live_tag; }
    const volatile int* h = c->live_host;
    const bool fresh = h[3] == c->live_tag;
    for (int r = 0; r < R.n; ++r) {
        const int w = MA.which[r];
        if (MA.train[r] || w < 1 || !c->grid[w].mask || c->grid[w].live_dirty) continue;
        DecArgs& A = MA.a[r];
        A.live = c->sorted ? c->ws.cur.lslot : c->ws.cur.lsamp; A.live_bit = 1u << (w - 1); A.live_cnt = c->live_cnt + (w - 1);
        counted[r] = true; c->dbg_counted[w - 1] = true;
        if (fresh) tasks[r] = dead_skip_tasks(ntasks, (int)h[w - 1], c->tune);
    }
}

// grid: bwd_grid of the form, the split and the riders
static void launch_bwd_roles(nsk_ctx* c, MultiArgs& MA, BwdKernel kernel, int grid, const DealRoles& deal)
{
    const size_t lds = bwd_form_lds_bytes(kernel, MA.n, MA.which, MA.train);
    ProfScope ps(c, "decode_bwd_multi");
    switch (kernel) {
    case BWD_TRACK:
        MA.dyn_seed = c->ws.tmp_rgb; MA.dyn_thr_out = c->scal + 1;
        k_decode_bwd_track<<<grid, 512, lds, c->stream>>>(MA);
        break;
    case BWD_MULTI_FULL_RAYS: k_decode_bwd_multi_full<true><<<grid, 512, lds, c->stream>>>(MA); break;
    case BWD_MULTI_FULL: k_decode_bwd_multi_full<false><<<grid, 512, lds, c->stream>>>(MA); break;
    case BWD_FROZEN: k_decode_bwd_frozen<<<grid, 64 * NSK_FROZEN_NW, lds, c->stream>>>(MA); break;
    case BWD_MULTI_RAYS: k_decode_bwd_multi<true><<<grid, 512, lds, c->stream>>>(MA); break;
    case BWD_MULTI_DEAL: k_decode_bwd_multi_deal<<<grid, 512, lds, c->stream>>>(MA, deal); break;
    case BWD_MULTI: k_decode_bwd_multi<false><<<grid, 512, lds, c->stream>>>(MA); break;
    case BWD_NONE: case BWD_SEPARATE: break;      // (backward_core has left before)
    }
}

// dyn_resid: the Tracker's deferred median mask (composite mode 5 wrote the residuals there and the seeds to ws.tmp_rgb): k_decode_bwd_track
static int backward_core(nsk_ctx* c, int stage, int N, int S, const float* ro, const float* rd, unsigned flags, float* g_ro, float* g_rd,
                         float* d_loss = nullptr, const float* dyn_resid = nullptr)
{
    const int M = N * S, ntasks = (M + 15) / 16;
    for (int k = 0; k < 3; ++k) { c->dbg_live[k] = -1; c->dbg_counted[k] = false; c->dbg_wgs[k] = 0; }      // (nsk_debug_live_tiles: this backward's, whichever way it leaves)
    c->dbg_ntasks = ntasks;
    CHK(flush_pending(c));                      // gradients accumulate across calls: the slabs are about to be overwritten
    struct Disarm { nsk_ctx* c; ~Disarm() { c->deal_armed = false; } } disarm{c};      // an arming holds for this backward only
    MultiArgs MA;
    memset(&MA, 0, sizeof(MA));
    BwdRoles R;
    CHK(collect_bwd_roles(c, MA, R, stage, N, S, ro, rd, flags, g_ro, g_rd, dyn_resid));
    BwdFormIn in;
    in.n = R.n; memcpy(in.which, MA.which, sizeof(in.which)); memcpy(in.train, MA.train, sizeof(in.train));
    in.rays = (flags & NSK_GRAD_RAYS) != 0; in.grids = (flags & NSK_GRAD_GRIDS) != 0;
    in.full = c->bwd_mode == 0; in.deterministic = c->deterministic != 0; in.track = dyn_resid != nullptr;
    in.N = N;
    in.no_frozen_kernel = c->tune_no_frozen_kernel; in.no_dead_skip = c->tune_no_dead_skip; in.static_deal = c->tune_static_deal;
    const BwdForm F = bwd_form(in);                 // which launch goes out, and what may ride in it: nsk_split.h
    const int n = R.n;
    if (!F.mask_ok) return fail("backward_core: the deferred median mask needs the Tracker's launch (frozen decoders, ray gradients)");
    if ((F.kernel == BWD_NONE || F.kernel == BWD_SEPARATE) && d_loss) { ProfScope ps(c, "loss_sum"); k_sum<<<1, 1024, 0, c->stream>>>(N, c->ws.ray_loss, d_loss); }
    memset(c->dbg_split[1], 0, sizeof(c->dbg_split[1]));
    if (F.kernel == BWD_NONE) return 0;
    for (int r = 0; r < n; ++r) if (!MA.train[r] && MA.which[r] >= 1) c->dbg_live[MA.which[r] - 1] = ntasks;      // until a role counts fewer
    if (F.kernel == BWD_SEPARATE) {      // rare configuration (several trainable decoders share one slab buffer), or the debug mode: one launch each
        record_split(c, 1, bwd_split_form(F.kernel), n, MA.which, MA.train, nullptr, 0, 0, ntasks, bwd_separate_grid(c->num_cu, ntasks, in.deterministic));
        for (int r = 0; r < n; ++r)
            CHK(launch_decode_bwd(c, MA.which[r], M, S, ro, rd, MA.train[r] != 0, in.rays, flags, g_ro, g_rd));
        return 0;
    }
    MA.n = n;
    int tasks[3]; bool counted[3];
    bwd_liveness(c, MA, R, F, stage, M, flags, tasks, counted);
    plan_bwd(c->num_cu, ntasks, n, R.cost, F.train_role, F.waves, tasks, MA.wg_end);
    // Queue dealing of the skipping roles (decode_bwd_body: Dealing), where bwd_deal_role finds rounds enough
    bool dealt = false; DealRoles DR;
    memset(&DR, 0, sizeof(DR));
    for (int r = 0; r < n; ++r) {
        if (!bwd_deal_role(ntasks, role_wgs(MA.wg_end, r), counted[r], F, c->tune_deal_min_rounds)) continue;
        DR.r[r] = DealArgs{c->deal_cur + (MA.which[r] - 1) * NSK_DEAL_STRIDE, c->tune_deal_head_pct, c->tune_deal_chunk};
        dealt = true;
    }
    // the cursors start at zero: the compositing launch in front of this one armed them (nsk_map_step, nsk_render_backward); a backward on its own arms here
    if (dealt && !c->deal_armed) HIPCHK(hipMemsetAsync(c->deal_cur, 0, 3 * NSK_DEAL_STRIDE * sizeof(int), c->stream));
    for (int r = 0; r < n; ++r) {
        if (counted[r]) MA.live_wgs += role_wgs(MA.wg_end, r);
        if (MA.which[r] >= 1) c->dbg_wgs[MA.which[r] - 1] = role_wgs(MA.wg_end, r);
    }
    MA.live_cnt = c->live_cnt; MA.live_out = c->live_host_dev; MA.live_tag = c->live_tag;
    const int loss_wg = d_loss ? 1 : 0;          // one more workgroup sums the per-ray losses written by k_composite
    if (d_loss) { MA.sum_src = c->ws.ray_loss; MA.sum_dst = d_loss; MA.sum_n = N; }
    const int scan_wgs = prep_ride_scan(c, MA, F.scan_may_ride, F.scan_halves);
    const int grid = bwd_grid(F, MA.wg_end, n, scan_wgs, loss_wg);
    record_split(c, 1, bwd_split_form(F.kernel), n, MA.which, MA.train, MA.wg_end, scan_wgs, loss_wg, ntasks, grid);
    c->dbg_split[1][15] = F.kernel == BWD_TRACK ? 1 : 0;
    launch_bwd_roles(c, MA, bwd_launch_kernel(F, dealt), grid, DR);
    HIPCHK(hipGetLastError());
    if (F.train_role >= 0) { c->pend_w = MA.which[F.train_role]; c->pend_nb = role_wgs(MA.wg_end, F.train_role); }      // summed by k_adam_multi, or by flush_pending when someone reads the slab first
    return 0;
}

extern "C" int nsk_render_backward(nsk_ctx* c, int stage, int N, const float* ro, const float* rd, const float* gt, float gtmax,
                                   const float* g_rgb, const float* g_depth, const float* g_var, unsigned flags, float* g_ro, float* g_rd)
{
    int S;
    CHK(common_checks(c, stage, N, ro, rd, &S, gt));
    if (!g_rgb || !g_depth) return fail("nsk_render_backward: g_rgb / g_depth is NULL");
    if ((flags & NSK_GRAD_RAYS) && (!g_ro || !g_rd)) return fail("nsk_render_backward: NSK_GRAD_RAYS needs g_rays_o and g_rays_d");
    CHK(forward_core(c, stage, N, S, ro, rd, gt, gtmax, true, sort_pays(c, stage, N * S, flags)));
    CompArgs A;
    comp_args(c, A, stage, N, S, ro, rd);
    A.mode = 1; A.g_rgb = g_rgb; A.g_depth = g_depth; A.g_var = g_var;
    if (flags & NSK_GRAD_RAYS) { A.g_rays_o = g_ro; A.g_rays_d = g_rd; }
    A.deal = c->deal_cur;
    { ProfScope ps(c, "composite"); k_composite<<<(N + 3) / 4, 256, 0, c->stream>>>(A); }
    HIPCHK(hipGetLastError());
    c->deal_armed = true;      // only now: the launch that zeroes the cursors is on the stream
    CHK(backward_core(c, stage, N, S, ro, rd, flags, g_ro, g_rd));
    account(c, stage, N * S, first_pass_samples(c, N, S), true, flags);
    return 0;
}

// Registers the NEXT batch.  Nothing is launched here: the nsk_map_step that follows carries the batch's sampling in its composite launch, its
// backward launch carries the offsets of the cell sort, the nsk_adam_step after it the placement -- three launches and their dependent round
// trips (30 us at 5000 rays, 20 us at 1000) leave the front of the next step.  Until round 3 the sampling ran on a side stream beside the
// exchange and the optimiser step: that needed two cross-stream waits per step and lost on one GPU (K3 0.511 against 0.500 ms).
// Whatever has not been carried when the batch's own step arrives is launched there, as for an unprepared batch.
extern "C" int nsk_map_prepare(nsk_ctx* c, int stage, int N, const float* ro, const float* rd, const float* gt, float gtmax, unsigned flags)
{
    int S;
    if (!gt) return fail("nsk_map_prepare: gt_depth is NULL");
    if (c && c->capturing) return fail("nsk_map_prepare: not inside a graph capture");
    CHK(common_checks(c, stage, N, ro, rd, &S, gt));
    if (c->n_importance > 0) return 0;           // no rider carries a resampling (its first pass reads the map this step's optimiser leaves): the batch's own step samples it
    const bool sorted = sort_pays(c, stage, N * S, flags);
    if (sorted) CHK(ensure_hist(c, stage_bins(c, stage)));
    CHK(ensure_next(c, sorted));
    nsk_ctx::Prep& P = c->req;
    P.valid = true; P.stage = stage; P.N = N; P.S = S; P.ro = ro; P.rd = rd; P.gt = gt; P.gtmax = gtmax; P.mask = c->ray_mask; P.sorted = sorted; P.done = PREP_NOTHING; P.R = c->R; P.dmax = c->dmax;
    return 0;
}

extern "C" int nsk_map_step(nsk_ctx* c, int stage, int N, const float* ro, const float* rd, const float* gt, const float* gtc,
                            float gtmax, float w_color, int use_color, unsigned flags, float* d_loss, float* rgb, float* depth,
                            float* var, float* g_ro, float* g_rd)
{
    int S;
    if (!gt) return fail("nsk_map_step: gt_depth is NULL");
    if (use_color && !gtc) return fail("nsk_map_step: use_color needs gt_color");
    CHK(common_checks(c, stage, N, ro, rd, &S, gt));
    if ((flags & NSK_GRAD_RAYS) && (!g_ro || !g_rd)) return fail("nsk_map_step: NSK_GRAD_RAYS needs g_rays_o and g_rays_d");
    CHK(forward_core(c, stage, N, S, ro, rd, gt, gtmax, true, sort_pays(c, stage, N * S, flags)));
    CompArgs A;
    comp_args(c, A, stage, N, S, ro, rd);
    A.mode = 2; A.gt_depth = gt; A.gt_color = gtc; A.w_color = w_color; A.use_color = use_color;
    A.rgb = rgb; A.depth = depth; A.var = var; A.loss = c->ws.ray_loss;
    if (flags & NSK_GRAD_RAYS) { A.g_rays_o = g_ro; A.g_rays_d = g_rd; }
    A.deal = c->deal_cur;      // the cursors of the backward's queues are zeroed by this launch, whichever form it takes
    SampArgs SA; int sb = 0;
    CHK(prep_ride_sample(c, SA, &sb));
    if (sb) {            // the next batch's sampling behind this batch's compositing, one launch (k_composite_sample)
        const int cb = (N + 7) / 8;
        ProfScope ps(c, "composite"); k_composite_sample<<<cb + sb, 512, 0, c->stream>>>(A, SA, cb);
    } else {
        ProfScope ps(c, "composite"); k_composite<<<(N + 3) / 4, 256, 0, c->stream>>>(A);
    }
    HIPCHK(hipGetLastError());
    c->deal_armed = true;      // only now: the launch is on the stream (an error return above leaves the next backward to arm with its memset)
    CHK(backward_core(c, stage, N, S, ro, rd, flags, g_ro, g_rd, d_loss));
    account(c, stage, N * S, first_pass_samples(c, N, S), true, flags);
    return 0;
}

static int median_thr(nsk_ctx* c, int N, const float* gt, const float* depth)
{
    int P2 = 1; while (P2 < N) P2 <<= 1;
    if (P2 > 16384) return fail("handle_dynamic median supports at most 16384 rays (got %d)", N);
    k_median_thr<<<1, 1024, P2 * 4, c->stream>>>(N, P2, gt, depth, c->ray_mask, c->scal + 1);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_track_step(nsk_ctx* c, int stage, int N, const float* ro, const float* rd, const float* gt, const float* gtc,
                              float gtmax, float w_color, int use_color, int handle_dynamic, int detach_var, unsigned flags,
                              float* d_loss, float* g_ro, float* g_rd)
{
    int S;
    if (!gt) return fail("nsk_track_step: gt_depth is NULL");
    if (use_color && !gtc) return fail("nsk_track_step: use_color needs gt_color");
    CHK(common_checks(c, stage, N, ro, rd, &S, gt));
    if ((flags & NSK_GRAD_RAYS) && (!g_ro || !g_rd)) return fail("nsk_track_step: NSK_GRAD_RAYS needs g_rays_o and g_rays_d");
    CHK(forward_core(c, stage, N, S, ro, rd, gt, gtmax, true, sort_pays(c, stage, N * S, flags)));
    CompArgs A;
    comp_args(c, A, stage, N, S, ro, rd);
    // which median form runs when: median_form (nsk_split.h).  any_trainable: by collect_bwd_roles' rule for a trainable role -- the two must agree
    bool any_trainable = false;
    for (int q = 0; q < 3; ++q) {
        const int w = STAGE_DEC[stage][q];
        if (w >= 0 && (flags & NSK_GRAD_DECODERS) && c->dec[w].trainable) any_trainable = true;
    }
    const MedianForm median = median_form(handle_dynamic != 0, c->deterministic != 0, c->tune_no_fused_median, c->tune_no_deferred_median, N, c->num_cu,
                                          (flags & NSK_GRAD_RAYS) != 0, c->bwd_mode == 0, any_trainable);
    if (median == MEDIAN_THREE) {                                            // forward pass for the median (Tracker.cpp:69-70)
        A.mode = 0; A.depth = c->ws.tmp_depth;
        k_composite<<<(N + 3) / 4, 256, 0, c->stream>>>(A);
        CHK(median_thr(c, N, gt, c->ws.tmp_depth));
        A.depth = nullptr;
    }
    A.gt_depth = gt; A.gt_color = gtc; A.w_color = w_color; A.use_color = use_color;
    A.thr = c->scal + 1; A.handle_dynamic = handle_dynamic; A.detach_var = detach_var; A.loss = c->ws.ray_loss;
    switch (median) {
    case MEDIAN_NONE: case MEDIAN_THREE: A.mode = 3; break;
    case MEDIAN_BARRIER:
        A.mode = 4; c->median_fused_pending = true;
        A.resid = c->ws.tmp_depth; A.bar = reinterpret_cast<unsigned*>(c->scal + 5); A.thr_out = c->scal + 1;
        break;
    case MEDIAN_DEFERRED: A.mode = 5; A.resid = c->ws.tmp_depth; A.g_seed = c->ws.tmp_rgb; break;      // the backward's workgroups apply the mask
    }
    if (flags & NSK_GRAD_RAYS) { A.g_rays_o = g_ro; A.g_rays_d = g_rd; }
    { ProfScope ps(c, "composite"); k_composite<<<(N + 3) / 4, 256, 0, c->stream>>>(A); }
    HIPCHK(hipGetLastError());
    CHK(backward_core(c, stage, N, S, ro, rd, flags, g_ro, g_rd, d_loss, median == MEDIAN_DEFERRED ? c->ws.tmp_depth : nullptr));
    account(c, stage, N * S, first_pass_samples(c, N, S), true, flags);
    return 0;
}

extern "C" int nsk_loss_map(nsk_ctx* c, int N, const float* depth, const float* rgb, const float* gt, const float* gtc, float w_color,
                            int use_color, float* g_depth, float* g_rgb, float* d_loss)
{
    if (!c || !depth || !rgb || !gt || !gtc || !g_depth || !g_rgb) return fail("nsk_loss_map: null argument");
    if (N < 1) return fail("nsk_loss_map: N must be >= 1");
    HIPCHK(hipSetDevice(c->device));
    CHK(ensure_ws(c, N, 1));
    k_loss_map<<<(N + 255) / 256, 256, 0, c->stream>>>(N, depth, rgb, gt, gtc, w_color, use_color, g_depth, g_rgb, c->ws.ray_loss);
    if (d_loss) k_sum<<<1, 1024, 0, c->stream>>>(N, c->ws.ray_loss, d_loss);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_loss_track(nsk_ctx* c, int N, const float* depth, const float* rgb, const float* var, const float* gt,
                              const float* gtc, float w_color, int use_color, int handle_dynamic, int detach_var, float* g_depth,
                              float* g_rgb, float* g_var, float* d_loss)
{
    if (!c || !depth || !rgb || !var || !gt || !gtc || !g_depth || !g_rgb) return fail("nsk_loss_track: null argument");
    if (N < 1) return fail("nsk_loss_track: N must be >= 1");
    HIPCHK(hipSetDevice(c->device));
    CHK(ensure_ws(c, N, 1));
    if (handle_dynamic) CHK(median_thr(c, N, gt, depth));
    k_loss_track<<<(N + 255) / 256, 256, 0, c->stream>>>(N, depth, rgb, var, gt, gtc, w_color, use_color, handle_dynamic, detach_var,
                                                         c->scal + 1, g_depth, g_rgb, g_var, c->ws.ray_loss);
    if (d_loss) k_sum<<<1, 1024, 0, c->stream>>>(N, c->ws.ray_loss, d_loss);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- rays / pose --------------------------------------------------------------------------------------------
static void intr(int mode, float& fx, float& fy, float& cx, float& cy)
{
    if (mode & 2) { fx = (float)(int)fx; fy = (float)(int)fy; cx = (float)(int)cx; cy = (float)(int)cy; }   // D10
}
static void invert4(const float* m, float* inv)          // Gauss-Jordan with partial pivoting, in double
{
    double a[4][8];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { a[i][j] = m[4 * i + j]; a[i][4 + j] = i == j; }
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r) if (fabs(a[r][c]) > fabs(a[p][c])) p = r;
        for (int j = 0; j < 8; ++j) std::swap(a[c][j], a[p][j]);
        double d = a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int r = 0; r < 4; ++r) if (r != c) { double f = a[r][c]; for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j]; }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) inv[4 * i + j] = (float)a[i][4 + j];
}

// ---- test aids: what the last step's forward decided at every ReLU, and the numbers it decided on ----------------------------------
// (read-only views of the workspace; nothing in the product path calls them.  tests/test_gpu_relu.py, tools/relu_flips.py)
extern "C" int nsk_debug_relu_bits(nsk_ctx* c, int which, int M, uint8_t* h_bits /*[M][5][32] by sample*/)
{
    if (!c || !h_bits) return fail("nsk_debug_relu_bits: null argument");
    if (which < 1 || which > 3) return fail("nsk_debug_relu_bits: decoder 1..3");
    if (M < 1 || M != c->dbg_M || M > c->ws.capM) return fail("nsk_debug_relu_bits: M = %d is not the last step's sample count (%d)", M, c->dbg_M);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> mk((size_t)M * 4);
    std::vector<int> perm;
    HIPCHK(hipMemcpy(mk.data(), c->ws.masks[which], mk.size() * 8, hipMemcpyDeviceToHost));
    if (c->sorted) { perm.resize(M); HIPCHK(hipMemcpy(perm.data(), c->ws.cur.perm, (size_t)M * 4, hipMemcpyDeviceToHost)); }
    for (int slot = 0; slot < M; ++slot) {
        const int m = c->sorted ? perm[slot] : slot;
        if (m < 0 || m >= M) return fail("nsk_debug_relu_bits: perm[%d] = %d out of range", slot, m);
        uint8_t* row = h_bits + (size_t)m * 160;
        for (int g = 0; g < 4; ++g) {
            const unsigned long long w = mk[(size_t)slot * 4 + g];
            for (int l = 0; l < 5; ++l)
                for (int r = 0; r < 2; ++r)
                    for (int i = 0; i < 4; ++i) row[32 * l + 16 * r + 4 * g + i] = (uint8_t)((w >> (8 * l + 4 * r + i)) & 1ull);
        }
    }
    return 0;
}
// per-sample arrays of the last step's workspace, by sample: what = 0..2 occupancy of decoder 0..2 [M], 3 colour decoder output [M][4], 4 g_raw [M][4], 5 z [M]
extern "C" int nsk_debug_fetch(nsk_ctx* c, int what, int M, float* h_out)
{
    if (!c || !h_out) return fail("nsk_debug_fetch: null argument");
    if (M < 1 || M != c->dbg_M || M > c->ws.capM) return fail("nsk_debug_fetch: M = %d is not the last step's sample count (%d)", M, c->dbg_M);
    const float* src = what >= 0 && what <= 2 ? c->ws.occ[what] : (what == 3 ? c->ws.rgb4 : (what == 4 ? c->ws.g_raw : (what == 5 ? c->ws.cur.z : (what == 6 ? c->scal + 1 : nullptr))));
    if (!src) return fail("nsk_debug_fetch: what = 0..6");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (what == 6) { HIPCHK(hipMemcpy(h_out, src, 4, hipMemcpyDeviceToHost)); return 0; }      // the Tracker's threshold: one float
    HIPCHK(hipMemcpy(h_out, src, (size_t)M * ((what == 3 || what == 4) ? 16 : 4), hipMemcpyDeviceToHost));
    return 0;
}
// the dead-tile skip of the last step's backward, after a synchronise: tiles run per level, the slot order and the slots' liveness bytes
extern "C" int nsk_debug_live_tiles(nsk_ctx* c, int M, int* h_counts, int32_t* h_perm, uint8_t* h_bytes)
{
    if (!c || !h_counts) return fail("nsk_debug_live_tiles: null argument");
    if (M < 1 || M != c->dbg_M || M > c->ws.capM) return fail("nsk_debug_live_tiles: M = %d is not the last step's sample count (%d)", M, c->dbg_M);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const volatile int* h = c->live_host;
    bool any = false;
    for (int k = 0; k < 3; ++k) { h_counts[k] = c->dbg_counted[k] ? (int)h[k] : c->dbg_live[k]; any = any || c->dbg_counted[k]; }
    h_counts[3] = any ? 1 : 0;
    for (int k = 0; k < 3; ++k) h_counts[4 + k] = c->dbg_wgs[k];
    h_counts[7] = c->dbg_ntasks;
    if (h_perm) {
        if (c->sorted) HIPCHK(hipMemcpy(h_perm, c->ws.cur.perm, (size_t)M * 4, hipMemcpyDeviceToHost));
        else for (int m = 0; m < M; ++m) h_perm[m] = m;
    }
    if (h_bytes) {
        if (c->live_ok) HIPCHK(hipMemcpy(h_bytes, c->sorted ? c->ws.cur.lslot : c->ws.cur.lsamp, (size_t)M, hipMemcpyDeviceToHost));
        else memset(h_bytes, 7, (size_t)M);
    }
    return 0;
}
// the workgroup split of the last forward decoder launch (dir 0) or the last backward (dir 1), as the host recorded it; launches nothing
extern "C" int nsk_debug_last_split(nsk_ctx* c, int dir, int* h_out)
{
    if (!c || !h_out) return fail("nsk_debug_last_split: null argument");
    if (dir != 0 && dir != 1) return fail("nsk_debug_last_split: dir = 0 (forward) or 1 (backward)");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(h_out, c->dbg_split[dir], sizeof(c->dbg_split[dir]));
    return 0;
}
// one of a decoder's device images, to the host (layout: include/nsk.h).  Reads only: the one thing it may launch is the rebuild of a stale fp16
// backward image (ensure_image), which the next backward that reads that image would launch itself.
extern "C" int nsk_debug_decoder_images(nsk_ctx* c, int which, int what, void* h_out, size_t capacity)
{
    if (!c || !which_ok(which)) return fail("nsk_debug_decoder_images: bad argument");
    if (what < 0 || what > 3) return fail("nsk_debug_decoder_images: what = 0 (fp32 forward), 1 (fp32 backward), 2 (forward in pieces), 3 (fp16 backward)");
    if (c->capturing) return fail("nsk_debug_decoder_images: not while a graph is being captured");
    DecState& D = c->dec[which];
    if (!D.loaded) return fail("decoder %d not uploaded", which);
    HIPCHK(hipSetDevice(c->device));
    CHK(ensure_image(c, which, what));
    const float* src = D.img[what].data;
    const size_t bytes = (size_t)D.img[what].spec.floats * 4;               // 0: the coarse decoder has no image in pieces
    if (bytes > (size_t)0x7fffffff) return fail("nsk_debug_decoder_images: image too large");
    if (h_out && bytes) {
        if (capacity < bytes) return fail("nsk_debug_decoder_images: the image has %zu bytes, the buffer %zu", bytes, capacity);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(h_out, src, bytes, hipMemcpyDeviceToHost));
    }
    return (int)bytes;
}
// the index table behind one of those images (nsk_images.h); needs no context and no device
extern "C" int nsk_decoder_image_table(int which, int what, int pieces, int32_t* h_idx, size_t capacity)
{
    if (!which_ok(which)) return fail("nsk_decoder_image_table: decoder %d out of range", which);
    if (what < 0 || what >= NSK_NUM_IMAGES) return fail("nsk_decoder_image_table: what = 0 (fp32 forward), 1 (fp32 backward), 2 (forward in pieces), 3 (fp16 backward)");
    if (pieces != 2 && pieces != 3) return fail("nsk_decoder_image_table: pieces = 2 (fp16) or 3 (bf16)");
    const int n = image_spec(which, what, pieces).entries;
    if (h_idx && n) {
        if (capacity < (size_t)n) return fail("nsk_decoder_image_table: the table has %d entries, capacity %zu", n, capacity);
        std::vector<int> idx;
        build_image_table(which, what, idx);
        memcpy(h_idx, idx.data(), (size_t)n * 4);
    }
    return n;
}
// the ReLU inputs of decoder `which` over the samples of the last step (same rays), by the forward body of the current matmul mode
extern "C" int nsk_debug_preact(nsk_ctx* c, int which, int N, const float* ro, const float* rd, float* d_out /*[M][5][32] device*/)
{
    if (!c || !ro || !rd || !d_out) return fail("nsk_debug_preact: null argument");
    if (which < 1 || which > 3) return fail("nsk_debug_preact: decoder 1..3");
    const int S = c->dbg_S, M = c->dbg_M;
    if (S < 1 || N * S != M) return fail("nsk_debug_preact: N = %d does not match the last step (%d samples, %d per ray)", N, M, S);
    HIPCHK(hipSetDevice(c->device));
    DecArgs A;
    fill_args(c, A, which, M, S, ro, rd, nullptr);
    A.dump = d_out;
    const int grid = std::max(1, std::min(((M + 15) / 16 + 7) / 8, c->num_cu));
    if (c->matmul_mode == 0) k_decode_fwd_dump<0><<<grid, 512, fwd_img_floats(which) * 4, c->stream>>>(A, which);
    else if (c->matmul_mode == 1) k_decode_fwd_dump<1><<<grid, 512, (size_t)c->dec[which].img[2].spec.floats * 4, c->stream>>>(A, which);
    else k_decode_fwd_dump<2><<<grid, 512, (size_t)c->dec[which].img[2].spec.floats * 4, c->stream>>>(A, which);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_frustum_mask(nsk_ctx* c, int level, const float* d_depth, int H, int W, float fx, float fy, float cx, float cy,
                                const float h_c2w[16], uint8_t* h_mask_out)
{
    if (!c || !which_ok(level) || !d_depth || !h_c2w) return fail("nsk_frustum_mask: bad argument");
    GridState& G = c->grid[level];
    if (!G.n) return fail("nsk_frustum_mask: grid level %d not uploaded", level);
    HIPCHK(hipSetDevice(c->device));
    const size_t nvox = G.n / 32;
    if (c->capturing) return fail("nsk_frustum_mask: not while a graph is being captured");
    G.midx_dirty = true; G.live_dirty = true; ++c->live_epoch;
    bool live = false;
    for (auto& R : c->graphs) live = live || !R.stale;
    if (live) { HIPCHK(hipStreamSynchronize(c->stream)); invalidate_graphs(c); }      // new mask contents: see nsk_set_mask
    if (c->slab) HIPCHK(hipMemsetAsync(c->slab + G.g_off, 0, G.n * 4, c->stream));       // see nsk_set_mask
    CHK(grow(c, G.mask, nvox, "the voxel mask", 0));
    if (level == NSK_COARSE) {                                   // src/Mapper.cpp:54-59
        HIPCHK(hipMemsetAsync(G.mask, 1, nvox, c->stream));
    } else {
        CHK(grow(c, c->fr_tmp, nvox * 9 + 16, "the frustum scratch", 0));
        float* dep = reinterpret_cast<float*>(c->fr_tmp.get()); float* zz = dep + nvox;
        uint8_t* inimg = reinterpret_cast<uint8_t*>(zz + nvox);
        unsigned int* dmax = reinterpret_cast<unsigned int*>(c->scal + 4);
        FrustumArgs A;
        memcpy(A.bound, c->R.bound, sizeof(A.bound));
        invert4(h_c2w, A.w2c);
        A.cam[0] = h_c2w[3]; A.cam[1] = h_c2w[7]; A.cam[2] = h_c2w[11];
        A.Z = G.Z; A.Y = G.Y; A.X = G.X; A.H = H; A.W = W; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy;
        HIPCHK(hipMemsetAsync(dmax, 0, 4, c->stream));
        int blocks = (int)((nvox + 255) / 256);
        k_frustum_pass1<<<blocks, 256, 0, c->stream>>>(A, d_depth, dep, zz, inimg, dmax);
        k_frustum_pass2<<<blocks, 256, 0, c->stream>>>(A, dep, zz, inimg, dmax, G.mask);
        HIPCHK(hipGetLastError());
    }
    if (h_mask_out) {
        HIPCHK(hipMemcpyAsync(h_mask_out, G.mask, nvox, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int nsk_keyframe_overlap(nsk_ctx* c, int N, const float* d_ro, const float* d_rd, const float* d_gt_depth, int n_samples,
                                    int H, int W, float fx, float fy, float cx, float cy, int K, const float* h_c2w, float* h_percent)
{
    if (!c || !d_ro || !d_rd || !d_gt_depth || !h_c2w || !h_percent) return fail("nsk_keyframe_overlap: null argument");
    if (N <= 0 || n_samples <= 0 || K < 0) return fail("nsk_keyframe_overlap: bad sizes");
    if (K == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    std::vector<float> w2c((size_t)K * 16);
    for (int k = 0; k < K; ++k) invert4(h_c2w + 16 * k, w2c.data() + 16 * k);
    CHK(grow(c, c->fr_tmp, (size_t)K * 17 * 4, "the keyframe scratch", 0));
    float* d_w2c = reinterpret_cast<float*>(c->fr_tmp.get()); float* d_pct = d_w2c + (size_t)K * 16;
    HIPCHK(hipMemcpyAsync(d_w2c, w2c.data(), (size_t)K * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));         // w2c is a stack-lifetime host buffer
    OverlapArgs A; A.N = N; A.ns = n_samples; A.H = H; A.W = W; A.K = K; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy;
    k_keyframe_overlap<<<K, 256, 0, c->stream>>>(A, d_ro, d_rd, d_gt_depth, d_w2c, d_pct);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_percent, d_pct, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int nsk_sample_pixels(nsk_ctx* c, unsigned long long seed, int n, int H0, int H1, int W0, int W1, int32_t* d_pix_i, int32_t* d_pix_j)
{
    if (!c || !d_pix_i || !d_pix_j) return fail("nsk_sample_pixels: null argument");
    if (n < 0 || H1 <= H0 || W1 <= W0) return fail("nsk_sample_pixels: empty window [%d,%d) x [%d,%d)", H0, H1, W0, W1);
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    k_sample_pixels<<<(n + 255) / 256, 256, 0, c->stream>>>(seed, n, H0, W0, W1 - W0, (unsigned long long)(H1 - H0) * (unsigned long long)(W1 - W0), d_pix_i, d_pix_j);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_gather_pixels(nsk_ctx* c, int n, const int32_t* d_pix_i, const int32_t* d_pix_j, int H, int W, const float* d_depth,
                                 const float* d_color, float* d_gt_depth, float* d_gt_color)
{
    if (!c || !d_pix_i || !d_pix_j || !d_depth || !d_gt_depth) return fail("nsk_gather_pixels: null argument");
    if (n < 0 || H <= 0 || W <= 0) return fail("nsk_gather_pixels: bad sizes");
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    k_gather_pixels<<<(n + 255) / 256, 256, 0, c->stream>>>(n, d_pix_i, d_pix_j, W, d_depth, d_color, d_gt_depth, d_gt_color);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_rays_from_pixels(nsk_ctx* c, int n, const int32_t* pi, const int32_t* pj, float fx, float fy, float cx, float cy,
                                    const float* c2w, int mode, float* ro, float* rd)
{
    if (!c || !pi || !pj || !c2w || !ro || !rd || n < 1) return fail("nsk_rays_from_pixels: bad argument");
    intr(mode, fx, fy, cx, cy);
    k_rays_from_pixels<<<(n + 255) / 256, 256, 0, c->stream>>>(n, pi, pj, fx, fy, cx, cy, c2w, mode, ro, rd);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_rays_backward(nsk_ctx* c, int n, const int32_t* pi, const int32_t* pj, float fx, float fy, float cx, float cy, int mode,
                                 const float* g_ro, const float* g_rd, float* g_c2w)
{
    if (!c || !pi || !pj || !g_ro || !g_rd || !g_c2w || n < 1) return fail("nsk_rays_backward: bad argument");
    intr(mode, fx, fy, cx, cy);
    k_rays_backward<<<1, 256, 0, c->stream>>>(n, pi, pj, fx, fy, cx, cy, mode, g_ro, g_rd, g_c2w);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_camera_from_tensor(nsk_ctx* c, const float* cam, float* c2w)
{
    if (!c || !cam || !c2w) return fail("nsk_camera_from_tensor: null argument");
    k_camera_from_tensor<<<1, 1, 0, c->stream>>>(cam, c2w);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_camera_backward(nsk_ctx* c, const float* cam, const float* g_c2w, float* g_cam)
{
    if (!c || !cam || !g_c2w || !g_cam) return fail("nsk_camera_backward: null argument");
    k_camera_backward<<<1, 1, 0, c->stream>>>(cam, g_c2w, g_cam);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_rays_from_camera(nsk_ctx* c, int n, const int32_t* pi, const int32_t* pj, float fx, float fy, float cx, float cy,
                                    const float* d_cam, int mode, float* ro, float* rd, float* d_c2w_out)
{
    if (!c || !pi || !pj || !d_cam || !ro || !rd || n < 1) return fail("nsk_rays_from_camera: bad argument");
    intr(mode, fx, fy, cx, cy);
    k_rays_from_camera<<<(n + 255) / 256, 256, 0, c->stream>>>(n, pi, pj, fx, fy, cx, cy, d_cam, mode, ro, rd, d_c2w_out);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_pose_step(nsk_ctx* c, int n, const int32_t* pi, const int32_t* pj, float fx, float fy, float cx, float cy, int mode,
                             const float* g_ro, const float* g_rd, float* d_cam, float* d_m, float* d_v, float lr, float b1, float b2, float eps,
                             int step, float* d_g_cam_out)
{
    if (!c || !pi || !pj || !g_ro || !g_rd || !d_cam || !d_m || !d_v || n < 1 || step < 1) return fail("nsk_pose_step: bad argument");
    intr(mode, fx, fy, cx, cy);
    float ss, bc2s; adam_consts(lr, b1, b2, step, ss, bc2s);
    k_pose_step<<<1, 256, 0, c->stream>>>(n, pi, pj, fx, fy, cx, cy, mode, g_ro, g_rd, d_cam, d_m, d_v, ss, bc2s, b1, b2, eps, d_g_cam_out);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_pose_step_multi(nsk_ctx* c, int nframes, const int* h_first, const int* h_count, const uint8_t* h_active, const int32_t* pi, const int32_t* pj,
                                   float fx, float fy, float cx, float cy, int mode, const float* g_ro, const float* g_rd, float* d_cams, float* d_m, float* d_v,
                                   float lr, float b1, float b2, float eps, int step, float* d_g_cams, const uint8_t* d_keep, int n_keep)
{
    if (!c || !h_first || !h_count || !h_active || !pi || !pj || !g_ro || !g_rd || !d_cams) return fail("nsk_pose_step_multi: null argument");
    if (nframes < 1 || nframes > NSK_MAX_POSE_FRAMES) return fail("nsk_pose_step_multi: 1 <= nframes <= %d (got %d)", NSK_MAX_POSE_FRAMES, nframes);
    if (step < 0 || (step > 0 && (!d_m || !d_v))) return fail("nsk_pose_step_multi: step >= 1 needs the Adam moments (step 0 = gradients only)");
    if (step == 0 && !d_g_cams) return fail("nsk_pose_step_multi: step 0 (gradients only) needs d_g_cams");
    HIPCHK(hipSetDevice(c->device));
    PoseFrames F; memset(&F, 0, sizeof(F));
    for (int f = 0; f < nframes; ++f) {
        if (h_first[f] < 0 || h_count[f] < 0) return fail("nsk_pose_step_multi: frame %d has a negative ray range", f);
        F.first[f] = h_first[f]; F.count[f] = h_count[f]; F.active[f] = h_active[f] ? 1 : 0;
    }
    intr(mode, fx, fy, cx, cy);
    float ss = 0.f, bc2s = 1.f;
    if (step > 0) adam_consts(lr, b1, b2, step, ss, bc2s);
    const int count_block = (d_g_cams && n_keep > 0) ? 1 : 0;
    ProfScope ps(c, "pose_multi");
    k_pose_multi<<<nframes + count_block, 256, 0, c->stream>>>(F, nframes, pi, pj, fx, fy, cx, cy, mode, g_ro, g_rd, d_cams, d_m, d_v, ss, bc2s, b1, b2, eps,
                                                             step > 0 ? 1 : 0, d_g_cams, d_keep, n_keep);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int nsk_set_depth_max_batch(nsk_ctx* c, const float* d_gt_depth, const uint8_t* d_keep, int n)
{
    if (!c) return fail("null ctx");
    if (n < 0 || (n > 0 && !d_gt_depth)) return fail("nsk_set_depth_max_batch: bad argument");
    c->dmax.gt = n > 0 ? d_gt_depth : nullptr; c->dmax.keep = n > 0 ? d_keep : nullptr; c->dmax.n = n;
    return 0;
}
extern "C" int nsk_grad_extra(nsk_ctx* c, float* d_buf, size_t n_floats)
{
    if (!c) return fail("null ctx");
    if (n_floats % 4 != 0 || (n_floats > 0 && !d_buf)) return fail("nsk_grad_extra: a device buffer of a multiple of 4 floats (or 0 floats to remove it)");
    if (((uintptr_t)d_buf & 15) != 0) return fail("nsk_grad_extra: the buffer must be 16-byte aligned");
    c->xextra = n_floats ? d_buf : nullptr; c->xextra_n = n_floats;
    return 0;
}
extern "C" int nsk_prepare_rays(nsk_ctx* c, int nframes, const nsk_frame_rays* fr, int per, int H0, int H1, int W0, int W1, int H, int W,
                                float fx, float fy, float cx, float cy, int mode, int32_t* pi, int32_t* pj, float* gd, float* gc,
                                float* ro, float* rd, uint8_t* keep)
{
    if (!c || !fr || !pi || !pj || !gd || !ro || !rd) return fail("nsk_prepare_rays: null argument");
    if (nframes < 1 || nframes > 64 || per < 1) return fail("nsk_prepare_rays: nframes must be 1..64 and rays_per_frame >= 1");
    if (H1 <= H0 || W1 <= W0 || H0 < 0 || W0 < 0 || H1 > H || W1 > W) return fail("nsk_prepare_rays: window [%d,%d) x [%d,%d) outside the %d x %d image", H0, H1, W0, W1, H, W);
    HIPCHK(hipSetDevice(c->device));
    intr(mode, fx, fy, cx, cy);
    for (int f0 = 0; f0 < nframes; f0 += 16) {
        PrepArgs A;
        memset(&A, 0, sizeof(A));
        A.nframes = std::min(16, nframes - f0);
        for (int i = 0; i < A.nframes; ++i) {
            const nsk_frame_rays& s = fr[f0 + i];
            if (!s.d_depth || !s.d_pose) return fail("nsk_prepare_rays: frame %d has no depth image or pose", f0 + i);
            A.f[i].depth = s.d_depth; A.f[i].color = s.d_color; A.f[i].pose = s.d_pose; A.f[i].cam7 = s.pose_is_cam7; A.f[i].seed = s.seed;
        }
        const size_t o = (size_t)f0 * per;
        A.per = per; A.H0 = H0; A.W0 = W0; A.Ww = W1 - W0; A.W = W; A.mode = mode;
        A.total = (unsigned long long)(H1 - H0) * (unsigned long long)(W1 - W0);
        A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy;
        A.pi = pi + o; A.pj = pj + o; A.gd = gd + o; A.gc = gc ? gc + 3 * o : nullptr; A.ro = ro + 3 * o; A.rd = rd + 3 * o; A.keep = keep ? keep + o : nullptr;
        A.R = c->R;
        { ProfScope ps(c, "prepare_rays"); k_prepare_rays<<<dim3((per + 255) / 256, A.nframes), 256, 0, c->stream>>>(A); }
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// ---- whole frames (nsk_image.h) ------------------------------------------------------------------------------------
// the view's extents; every argument is checked here, before anything is launched
static int view_checks(const char* fn, nsk_ctx* c, int H0, int H1, int W0, int W1, int stride, int H, int W, int* Hv, int* Wv)
{
    if (!c) return fail("%s: null ctx", fn);
    if (H < 1 || W < 1) return fail("%s: H, W = %d x %d, the image must have at least one pixel", fn, H, W);
    if (stride < 1) return fail("%s: stride = %d, must be >= 1", fn, stride);
    if (H0 < 0 || H1 <= H0 || H1 > H) return fail("%s: window rows H0, H1 = [%d,%d) outside the %d x %d image", fn, H0, H1, H, W);
    if (W0 < 0 || W1 <= W0 || W1 > W) return fail("%s: window columns W0, W1 = [%d,%d) outside the %d x %d image", fn, W0, W1, H, W);
    *Hv = (H1 - H0 + stride - 1) / stride; *Wv = (W1 - W0 + stride - 1) / stride;
    if ((long long)*Hv * *Wv > (1LL << 30)) return fail("%s: the view has %lld pixels (at most 2^30)", fn, (long long)*Hv * *Wv);
    return 0;
}
static int launch_image_rays(nsk_ctx* c, int first, int n, int H0, int W0, int stride, int Wv, int W, float fx, float fy, float cx, float cy,
                             const float* pose, int cam7, int mode, const float* depth_img, float* ro, float* rd, float* gd)
{
    ImgView V;
    V.H0 = H0; V.W0 = W0; V.stride = stride; V.Wv = Wv; V.W = W; V.first = first; V.n = n; V.mode = mode;
    V.fx = fx; V.fy = fy; V.cx = cx; V.cy = cy;
    { ProfScope ps(c, "image_rays"); k_image_rays<<<(n + 255) / 256, 256, 0, c->stream>>>(V, pose, cam7, depth_img, ro, rd, depth_img ? gd : nullptr); }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_image_rays(nsk_ctx* c, int first, int n, int H0, int H1, int W0, int W1, int stride, int H, int W, float fx, float fy,
                              float cx, float cy, const float* d_pose, int pose_is_cam7, int mode, const float* d_depth_img, float* d_rays_o,
                              float* d_rays_d, float* d_gt_depth)
{
    int Hv, Wv;
    CHK(view_checks("nsk_image_rays", c, H0, H1, W0, W1, stride, H, W, &Hv, &Wv));
    if (first < 0 || n < 1 || (long long)first + n > (long long)Hv * Wv)
        return fail("nsk_image_rays: first, n = %d, %d outside the view's %lld pixels", first, n, (long long)Hv * Wv);
    if (!d_pose) return fail("nsk_image_rays: d_pose is NULL");
    if (!d_rays_o || !d_rays_d) return fail("nsk_image_rays: d_rays_o / d_rays_d is NULL");
    if ((d_depth_img != nullptr) != (d_gt_depth != nullptr)) return fail("nsk_image_rays: d_gt_depth must be given exactly when d_depth_img is");
    HIPCHK(hipSetDevice(c->device));
    intr(mode, fx, fy, cx, cy);
    return launch_image_rays(c, first, n, H0, W0, stride, Wv, W, fx, fy, cx, cy, d_pose, pose_is_cam7, mode, d_depth_img, d_rays_o, d_rays_d, d_gt_depth);
}

extern "C" int nsk_render_image(nsk_ctx* c, int stage, int H0, int H1, int W0, int W1, int stride, int H, int W, float fx, float fy, float cx,
                                float cy, const float* d_pose, int pose_is_cam7, int mode, const float* d_depth_img, float gt_depth_max,
                                int chunk_rays, float* d_rgb, float* d_depth, float* d_var)
{
    int Hv, Wv;
    CHK(view_checks("nsk_render_image", c, H0, H1, W0, W1, stride, H, W, &Hv, &Wv));
    if (!d_pose) return fail("nsk_render_image: d_pose is NULL");
    if (!d_rgb || !d_depth || !d_var) return fail("nsk_render_image: d_rgb / d_depth / d_var is NULL");
    CHK(check_stage(c, stage));
    const int S = c->R.n_samples + (d_depth_img ? c->R.n_surface : 0) + c->n_importance;
    const int chunk_max = (int)(((1LL << 26) - 1) / S);
    if (chunk_rays < 1 || chunk_rays > chunk_max)
        return fail("nsk_render_image: chunk_rays = %d, must be 1..%d (%d samples per ray, fewer than 2^26 samples per chunk)", chunk_rays, chunk_max, S);
    if (c->capturing) return fail("nsk_render_image: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    const int total = Hv * Wv, chunk = std::min(chunk_rays, total);
    CHK(ensure_ws(c, chunk, chunk * S));
    nsk_ctx::Image& I = c->img;
    if ((size_t)chunk > I.gd.cap()) {
        CHK(grow_begin(c, GROW_NO_CAPTURE));
        const int r = [&]() -> int {
            CHK(dev_alloc(I.ro, (size_t)chunk * 3, "the chunk's ray origins")); CHK(dev_alloc(I.rd, (size_t)chunk * 3, "the chunk's ray directions"));
            CHK(dev_alloc(I.gd, (size_t)chunk, "the chunk's depths"));
            return 0;
        }();
        if (r != 0) { reset_all(I.ro, I.rd, I.gd); return r; }
    }
    intr(mode, fx, fy, cx, cy);
    const nsk_ctx::DMax own;                                // a chunk's maximum is its own: an installed depth-max batch describes another batch
    const float* gt = d_depth_img ? I.gd.get() : nullptr;
    for (int first = 0; first < total; first += chunk) {
        const int n = std::min(chunk, total - first);
        CHK(launch_image_rays(c, first, n, H0, W0, stride, Wv, W, fx, fy, cx, cy, d_pose, pose_is_cam7, mode, d_depth_img, I.ro, I.rd, I.gd));
        CHK(forward_core(c, stage, n, S, I.ro, I.rd, gt, gt ? gt_depth_max : -1.f, false, false, &own));
        CompArgs A;
        comp_args(c, A, stage, n, S, I.ro, I.rd);
        A.keep = nullptr;                                   // (mode 0 does not read it: a render shows every ray)
        A.rgb = d_rgb + 3 * (size_t)first; A.depth = d_depth + first; A.var = d_var + first; A.weights = nullptr; A.mode = 0;
        { ProfScope ps(c, "composite"); k_composite<<<(n + 3) / 4, 256, 0, c->stream>>>(A); }
        HIPCHK(hipGetLastError());
    }
    account(c, stage, S, first_pass_samples(c, 1, S), false, 0);
    c->last_bytes *= total; c->last_flops *= total; c->last_samples = (int)std::min<long long>((long long)total * c->last_samples, 0x7fffffffLL);
    return 0;
}

extern "C" int nsk_image_metrics(nsk_ctx* c, int Hv, int Wv, const float* d_rgb, const float* d_depth, const float* d_gt_depth,
                                 const float* d_gt_color, float* d_res_depth, float* d_res_color, double h_out[8])
{
    if (!c) return fail("nsk_image_metrics: null ctx");
    if (Hv < 1 || Wv < 1 || (long long)Hv * Wv > (1LL << 30)) return fail("nsk_image_metrics: Hv, Wv = %d x %d, need 1 .. 2^30 pixels", Hv, Wv);
    if (!d_rgb || !d_depth) return fail("nsk_image_metrics: d_rgb / d_depth is NULL");
    if (!h_out) return fail("nsk_image_metrics: h_out is NULL");
    if (d_res_depth && !d_gt_depth) return fail("nsk_image_metrics: d_res_depth asked for without d_gt_depth");
    if (d_res_color && !d_gt_color) return fail("nsk_image_metrics: d_res_color asked for without d_gt_color");
    if (c->capturing) return fail("nsk_image_metrics: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    const int n = Hv * Wv;
    double cols[IMG_COLS];
    CHK(rows_reduce<RowSums<IMG_COLS>>(c, "image_metrics", "the metrics' partial sums", 1, n, 256, IMG_MAX_ROWS, [&](int nrows, double* rows) {
        k_image_metrics<<<nrows, 256, 0, c->stream>>>(n, d_rgb, d_depth, d_gt_depth, d_gt_color, d_res_depth, d_res_color, rows); }, cols));
    // h_out: 0 pixels, 1 depth pixels, 2 depth sum, 3 colour components, 4 colour sum, 5 non-finite pixels, 6 / 7 spare
    h_out[0] = (double)n;
    for (int k = 0; k < 4; ++k) h_out[1 + k] = cols[k];
    h_out[5] = cols[4]; h_out[6] = h_out[7] = 0.0;
    return 0;
}

// ---- structural similarity (nsk_ssim.h) ------------------------------------------------------------------------------------------
template <int C, class T>
static int ssim_level(nsk_ctx* c, const SsimArgs& A, const T* a, const T* b, float* d_map, double* rows, double* out)
{
    const int n = A.Hm * A.Wm;
    double* terms = c->ssim.terms;
    { ProfScope ps(c, "ssim_tile");
      k_ssim_tile<T><<<dim3((unsigned)(A.tiles_x * ((A.Hm + SSIM_TILE_H - 1) / SSIM_TILE_H)), (unsigned)C), 256, 0, c->stream>>>(A, a, b, terms, d_map); }
    HIPCHK(hipGetLastError());
    return rows_launch<RowSums<3 * C>>(c, "ssim_sums", 1, rows_count(n, 256, IMG_MAX_ROWS), rows, out, [&](int nrows, double* r) {
        k_ssim_sums<C><<<nrows, 256, 0, c->stream>>>(n, terms, r); });
}

template <int C>
static int ssim_run(nsk_ctx* c, int levels, const int* Hl, const int* Wl, const float* d_a, const float* d_b, int win, const double* g, double C1,
                    double C2, float* d_map, double* h_sums)
{
    // per level its partial rows, then every level's 3 C results side by side: one copy, one synchronisation
    const size_t per = (size_t)IMG_MAX_ROWS * 3 * C;
    double* rows = c->rows;
    double* out = rows + (size_t)levels * per;
    size_t off = 0, half = 0;
    for (int l = 1; l < levels; ++l) half += (size_t)Hl[l] * Wl[l] * C;
    const double* pa = nullptr; const double* pb = nullptr;
    for (int l = 0; l < levels; ++l) {
        if (l > 0) {                                        // level l from level l - 1
            double* na = c->ssim.pyr.get() + off; double* nb = na + half;
            const size_t n = (size_t)Hl[l] * Wl[l] * C;
            const dim3 grid((unsigned)((n + 255) / 256), 2);
            { ProfScope ps(c, "ssim_pool");
              if (l == 1) k_ssim_pool<float><<<grid, 256, 0, c->stream>>>(Hl[0], Wl[0], C, Hl[1], Wl[1], d_a, d_b, na, nb);
              else k_ssim_pool<double><<<grid, 256, 0, c->stream>>>(Hl[l - 1], Wl[l - 1], C, Hl[l], Wl[l], pa, pb, na, nb); }
            HIPCHK(hipGetLastError());
            pa = na; pb = nb; off += n;
        }
        SsimArgs A;
        A.H = Hl[l]; A.W = Wl[l]; A.C = C; A.win = win; A.Hm = Hl[l] - win + 1; A.Wm = Wl[l] - win + 1;
        A.tiles_x = (A.Wm + SSIM_TILE_W - 1) / SSIM_TILE_W; A.C1 = C1; A.C2 = C2;
        for (int k = 0; k < SSIM_MAX_WIN; ++k) A.g[k] = k < win ? g[k] : 0.0;
        if (l == 0) CHK((ssim_level<C, float>(c, A, d_a, d_b, d_map, rows, out)));
        else CHK((ssim_level<C, double>(c, A, pa, pb, nullptr, rows + l * per, out + (size_t)l * 3 * C)));
    }
    HIPCHK(hipMemcpyAsync(h_sums, out, (size_t)levels * 3 * C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static bool pos_finite(double v) { return v > 0.0 && v < std::numeric_limits<double>::infinity(); }

extern "C" int nsk_image_ssim(nsk_ctx* c, int Hv, int Wv, int C, const float* d_a, const float* d_b, int win, double sigma, double data_range,
                              double k1, double k2, int levels, const double* h_weights, float* d_map, double h_out[8], double* h_levels)
{
    if (!c) return fail("nsk_image_ssim: null ctx");
    if (!d_a || !d_b) return fail("nsk_image_ssim: d_a / d_b is NULL");
    if (!h_out) return fail("nsk_image_ssim: h_out is NULL");
    if (C < 1 || C > SSIM_MAX_C) return fail("nsk_image_ssim: C = %d, must be 1..%d", C, SSIM_MAX_C);
    if (win < 3 || win > SSIM_MAX_WIN || win % 2 == 0) return fail("nsk_image_ssim: win = %d, must be odd and 3..%d", win, SSIM_MAX_WIN);
    if (!pos_finite(sigma)) return fail("nsk_image_ssim: sigma = %g, must be positive and finite", sigma);
    if (!pos_finite(data_range)) return fail("nsk_image_ssim: data_range = %g, must be positive and finite", data_range);
    if (!pos_finite(k1)) return fail("nsk_image_ssim: k1 = %g, must be positive and finite", k1);
    if (!pos_finite(k2)) return fail("nsk_image_ssim: k2 = %g, must be positive and finite", k2);
    if (Hv < win || Wv < win || (long long)Hv * Wv > (1LL << 30) / SSIM_MAX_C)
        return fail("nsk_image_ssim: Hv, Wv = %d x %d, need at least win = %d on both sides and at most 2^28 pixels", Hv, Wv, win);
    if (levels < 1 || levels > SSIM_MAX_LEVELS) return fail("nsk_image_ssim: levels = %d, must be 1..%d", levels, SSIM_MAX_LEVELS);
    if (!h_weights && levels != 1 && levels != 5) return fail("nsk_image_ssim: h_weights is NULL (only levels = 1, or 5 with the standard weights, need none)");
    int Hl[SSIM_MAX_LEVELS], Wl[SSIM_MAX_LEVELS];
    const int bad = ssim_plan_levels(Hv, Wv, win, levels, Hl, Wl);
    if (bad >= 0)
        return fail("nsk_image_ssim: level %d of %d x %d is %d x %d, smaller than win = %d; with levels = %d the smallest side that would do is %lld",
                    bad, Hv, Wv, Hl[bad], Wl[bad], win, levels, ssim_min_side(win, levels));
    if (c->capturing) return fail("nsk_image_ssim: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    size_t pyr = 0;
    for (int l = 1; l < levels; ++l) pyr += (size_t)Hl[l] * Wl[l] * C * 2;
    CHK(grow(c, c->ssim.pyr, pyr, "the pooled levels", GROW_NO_CAPTURE));
    CHK(grow(c, c->ssim.terms, (size_t)(Hv - win + 1) * (Wv - win + 1) * C * 2, "the windows' values", GROW_NO_CAPTURE));
    CHK(grow(c, c->rows, (size_t)levels * (IMG_MAX_ROWS + 1) * 3 * C, "the similarity's partial sums", GROW_NO_CAPTURE));
    double g[SSIM_MAX_WIN];
    ssim_window(win, sigma, g);
    const double C1 = (k1 * data_range) * (k1 * data_range), C2 = (k2 * data_range) * (k2 * data_range);
    double sums[SSIM_MAX_LEVELS * SSIM_MAX_C * 3];
    switch (C) {
        case 1: CHK(ssim_run<1>(c, levels, Hl, Wl, d_a, d_b, win, g, C1, C2, d_map, sums)); break;
        case 2: CHK(ssim_run<2>(c, levels, Hl, Wl, d_a, d_b, win, g, C1, C2, d_map, sums)); break;
        case 3: CHK(ssim_run<3>(c, levels, Hl, Wl, d_a, d_b, win, g, C1, C2, d_map, sums)); break;
        default: CHK(ssim_run<4>(c, levels, Hl, Wl, d_a, d_b, win, g, C1, C2, d_map, sums)); break;
    }
    ssim_combine(levels, C, sums, h_weights ? h_weights : ssim_standard_weights(), h_levels, h_out);
    double counted = 0.0, windows = 0.0;
    for (int l = 0; l < levels; ++l) {
        windows += (double)(Hl[l] - win + 1) * (Wl[l] - win + 1) * C;
        for (int ch = 0; ch < C; ++ch) counted += sums[(l * C + ch) * 3 + 2];
    }
    h_out[2] = counted; h_out[3] = windows - counted; h_out[4] = (double)levels;
    h_out[5] = (double)(Hv - win + 1); h_out[6] = (double)(Wv - win + 1); h_out[7] = 0.0;
    return 0;
}

// ---- reconstruction metrics (nsk_cloud.h) -----------------------------------------------------------------------------------------
extern "C" int nsk_mesh_sample(nsk_ctx* c, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles,
                               unsigned long long seed, int n, float* d_points, int32_t* d_tri, double* h_area, int* h_degenerate)
{
    if (!c) return fail("nsk_mesh_sample: null ctx");
    if (n_triangles < 0 || n_vertices < 0 || n < 0) return fail("nsk_mesh_sample: negative count");
    if (n_triangles == 0) return fail("nsk_mesh_sample: the mesh has no triangle");
    if (!d_vertices || !d_triangles) return fail("nsk_mesh_sample: d_vertices / d_triangles is NULL");
    if (n > 0 && !d_points) return fail("nsk_mesh_sample: d_points is NULL");
    if (c->capturing) return fail("nsk_mesh_sample: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Cloud& K = c->cloud;
    const int nb = (int)(((long long)n_triangles + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
    CHK(grow(c, K.cum, (size_t)n_triangles, "the cumulative triangle areas", GROW_NO_CAPTURE));
    CHK(grow(c, K.bsum, (size_t)nb, "the area sums of the workgroups", GROW_NO_CAPTURE));
    CHK(grow(c, K.degenerate, 16, "the degenerate-triangle count", GROW_NO_CAPTURE));
    double total = 0.0; unsigned degenerate = 0;
    { ProfScope ps(c, "mesh_area");
      HIPCHK(hipMemsetAsync(K.degenerate, 0, 4, c->stream));
      k_tri_area<<<nb, CLOUD_BLOCK, 0, c->stream>>>(n_vertices, n_triangles, d_vertices, d_triangles, K.cum, K.bsum, K.degenerate);
      k_tri_area_sums<<<1, CLOUD_BLOCK, 0, c->stream>>>(nb, K.bsum);
      k_tri_area_add<<<nb, CLOUD_BLOCK, 0, c->stream>>>(n_triangles, K.cum, K.bsum);
      HIPCHK(hipGetLastError()); }
    HIPCHK(hipMemcpyAsync(&total, K.cum.get() + (n_triangles - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&degenerate, K.degenerate, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h_area) *h_area = total;
    if (h_degenerate) *h_degenerate = (int)degenerate;
    if (!(total > 0.0)) return fail("nsk_mesh_sample: the mesh has no area (%u of %d triangles degenerate)", degenerate, n_triangles);
    if (n == 0) return 0;
    { ProfScope ps(c, "mesh_sample");
      k_mesh_sample<<<(n + CLOUD_BLOCK - 1) / CLOUD_BLOCK, CLOUD_BLOCK, 0, c->stream>>>(seed, n, n_triangles, K.cum, d_vertices, d_triangles, d_points, d_tri);
      HIPCHK(hipGetLastError()); }
    return 0;
}

// The grid of nsk_cloud_nearest from the box of the finite targets: cubic cells, about cells_x4 / 4 of them per target, at most 2^22.
// An axis shorter than the edge (zero extent included) gets one cell, and the edge is found again from the other axes.
static CloudGrid cloud_grid(const float* box, unsigned nfinite, int cells_x4)
{
    CloudGrid G;
    G.nfinite = (int)nfinite;
    for (int a = 0; a < 3; ++a) { G.lo[a] = nfinite ? box[a] : 0.f; G.dim[a] = 1; }
    G.h = 1.f; G.inv_h = 1.f;
    if (!nfinite) return G;
    double ext[3], big = 0.0;
    bool on[3];
    for (int a = 0; a < 3; ++a) {
        ext[a] = (double)box[3 + a] - (double)box[a]; on[a] = ext[a] > 0.0;
        big = std::max(big, std::max(std::fabs((double)box[a]), std::fabs((double)box[3 + a])));
    }
    const double want = std::min((double)CLOUD_MAX_CELLS, std::max(1.0, (double)nfinite * cells_x4 / 4.0));
    double h = 1.0;
    for (;;) {
        int k = 0; double logv = 0.0;
        for (int a = 0; a < 3; ++a) if (on[a]) { ++k; logv += std::log(ext[a]); }
        if (k == 0) return G;                                  // every target at one point: one cell
        h = std::exp((logv - std::log(want)) / k);
        bool dropped = false;
        for (int a = 0; a < 3; ++a) if (on[a] && ext[a] < h) { on[a] = false; dropped = true; }
        if (!dropped) break;
    }
    h = std::max(h, std::max(big * 9.5367431640625e-7, 1e-30));        // 8 ulp of the largest coordinate: the planes lo + k h stay distinct
    h = std::min(h, 1e37);
    for (;;) {
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) { G.dim[a] = on[a] ? (int)std::min(std::floor(ext[a] / h) + 1.0, (double)CLOUD_MAX_CELLS) : 1; cells *= G.dim[a]; }
        if (cells <= (double)CLOUD_MAX_CELLS) break;
        h *= 1.25;
    }
    G.h = (float)h; G.inv_h = 1.f / G.h;
    return G;
}

// the box {min x y z, max x y z} of the finite points and their number (one synchronisation)
static int cloud_box(nsk_ctx* c, const float* d_pts, int n, float box[6], unsigned& nfinite)
{
    double cols[7];
    CHK(rows_reduce<CloudBoxCols>(c, "cloud_box", "the partial boxes", 1, n, CLOUD_BLOCK, CLOUD_MAX_ROWS, [&](int nrows, double* rows) {
        k_cloud_box<<<nrows, CLOUD_BLOCK, 0, c->stream>>>(n, d_pts, rows); }, cols));
    for (int k = 0; k < 6; ++k) box[k] = (float)cols[k];     // (floats widened by the kernel: the same floats)
    nfinite = (unsigned)cols[6];
    return 0;
}

// nsk_cloud_nearest in two halves, so that nsk_cloud_icp builds the targets' grid once and queries it at every evaluation.
struct CloudBuilt { CloudGrid G; size_t cells = 0, words = 0; unsigned nfinite = 0; };
// the box (one synchronisation) and, with `place`, the grid: cells -> scan -> placement into c->cloud.start / sorted
static int cloud_build(nsk_ctx* c, const float* d_target, int n_target, bool place, CloudBuilt& B)
{
    nsk_ctx::Cloud& K = c->cloud;
    float box[6];
    CHK(cloud_box(c, d_target, n_target, box, B.nfinite));                                                     // pass 1
    if (!place) return 0;
    B.G = cloud_grid(box, B.nfinite, K.cells_x4);
    B.cells = (size_t)B.G.dim[0] * B.G.dim[1] * B.G.dim[2]; B.words = mc_scan_words(B.cells + 1);
    if (B.nfinite) {
        const int tb = (int)(((long long)n_target + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
        CHK(grow(c, K.tcell, (size_t)n_target, "the targets' cells", GROW_NO_CAPTURE));
        CHK(grow(c, K.sorted, (size_t)n_target, "the targets in cell order", GROW_NO_CAPTURE));
        CHK(grow(c, K.start, B.words, "the cells' first targets", GROW_NO_CAPTURE));
        CHK(grow(c, K.cursor, B.cells, "the cells' placement cursors", GROW_NO_CAPTURE));
        ProfScope ps(c, "cloud_grid");
        HIPCHK(hipMemsetAsync(K.start, 0, B.words * 4, c->stream));
        HIPCHK(hipMemsetAsync(K.cursor, 0, B.cells * 4, c->stream));
        k_cloud_cells<<<tb, CLOUD_BLOCK, 0, c->stream>>>(B.G, n_target, d_target, 0, K.tcell, K.start);        // pass 2
        HIPCHK(hipGetLastError());
        CHK(mc_scan(c, K.start, (int)B.cells + 1));                                                           // pass 3
        k_cloud_place<<<tb, CLOUD_BLOCK, 0, c->stream>>>(n_target, d_target, K.tcell, K.start, K.cursor, K.sorted, nullptr);      // pass 4
        HIPCHK(hipGetLastError());
    }
    return 0;
}
// the queries against a built grid; with X they are the sources of an ICP evaluation, transformed on load (nsk_icp.h)
static int cloud_query(nsk_ctx* c, const CloudBuilt& B, const float* d_query, int n_query, const CloudXform* X, float* d_dist, int32_t* d_index)
{
    nsk_ctx::Cloud& K = c->cloud;
    const CloudGrid& G = B.G;
    // queries in cell order: the ordering passes cost more than they save below about half a million queries
    const bool ordered = B.nfinite > 0 && ((K.query_mode & 4) || (!(K.query_mode & 2) && n_query >= CLOUD_ORDER_MIN));
    const int qb = (int)(((long long)n_query + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
    if (ordered) {
        CHK(grow(c, K.qcell, (size_t)n_query, "the queries' cells", GROW_NO_CAPTURE));
        CHK(grow(c, K.qperm, (size_t)n_query, "the queries in cell order", GROW_NO_CAPTURE));
        CHK(grow(c, K.qstart, B.words, "the cells' first queries", GROW_NO_CAPTURE));
        CHK(grow(c, K.qcursor, B.cells, "the cells' query cursors", GROW_NO_CAPTURE));
        ProfScope ps(c, X ? "icp_order" : "cloud_order");
        HIPCHK(hipMemsetAsync(K.qstart, 0, B.words * 4, c->stream));
        HIPCHK(hipMemsetAsync(K.qcursor, 0, B.cells * 4, c->stream));
        if (X) k_icp_cells<<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, *X, n_query, d_query, K.qcell, K.qstart);
        else k_cloud_cells<<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, n_query, d_query, 1, K.qcell, K.qstart);
        HIPCHK(hipGetLastError());
        CHK(mc_scan(c, K.qstart, (int)B.cells + 1));
        k_cloud_place<<<qb, CLOUD_BLOCK, 0, c->stream>>>(n_query, d_query, K.qcell, K.qstart, K.qcursor, nullptr, K.qperm);
        HIPCHK(hipGetLastError());
    }
    { ProfScope ps(c, X ? "icp_query" : "cloud_query");
      const unsigned* qperm = ordered ? K.qperm.get() : nullptr;
      if (K.query_mode & 1) {
          const long long wg = ((long long)n_query * 64 + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
          if (X) k_icp_query<64><<<(unsigned)wg, CLOUD_BLOCK, 0, c->stream>>>(G, *X, n_query, d_query, qperm, K.start, K.sorted, d_dist, d_index);
          else k_cloud_query<64><<<(unsigned)wg, CLOUD_BLOCK, 0, c->stream>>>(G, n_query, d_query, qperm, K.start, K.sorted, d_dist, d_index);
      } else if (X)
          k_icp_query<1><<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, *X, n_query, d_query, qperm, K.start, K.sorted, d_dist, d_index);
      else
          k_cloud_query<1><<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, n_query, d_query, qperm, K.start, K.sorted, d_dist, d_index);
      HIPCHK(hipGetLastError()); }
    return 0;
}

extern "C" int nsk_cloud_nearest(nsk_ctx* c, const float* d_query, int n_query, const float* d_target, int n_target, float* d_dist,
                                 int32_t* d_index, int* h_target_skipped)
{
    if (!c) return fail("nsk_cloud_nearest: null ctx");
    if (n_query < 0 || n_target < 0) return fail("nsk_cloud_nearest: negative count");
    if (n_target == 0) return fail("nsk_cloud_nearest: no target");
    if (!d_target) return fail("nsk_cloud_nearest: d_target is NULL");
    if (n_query > 0 && (!d_query || !d_dist)) return fail("nsk_cloud_nearest: d_query / d_dist is NULL");
    if (c->capturing) return fail("nsk_cloud_nearest: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    CloudBuilt B;
    CHK(cloud_build(c, d_target, n_target, n_query > 0, B));
    if (h_target_skipped) *h_target_skipped = (int)((unsigned)n_target - B.nfinite);
    if (n_query == 0) return 0;
    return cloud_query(c, B, d_query, n_query, nullptr, d_dist, d_index);
}

extern "C" int nsk_cloud_stats(nsk_ctx* c, const float* d_dist, int n, float threshold, double h_out[4])
{
    if (!c) return fail("nsk_cloud_stats: null ctx");
    if (n < 0) return fail("nsk_cloud_stats: negative count");
    if (!h_out) return fail("nsk_cloud_stats: h_out is NULL");
    if (n > 0 && !d_dist) return fail("nsk_cloud_stats: d_dist is NULL");
    if (c->capturing) return fail("nsk_cloud_stats: not while a graph is being captured");
    for (int k = 0; k < 4; ++k) h_out[k] = 0.0;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return rows_reduce<CloudStatCols>(c, "cloud_stats", "the distance sums of the workgroups", 1, n, CLOUD_BLOCK, CLOUD_MAX_ROWS,
                                      [&](int nrows, double* rows) { k_cloud_stats<<<nrows, CLOUD_BLOCK, 0, c->stream>>>(n, d_dist, threshold, rows); }, h_out);
}

// ---- alignment: point-to-point ICP (nsk_icp.h, nsk_rigid.h) ------------------------------------------------------------------------
static void cloud_xform_of(const double* h_M, CloudXform& X)
{
    double I[16]; nsk_rigid::identity4(I);
    for (int k = 0; k < 12; ++k) X.m[k] = (h_M ? h_M : I)[k];
}
// one evaluation of the pairs under X against a built grid: query, sums, the ICP_COLS doubles back (the evaluation's one synchronisation)
static int cloud_pair_eval(nsk_ctx* c, const CloudBuilt& B, const float* d_source, int n_source, const float* d_target, const CloudXform& X,
                           float threshold, float* d_dist, int32_t* d_index, double* h_cols)
{
    CHK(cloud_query(c, B, d_source, n_source, &X, d_dist, d_index));
    return rows_reduce<RowSums<ICP_COLS>>(c, "icp_sums", "the pair sums of the workgroups", 1, n_source, CLOUD_BLOCK, CLOUD_MAX_ROWS, [&](int nrows, double* rows) {
        k_icp_sums<<<nrows, CLOUD_BLOCK, 0, c->stream>>>(X, n_source, d_source, d_dist, d_index, d_target, threshold, rows); }, h_cols);
}
// the arguments both entry points share, the grid (once) and the buffers of an evaluation
static int cloud_pair_setup(nsk_ctx* c, const char* who, const float* d_source, int n_source, const float* d_target, int n_target, float threshold,
                            float** d_dist, int32_t** d_index, CloudBuilt& B)
{
    if (!c) return fail("%s: null ctx", who);
    if (n_source < 0 || n_target < 0) return fail("%s: negative count", who);
    if (n_target == 0) return fail("%s: no target", who);
    if (!d_target) return fail("%s: d_target is NULL", who);
    if (n_source > 0 && !d_source) return fail("%s: d_source is NULL", who);
    if (!(threshold >= 0.f)) return fail("%s: the threshold must not be negative", who);
    if (c->capturing) return fail("%s: not while a graph is being captured", who);
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Cloud& K = c->cloud;
    if (n_source > 0) {
        if (!*d_dist) { CHK(grow(c, K.icp_dist, (size_t)n_source, "the correspondences' distances", GROW_NO_CAPTURE)); *d_dist = K.icp_dist; }
        if (!*d_index) { CHK(grow(c, K.icp_index, (size_t)n_source, "the correspondences", GROW_NO_CAPTURE)); *d_index = K.icp_index; }
    }
    return cloud_build(c, d_target, n_target, n_source > 0, B);
}

extern "C" int nsk_cloud_pair_sums(nsk_ctx* c, const float* d_source, int n_source, const float* d_target, int n_target, const double* h_M,
                                   float threshold, double* h_sums, float* d_dist, int32_t* d_index, int* h_target_skipped)
{
    if (!h_sums) return fail("nsk_cloud_pair_sums: h_sums is NULL");
    CloudBuilt B;
    CHK(cloud_pair_setup(c, "nsk_cloud_pair_sums", d_source, n_source, d_target, n_target, threshold, &d_dist, &d_index, B));
    if (h_target_skipped) *h_target_skipped = (int)((unsigned)n_target - B.nfinite);
    for (int k = 0; k < 17; ++k) h_sums[k] = 0.0;
    if (n_source == 0) return 0;
    CloudXform X; cloud_xform_of(h_M, X);
    double cols[ICP_COLS];
    CHK(cloud_pair_eval(c, B, d_source, n_source, d_target, X, threshold, d_dist, d_index, cols));
    for (int k = 0; k < 17; ++k) h_sums[k] = cols[k];
    return 0;
}

extern "C" int nsk_rigid_from_sums(const double* h_sums, double* h_U, int* h_rank)
{
    if (!h_sums || !h_U) return fail("nsk_rigid_from_sums: null argument");
    if (nsk_rigid::from_sums(h_sums, h_U, h_rank) != 0) return fail("nsk_rigid_from_sums: a sum is not finite");
    return 0;
}

extern "C" int nsk_cloud_icp(nsk_ctx* c, const float* d_source, int n_source, const float* d_target, int n_target, float threshold, int max_iter,
                             double rel_fitness, double rel_rmse, const double* h_init, double* h_M, double* h_info)
{
    if (!h_M || !h_info) return fail("nsk_cloud_icp: h_M / h_info is NULL");
    if (max_iter < 0) return fail("nsk_cloud_icp: max_iter must not be negative");
    float* d_dist = nullptr; int32_t* d_index = nullptr;
    CloudBuilt B;
    CHK(cloud_pair_setup(c, "nsk_cloud_icp", d_source, n_source, d_target, n_target, threshold, &d_dist, &d_index, B));
    double M[16];
    if (h_init) memcpy(M, h_init, sizeof(M)); else nsk_rigid::identity4(M);
    M[12] = M[13] = M[14] = 0.0; M[15] = 1.0;
    for (int k = 0; k < 8; ++k) h_info[k] = 0.0;
    h_info[5] = (double)((unsigned)n_target - B.nfinite);
    memcpy(h_M, M, sizeof(M));
    if (n_source == 0) return 0;
    double cols[ICP_COLS];
    CloudXform X; cloud_xform_of(M, X);
    CHK(cloud_pair_eval(c, B, d_source, n_source, d_target, X, threshold, d_dist, d_index, cols));
    auto fitness = [&]() { return cols[0] / (double)n_source; };
    auto rmse = [&]() { return cols[0] > 0 ? std::sqrt(cols[1] / cols[0]) : 0.0; };
    double fit = fitness(), err = rmse();
    int updates = 0, converged = 0, degenerate = 0;
    while (updates < max_iter && cols[0] > 0) {
        double U[16], next[16];
        int rank = 0;
        if (nsk_rigid::from_sums(cols, U, &rank) != 0) return fail("nsk_cloud_icp: a pair sum is not finite");
        if (rank <= 1) degenerate = 1;
        nsk_rigid::mul4(U, M, next);
        memcpy(M, next, sizeof(M));
        ++updates;
        cloud_xform_of(M, X);
        CHK(cloud_pair_eval(c, B, d_source, n_source, d_target, X, threshold, d_dist, d_index, cols));
        const double f2 = fitness(), e2 = rmse();
        const bool still = std::fabs(f2 - fit) < rel_fitness && std::fabs(e2 - err) < rel_rmse;
        fit = f2; err = e2;
        if (cols[0] > 0 && still) { converged = 1; break; }
    }
    memcpy(h_M, M, sizeof(M));
    h_info[0] = updates; h_info[1] = fit; h_info[2] = err; h_info[3] = cols[0]; h_info[4] = converged; h_info[6] = cols[17]; h_info[7] = degenerate;
    return 0;
}

extern "C" int nsk_cloud_transform(nsk_ctx* c, const double* h_M, const float* d_in, int n, float* d_out)
{
    if (!c) return fail("nsk_cloud_transform: null ctx");
    if (n < 0) return fail("nsk_cloud_transform: negative count");
    if (n == 0) return 0;
    if (!d_in || !d_out) return fail("nsk_cloud_transform: d_in / d_out is NULL");
    if (c->capturing) return fail("nsk_cloud_transform: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    CloudXform X; cloud_xform_of(h_M, X);
    { ProfScope ps(c, "cloud_transform");
      k_cloud_transform<<<(unsigned)(((long long)n + CLOUD_BLOCK - 1) / CLOUD_BLOCK), CLOUD_BLOCK, 0, c->stream>>>(X, n, d_in, d_out);
      HIPCHK(hipGetLastError()); }
    return 0;
}

// ---- distances to the surface (nsk_surface.h) -------------------------------------------------------------------------------------
extern "C" int nsk_mesh_nearest(nsk_ctx* c, const float* d_query, int n_query, const float* d_vertices, int n_vertices,
                                const int32_t* d_triangles, int n_triangles, float* d_dist, int32_t* d_tri, float* d_point, int* h_skipped)
{
    if (!c) return fail("nsk_mesh_nearest: null ctx");
    if (n_query < 0 || n_vertices < 0 || n_triangles < 0) return fail("nsk_mesh_nearest: negative count");
    if (n_triangles == 0) return fail("nsk_mesh_nearest: the mesh has no triangle");
    if (!d_triangles || (n_vertices > 0 && !d_vertices)) return fail("nsk_mesh_nearest: d_vertices / d_triangles is NULL");
    if (n_query > 0 && (!d_query || !d_dist)) return fail("nsk_mesh_nearest: d_query / d_dist is NULL");
    if (c->capturing) return fail("nsk_mesh_nearest: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Surface& S = c->surface;
    nsk_ctx::Cloud& K = c->cloud;
    const int nt = n_triangles;
    const int tb = (int)(((long long)nt + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
    const int qb = (int)(((long long)n_query + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
    CHK(grow(c, S.rec, (size_t)nt, "the packed triangles", GROW_NO_CAPTURE));
    double cols[7];
    CHK(rows_reduce<CloudBoxCols>(c, "surface_records", "the partial boxes", 1, nt, CLOUD_BLOCK, CLOUD_MAX_ROWS, [&](int nrows, double* rows) {
        k_surf_records<<<nrows, CLOUD_BLOCK, 0, c->stream>>>(n_vertices, nt, d_vertices, d_triangles, S.rec, rows); }, cols));       // pass 1
    const long long n_valid = (long long)cols[6];
    if (h_skipped) *h_skipped = (int)(nt - n_valid);
    if (n_query == 0) return 0;
    CloudGrid G;
    G.nfinite = (int)n_valid; G.h = G.inv_h = 1.f;
    for (int a = 0; a < 3; ++a) { G.lo[a] = 0.f; G.dim[a] = 1; }
    if (n_valid == 0) {                                         // every query: +inf / -1 / NaN (NaN for a non-finite one); no grid is read
        ProfScope ps(c, "surface_query");
        k_surf_query<<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, n_query, d_query, nullptr, nullptr, nullptr, S.rec, nullptr, 0, d_dist, d_tri, d_point);
        HIPCHK(hipGetLastError());
        return 0;
    }
    float box[6];
    for (int k = 0; k < 6; ++k) box[k] = (float)cols[k];       // (floats widened by the kernel: the same floats)
    SurfPlan P = surf_plan(box, n_valid, S.cells_x4);
    const long long cap = surf_ref_cap(n_valid);
    CHK(grow(c, S.wide, (size_t)nt, "the wide triangles", GROW_NO_CAPTURE));
    CHK(grow(c, S.counters, 2, "the reference counts", GROW_NO_CAPTURE));
    size_t cells = 0, words = 0;
    unsigned long long counts[2] = {0, 0};
    for (int round = 0;; ++round) {
        for (int a = 0; a < 3; ++a) { G.lo[a] = P.lo[a]; G.dim[a] = P.dim[a]; }
        G.h = P.h; G.inv_h = P.inv_h;
        cells = (size_t)P.cells(); words = mc_scan_words(cells + 1);
        CHK(grow(c, S.start, words, "the cells' first references", GROW_NO_CAPTURE));
        { ProfScope ps(c, "surface_grid");
          HIPCHK(hipMemsetAsync(S.start, 0, words * 4, c->stream));
          HIPCHK(hipMemsetAsync(S.counters, 0, 16, c->stream));
          k_surf_count<<<tb, CLOUD_BLOCK, 0, c->stream>>>(G, nt, S.rec, S.start, S.wide, S.counters);                              // pass 2
          HIPCHK(hipGetLastError()); }
        HIPCHK(hipMemcpyAsync(counts, S.counters, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((long long)counts[0] <= cap) break;
        if (round >= SURF_MAX_GROW || !surf_plan_grow(P)) return fail("nsk_mesh_nearest: %llu cell references do not fit %lld", counts[0], cap);
    }
    CHK(grow(c, S.cursor, cells, "the cells' placement cursors", GROW_NO_CAPTURE));
    CHK(grow(c, S.refs, (size_t)std::max<unsigned long long>(counts[0], 1), "the cells' triangles", GROW_NO_CAPTURE));
    { ProfScope ps(c, "surface_grid");
      HIPCHK(hipMemsetAsync(S.cursor, 0, cells * 4, c->stream));
      CHK(mc_scan(c, S.start, (int)cells + 1));                                                                                      // pass 3
      k_surf_place<<<tb, CLOUD_BLOCK, 0, c->stream>>>(G, nt, S.rec, S.start, S.cursor, S.refs);                                     // pass 4
      HIPCHK(hipGetLastError()); }
    // queries in cell order, as nsk_cloud_nearest orders them (the same kernels, the same scratch)
    const bool ordered = (S.query_mode & 4) || (!(S.query_mode & 2) && n_query >= CLOUD_ORDER_MIN);
    if (ordered) {
        CHK(grow(c, K.qcell, (size_t)n_query, "the queries' cells", GROW_NO_CAPTURE));
        CHK(grow(c, K.qperm, (size_t)n_query, "the queries in cell order", GROW_NO_CAPTURE));
        CHK(grow(c, K.qstart, words, "the cells' first queries", GROW_NO_CAPTURE));
        CHK(grow(c, K.qcursor, cells, "the cells' query cursors", GROW_NO_CAPTURE));
        ProfScope ps(c, "surface_order");
        HIPCHK(hipMemsetAsync(K.qstart, 0, words * 4, c->stream));
        HIPCHK(hipMemsetAsync(K.qcursor, 0, cells * 4, c->stream));
        k_cloud_cells<<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, n_query, d_query, 1, K.qcell, K.qstart);
        HIPCHK(hipGetLastError());
        CHK(mc_scan(c, K.qstart, (int)cells + 1));
        k_cloud_place<<<qb, CLOUD_BLOCK, 0, c->stream>>>(n_query, d_query, K.qcell, K.qstart, K.qcursor, nullptr, K.qperm);
        HIPCHK(hipGetLastError());
    }
    { ProfScope ps(c, "surface_query");
      k_surf_query<<<qb, CLOUD_BLOCK, 0, c->stream>>>(G, n_query, d_query, ordered ? K.qperm.get() : nullptr, S.start, S.refs, S.rec, S.wide,
                                                      (int)counts[1], d_dist, d_tri, d_point);
      HIPCHK(hipGetLastError()); }
    return 0;
}

extern "C" int nsk_normal_stats(nsk_ctx* c, int n, const float* d_va, int nva, const int32_t* d_ta, int nta, const int32_t* d_ia,
                                const float* d_vb, int nvb, const int32_t* d_tb, int ntb, const int32_t* d_ib, double h_out[3])
{
    if (!c) return fail("nsk_normal_stats: null ctx");
    if (n < 0 || nva < 0 || nta < 0 || nvb < 0 || ntb < 0) return fail("nsk_normal_stats: negative count");
    if (!h_out) return fail("nsk_normal_stats: h_out is NULL");
    if (n > 0 && (!d_ia || !d_ib)) return fail("nsk_normal_stats: d_ia / d_ib is NULL");
    if ((nta > 0 && (!d_ta || (nva > 0 && !d_va))) || (ntb > 0 && (!d_tb || (nvb > 0 && !d_vb)))) return fail("nsk_normal_stats: a mesh pointer is NULL");
    if (c->capturing) return fail("nsk_normal_stats: not while a graph is being captured");
    for (int k = 0; k < 3; ++k) h_out[k] = 0.0;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return rows_reduce<RowSums<3>>(c, "normal_stats", "the normal sums of the workgroups", 1, n, CLOUD_BLOCK, CLOUD_MAX_ROWS, [&](int nrows, double* rows) {
        k_normal_stats<<<nrows, CLOUD_BLOCK, 0, c->stream>>>(n, d_va, nva, d_ta, nta, d_ia, d_vb, nvb, d_tb, ntb, d_ib, rows); }, h_out);
}

// ---- depth views of a mesh (nsk_raster.h) -----------------------------------------------------------------------------------------
extern "C" int nsk_mesh_depth(nsk_ctx* c, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles, int V,
                              const float* h_w2c, int H, int W, float fx, float fy, float cx, float cy, float* d_depth, int* h_skipped)
{
    if (!c) return fail("nsk_mesh_depth: null ctx");
    if (n_vertices < 0 || n_triangles < 0 || V < 0) return fail("nsk_mesh_depth: negative count");
    if (H < 1 || W < 1 || (long long)H * W > (1LL << 24)) return fail("nsk_mesh_depth: image %d x %d, need 1 .. 2^24 pixels", H, W);
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy)) return fail("nsk_mesh_depth: intrinsics are not finite");
    if (n_triangles > 0 && (!d_triangles || (n_vertices > 0 && !d_vertices))) return fail("nsk_mesh_depth: d_vertices / d_triangles is NULL");
    if (V > 0 && (!d_depth || !h_w2c)) return fail("nsk_mesh_depth: d_depth / h_w2c is NULL with V = %d", V);
    if (c->capturing) return fail("nsk_mesh_depth: not while a graph is being captured");
    if (h_skipped) *h_skipped = 0;
    if (V == 0 && !(h_skipped && n_triangles > 0)) return 0;
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::Raster& R = c->raster;
    const size_t img = (size_t)H * W, total = img * (size_t)V;
    unsigned* bits = reinterpret_cast<unsigned*>(d_depth);
    if (total) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)bits, (int)RASTER_INF_BITS, total, c->stream));
    if (n_triangles > 0) {
        CHK(grow(c, R.queue, (size_t)R.queue_cap, "the rasteriser's queue", GROW_NO_CAPTURE));
        CHK(grow(c, R.counters, 16, "the rasteriser's counters", GROW_NO_CAPTURE));
        if (h_skipped) HIPCHK(hipMemsetAsync(R.counters.get() + 1, 0, 4, c->stream));
        RasterArgs A;
        memset(&A, 0, sizeof(A));
        A.H = H; A.W = W; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.nv = n_vertices; A.nt = n_triangles;
        A.inline_max = R.inline_max; A.queue_cap = (unsigned)R.queue_cap; A.load_first = R.load_first;
        const int nb = (int)(((long long)n_triangles + RASTER_BLOCK - 1) / RASTER_BLOCK);
        int k0 = 0;
        do {                                                // (V = 0 still launches once: it counts the skipped triangles)
            A.K = std::min(V - k0, RASTER_MAX_V);
            view_matrices(A.w, h_w2c, k0, A.K);
            HIPCHK(hipMemsetAsync(R.counters, 0, 4, c->stream));
            { ProfScope ps(c, "raster_tris");
              k_raster_tris<<<nb, RASTER_BLOCK, 0, c->stream>>>(A, d_vertices, d_triangles, bits + (size_t)k0 * img, R.queue, R.counters,
                                                               k0 == 0 && h_skipped ? R.counters.get() + 1 : nullptr); }
            HIPCHK(hipGetLastError());
            if (A.K > 0) {
                ProfScope ps(c, "raster_queue");
                k_raster_queue<<<RASTER_QUEUE_WG, RASTER_BLOCK, 0, c->stream>>>(A, d_vertices, d_triangles, bits + (size_t)k0 * img, R.queue, R.counters);
            }
            HIPCHK(hipGetLastError());
            k0 += A.K;
        } while (k0 < V);
    }
    if (total) {
        ProfScope ps(c, "raster_finish");
        k_raster_finish<<<(unsigned)std::min<size_t>((total + RASTER_BLOCK - 1) / RASTER_BLOCK, 65536), RASTER_BLOCK, 0, c->stream>>>(total, bits);
        HIPCHK(hipGetLastError());
    }
    if (h_skipped && n_triangles > 0) {
        unsigned cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, R.counters.get() + 1, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *h_skipped = (int)cnt;
    }
    return 0;
}

extern "C" int nsk_depth_pair_stats(nsk_ctx* c, const float* d_a, const float* d_b, int V, int n_pix, double* h_out)
{
    if (!c) return fail("nsk_depth_pair_stats: null ctx");
    if (V < 0 || n_pix < 1 || n_pix > (1 << 24)) return fail("nsk_depth_pair_stats: V = %d, n_pix = %d, need V >= 0 and 1 .. 2^24 pixels", V, n_pix);
    if (V == 0) return 0;
    if (V > (1 << 20)) return fail("nsk_depth_pair_stats: V = %d, at most 2^20 views per call", V);
    if (!d_a || !d_b || !h_out) return fail("nsk_depth_pair_stats: d_a / d_b / h_out is NULL");
    if (c->capturing) return fail("nsk_depth_pair_stats: not while a graph is being captured");
    HIPCHK(hipSetDevice(c->device));
    return rows_reduce<RowSums<4>>(c, "depth_stats", "the depth sums of the workgroups", V, n_pix, RASTER_BLOCK, RASTER_STAT_ROWS, [&](int R, double* rows) {
        k_depth_pair_stats<<<(unsigned)((size_t)V * R), RASTER_BLOCK, 0, c->stream>>>(n_pix, R, d_a, d_b, rows); }, h_out);
}

// the counter hash of nsk_sample_pixels on the host (hash_u32 of nsk_device.h, which is device code)
static uint32_t host_hash_u32(unsigned long long seed, uint32_t a, uint32_t b)
{
    unsigned long long x = seed ^ (0x9E3779B97F4A7C15ull * ((unsigned long long)a + 1)) ^ (0xC2B2AE3D27D4EB4Full * ((unsigned long long)b + 1));
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return (uint32_t)(x >> 32);
}
// one view of the draw stated in include/nsk.h: every operation a double operation of its own, in the order written there
static void depth_view(const double lo[3], const double ext[3], const double ctr[3], double shrink, unsigned long long seed, uint32_t view,
                       float* w)
{
#pragma clang fp contract(off)
    double u[6], o[3], f[3];
    for (int k = 0; k < 6; ++k) u[k] = (double)(host_hash_u32(seed, view, (uint32_t)k) >> 8) * (1.0 / 16777216.0);
    for (int a = 0; a < 3; ++a) {
        o[a] = ctr[a] + (u[a] - 0.5) * (shrink * ext[a]);
        const double target = lo[a] + u[3 + a] * ext[a];
        f[a] = target - o[a];
    }
    const double fl = std::sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    for (int a = 0; a < 3; ++a) f[a] = f[a] / fl;
    const double sl = std::sqrt(f[1] * f[1] + f[0] * f[0]);
    const double s[3] = {f[1] / sl, -f[0] / sl, 0.0};
    double v[3] = {f[1] * s[2] - f[2] * s[1], f[2] * s[0] - f[0] * s[2], f[0] * s[1] - f[1] * s[0]};
    const double vl = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int a = 0; a < 3; ++a) v[a] = v[a] / vl;
    const double rows[3][3] = {{s[0], s[1], s[2]}, {-v[0], -v[1], -v[2]}, {-f[0], -f[1], -f[2]}};
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) w[4 * a + b] = (float)rows[a][b];
        w[4 * a + 3] = (float)-((rows[a][0] * o[0] + rows[a][1] * o[1]) + rows[a][2] * o[2]);
    }
    w[12] = w[13] = w[14] = 0.f; w[15] = 1.f;
}

// views first .. first + V - 1 of the stream: host only
extern "C" int nsk_depth_views_range(const float h_box[6], unsigned long long seed, double shrink, long long first, int V, float* h_w2c)
{
    if (!h_box) return fail("nsk_depth_views_range: h_box is NULL");
    if (V < 0 || (V > 0 && !h_w2c)) return fail("nsk_depth_views_range: V = %d, or h_w2c is NULL", V);
    if (first < 0 || first + (long long)V > (1LL << 32)) return fail("nsk_depth_views_range: views %lld .. %lld, the stream has 2^32", first, first + (long long)V);
    if (!std::isfinite(shrink)) return fail("nsk_depth_views_range: shrink is not finite");
    double lo[3], ext[3], ctr[3];
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(h_box[a]) || !std::isfinite(h_box[3 + a])) return fail("nsk_depth_views_range: the box is not finite");
        lo[a] = (double)h_box[a]; ext[a] = (double)h_box[3 + a] - lo[a]; ctr[a] = 0.5 * (lo[a] + (double)h_box[3 + a]);
    }
    for (int k = 0; k < V; ++k) depth_view(lo, ext, ctr, shrink, seed, (uint32_t)(first + k), h_w2c + 16 * (size_t)k);
    return 0;
}

extern "C" int nsk_depth_views(nsk_ctx* c, const float* d_vertices, int n_vertices, float h_box[6], unsigned long long seed, double shrink,
                               int V, float* h_w2c)
{
    if (!h_box) return fail("nsk_depth_views: h_box is NULL");
    if (V < 0 || (V > 0 && !h_w2c)) return fail("nsk_depth_views: V = %d, or h_w2c is NULL", V);
    if (!std::isfinite(shrink)) return fail("nsk_depth_views: shrink is not finite");
    if (d_vertices) {
        if (!c) return fail("nsk_depth_views: null ctx");
        if (n_vertices < 1) return fail("nsk_depth_views: no vertex");
        if (c->capturing) return fail("nsk_depth_views: not while a graph is being captured");
        HIPCHK(hipSetDevice(c->device));
        float box[6];
        unsigned nfinite;
        CHK(cloud_box(c, d_vertices, n_vertices, box, nfinite));
        if (!nfinite) return fail("nsk_depth_views: no vertex with finite coordinates");
        memcpy(h_box, box, sizeof(box));
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(h_box[a]) || !std::isfinite(h_box[3 + a])) return fail("nsk_depth_views: the box is not finite");
    return nsk_depth_views_range(h_box, seed, shrink, 0, V, h_w2c);
}

// ---- culling to what a trajectory saw (kernels and entry points: nsk_cull.h) ---------------------------------------------------------
#include "nsk_cull.h"

// ---- depth frames fused into a TSDF on a lattice (kernels and entry points: nsk_tsdf.h) -------------------------------------------------
#include "nsk_tsdf.h"

// ---- vertex normals, rays along them, the colours they composite (kernels and entry points: nsk_normals.h) ---------------------------------
#include "nsk_normals.h"

// ---- convex hull of a point cloud, lattice nodes inside the scaled hull (kernels and entry points: nsk_hull.h) ---------------------------
#include "nsk_hull.h"

// ---- mesh simplification by uniform vertex clustering (kernels and entry points: nsk_simplify.h) -----------------------------------------
#include "nsk_simplify.h"

// ---- raw frames prepared on the device: undistort, resize, crop (kernel and entry points: nsk_frame.h) -----------------------------------
#include "nsk_frame.h"

extern "C" int nsk_inside_filter(nsk_ctx* c, int N, const float* ro, const float* rd, const float* gt, uint8_t* keep)
{
    if (!c || !ro || !rd || !gt || !keep || N < 1) return fail("nsk_inside_filter: bad argument");
    k_inside_filter<<<(N + 255) / 256, 256, 0, c->stream>>>(c->R, N, ro, rd, gt, keep);
    HIPCHK(hipGetLastError());
    return 0;
}

static void adam_consts(float lr, float b1, float b2, int step, float& step_size, float& bc2s)
{
    float bc1 = 1.f - (float)pow((double)b1, step);
    float bc2 = 1.f - (float)pow((double)b2, step);
    step_size = lr / bc1; bc2s = sqrtf(bc2);
}

extern "C" int nsk_adam_vector(nsk_ctx* c, int n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, int step)
{
    if (!c || !p || !g || !m || !v || n < 1 || step < 1) return fail("nsk_adam_vector: bad argument");
    float ss, bc2s; adam_consts(lr, b1, b2, step, ss, bc2s);
    if (c->capturing) c->cap_vecs.push_back(nsk_ctx::CapVec{n, p, g, m, v, lr, b1, b2, eps, step, nullptr, ss, bc2s});
    k_adam_scalar<<<(n + 255) / 256, 256, 0, c->stream>>>(n, p, g, m, v, ss, bc2s, b1, b2, eps);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- optimiser ------------------------------------------------------------------------------------------------
// where the launch rewrites a trainable decoder's images: every image the decoder has, image 3 included (it stays as fresh or as stale as it was)
static void adam_images(AdamSeg& S, DecState& D)
{
    const DecImage* I = D.img;
    S.inv_f = I[0].inv; S.inv_b = I[1].inv; S.fimg = I[0].data; S.bimg = I[1].data;
    if (I[2].data) { S.inv16 = I[2].inv; S.img16 = reinterpret_cast<unsigned short*>(I[2].data.get()); S.img16_tail = I[2].data + I[2].spec.tail_off; S.tail_off = I[2].spec.sib_off; S.np16 = I[2].spec.pieces; }
    if (I[3].data) { S.invh = I[3].inv; S.imgh = reinterpret_cast<unsigned short*>(I[3].data.get()); S.imgh_tail = I[3].data + I[3].spec.tail_off; S.btail_off = I[3].spec.sib_off; }
}

extern "C" int nsk_adam_step(nsk_ctx* c, const float lr[NSK_NUM_GROUPS], float b1, float b2, float eps)
{
    if (!c || !lr) return fail("nsk_adam_step: null argument");
    HIPCHK(hipSetDevice(c->device));
    AdamArgs AA; memset(&AA, 0, sizeof(AA));
    AA.b1 = b1; AA.b2 = b2; AA.eps = eps;
    int blocks = 0;
    int seg_group[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int lv = 0; lv < 4; ++lv) {
        int grp = NSK_GROUP_COARSE + lv;
        if (!c->touched[grp] || !c->grid[lv].n) continue;
        int step = ++c->adam_step[grp];
        if (c->capturing) ++c->cap_rollback[grp];
        GridState& G = c->grid[lv];
        seg_group[AA.n] = grp;
        AdamSeg& S = AA.s[AA.n++];
        adam_consts(lr[grp], b1, b2, step, S.step_size, S.bc2s);
        CHK(ensure_midx(c, lv));
        S.p = G.v; S.g = c->slab + G.g_off; S.m = G.m; S.v = G.s; S.n = (int)G.n;
        S.idx = G.mask ? G.midx : nullptr; S.nidx = G.mask ? G.nmask : 0;
        blocks += G.mask ? std::max(1, (G.nmask * 8 + 255) / 256) : ((int)G.n / 4 + 255) / 256; S.blk_end = blocks;
        c->touched[grp] = false;
    }
    if (c->touched[NSK_GROUP_DECODERS]) {
        int step = ++c->adam_step[NSK_GROUP_DECODERS];
        if (c->capturing) ++c->cap_rollback[NSK_GROUP_DECODERS];
        for (int w = 0; w < 4; ++w) {
            DecState& D = c->dec[w];
            if (!D.trainable || !D.loaded) continue;
            int n4 = (D.n + 3) & ~3;
            seg_group[AA.n] = NSK_GROUP_DECODERS;
            AdamSeg& S = AA.s[AA.n++];
            adam_consts(lr[NSK_GROUP_DECODERS], b1, b2, step, S.step_size, S.bc2s);
            S.p = D.p; S.g = c->slab + D.g_off; S.m = D.m; S.v = D.s; S.idx = nullptr; S.nidx = 0; S.n = n4;
            adam_images(S, D);
            if (c->pend_w == w) {
                S.slabs = c->ws.dec_slabs; S.nslabs = c->pend_nb; S.slab_stride = n4; c->pend_w = -1;
                blocks += (n4 / 4 + 7) / 8 - (n4 / 4 + 255) / 256;         // 8 float4 per block (see k_adam_multi)
            }
            blocks += (n4 / 4 + 255) / 256; S.blk_end = blocks;
        }
        c->touched[NSK_GROUP_DECODERS] = false;
    }
    if (AA.n && c->capturing) {
        nsk_ctx::CapAdam ca; ca.args = AA;
        for (int i = 0; i < AA.n; ++i) { ca.group[i] = seg_group[i]; ca.lr[i] = lr[seg_group[i]]; }
        c->cap_adams.push_back(ca);
    }
    const int place_wgs = prep_ride_place(c, AA, blocks);
    if (AA.n) { ProfScope ps(c, "adam_multi"); k_adam_multi<<<blocks + place_wgs, 256, 0, c->stream>>>(AA); }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- hipGraph capture (see nsk_ctx::GraphRec) ---------------------------------------------------------------------
extern "C" int nsk_graph_begin(nsk_ctx* c)
{
    if (!c) return fail("null ctx");
    if (c->capturing) return fail("nsk_graph_begin: a capture is already open");
    HIPCHK(hipSetDevice(c->device));
    CHK(flush_pending(c));
    // A batch registered with nsk_map_prepare is settled BEFORE the capture opens: whatever of its sampling / cell sort has not run yet runs now,
    // eagerly (inside the capture forward_core's prep_finish would have recorded those launches into the graph instead of running them, and the
    // batch's own step would then have swapped in buffers nobody filled); the batch stays prepared for its own eager step.
    CHK(prep_finish(c));
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    c->cap_adams.clear(); c->cap_vecs.clear();
    for (int g = 0; g < NSK_NUM_GROUPS; ++g) c->cap_rollback[g] = 0;
    return 0;
}

extern "C" int nsk_graph_end(nsk_ctx* c, int* graph_id)
{
    if (!c || !graph_id) return fail("nsk_graph_end: null argument");
    if (!c->capturing) return fail("nsk_graph_end: no capture is open");
    c->capturing = false;
    nsk_ctx::GraphRec R;
    hipError_t e = hipStreamEndCapture(c->stream, &R.graph);
    for (int g = 0; g < NSK_NUM_GROUPS; ++g) c->adam_step[g] -= c->cap_rollback[g];      // nothing ran during the capture
    c->pend_w = -1;
    if (e != hipSuccess || !R.graph) return fail("nsk_graph_end: hipStreamEndCapture: %s", hipGetErrorString(e));
    if (c->cap_adams.size() > 1) { hipGraphDestroy(R.graph); return fail("nsk_graph_end: at most one nsk_adam_step per captured graph"); }
    R.vecs = c->cap_vecs;
    if (!c->cap_adams.empty()) { R.has_adam = true; R.adam = c->cap_adams[0]; }
    if (R.has_adam || !R.vecs.empty()) {
        size_t nn = 0;
        HIPCHK(hipGraphGetNodes(R.graph, nullptr, &nn));
        std::vector<hipGraphNode_t> nodes(nn);
        HIPCHK(hipGraphGetNodes(R.graph, nodes.data(), &nn));
        for (hipGraphNode_t nd : nodes) {
            hipGraphNodeType t;
            HIPCHK(hipGraphNodeGetType(nd, &t));
            if (t != hipGraphNodeTypeKernel) continue;
            hipKernelNodeParams kp;
            HIPCHK(hipGraphKernelNodeGetParams(nd, &kp));
            if (kp.func == reinterpret_cast<void*>(k_adam_multi)) R.adam_node = nd;
            if (kp.func == reinterpret_cast<void*>(k_adam_scalar) && kp.kernelParams)
                for (auto& V : R.vecs) if (!V.node && *reinterpret_cast<float**>(kp.kernelParams[1]) == V.p) { V.node = nd; break; }
        }
        if (R.has_adam && !R.adam_node) { hipGraphDestroy(R.graph); return fail("nsk_graph_end: the Adam kernel node was not found in the captured graph"); }
        for (auto& V : R.vecs) if (!V.node) { hipGraphDestroy(R.graph); return fail("nsk_graph_end: an nsk_adam_vector node was not found in the captured graph"); }
    }
    HIPCHK(hipGraphInstantiate(&R.exec, R.graph, nullptr, nullptr, 0));
    R.flip = c->ws_flip;
    c->graphs.push_back(R);
    *graph_id = (int)c->graphs.size() - 1;
    return 0;
}

extern "C" int nsk_graph_launch(nsk_ctx* c, int id)
{
    if (!c || id < 0 || id >= (int)c->graphs.size()) return fail("nsk_graph_launch: bad graph id %d", id);
    if (c->graphs[id].stale) return fail("nsk_graph_launch: graph %d is stale -- a workspace, grid or gradient buffer it recorded was reallocated after the capture (larger batch, new grid shape or mask); capture it again", id);
    if (!c->graphs[id].exec) return fail("nsk_graph_launch: graph %d was destroyed", id);
    HIPCHK(hipSetDevice(c->device));
    nsk_ctx::GraphRec& R = c->graphs[id];
    // A prepared batch (nsk_map_prepare) and a replay share the cell histogram and, after an odd number of set swaps since the capture, the very
    // buffers the graph writes: finish the batch's pending stages first (a histogram still holding its counts would be added onto by the
    // replayed sampling), and where the graph's recorded set is the one the batch lives in, drop the batch -- its own step samples it again.
    CHK(prep_finish(c));
    if (c->prep.valid && R.flip != c->ws_flip) CHK(prep_drop(c));
    if (R.has_adam) {                            // this replay is one more Adam step for the groups the graph updates
        AdamArgs& A = R.adam.args;
        int stepped[NSK_NUM_GROUPS] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < A.n; ++i) {
            const int g = R.adam.group[i];
            if (!stepped[g]) { ++c->adam_step[g]; stepped[g] = 1; }
            adam_consts(R.adam.lr[i], A.b1, A.b2, c->adam_step[g], A.s[i].step_size, A.s[i].bc2s);
        }
        hipKernelNodeParams kp;
        HIPCHK(hipGraphKernelNodeGetParams(R.adam_node, &kp));
        void* args[1] = {&A};
        kp.kernelParams = args; kp.extra = nullptr;
        HIPCHK(hipGraphExecKernelNodeSetParams(R.exec, R.adam_node, &kp));
    }
    for (auto& V : R.vecs) {                      // the pose (or any plain vector) Adam: one more step per replay
        adam_consts(V.lr, V.b1, V.b2, V.step, V.ss, V.bc2s);
        ++V.step;
        hipKernelNodeParams kp;
        HIPCHK(hipGraphKernelNodeGetParams(V.node, &kp));
        void* args[10] = {&V.n, &V.p, &V.g, &V.m, &V.v, &V.ss, &V.bc2s, &V.b1, &V.b2, &V.eps};
        kp.kernelParams = args; kp.extra = nullptr;
        HIPCHK(hipGraphExecKernelNodeSetParams(R.exec, V.node, &kp));
    }
    HIPCHK(hipGraphLaunch(R.exec, c->stream));
    return 0;
}

extern "C" int nsk_graph_destroy(nsk_ctx* c, int id)
{
    if (!c || id < 0 || id >= (int)c->graphs.size()) return fail("nsk_graph_destroy: bad graph id %d", id);
    nsk_ctx::GraphRec& R = c->graphs[id];
    if (R.exec) { HIPCHK(hipStreamSynchronize(c->stream)); hipGraphExecDestroy(R.exec); hipGraphDestroy(R.graph); R.exec = nullptr; R.graph = nullptr; }
    return 0;
}

extern "C" int nsk_adam_reset(nsk_ctx* c)
{
    if (!c) return fail("null ctx");
    for (int i = 0; i < 4; ++i) {
        if (c->grid[i].n) { HIPCHK(hipMemsetAsync(c->grid[i].m, 0, c->grid[i].n * 4, c->stream)); HIPCHK(hipMemsetAsync(c->grid[i].s, 0, c->grid[i].n * 4, c->stream)); }
        if (c->dec[i].p) { size_t n4 = (c->dec[i].n + 3) & ~3; HIPCHK(hipMemsetAsync(c->dec[i].m, 0, n4 * 4, c->stream)); HIPCHK(hipMemsetAsync(c->dec[i].s, 0, n4 * 4, c->stream)); }
    }
    for (int g = 0; g < NSK_NUM_GROUPS; ++g) { c->adam_step[g] = 0; c->touched[g] = false; }
    return 0;
}

extern "C" int nsk_zero_grads(nsk_ctx* c)
{
    if (!c) return fail("null ctx");
    c->pend_w = -1;
    if (c->slab) HIPCHK(hipMemsetAsync(c->slab, 0, c->slab_n * 4, c->stream));
    for (int g = 0; g < NSK_NUM_GROUPS; ++g) c->touched[g] = false;
    return 0;
}

// ---- multi-GPU ------------------------------------------------------------------------------------------------
extern "C" int nsk_grad_slab(nsk_ctx* c, float** p, size_t* n)
{
    if (!c || !p || !n) return fail("nsk_grad_slab: null argument");
    CHK(flush_pending(c));
    *p = c->slab; *n = c->slab_n;
    return 0;
}

// ascending list of a level's marked voxels (used by the optimiser launch and by the packed exchange); rebuilt when the mask changed
static int ensure_midx(nsk_ctx* c, int l)
{
    GridState& G = c->grid[l];
    if (!G.mask || !G.midx_dirty) return 0;
    if (c->capturing) return fail("graph capture: a mask changed since the last eager step (run the step once after installing masks, then capture)");
    const int nvox = (int)(G.n / 32);
    if (!G.midx) CHK(dev_alloc(G.midx, (size_t)nvox, "the marked-voxel list"));
    int* d_count = reinterpret_cast<int*>(c->scal + 8);
    k_mask_index<<<1, 1024, 0, c->stream>>>(nvox, G.mask, G.midx, d_count);
    HIPCHK(hipMemcpyAsync(&G.nmask, d_count, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // once per mask, not per step
    G.midx_dirty = false;
    return 0;
}

// Which parts of the slab a step's exchange must carry: the grid levels and trainable decoders that received gradients since the
// last optimiser step (the same on every rank: it follows from the stage and the flags) and the loss scalars.
static int pack_layout(nsk_ctx* c, size_t* total)
{
    size_t n = 0;
    for (int l = 0; l < 4; ++l) {
        GridState& G = c->grid[l];
        c->xlevels[l] = G.n && c->touched[NSK_GROUP_COARSE + l];
        if (!c->xlevels[l]) continue;
        CHK(ensure_midx(c, l));
        n += (size_t)(G.mask ? G.nmask : (int)(G.n / 32)) * 32;
    }
    for (int w = 0; w < 4; ++w) {
        c->xdecs[w] = c->dec[w].loaded && c->dec[w].trainable && c->touched[NSK_GROUP_DECODERS];
        if (c->xdecs[w]) n += (size_t)((c->dec[w].n + 3) & ~3);
    }
    n += 4;
    n += c->xextra_n;
    *total = n;
    return 0;
}

static int pack_move(nsk_ctx* c, bool gather)
{
    XArgs A;
    memset(&A, 0, sizeof(A));
    A.gather = gather ? 1 : 0;
    size_t o = 0;
    int blocks = 0;
    auto add = [&](const int* idx, size_t n4, float* slab, int pend_w = -1) {
        if (n4 == 0) return;
        XSeg& S = A.s[A.n++];
        S.idx = idx; S.n4 = (int)n4; S.slab = slab; S.buf = c->xbuf + o;
        if (gather && pend_w >= 0 && c->pend_w == pend_w) {      // its gradient is still in the backward's per-workgroup slabs: summed by this launch
            S.slabs = c->ws.dec_slabs; S.nslabs = c->pend_nb; S.slab_stride = (int)(n4 * 4);
            blocks += (int)((n4 + 7) / 8);
            c->pend_w = -1;
        } else blocks += (int)((n4 + 255) / 256);
        S.blk_end = blocks;
        o += n4 * 4;
    };
    for (int l = 0; l < 4; ++l) {
        if (!c->xlevels[l]) continue;
        GridState& G = c->grid[l];
        const int nv = G.mask ? G.nmask : (int)(G.n / 32);
        add(G.mask ? G.midx : nullptr, (size_t)nv * 8, c->slab + G.g_off);
    }
    for (int w = 0; w < 4; ++w) {
        if (!c->xdecs[w]) continue;
        add(nullptr, (size_t)((c->dec[w].n + 3) & ~3) / 4, c->slab + c->dec[w].g_off, w);
    }
    add(nullptr, 1, c->slab + c->slab_n - 4);                 // loss scalars
    if (c->xextra_n) add(nullptr, c->xextra_n / 4, c->xextra); // the caller's vector (nsk_grad_extra: pose gradients of a bundle-adjustment step)
    if (blocks > 0) k_xchg_multi<<<blocks, 256, 0, c->stream>>>(A);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int nsk_grad_pack(nsk_ctx* c, float** p, size_t* n)
{
    if (!c || !p || !n) return fail("nsk_grad_pack: null argument");
    HIPCHK(hipSetDevice(c->device));
    size_t total = 0;
    CHK(pack_layout(c, &total));
    bool any_mask = false;
    for (int l = 0; l < 4; ++l) any_mask = any_mask || (c->xlevels[l] && c->grid[l].mask);
    if (!any_mask && !c->xextra_n) {                   // nothing to compact: exchange the slab in place (no copies); unpack is then a no-op
        CHK(flush_pending(c));
        c->xbuf_n = 0; c->x_identity = true;
        *p = c->slab; *n = c->slab_n;
        return 0;
    }
    c->x_identity = false;
    c->xbuf_n = 0;
    CHK(grow(c, c->xbuf, total, "the exchange buffer", GROW_STALE_GRAPHS));
    c->xbuf_n = total;
    { ProfScope ps(c, "grad_pack"); CHK(pack_move(c, true)); }
    *p = c->xbuf; *n = total;
    return 0;
}

extern "C" int nsk_grad_unpack(nsk_ctx* c)
{
    if (!c) return fail("null ctx");
    if (c->x_identity) return 0;
    if (!c->xbuf || !c->xbuf_n) return fail("nsk_grad_unpack: nothing was packed (call nsk_grad_pack after nsk_map_step)");
    HIPCHK(hipSetDevice(c->device));
    ProfScope ps(c, "grad_unpack");
    return pack_move(c, false);
}

extern "C" int nsk_allreduce_grads(nsk_ctx* c, void* comm)
{
    if (!c || !comm) return fail("nsk_allreduce_grads: null argument");
    typedef int (*allreduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static allreduce_t fn = nullptr;
    if (!fn) {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return fail("nsk_allreduce_grads: cannot load librccl.so: %s", dlerror());
        fn = (allreduce_t)dlsym(h, "ncclAllReduce");
        if (!fn) return fail("nsk_allreduce_grads: ncclAllReduce not found");
    }
    float* buf = nullptr; size_t n = 0;
    CHK(nsk_grad_pack(c, &buf, &n));
    const int ncclFloat32 = 7, ncclSum = 0;
    int r;
    { ProfScope ps(c, "allreduce"); r = fn(buf, buf, n, ncclFloat32, ncclSum, comm, c->stream); }      // HIP events on the context's stream: the collective alone
    if (r != 0) return fail("ncclAllReduce failed with %d", r);
    return nsk_grad_unpack(c);
}

extern "C" int nsk_profile_begin(nsk_ctx* c)
{
    if (!c) return fail("null ctx");
    for (auto& r : c->prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    c->prof_recs.clear();
    c->prof = true;
    return 0;
}

extern "C" int nsk_profile_end(nsk_ctx* c, char* buf, size_t n)
{
    if (!c || !buf || n < 2) return fail("nsk_profile_end: bad argument");
    c->prof = false;
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<std::string> names; std::vector<double> tot; std::vector<int> cnt;
    for (auto& r : c->prof_recs) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.a, r.b);
        size_t k = 0;
        for (; k < names.size(); ++k) if (names[k] == r.name) break;
        if (k == names.size()) { names.push_back(r.name); tot.push_back(0); cnt.push_back(0); }
        tot[k] += ms; cnt[k] += 1;
        hipEventDestroy(r.a); hipEventDestroy(r.b);
    }
    c->prof_recs.clear();
    std::string out;
    for (size_t k = 0; k < names.size(); ++k) { char line[160]; snprintf(line, sizeof(line), "%s %d %.6f\n", names[k].c_str(), cnt[k], tot[k]); out += line; }
    if (out.size() + 1 > n) return fail("nsk_profile_end: buffer too small (%zu needed)", out.size() + 1);
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}

extern "C" int nsk_last_call_stats(nsk_ctx* c, double* b, double* f, int* s)
{
    if (!c) return fail("null ctx");
    if (b) *b = c->last_bytes; if (f) *f = c->last_flops; if (s) *s = c->last_samples;
    return 0;
}

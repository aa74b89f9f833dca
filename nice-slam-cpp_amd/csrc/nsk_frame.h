// nsk_frame.h -- raw frames prepared on the device: conversion, undistortion, colour to the depth size, crop_size, crop_edge (upstream
// NICE-SLAM's dataset layer).  include/nsk.h states the rule (S0 .. S4) and the contract; tests/frame_checks.py restates it one numpy
// operation per fp32 operation.  This file is included by nsk.hip behind the context and the count helpers.
//
// One thread per output pixel does the three colour channels and the depth.  A workgroup is 64 x 4: a wave covers 64 consecutive pixels
// of one row, so neighbouring lanes gather neighbouring raw bytes and the 12 bytes a lane stores are contiguous across the wave.  The
// frame sits in blockIdx.z, the options in kernel arguments.  No LDS, no intermediate image: the stages that are on are evaluated by
// recursion over taps -- S3's four taps each evaluate S1 or S2 (four raw taps), 16 raw taps per channel at most -- and since every
// stage's value is a rounded fp32 in a register, the bytes are those of running the stages one after the other over stored images.
// Every product goes through mul_rn and every function switches contraction off, so no operation fuses with its neighbour.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "nsk_frame_plan.h"
#include "nsk_view.h"

struct FrameArgs {
    int Hc, Wc, Hd, Wd;             // raw sizes
    int Hs, Ws, e, H, W;            // the image crop_edge cuts from, the edge, the output size
    int s1, s2, s3, swap;
    float fx, fy, cx, cy, k[8];     // S1: k1 k2 p1 p2 k3 k4 k5 k6
    float png, scale;               // S0 of the depth
    float sy2, sx2;                 // S2: float(in) / float(out) per axis
    float sy3, sx3;                 // S3 colour: float(in - 1) / float(out - 1), 0 when out == 1
    float ny3, nx3;                 // S3 depth: float(in) / float(out)
};

// float(v) / 255.0f, correctly rounded, in three operations instead of the division's expansion: with y = RN(1 / 255), q = RN(a y), the
// residual r = a - 255 q is exact in an FMA and RN(q + r y) is the correctly rounded quotient (Markstein's correction step; no scaling is
// needed, a is 0 .. 255).  The FMAs are this function's own, not a contraction of the rule's operations; q alone is wrong for 126 of the 256
// bytes.  tests/test_frame_cpu.py proves all 256 in exact arithmetic, tests/test_gpu_frame.py compares all 256 on the device.
__device__ __forceinline__ float frame_value(uint8_t v)
{
    const float a = (float)v, y = 0x1.010102p-8f;
    const float q = mul_rn(a, y);
    const float r = __fmaf_rn(-255.0f, q, a);
    return __fmaf_rn(r, y, q);
}
__device__ __forceinline__ float frame_value(float v) { return v; }

template <typename CT>
__device__ __forceinline__ void frame_raw(const CT* __restrict__ img, int Wc, int y, int x, bool ok, float c[3])
{
    const CT* p = img + ((size_t)y * Wc + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = ok ? frame_value(p[ch]) : 0.f;
}

// top = lx0 v00 + lx1 v01, bot = lx0 v10 + lx1 v11, out = ly0 top + ly1 bot: six products and three sums, each rounded
__device__ __forceinline__ float frame_bilinear(float v00, float v01, float v10, float v11, float lx0, float lx1, float ly0, float ly1)
{
#pragma clang fp contract(off)
    const float top = __fadd_rn(mul_rn(lx0, v00), mul_rn(lx1, v01));
    const float bot = __fadd_rn(mul_rn(lx0, v10), mul_rn(lx1, v11));
    return __fadd_rn(mul_rn(ly0, top), mul_rn(ly1, bot));
}

// the taps of one axis for a source coordinate r >= 0: i0 = min(int(r), in - 1), i1 = min(i0 + 1, in - 1), l1 = r - float(i0)
__device__ __forceinline__ void frame_taps(float r, int n_in, int& i0, int& i1, float& l0, float& l1)
{
#pragma clang fp contract(off)
    i0 = min((int)r, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    l1 = __fsub_rn(r, (float)i0);
    l0 = __fsub_rn(1.f, l1);
}

// The colour at pixel (y, x) of the depth-size image: S1 or S2 over the converted raw image, or the raw pixel itself.  Returns whether
// S1 read a tap outside the image.  (y, x) is inside Hd x Wd; the caller's clamps see to that.
template <typename CT>
__device__ __forceinline__ bool frame_mid(const FrameArgs& A, const CT* __restrict__ img, int y, int x, float c[3])
{
#pragma clang fp contract(off)
    if (A.s1) {
        const float px = __fdiv_rn(__fsub_rn((float)x, A.cx), A.fx), py = __fdiv_rn(__fsub_rn((float)y, A.cy), A.fy);
        const float xx = mul_rn(px, px), yy = mul_rn(py, py), xy = mul_rn(px, py);
        const float r2 = __fadd_rn(xx, yy), r4 = mul_rn(r2, r2), r6 = mul_rn(r4, r2);
        const float num = __fadd_rn(__fadd_rn(__fadd_rn(1.f, mul_rn(A.k[0], r2)), mul_rn(A.k[1], r4)), mul_rn(A.k[4], r6));
        const float den = __fadd_rn(__fadd_rn(__fadd_rn(1.f, mul_rn(A.k[5], r2)), mul_rn(A.k[6], r4)), mul_rn(A.k[7], r6));
        const float rad = __fdiv_rn(num, den);
        const float xd = __fadd_rn(__fadd_rn(mul_rn(px, rad), mul_rn(mul_rn(2.f, A.k[2]), xy)), mul_rn(A.k[3], __fadd_rn(r2, mul_rn(2.f, xx))));
        const float yd = __fadd_rn(__fadd_rn(mul_rn(py, rad), mul_rn(A.k[2], __fadd_rn(r2, mul_rn(2.f, yy)))), mul_rn(mul_rn(2.f, A.k[3]), xy));
        const float us = __fadd_rn(mul_rn(A.fx, xd), A.cx), vs = __fadd_rn(mul_rn(A.fy, yd), A.cy);
        if (!(us > -1.f && us < (float)A.Wc && vs > -1.f && vs < (float)A.Hc)) {      // (NaN lands here)
            c[0] = 0.f; c[1] = 0.f; c[2] = 0.f;
            return true;
        }
        const float fi = floorf(us), fj = floorf(vs);
        const int i0 = (int)fi, j0 = (int)fj;                  // -1 .. Wc - 1, -1 .. Hc - 1
        const float lx1 = __fsub_rn(us, fi), ly1 = __fsub_rn(vs, fj), lx0 = __fsub_rn(1.f, lx1), ly0 = __fsub_rn(1.f, ly1);
        const bool x0 = i0 >= 0, x1 = i0 + 1 < A.Wc, y0 = j0 >= 0, y1 = j0 + 1 < A.Hc;
        const int ia = max(i0, 0), ib = min(i0 + 1, A.Wc - 1), ja = max(j0, 0), jb = min(j0 + 1, A.Hc - 1);      // (loads stay inside; a tap outside is 0)
        float v00[3], v01[3], v10[3], v11[3];
        frame_raw(img, A.Wc, ja, ia, y0 && x0, v00); frame_raw(img, A.Wc, ja, ib, y0 && x1, v01);
        frame_raw(img, A.Wc, jb, ia, y1 && x0, v10); frame_raw(img, A.Wc, jb, ib, y1 && x1, v11);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = frame_bilinear(v00[ch], v01[ch], v10[ch], v11[ch], lx0, lx1, ly0, ly1);
        return !(x0 && x1 && y0 && y1);
    }
    if (A.s2) {
        const float ry = fmaxf(__fsub_rn(mul_rn(__fadd_rn((float)y, 0.5f), A.sy2), 0.5f), 0.f);
        const float rx = fmaxf(__fsub_rn(mul_rn(__fadd_rn((float)x, 0.5f), A.sx2), 0.5f), 0.f);
        int i0, i1, j0, j1; float lx0, lx1, ly0, ly1;
        frame_taps(rx, A.Wc, i0, i1, lx0, lx1); frame_taps(ry, A.Hc, j0, j1, ly0, ly1);
        float v00[3], v01[3], v10[3], v11[3];
        frame_raw(img, A.Wc, j0, i0, true, v00); frame_raw(img, A.Wc, j0, i1, true, v01);
        frame_raw(img, A.Wc, j1, i0, true, v10); frame_raw(img, A.Wc, j1, i1, true, v11);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = frame_bilinear(v00[ch], v01[ch], v10[ch], v11[ch], lx0, lx1, ly0, ly1);
        return false;
    }
    frame_raw(img, A.Wc, y, x, true, c);
    return false;
}

template <typename CT, typename DT>
__global__ __launch_bounds__(256) void k_frame_prepare(FrameArgs A, const CT* __restrict__ color_raw, const DT* __restrict__ depth_raw,
                                                       float* __restrict__ color_out, float* __restrict__ depth_out,
                                                       unsigned long long* __restrict__ count)
{
#pragma clang fp contract(off)
    const int xo = blockIdx.x * 64 + threadIdx.x, yo = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    const bool live = xo < A.W && yo < A.H;
    bool border = false;
    if (live) {
        const int X = xo + A.e, Y = yo + A.e;                   // the pixel of the image crop_edge cuts from
        const size_t o = ((size_t)f * A.H + yo) * A.W + xo;
        if (color_out) {
            const CT* img = color_raw + (size_t)f * A.Hc * A.Wc * 3;
            float c[3];
            if (A.s3) {
                int i0, i1, j0, j1; float lx0, lx1, ly0, ly1;
                frame_taps(mul_rn((float)X, A.sx3), A.Wd, i0, i1, lx0, lx1); frame_taps(mul_rn((float)Y, A.sy3), A.Hd, j0, j1, ly0, ly1);
                float v00[3], v01[3], v10[3], v11[3];
                border = frame_mid(A, img, j0, i0, v00);
                border = frame_mid(A, img, j0, i1, v01) || border;
                border = frame_mid(A, img, j1, i0, v10) || border;
                border = frame_mid(A, img, j1, i1, v11) || border;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch] = frame_bilinear(v00[ch], v01[ch], v10[ch], v11[ch], lx0, lx1, ly0, ly1);
            } else {
                border = frame_mid(A, img, Y, X, c);
            }
            color_out[o * 3 + 0] = A.swap ? c[2] : c[0];
            color_out[o * 3 + 1] = c[1];
            color_out[o * 3 + 2] = A.swap ? c[0] : c[2];
        }
        if (depth_out) {
            int sx = X, sy = Y;
            if (A.s3) {
                sx = min((int)floorf(mul_rn((float)X, A.nx3)), A.Wd - 1);
                sy = min((int)floorf(mul_rn((float)Y, A.ny3)), A.Hd - 1);
            }
            const float v = (float)depth_raw[((size_t)f * A.Hd + sy) * A.Wd + sx];
            depth_out[o] = mul_rn(__fdiv_rn(v, A.png), A.scale);
        }
    }
    if (count) wave_count(border, count);                       // (blockDim.x = 64: a wave is a row of the workgroup, every lane arrives)
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
extern "C" int nsk_frame_plan(const nsk_frame_opts* opts, int Hc, int Wc, int Hd, int Wd, int* H_out, int* W_out, float intr_out[4])
{
    if (!opts) return fail("nsk_frame_plan: opts is NULL");
    FramePlan p;
    char msg[256];
    if (frame_plan(*opts, Hc, Wc, Hd, Wd, p, msg, sizeof(msg)) != 0) return fail("nsk_frame_plan: %s", msg);
    if (H_out) *H_out = p.H;
    if (W_out) *W_out = p.W;
    if (intr_out) for (int i = 0; i < 4; ++i) intr_out[i] = p.intr[i];
    return 0;
}

extern "C" int nsk_frame_prepare(nsk_ctx* c, const nsk_frame_opts* opts, int n, const void* color_raw, int color_type, int Hc, int Wc,
                                 const void* depth_raw, int depth_type, int Hd, int Wd, float* color_out, float* depth_out, int* h_n_border)
{
    if (!c) return fail("nsk_frame_prepare: null ctx");
    if (!opts) return fail("nsk_frame_prepare: opts is NULL");
    if (c->capturing) return fail("nsk_frame_prepare: not while a graph is being captured");
    FramePlan p;
    char msg[256];
    if (frame_plan(*opts, Hc, Wc, Hd, Wd, p, msg, sizeof(msg)) != 0) return fail("nsk_frame_prepare: %s", msg);
    if (n < 0 || n > 65535) return fail("nsk_frame_prepare: n = %d, must be 0 .. 65535", n);
    if ((long long)n * p.H * p.W >= (1ll << 31)) return fail("nsk_frame_prepare: n H' W' = %lld, must be below 2^31", (long long)n * p.H * p.W);
    if ((p.H + 3) / 4 > 65535) return fail("nsk_frame_prepare: H' = %d, at most 262140", p.H);
    if (h_n_border) *h_n_border = 0;
    if (n == 0) return 0;
    if ((color_raw == nullptr) != (color_out == nullptr)) return fail("nsk_frame_prepare: d_color_raw and d_color_out must both be given or both be NULL");
    if ((depth_raw == nullptr) != (depth_out == nullptr)) return fail("nsk_frame_prepare: d_depth_raw and d_depth_out must both be given or both be NULL");
    if (!color_raw && !depth_raw) return fail("nsk_frame_prepare: neither a colour nor a depth image");
    if (color_raw && color_type != NSK_FRAME_U8 && color_type != NSK_FRAME_F32) return fail("nsk_frame_prepare: color_type = %d, must be NSK_FRAME_U8 or NSK_FRAME_F32", color_type);
    if (depth_raw && depth_type != NSK_FRAME_U16 && depth_type != NSK_FRAME_F32) return fail("nsk_frame_prepare: depth_type = %d, must be NSK_FRAME_U16 or NSK_FRAME_F32", depth_type);
    HIPCHK(hipSetDevice(c->device));
    long long cnt = 0;
    long long* pcnt = h_n_border && color_raw && p.s1 ? &cnt : nullptr;
    CHK(count_begin(c, pcnt, "the border count"));
    FrameArgs A;
    A.Hc = Hc; A.Wc = Wc; A.Hd = Hd; A.Wd = Wd; A.Hs = p.Hs; A.Ws = p.Ws; A.e = p.e; A.H = p.H; A.W = p.W;
    A.s1 = p.s1; A.s2 = p.s2; A.s3 = p.s3; A.swap = opts->swap_rb ? 1 : 0;
    A.fx = opts->fx; A.fy = opts->fy; A.cx = opts->cx; A.cy = opts->cy;
    for (int i = 0; i < 8; ++i) A.k[i] = p.k[i];
    A.png = opts->png_depth_scale; A.scale = opts->scale;
    A.sy2 = (float)Hc / (float)Hd; A.sx2 = (float)Wc / (float)Wd;
    A.sy3 = p.Hs > 1 ? (float)(Hd - 1) / (float)(p.Hs - 1) : 0.f; A.sx3 = p.Ws > 1 ? (float)(Wd - 1) / (float)(p.Ws - 1) : 0.f;
    A.ny3 = (float)Hd / (float)p.Hs; A.nx3 = (float)Wd / (float)p.Ws;
    const dim3 grid((unsigned)((p.W + 63) / 64), (unsigned)((p.H + 3) / 4), (unsigned)n), block(64, 4);
    unsigned long long* d_cnt = pcnt ? c->count.get() : nullptr;
    const bool c8 = color_raw && color_type == NSK_FRAME_U8, d16 = depth_raw && depth_type == NSK_FRAME_U16;
    { ProfScope ps(c, "frame_prepare");
      if (c8 && d16) k_frame_prepare<<<grid, block, 0, c->stream>>>(A, (const uint8_t*)color_raw, (const uint16_t*)depth_raw, color_out, depth_out, d_cnt);
      else if (c8) k_frame_prepare<<<grid, block, 0, c->stream>>>(A, (const uint8_t*)color_raw, (const float*)depth_raw, color_out, depth_out, d_cnt);
      else if (d16) k_frame_prepare<<<grid, block, 0, c->stream>>>(A, (const float*)color_raw, (const uint16_t*)depth_raw, color_out, depth_out, d_cnt);
      else k_frame_prepare<<<grid, block, 0, c->stream>>>(A, (const float*)color_raw, (const float*)depth_raw, color_out, depth_out, d_cnt); }
    HIPCHK(hipGetLastError());
    CHK(count_end(c, pcnt));
    if (h_n_border) *h_n_border = (int)cnt;
    return 0;
}

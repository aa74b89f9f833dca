// nsk_frame_plan.h -- the host side of nsk_frame_prepare (include/nsk.h states the rule): the options validated, which stages run, the
// output size and the intrinsics moved along.  Nothing here needs HIP: nsk.hip includes it, and a host program may include it alone.
#pragma once
#include <cstdio>
#include "../../include/nsk.h"

struct FramePlan {
    int s1, s2, s3;                 // undistort, colour to the depth size, crop_size: on or off
    int Hs, Ws;                     // the size crop_edge cuts from: crop_size, or the depth size without one
    int e;                          // crop_edge
    int H, W;                       // the output size
    float intr[4];                  // fx fy cx cy of the output
    float k[8];                     // k1 k2 p1 p2 k3 k4 k5 k6, zeros beyond n_dist
};

// 0, or -1 with the reason in msg (the text names the option that is wrong)
inline int frame_plan(const nsk_frame_opts& o, int Hc, int Wc, int Hd, int Wd, FramePlan& p, char* msg, size_t cap)
{
    if (Hc < 1 || Wc < 1 || Hd < 1 || Wd < 1) { std::snprintf(msg, cap, "image size %d x %d (colour), %d x %d (depth): every side must be >= 1", Hc, Wc, Hd, Wd); return -1; }
    if (o.n_dist != 0 && o.n_dist != 4 && o.n_dist != 5 && o.n_dist != 8) { std::snprintf(msg, cap, "n_dist = %d, must be 0, 4, 5 or 8", o.n_dist); return -1; }
    if (o.crop_edge < 0) { std::snprintf(msg, cap, "crop_edge = %d, must be >= 0", o.crop_edge); return -1; }
    if (o.crop_H < 0 || o.crop_W < 0 || ((o.crop_H > 0) != (o.crop_W > 0))) {
        std::snprintf(msg, cap, "crop_size = (%d, %d): both positive, or both 0 for none", o.crop_H, o.crop_W); return -1; }
    const bool same = Hc == Hd && Wc == Wd;
    if (o.n_dist > 0 && !same) {
        std::snprintf(msg, cap, "undistort (n_dist = %d) needs equal sizes: colour %d x %d, depth %d x %d", o.n_dist, Hc, Wc, Hd, Wd); return -1; }
    p.s1 = o.n_dist > 0; p.s2 = !same; p.s3 = o.crop_H > 0;
    p.Hs = p.s3 ? o.crop_H : Hd; p.Ws = p.s3 ? o.crop_W : Wd;
    p.e = o.crop_edge;
    if (2ll * p.e >= p.Hs || 2ll * p.e >= p.Ws) { std::snprintf(msg, cap, "crop_edge = %d: 2 crop_edge must be below both sides of %d x %d", p.e, p.Hs, p.Ws); return -1; }
    p.H = p.Hs - 2 * p.e; p.W = p.Ws - 2 * p.e;
    float fx = o.fx, fy = o.fy, cx = o.cx, cy = o.cy;
    if (p.s3) {
        const float sx = (float)o.crop_W / (float)Wd, sy = (float)o.crop_H / (float)Hd;
        fx = fx * sx; cx = cx * sx; fy = fy * sy; cy = cy * sy;
    }
    if (p.e > 0) { cx = cx - (float)p.e; cy = cy - (float)p.e; }
    p.intr[0] = fx; p.intr[1] = fy; p.intr[2] = cx; p.intr[3] = cy;
    for (int i = 0; i < 8; ++i) p.k[i] = i < o.n_dist ? o.dist[i] : 0.f;
    return 0;
}

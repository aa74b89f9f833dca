// nsk_surface_plan.h -- the host side of nsk_mesh_nearest's grid (include/nsk.h states the rule; nsk_surface.h holds the kernels): the box, the
// cell edge h, the two caps and the wide-list limit.  Nothing here needs HIP: nsk.hip includes it, and host/test/surface_plan_test.cpp runs it
// alone under the sanitizers.  Nothing here can change a byte of the result: the grid only decides which triangles a query looks at.
//
// First choices, not tuned: SURF_CELLS_X4 cells aimed at per participating triangle, SURF_WIDE_CELLS, surf_ref_cap.
#pragma once
#include <algorithm>
#include <cmath>

#define SURF_MAX_CELLS (1 << 22)            // as the point grid's CLOUD_MAX_CELLS
#define SURF_WIDE_CELLS 64                  // a triangle whose box overlaps more cells than this is tested by every query instead (the wide list)
#define SURF_CELLS_X4 16                    // default of nsk_set_tuning "surface_cells_x4": four cells per participating triangle
#define SURF_MAX_GROW 400                   // h * 1.25^400 overflows any box: the growth loop cannot spin

// the most cell references the grid may hold: 16 per participating triangle, at least 2^22, below 2^31 (the scan counts in 32 bits)
inline long long surf_ref_cap(long long n_valid) { return std::min<long long>(std::max<long long>(1LL << 22, 16 * n_valid), 0x7fffffffLL); }

struct SurfPlan {
    float lo[3] = {0.f, 0.f, 0.f};      // the box's lower corner: plane 0 of every axis
    float h = 1.f, inv_h = 1.f;         // the cell edge as the kernels use it, and fl(1 / h)
    int dim[3] = {1, 1, 1};
    double hd = 1.0;                    // the edge before rounding: what surf_plan_grow multiplies
    double ext[3] = {0.0, 0.0, 0.0};
    bool on[3] = {false, false, false}; // an axis shorter than the edge (zero extent included) has one cell
    long long cells() const { return (long long)dim[0] * dim[1] * dim[2]; }
};

// dim and the rounded edge from hd; an axis whose extent is below the edge falls back to one cell.  Grows hd until the cells fit the cap
inline void surf_plan_dims(SurfPlan& P)
{
    for (int it = 0; it < SURF_MAX_GROW; ++it) {
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) {
            P.dim[a] = P.on[a] ? (int)std::min(std::floor(P.ext[a] / P.hd) + 1.0, (double)SURF_MAX_CELLS) : 1;
            cells *= P.dim[a];
        }
        if (cells <= (double)SURF_MAX_CELLS) break;
        P.hd *= 1.25;
    }
    if (P.cells() > SURF_MAX_CELLS) P.dim[0] = P.dim[1] = P.dim[2] = 1;       // (unreachable: 1.25^400 is past every finite extent)
    P.h = (float)P.hd; P.inv_h = 1.f / P.h;
}

// The grid over box = {min x y z, max x y z} of the vertices of the n_valid participating triangles: cubic cells, about cells_x4 / 4 per
// triangle, at most 2^22; h stays above 8 ulp of the largest coordinate, so the planes lo + k h are distinct fp32 numbers.
inline SurfPlan surf_plan(const float box[6], long long n_valid, int cells_x4)
{
    SurfPlan P;
    if (n_valid <= 0) return P;
    double big = 0.0;
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = box[a];
        P.ext[a] = (double)box[3 + a] - (double)box[a]; P.on[a] = P.ext[a] > 0.0;
        big = std::max(big, std::max(std::fabs((double)box[a]), std::fabs((double)box[3 + a])));
    }
    const double want = std::min((double)SURF_MAX_CELLS, std::max(1.0, (double)n_valid * cells_x4 / 4.0));
    double h = 1.0;
    for (;;) {                                                 // (at most three rounds: every round but the last drops an axis)
        int k = 0; double logv = 0.0;
        for (int a = 0; a < 3; ++a) if (P.on[a]) { ++k; logv += std::log(P.ext[a]); }
        if (k == 0) return P;                                  // every vertex at one point: one cell
        h = std::exp((logv - std::log(want)) / k);
        bool dropped = false;
        for (int a = 0; a < 3; ++a) if (P.on[a] && P.ext[a] < h) { P.on[a] = false; dropped = true; }
        if (!dropped) break;
    }
    h = std::max(h, std::max(big * 9.5367431640625e-7, 1e-30));        // 8 ulp of the largest coordinate
    P.hd = std::min(h, 1e37);
    surf_plan_dims(P);
    return P;
}

// too many references: the edge times 1.25.  false when the grid is one cell already (then every triangle has one reference, which fits)
inline bool surf_plan_grow(SurfPlan& P)
{
    if (P.cells() <= 1) return false;
    const bool at_cap = P.hd >= 1e37;                          // the edge cannot grow further: one cell
    P.hd = std::min(P.hd * 1.25, 1e37);
    for (int a = 0; a < 3; ++a) if (P.on[a] && (at_cap || P.ext[a] < P.hd)) P.on[a] = false;
    surf_plan_dims(P);
    return true;
}

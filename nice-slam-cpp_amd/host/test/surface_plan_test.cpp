// surface_plan_test -- the host side of nsk_mesh_nearest's grid (csrc/nsk_surface_plan.h) alone, under the sanitizers
// (tests/test_surface_cpu.py): the box, the cell edge, the caps on cells and references, the growth loop and its end.
#include <cmath>
#include <cstdio>

#include "nsk_surface_plan.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

// what every plan must satisfy: cells within the cap, planes that stay distinct, a grid that covers the box
static void check(const SurfPlan& P, const float box[6])
{
    EXPECT(P.cells() >= 1 && P.cells() <= SURF_MAX_CELLS);
    EXPECT(P.h > 0.f && std::isfinite(P.h) && std::isfinite(P.inv_h));
    double big = 0.0;
    for (int a = 0; a < 3; ++a) big = std::fmax(big, std::fmax(std::fabs((double)box[a]), std::fabs((double)box[3 + a])));
    for (int a = 0; a < 3; ++a) {
        EXPECT(P.dim[a] >= 1);
        if (P.dim[a] > 1) {
            EXPECT((double)P.h >= big * 9.5e-7);                                // 8 ulp of the largest coordinate
            EXPECT((double)P.dim[a] * P.hd > (double)box[3 + a] - (double)box[a]);       // the last cell reaches past the box
            EXPECT(P.lo[a] == box[a]);
        }
    }
}

int main()
{
    // a unit sheet of 286 triangles: z has one cell, about four cells per triangle at the default
    {
        const float box[6] = {0.f, 0.f, 0.25f, 1.f, 1.f, 0.25f};
        SurfPlan P = surf_plan(box, 286, SURF_CELLS_X4);
        check(P, box);
        EXPECT(P.dim[2] == 1 && P.dim[0] == P.dim[1] && P.cells() >= 286 * 3 && P.cells() <= 286 * 6);
        SurfPlan Q = surf_plan(box, 286, 1);
        check(Q, box);
        EXPECT(Q.cells() < P.cells() && Q.h > P.h);
        // growing: the edge times 1.25 every time, down to one cell, and then no further
        int rounds = 0;
        float before = P.h;
        while (surf_plan_grow(P)) { check(P, box); EXPECT(P.h > before); before = P.h; ++rounds; EXPECT(rounds < SURF_MAX_GROW); if (rounds >= SURF_MAX_GROW) break; }
        EXPECT(P.cells() == 1 && rounds > 3 && !surf_plan_grow(P));
    }
    // nothing takes part, one point, a segment
    {
        const float box[6] = {3.f, 3.f, 3.f, 3.f, 3.f, 3.f};
        SurfPlan P = surf_plan(box, 0, 16);
        EXPECT(P.cells() == 1);
        P = surf_plan(box, 5, 16);
        check(P, box); EXPECT(P.cells() == 1 && !surf_plan_grow(P));
        const float seg[6] = {-1.f, 2.f, 0.f, 1.f, 2.f, 0.f};
        P = surf_plan(seg, 100, 4);
        check(P, seg); EXPECT(P.dim[0] >= 100 && P.dim[0] <= 101 && P.dim[1] == 1 && P.dim[2] == 1);
    }
    // the cell cap: many triangles in a cube, and a box so thin and long that one axis alone wants more than 2^22 cells
    {
        const float box[6] = {-4.f, -4.f, -4.f, 4.f, 4.f, 4.f};
        SurfPlan P = surf_plan(box, 100000000LL, 256);
        check(P, box); EXPECT(P.cells() > SURF_MAX_CELLS / 4);
        const float thin[6] = {0.f, 0.f, 0.f, 1e6f, 1e-3f, 1e-3f};
        P = surf_plan(thin, 50000000LL, 256);
        check(P, thin);
    }
    // far from the origin the edge is held above 8 ulp: a box of a few ulp gets one cell per axis or few
    {
        const float lo = 1e6f, hi = std::nextafter(std::nextafter(1e6f, 2e6f), 2e6f);
        const float box[6] = {lo, lo, lo, hi, hi, hi};
        SurfPlan P = surf_plan(box, 1000, 16);
        check(P, box); EXPECT(P.cells() == 1);
    }
    // the largest floats: nothing overflows, the growth loop ends
    {
        const float m = 3.0e38f;
        const float box[6] = {-m, -m, -m, m, m, m};
        SurfPlan P = surf_plan(box, 1000, 16);
        check(P, box);
        int rounds = 0;
        while (surf_plan_grow(P) && rounds < SURF_MAX_GROW) ++rounds;
        EXPECT(rounds < SURF_MAX_GROW);
    }
    // the reference cap: 16 per triangle, at least 2^22, below 2^31
    EXPECT(surf_ref_cap(0) == (1LL << 22) && surf_ref_cap(286) == (1LL << 22) && surf_ref_cap(1 << 20) == (1LL << 24));
    EXPECT(surf_ref_cap(2000000000LL) == 0x7fffffffLL && surf_ref_cap(1 << 20) >= (1 << 20));
    EXPECT(SURF_WIDE_CELLS >= 8 && SURF_WIDE_CELLS <= 4096);
    if (failures) { std::printf("surface_plan_test: %d FAILED\n", failures); return 1; }
    std::printf("surface_plan_test: ok\n");
    return 0;
}

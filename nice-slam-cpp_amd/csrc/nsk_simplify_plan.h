// nsk_simplify_plan.h -- the host side of nsk_mesh_simplify (include/nsk.h states the rule; nsk_simplify.h holds the kernels): the argument
// checks, the grid's dimensions from the finite vertices' box, the caps, the scratch's byte counts and the list threshold.  Nothing here
// needs HIP: nsk.hip includes it, and host/test/simplify_plan_test.cpp runs it alone under the sanitizers.
//
// First choice, not tuned: SIMP_LIST_SHORT.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#define SIMP_MAX_CELLS (1ll << 28)          // cells of the grid: the cell index and the occupied cells' ranks stay below 2^31
#define SIMP_MAX_AXIS ((1ll << 21) - 1)     // cells along one axis: h_info[7] packs 21 bits per axis
#define SIMP_FRAC_BITS 20                   // the fixed point of a vertex inside its cell: q in [0, 2^20]
#define SIMP_MAX_COUNT (0x7fffffff / 3)     // vertices, triangles: 3 n stays an int, and a cell's sums stay below 2^51
#define SIMP_LIST_SHORT 32                  // a smallest-corner list of up to this many triangles is searched by one thread, a longer one by a workgroup
#define SIMP_SCAN_BLOCK 256                 // elements per workgroup of the multi-launch scan (MC_BLOCK)

enum { SIMP_OK = 0, SIMP_BAD_CELL = 1, SIMP_TOO_MANY_CELLS = 2, SIMP_AXIS_TOO_LONG = 3 };

struct SimplifyPlan {
    double lo[3] = {0.0, 0.0, 0.0};         // the finite vertices' minima: plane 0 of every axis
    double cell = 1.0;                      // double(cell)
    long long n[3] = {0, 0, 0};             // cells per axis (0: no finite vertex)
    long long cells = 0;
    double cells_approx = 0.0;              // the product in double: what an error names when it is past 2^62
    long long packed() const { return n[0] | (n[1] << 21) | (n[2] << 42); }
};

// c_a of a coordinate: g = (double(p) - lo) / cell, floor(g); each operation an fp64 operation of its own
inline double simplify_g(double p, double lo, double cell) { const volatile double d = p - lo; return d / cell; }
inline long long simplify_cell_coord(float p, double lo, double cell) { return (long long)std::floor(simplify_g((double)p, lo, cell)); }
// q_a: rint((g - c) 2^20), ties to even (the default rounding mode)
inline long long simplify_frac(float p, double lo, double cell)
{
    const double g = simplify_g((double)p, lo, cell);
    return (long long)std::nearbyint((g - std::floor(g)) * (double)(1 << SIMP_FRAC_BITS));
}
// the representative of cell coordinate c with the sum of its members' q and their count
inline float simplify_position(double lo, double cell, long long c, unsigned long long sum, unsigned count)
{
    const double m = (double)sum / (double)count;
    const volatile double t = ((double)c + m / (double)(1 << SIMP_FRAC_BITS)) * cell;
    return (float)(lo + t);
}

// The grid over the finite vertices' box (lo, hi: their minima and maxima widened to double; finite: how many there are).
inline int simplify_plan(const double lo[3], const double hi[3], float cell, long long finite, SimplifyPlan& P)
{
    P = SimplifyPlan();
    if (!(std::isfinite(cell) && cell > 0.f)) return SIMP_BAD_CELL;
    P.cell = (double)cell;
    if (finite <= 0) return SIMP_OK;
    bool long_axis = false;
    double approx = 1.0;
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = lo[a];
        const double top = std::floor(simplify_g(hi[a], lo[a], P.cell));       // c_a(hi_a): finite, the box and the cell are
        approx *= top + 1.0;
        if (top + 1.0 > (double)SIMP_MAX_CELLS) { P.n[a] = SIMP_MAX_CELLS + 1; long_axis = true; continue; }
        P.n[a] = (long long)top + 1;
        if (P.n[a] > SIMP_MAX_AXIS) long_axis = true;
    }
    P.cells_approx = approx;
    if (approx > (double)SIMP_MAX_CELLS) { P.cells = approx < 4.0e18 ? P.n[0] * P.n[1] * P.n[2] : -1; return SIMP_TOO_MANY_CELLS; }
    P.cells = P.n[0] * P.n[1] * P.n[2];
    if (long_axis) return SIMP_AXIS_TOO_LONG;
    return SIMP_OK;
}

// words of the multi-launch scan over n values: every level at a 64-word boundary, until one workgroup covers a level (mc_scan_words)
inline size_t simplify_scan_words(size_t n)
{
    size_t words = 0;
    for (;;) { words += (n + 63) & ~(size_t)63; if (n <= SIMP_SCAN_BLOCK) return words; n = (n + SIMP_SCAN_BLOCK - 1) / SIMP_SCAN_BLOCK; }
}
// entries of the queue of long lists: a long list holds more than SIMP_LIST_SHORT of the nt triangles
inline size_t simplify_long_cap(size_t nt) { return nt / (SIMP_LIST_SHORT + 1) + 1; }

// the scratch of one call, in bytes
struct SimplifyBytes {
    size_t per_vertex, per_cell, per_occupied, per_triangle, fixed;
    size_t total() const { return per_vertex + per_cell + per_occupied + per_triangle + fixed; }
};
inline SimplifyBytes simplify_bytes(size_t nv, size_t nt, size_t cells, size_t occupied)
{
    SimplifyBytes B;
    B.per_vertex = nv * 4;                                                     // the vertex's cell
    B.per_cell = simplify_scan_words(cells + 1) * 4;                           // occupancy flag -> rank
    B.per_occupied = occupied * (4 + 24 + 4) + 2 * simplify_scan_words(occupied + 1) * 4;     // count, three sums, the cell; the lists' ends; the referenced flags
    B.per_triangle = nt * (12 + 4) + simplify_scan_words(nt + 1) * 4 + simplify_long_cap(nt) * 4;      // corner ranks, list slot; kept flag; the long queue
    B.fixed = 8 * 1024 * 4 + 8 * 4;                                            // the bounds' partial boxes, the counters
    return B;
}

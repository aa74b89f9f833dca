// simplify_plan_test -- the host side of nsk_mesh_simplify (csrc/nsk_simplify_plan.h) alone, under the sanitizers
// (tests/test_simplify_cpu.py): the argument check, the grid's dimensions, the caps and their errors, the byte counts and the list
// threshold on known values; and, given a file, the records tests/simplify_checks.py made: per case the box, the cell and what the plan
// must answer, points with their cell coordinates and fixed-point fractions, cells with their sums and the representative's coordinate.
//   simplify_plan_test [CASES.bin]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nsk_simplify_plan.h"

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

template <typename T>
static bool get(FILE* f, T& v) { return std::fread(&v, sizeof(T), 1, f) == 1; }

static void run_file(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("FAILED: cannot open %s\n", path); ++failures; return; }
    int32_t n_cases = 0;
    bool ok = get(f, n_cases);
    long long points = 0, reps = 0;
    for (int k = 0; ok && k < n_cases; ++k) {
        float cell; double lo[3], hi[3]; int64_t finite, n[3], cells; int32_t rc, n_pts, n_rep;
        ok = get(f, cell) && get(f, lo) && get(f, hi) && get(f, finite) && get(f, rc) && get(f, n) && get(f, cells) && get(f, n_pts);
        if (!ok) break;
        SimplifyPlan P;
        const int r = simplify_plan(lo, hi, cell, finite, P);
        EXPECT(r == rc);
        if (r == SIMP_OK) {
            EXPECT(P.n[0] == n[0] && P.n[1] == n[1] && P.n[2] == n[2] && P.cells == cells);
            EXPECT(P.packed() == (long long)(n[0] | (n[1] << 21) | (n[2] << 42)));
        }
        for (int i = 0; ok && i < n_pts; ++i, ++points) {
            float p[3]; int64_t c[3], q[3];
            ok = get(f, p) && get(f, c) && get(f, q);
            if (!ok) break;
            for (int a = 0; a < 3; ++a) {
                EXPECT(simplify_cell_coord(p[a], lo[a], (double)cell) == c[a]);
                EXPECT(simplify_frac(p[a], lo[a], (double)cell) == q[a]);
                EXPECT(c[a] >= 0 && c[a] < P.n[a] && q[a] >= 0 && q[a] <= (1 << SIMP_FRAC_BITS));
            }
        }
        ok = ok && get(f, n_rep);
        for (int i = 0; ok && i < n_rep; ++i, ++reps) {
            int32_t axis; int64_t c; uint64_t sum; uint32_t count; float pos;
            ok = get(f, axis) && get(f, c) && get(f, sum) && get(f, count) && get(f, pos);
            if (!ok) break;
            const float mine = simplify_position(lo[axis], (double)cell, c, sum, count);
            EXPECT(std::memcmp(&mine, &pos, 4) == 0);
        }
    }
    if (!ok) { std::printf("FAILED: %s is truncated\n", path); ++failures; }
    std::fclose(f);
    std::printf("simplify_plan_test: %d cases, %lld points, %lld representatives from %s\n", (int)n_cases, points, reps, path);
}

int main(int argc, char** argv)
{
    SimplifyPlan P;
    const double lo[3] = {-1.0, 0.0, 2.0}, hi[3] = {1.0, 0.0, 2.5};
    // the cell: finite and positive
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float bad : {0.f, -0.f, -1.f, inf, -inf, nan}) EXPECT(simplify_plan(lo, hi, bad, 10, P) == SIMP_BAD_CELL);
    EXPECT(simplify_plan(lo, hi, std::numeric_limits<float>::denorm_min(), 10, P) == SIMP_TOO_MANY_CELLS && P.cells == -1 && P.cells_approx > 1e40);
    // no finite vertex: no grid
    EXPECT(simplify_plan(lo, hi, 0.5f, 0, P) == SIMP_OK && P.cells == 0 && P.packed() == 0);
    // n_a = floor((hi - lo) / cell) + 1: a vertex on the last plane opens a cell of its own; an axis without extent has one cell
    EXPECT(simplify_plan(lo, hi, 0.5f, 10, P) == SIMP_OK && P.n[0] == 5 && P.n[1] == 1 && P.n[2] == 2 && P.cells == 10);
    EXPECT(P.packed() == (5ll | (1ll << 21) | (2ll << 42)));
    EXPECT(simplify_plan(lo, hi, 0.75f, 10, P) == SIMP_OK && P.n[0] == 3 && P.n[2] == 1);
    EXPECT(simplify_plan(lo, hi, 1e30f, 10, P) == SIMP_OK && P.cells == 1);
    // the caps: 2^28 cells pass, one more plane does not; an axis of 2^21 cells does not although its cells do
    {
        const double l[3] = {0.0, 0.0, 0.0}, h1[3] = {1023.0, 511.0, 511.0}, h2[3] = {1024.0, 511.0, 511.0}, h3[3] = {2097151.0, 0.0, 0.0},
                     h4[3] = {2097150.0, 127.0, 0.0};
        EXPECT(simplify_plan(l, h1, 1.f, 5, P) == SIMP_OK && P.cells == SIMP_MAX_CELLS);
        EXPECT(simplify_plan(l, h2, 1.f, 5, P) == SIMP_TOO_MANY_CELLS && P.cells == 1025ll * 512 * 512);
        EXPECT(simplify_plan(l, h3, 1.f, 5, P) == SIMP_AXIS_TOO_LONG && P.n[0] == (1ll << 21));
        EXPECT(simplify_plan(l, h4, 1.f, 5, P) == SIMP_OK && P.n[0] == SIMP_MAX_AXIS && P.cells == SIMP_MAX_AXIS * 128);
        const double big[3] = {3.0e38, 3.0e38, 3.0e38}, small[3] = {-3.0e38, -3.0e38, -3.0e38};
        EXPECT(simplify_plan(small, big, 1e-30f, 5, P) == SIMP_TOO_MANY_CELLS && P.cells == -1 && std::isfinite(P.cells_approx));
        EXPECT(simplify_plan(small, big, 2.9e38f, 5, P) == SIMP_OK && P.cells == 27);
    }
    // the fixed point: [0, 2^20], ties to even; the representative of one vertex is that vertex up to the quantum
    EXPECT(simplify_cell_coord(1.f, -1.0, 0.5) == 4 && simplify_frac(1.f, -1.0, 0.5) == 0);
    EXPECT(simplify_cell_coord(0.875f, -1.0, 0.5) == 3 && simplify_frac(0.875f, -1.0, 0.5) == 3 << 18);
    EXPECT(simplify_frac((float)(0.5 / 1048576.0), 0.0, 1.0) == 0 && simplify_frac((float)(1.5 / 1048576.0), 0.0, 1.0) == 2);
    EXPECT(simplify_position(-1.0, 0.5, 3, 3ull << 18, 1) == 0.875f && simplify_position(-1.0, 0.5, 3, (3ull << 18) * 7, 7) == 0.875f);
    EXPECT(simplify_position(0.0, 1.0, 2, 3ull << 19, 2) == 2.75f);
    // the scan's levels and the byte counts
    EXPECT(simplify_scan_words(1) == 64 && simplify_scan_words(256) == 256 && simplify_scan_words(257) == 320 + 64);
    EXPECT(simplify_scan_words(65537) == 65600 + 320 + 64);
    EXPECT(simplify_long_cap(0) == 1 && simplify_long_cap(33) == 2 && simplify_long_cap(1000) * (SIMP_LIST_SHORT + 1) > 1000);
    {
        const SimplifyBytes B = simplify_bytes(1000, 2000, 4096, 500);
        EXPECT(B.per_vertex == 4000 && B.per_cell == simplify_scan_words(4097) * 4 && B.per_occupied == 500 * 32 + 2 * simplify_scan_words(501) * 4);
        EXPECT(B.per_triangle == 2000 * 16 + simplify_scan_words(2001) * 4 + simplify_long_cap(2000) * 4 && B.total() > B.per_triangle);
        const SimplifyBytes Z = simplify_bytes(0, 0, 0, 0);
        EXPECT(Z.per_vertex == 0 && Z.total() == Z.fixed + 3 * 64 * 4 + 64 * 4 + 4);
    }
    EXPECT(SIMP_LIST_SHORT >= 4 && SIMP_LIST_SHORT <= 1024 && SIMP_MAX_COUNT == 715827882);
    if (argc > 1) run_file(argv[1]);
    if (failures) { std::printf("simplify_plan_test: %d FAILED\n", failures); return 1; }
    std::printf("simplify_plan_test: ok\n");
    return 0;
}

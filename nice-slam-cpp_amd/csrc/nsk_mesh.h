// nsk_mesh.h -- scene mesh extraction: lattice points for the decoders' forward, marching cubes on the occupancy volume.
// (The reference has no mesher; the behaviour follows the `meshing:` keys of its config/nice_slam.yaml.  include/nsk.h states the contract.)
//
// Numbering (also what nsk_mesh_table reports):
//   corner c of a cell = (x, y, z) offsets (c & 1, (c >> 1) & 1, c >> 2); case index bit c is set when corner c is INSIDE (value > level);
//   edge e = 4 * axis + idx runs along `axis` (0 x, 1 y, 2 z) from the corner whose two other offsets are (idx & 1, idx >> 1) in axis order:
//     0..3  along x from (0, y, z) with idx = y + 2 z;   4..7 along y from (x, 0, z) with idx = x + 2 z;   8..11 along z from (x, y, 0) with idx = x + 2 y.
// The 256-case table is derived, not typed: on each of the six faces the crossing edges are joined by a rule that reads that face's four
// corner signs only (an ambiguous face -- two inside corners on a diagonal -- always cuts the inside corners off one by one), so two cells
// that share a face leave the same segments on it, in opposite directions: the mesh has no cracks whatever the cases are.  The directed
// segments are the boundary of the inside region on the cube's surface (inside on the right, seen from outside the cube: clockwise round
// an inside corner); they chain into closed loops, and a fan over each loop gives triangles whose normal points from the inside to the outside.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "nsk_reduce.h"
#include "nsk_view.h"

#define MC_ROW 16                   // table row stride in edge numbers: the largest case has 5 triangles (tests/test_mesh_cpu.py asserts it)
#define MC_BLOCK 256                // nodes per workgroup of the extraction passes, elements per workgroup of the scan passes
#define MC_MAX_NODES (1ll << 28)    // keeps every 32-bit sum (at most 5 triangles / 3 vertices per node) below 2^32

struct McTable {
    int8_t edges[256][MC_ROW];      // three edge numbers per triangle, -1 behind the last
    uint8_t ntri[256];
    int max_tri;
};

static inline int mc_edge_of(int p, int q)       // the edge between two corners that differ along one axis
{
    const int lo = p < q ? p : q, d = p ^ q;
    const int x = lo & 1, y = (lo >> 1) & 1, z = lo >> 2;
    if (d == 1) return 0 + y + 2 * z;
    if (d == 2) return 4 + x + 2 * z;
    return 8 + x + 2 * y;
}

static inline McTable mc_build_table()
{
    McTable T;
    memset(T.edges, -1, sizeof(T.edges));
    memset(T.ntri, 0, sizeof(T.ntri));
    T.max_tri = 0;
    // the four corners of each face, counter-clockwise seen from outside the cube, and which faces an edge lies in
    int fc[6][4], face_mask[12] = {0};
    for (int a = 0; a < 3; ++a)
        for (int s = 0; s < 2; ++s) {
            const int u = (a + 1) % 3, v = (a + 2) % 3;
            static const int ccw[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
            for (int k = 0; k < 4; ++k) {
                const int kk = s ? k : (4 - k) % 4;                 // seen from the -axis side the same square runs the other way round
                fc[2 * a + s][k] = (s << a) | (ccw[kk][0] << u) | (ccw[kk][1] << v);
            }
            for (int k = 0; k < 4; ++k) face_mask[mc_edge_of(fc[2 * a + s][k], fc[2 * a + s][(k + 1) & 3])] |= 1 << (2 * a + s);
        }
    for (int cs = 0; cs < 256; ++cs) {
        int next[12];
        for (int e = 0; e < 12; ++e) next[e] = -1;
        for (int f = 0; f < 6; ++f) {
            bool in[4]; int nin = 0;
            for (int k = 0; k < 4; ++k) { in[k] = (cs >> fc[f][k]) & 1; nin += in[k]; }
            if (nin == 0 || nin == 4) continue;
            for (int k = 0; k < 4; ++k) {
                if (!in[k] || in[(k + 3) & 3]) continue;           // k starts a run of inside corners
                int j = k;
                while (in[(j + 1) & 3]) j = (j + 1) & 3;
                next[mc_edge_of(fc[f][(k + 3) & 3], fc[f][k])] = mc_edge_of(fc[f][j], fc[f][(j + 1) & 3]);
            }
        }
        bool seen[12] = {false};
        int nt = 0;
        for (int e0 = 0; e0 < 12; ++e0) {
            if (next[e0] < 0 || seen[e0]) continue;
            int loop[12], n = 0;
            for (int e = e0; !seen[e]; e = next[e]) { seen[e] = true; loop[n++] = e; }
            // fan apex: the corner whose diagonals run through the cell, not inside a face (first such corner; ties to the lowest position)
            int best = 0, best_bad = 1 << 30;
            for (int r = 0; r < n; ++r) {
                int bad = 0;
                for (int i = 2; i + 1 < n; ++i) bad += (face_mask[loop[r]] & face_mask[loop[(r + i) % n]]) != 0;
                if (bad < best_bad) { best_bad = bad; best = r; }
            }
            for (int i = 1; i + 1 < n; ++i, ++nt) {
                T.edges[cs][3 * nt] = (int8_t)loop[best];
                T.edges[cs][3 * nt + 1] = (int8_t)loop[(best + i) % n];
                T.edges[cs][3 * nt + 2] = (int8_t)loop[(best + i + 1) % n];
            }
        }
        T.ntri[cs] = (uint8_t)nt;
        if (nt > T.max_tri) T.max_tri = nt;
    }
    return T;
}

static inline const McTable& mc_table()
{
    static const McTable T = mc_build_table();
    return T;
}

// ---- device ------------------------------------------------------------------------------------------------
struct McGeom {
    int nx, ny, nz, nn;            // nodes per axis, nodes in all (<= MC_MAX_NODES)
    float o[3], s[3];              // node (i, j, k) sits at o + (i, j, k) * s, each product and sum rounded on its own
    float level;
};

__device__ __forceinline__ float mc_coord(float o, int i, float s) { return __fadd_rn(o, mul_rn((float)i, s)); }       // (mul_rn: never fused)
// node n (x fastest) as a point
__device__ __forceinline__ void lattice_node(const McGeom& G, int n, float p[3])
{
    const int i = n % G.nx, r = n / G.nx, j = r % G.ny, k = r / G.ny;
    p[0] = mc_coord(G.o[0], i, G.s[0]); p[1] = mc_coord(G.o[1], j, G.s[1]); p[2] = mc_coord(G.o[2], k, G.s[2]);
}

// the lattice nodes [n0, n0 + cnt) as points for the decoders' forward
__global__ __launch_bounds__(256) void k_lattice_points(McGeom G, long long n0, int cnt, float* __restrict__ pts)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= cnt) return;
    const long long n = n0 + m, r = n / G.nx;
    const int i = (int)(n % G.nx), j = (int)(r % G.ny), k = (int)(r / G.ny);
    pts[3 * (size_t)m] = mc_coord(G.o[0], i, G.s[0]);
    pts[3 * (size_t)m + 1] = mc_coord(G.o[1], j, G.s[1]);
    pts[3 * (size_t)m + 2] = mc_coord(G.o[2], k, G.s[2]);
}

// occupancy of the slab with the in-bound rule of eval_points (reference src/Renderer.cpp:26-36)
__global__ __launch_bounds__(256) void k_lattice_finish(int cnt, const float* __restrict__ pts, const float* __restrict__ bound6,
                                                        const float* __restrict__ occ_a, const float* __restrict__ occ_b, float* __restrict__ vol)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= cnt) return;
    const float px = pts[3 * (size_t)m], py = pts[3 * (size_t)m + 1], pz = pts[3 * (size_t)m + 2];
    const bool inb = px < bound6[1] && px > bound6[0] && py < bound6[3] && py > bound6[2] && pz < bound6[5] && pz > bound6[4];
    float occ = occ_a[m];
    if (occ_b) occ = occ_b[m] + occ;
    vol[m] = inb ? occ : 100.f;
}

// (D) per cell: case index (0 for a cell that is not processed: such a cell and the two uniform cases emit nothing) and triangle count
__global__ __launch_bounds__(256) void k_mc_cells(McGeom G, const float* __restrict__ vol, const uint8_t* __restrict__ valid,
                                                  const uint8_t* __restrict__ ntri, uint8_t* __restrict__ cellcase, unsigned* __restrict__ bsum)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    unsigned cnt = 0;
    if (n < G.nn) {
        const int i = n % G.nx, r = n / G.nx, j = r % G.ny, k = r / G.ny;
        unsigned code = 0;
        if (i < G.nx - 1 && j < G.ny - 1 && k < G.nz - 1) {
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const size_t q = (size_t)n + (c & 1) + (size_t)((c >> 1) & 1) * G.nx + (size_t)(c >> 2) * G.nx * G.ny;
                const float v = vol[q];
                ok = ok && (fabsf(v) <= 3.402823466e38f) && (!valid || valid[q]);       // (the comparison fails for NaN and +-inf)
                code |= (v > G.level ? 1u : 0u) << c;
            }
            if (!ok) code = 0;
        }
        cellcase[n] = (uint8_t)code;
        cnt = ntri[code];
    }
    unsigned total;
    block_scan(cnt, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// the three edges a node owns (+x, +y, +z): an edge carries a vertex when its ends lie on different sides of the level and one of the
// (up to four) cells around it is processed
__device__ __forceinline__ unsigned mc_edge_flags(const McGeom& G, const float* __restrict__ vol, const uint8_t* __restrict__ cellcase, int n,
                                                  int i, int j, int k, float v0, float* v1)
{
    const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
    const bool in0 = v0 > G.level;
    unsigned flags = 0;
    if (i < G.nx - 1) {
        v1[0] = vol[(size_t)n + 1];
        if ((v1[0] > G.level) != in0) {
            bool p = cellcase[n] != 0;
            if (j > 0) p = p || cellcase[n - sy] != 0;
            if (k > 0) p = p || cellcase[n - sz] != 0;
            if (j > 0 && k > 0) p = p || cellcase[n - sy - sz] != 0;
            if (p) flags |= 1u;
        }
    }
    if (j < G.ny - 1) {
        v1[1] = vol[(size_t)n + sy];
        if ((v1[1] > G.level) != in0) {
            bool p = cellcase[n] != 0;
            if (i > 0) p = p || cellcase[n - 1] != 0;
            if (k > 0) p = p || cellcase[n - sz] != 0;
            if (i > 0 && k > 0) p = p || cellcase[n - 1 - sz] != 0;
            if (p) flags |= 2u;
        }
    }
    if (k < G.nz - 1) {
        v1[2] = vol[(size_t)n + sz];
        if ((v1[2] > G.level) != in0) {
            bool p = cellcase[n] != 0;
            if (i > 0) p = p || cellcase[n - 1] != 0;
            if (j > 0) p = p || cellcase[n - sy] != 0;
            if (i > 0 && j > 0) p = p || cellcase[n - 1 - sy] != 0;
            if (p) flags |= 4u;
        }
    }
    return flags;
}

// (A) EMIT = false: vertices per workgroup.  (C) EMIT = true: vertex ids by rank (boff = scanned workgroup counts), the edge -> vertex
// map emap[3 n + axis] (-1: no vertex) and the positions p0 + t (p1 - p0), t = (level - v0) / (v1 - v0), every operation rounded on its own
template <bool EMIT>
__global__ __launch_bounds__(256) void k_mc_edges(McGeom G, const float* __restrict__ vol, const uint8_t* __restrict__ cellcase,
                                                  unsigned* __restrict__ bsum, const unsigned* __restrict__ boff, int* __restrict__ emap,
                                                  float* __restrict__ verts)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    unsigned flags = 0;
    int i = 0, j = 0, k = 0;
    float v0 = 0.f, v1[3] = {0.f, 0.f, 0.f};
    if (n < G.nn) {
        i = n % G.nx; const int r = n / G.nx; j = r % G.ny; k = r / G.ny;
        v0 = vol[n];
        flags = mc_edge_flags(G, vol, cellcase, n, i, j, k, v0, v1);
    }
    unsigned total;
    const unsigned cnt = __popc(flags), excl = block_scan(cnt, &total) - cnt;
    if (!EMIT) { if (threadIdx.x == 0) bsum[blockIdx.x] = total; return; }
    if (n >= G.nn) return;
    unsigned id = boff[blockIdx.x] + excl;
    const int idx[3] = {i, j, k};
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = mc_coord(G.o[a], idx[a], G.s[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(flags & (1u << a))) { emap[3 * (size_t)n + a] = -1; continue; }
        const float p1 = mc_coord(G.o[a], idx[a] + 1, G.s[a]);
        const float t = __fdiv_rn(__fsub_rn(G.level, v0), __fsub_rn(v1[a], v0));
        float q[3] = {p[0], p[1], p[2]};
        q[a] = __fadd_rn(p[a], mul_rn(t, __fsub_rn(p1, p[a])));
        verts[3 * (size_t)id] = q[0]; verts[3 * (size_t)id + 1] = q[1]; verts[3 * (size_t)id + 2] = q[2];
        emap[3 * (size_t)n + a] = (int)id;
        ++id;
    }
}

// (F) triangles by cell index, then table order; vertex ids through the edge map of the node that owns each edge
__global__ __launch_bounds__(256) void k_mc_tris(McGeom G, const uint8_t* __restrict__ cellcase, const uint8_t* __restrict__ ntri,
                                                 const int8_t* __restrict__ table, const unsigned* __restrict__ boff, const int* __restrict__ emap,
                                                 int* __restrict__ tris)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    unsigned code = 0, cnt = 0;
    if (n < G.nn) { code = cellcase[n]; cnt = ntri[code]; }
    unsigned total;
    const unsigned excl = block_scan(cnt, &total) - cnt;
    if (!cnt) return;
    const size_t first = (size_t)boff[blockIdx.x] + excl, sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
    for (unsigned t = 0; t < 3 * cnt; ++t) {
        const int e = table[code * MC_ROW + t], a = e >> 2, b0 = e & 1, b1 = (e >> 1) & 1;
        const size_t node = (size_t)n + (a == 0 ? b0 * sy + b1 * sz : a == 1 ? b0 + b1 * sz : b0 + b1 * sy);
        tris[3 * first + t] = emap[3 * node + a];
    }
}

// device-wide exclusive scan in three kinds of launches (workgroup scans -> scan of the workgroup sums -> add): no workgroup waits on another
__global__ __launch_bounds__(256) void k_mc_scan_block(unsigned* __restrict__ d, int n, unsigned* __restrict__ sums)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    unsigned total;
    const unsigned v = q < n ? d[q] : 0u, excl = block_scan(v, &total) - v;
    if (q < n) d[q] = excl;
    if (sums && threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void k_mc_scan_add(unsigned* __restrict__ d, int n, const unsigned* __restrict__ sums)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) d[q] += sums[blockIdx.x];
}

// ---- lattice evaluation at the nodes a mask keeps (nsk_eval_lattice_masked) -----------------------------------------------
// The set nodes (any non-zero byte) go into an ascending list of node indices, the decoders run on that list, the rest receives `fill`.
// Count per workgroup -> mc_scan over the counts -> rank inside the workgroup: the list's order does not depend on scheduling.
__global__ __launch_bounds__(256) void k_lattice_flags(int nn, const uint8_t* __restrict__ valid, unsigned* __restrict__ bsum)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    unsigned total;
    block_scan(n < nn && valid[n] != 0 ? 1u : 0u, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// recomputes the flags; set node: idx[rank] = n (rank < n_set by construction: the guard only matters when the caller's mask changed
// between the two passes); unset node: the volume receives the bits of `fill` here, so no later pass visits it
__global__ __launch_bounds__(256) void k_lattice_compact(int nn, const uint8_t* __restrict__ valid, const unsigned* __restrict__ boff, unsigned n_set,
                                                         unsigned fill_bits, unsigned* __restrict__ idx, unsigned* __restrict__ vol_bits)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool live = n < nn, set = live && valid[n] != 0;
    unsigned total;
    const unsigned one = set ? 1u : 0u, rank = boff[blockIdx.x] + (block_scan(one, &total) - one);
    if (set) { if (rank < n_set) idx[rank] = (unsigned)n; }
    else if (live) vol_bits[n] = fill_bits;
}
// k_lattice_points for the listed nodes idx[0 .. cnt): the same products and sums, so the same bits
__global__ __launch_bounds__(256) void k_lattice_points_idx(McGeom G, const unsigned* __restrict__ idx, int cnt, float* __restrict__ pts)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= cnt) return;
    const int n = (int)idx[m], r = n / G.nx;
    const int i = n % G.nx, j = r % G.ny, k = r / G.ny;
    pts[3 * (size_t)m] = mc_coord(G.o[0], i, G.s[0]);
    pts[3 * (size_t)m + 1] = mc_coord(G.o[1], j, G.s[1]);
    pts[3 * (size_t)m + 2] = mc_coord(G.o[2], k, G.s[2]);
}
// k_lattice_finish scattered to the listed nodes (ascending indices: near-coalesced runs)
__global__ __launch_bounds__(256) void k_lattice_finish_idx(int cnt, const float* __restrict__ pts, const float* __restrict__ bound6,
                                                            const float* __restrict__ occ_a, const float* __restrict__ occ_b,
                                                            const unsigned* __restrict__ idx, float* __restrict__ vol)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= cnt) return;
    const float px = pts[3 * (size_t)m], py = pts[3 * (size_t)m + 1], pz = pts[3 * (size_t)m + 2];
    const bool inb = px < bound6[1] && px > bound6[0] && py < bound6[3] && py > bound6[2] && pz < bound6[5] && pz > bound6[4];
    float occ = occ_a[m];
    if (occ_b) occ = occ_b[m] + occ;
    vol[idx[m]] = inb ? occ : 100.f;
}

// ---- seen mask of a lattice (nsk_lattice_seen) -------------------------------------------------------------------------
// One thread per node, x fastest.  A node is seen by keyframe k when it lies in front of the camera (which looks along -z), projects onto
// a pixel at least `edge` pixels inside the image, that pixel carries a finite positive depth D, and the node is no farther than
// D + trunc: the rule of nsk_view.h, with reach = trunc.
__global__ __launch_bounds__(256) void k_lattice_seen(McGeom G, ViewArgs A, const float* __restrict__ depth, uint8_t* __restrict__ valid,
                                                      unsigned long long* __restrict__ count)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool live = n < G.nn;
    bool seen = false;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        lattice_node(G, n, p);
        seen = A.accumulate && valid[n] != 0;
    }
    for (int kf = 0; kf < A.K; ++kf) {
        if (__all(seen || !live)) break;                    // the whole wave is done
        if (seen || !live) continue;
        float d, fi, fj;
        if (!view_project(A, A.w[kf], p, d, fi, fj)) continue;
        const float D = view_pixel(A, depth, kf, fi, fj);
        if (!view_measured(D)) continue;
        seen = d <= __fadd_rn(D, A.reach);
    }
    if (live) valid[n] = seen ? 1 : 0;
    if (count) wave_count(live && seen, count);
}

// ---- connected components of the extracted mesh (nsk_mesh_filter) ----------------------------------------------------------
// Union-find over the vertices: a root is only ever hooked below a SMALLER index (compare-and-swap on the root's own slot), so the links
// never form a cycle and a component's final root is its smallest vertex index whatever order the hooks ran in.  find() halves the path it
// walks; the halving stores race with other walkers, but every value ever stored in a slot is an ancestor of that vertex.
__device__ __forceinline__ int cc_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ int cc_find(int* __restrict__ parent, int x)
{
    for (;;) {
        const int q = cc_load(parent + x);
        if (q == x) return x;
        const int g = cc_load(parent + q);
        if (g != q) __atomic_store_n(parent + x, g, __ATOMIC_RELAXED);
        x = g;
    }
}
__device__ __forceinline__ void cc_union(int* __restrict__ parent, int a, int b)
{
    for (;;) {
        a = cc_find(parent, a); b = cc_find(parent, b);
        if (a == b) return;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;  // hi was still a root: hooked.  Otherwise somebody hooked it first: walk on
    }
}

__global__ __launch_bounds__(256) void k_cc_init(int nv, int* __restrict__ parent, double* __restrict__ area, uint8_t* __restrict__ used)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nv) { parent[v] = v; area[v] = 0.0; used[v] = 0; }
}
__global__ __launch_bounds__(256) void k_cc_hook(int nt, const int* __restrict__ tris, int* __restrict__ parent, uint8_t* __restrict__ used)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    used[a] = 1; used[b] = 1; used[c] = 1;
    cc_union(parent, a, b);
    cc_union(parent, a, c);
}
// (after every hook has landed) each vertex points at its root
__global__ __launch_bounds__(256) void k_cc_flatten(int nv, int* __restrict__ parent)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int r = v;
    for (int q = cc_load(parent + r); q != r; q = cc_load(parent + r)) r = q;
    __atomic_store_n(parent + v, r, __ATOMIC_RELAXED);
}
// triangle areas 0.5 |(v1 - v0) x (v2 - v0)| in fp32, summed per component in fp64.  A workgroup walks CC_AREA_ITERS * 256 consecutive
// triangles; while the triangles of a wave stay in one component (the usual case: triangles are ordered by cell) every lane sums in a
// register, and the wave adds once when the component changes or the walk ends; a wave that holds several components adds once per
// component -- a component of millions of triangles receives some thousand atomic adds on its one address, not one per triangle
#define CC_AREA_ITERS 32
__device__ __forceinline__ void cc_area_flush(double* __restrict__ area, int run, double acc)
{
    if (run < 0) return;                                    // (wave-uniform)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(area + run, acc);
}
__global__ __launch_bounds__(256) void k_cc_area(int nt, const int* __restrict__ tris, const float* __restrict__ verts, const int* __restrict__ label,
                                                 double* __restrict__ area)
{
    int run = -1;                                           // the component the wave is summing for (wave-uniform), -1: none
    double acc = 0.0;
    for (int it = 0; it < CC_AREA_ITERS; ++it) {
        const long long tl = ((long long)blockIdx.x * CC_AREA_ITERS + it) * 256 + threadIdx.x;
        const bool live = tl < nt;
        const int t = (int)tl;
        int l = -1;
        double a = 0.0;
        if (live) {
            const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
            l = label[i0];
            float e[3], f[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float v0 = verts[3 * (size_t)i0 + q];
                e[q] = __fsub_rn(verts[3 * (size_t)i1 + q], v0); f[q] = __fsub_rn(verts[3 * (size_t)i2 + q], v0);
            }
            const float x = __fsub_rn(mul_rn(e[1], f[2]), mul_rn(e[2], f[1])), y = __fsub_rn(mul_rn(e[2], f[0]), mul_rn(e[0], f[2])),
                        z = __fsub_rn(mul_rn(e[0], f[1]), mul_rn(e[1], f[0]));
            a = (double)mul_rn(0.5f, __fsqrt_rn(__fadd_rn(__fadd_rn(mul_rn(x, x), mul_rn(y, y)), mul_rn(z, z))));
        }
        const int first = __ffsll((unsigned long long)__ballot(live)) - 1;
        if (first < 0) break;                               // (wave-uniform: nothing left for this wave)
        const int l0 = __shfl(l, first, 64);
        if (__all(!live || l == l0)) {
            if (l0 != run) { cc_area_flush(area, run, acc); run = l0; acc = 0.0; }
            acc += a;
        } else {
            // several components in one wave (a small one between the triangles of a large one): one add per component, not per lane
            cc_area_flush(area, run, acc); run = -1; acc = 0.0;
            unsigned long long pend = __ballot(live);
            while (pend) {                                  // (wave-uniform)
                const int lc = __shfl(l, __ffsll(pend) - 1, 64);
                const bool mine = live && l == lc;
                cc_area_flush(area, lc, mine ? a : 0.0);
                pend &= ~(unsigned long long)__ballot(mine);
            }
        }
    }
    cc_area_flush(area, run, acc);
}
struct CcStats { unsigned long long best; int best_label; unsigned n_components, n_kept; };     // best: bits of the largest area (non-negative doubles order like their bits)
// per root with a triangle: one component.  largest_only: the largest area; else keep = area > min_area
__global__ __launch_bounds__(256) void k_cc_roots(int nv, const int* __restrict__ label, const uint8_t* __restrict__ used, const double* __restrict__ area,
                                                  double min_area, int largest_only, uint8_t* __restrict__ keepc, CcStats* __restrict__ S)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    keepc[v] = 0;
    if (label[v] != v || !used[v]) return;
    atomicAdd(&S->n_components, 1u);
    if (largest_only) { atomicMax(&S->best, (unsigned long long)__double_as_longlong(area[v])); return; }
    if (area[v] > min_area) { keepc[v] = 1; atomicAdd(&S->n_kept, 1u); }
}
// largest_only: ties go to the smaller label
__global__ __launch_bounds__(256) void k_cc_pick(int nv, const int* __restrict__ label, const uint8_t* __restrict__ used, const double* __restrict__ area,
                                                 CcStats* __restrict__ S)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || label[v] != v || !used[v]) return;
    if ((unsigned long long)__double_as_longlong(area[v]) == S->best) atomicMin(&S->best_label, v);
}
__global__ __launch_bounds__(256) void k_cc_pick_done(uint8_t* __restrict__ keepc, CcStats* __restrict__ S)
{
    if (S->best_label != 0x7fffffff) { keepc[S->best_label] = 1; S->n_kept = 1; }
}
// 0 / 1 per vertex and per triangle for the scans (a triangle goes where its component goes; a vertex without a triangle goes nowhere)
__global__ __launch_bounds__(256) void k_cc_flags(int nv, int nt, const int* __restrict__ tris, const int* __restrict__ label, const uint8_t* __restrict__ used,
                                                  const uint8_t* __restrict__ keepc, unsigned* __restrict__ vflag, unsigned* __restrict__ tflag)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < nv) vflag[q] = used[q] && keepc[label[q]] ? 1u : 0u;
    if (q < nt) tflag[q] = keepc[label[tris[3 * (size_t)q]]] ? 1u : 0u;
}
// voff / toff: the exclusive scans of the flags, one slot more than elements (the last is the total).  vsrc (or NULL): the source index of
// every vertex kept.  nsk_mesh_filter's flags come from k_cc_flags, nsk_mesh_select's (nsk_cull.h) from k_select_flags
__global__ __launch_bounds__(256) void k_mesh_compact(int nv, int nt, const float* __restrict__ verts, const int* __restrict__ tris,
                                                      const unsigned* __restrict__ voff, const unsigned* __restrict__ toff,
                                                      float* __restrict__ verts2, int* __restrict__ tris2, int* __restrict__ vsrc)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q < nv) {
        const unsigned d = voff[q];
        if (voff[q + 1] != d) {
            for (int a = 0; a < 3; ++a) verts2[3 * (size_t)d + a] = verts[3 * (size_t)q + a];
            if (vsrc) vsrc[d] = (int)q;
        }
    }
    if (q < nt) {
        const unsigned d = toff[q];
        if (toff[q + 1] != d)                               // (a kept triangle: its indices are in range)
            for (int a = 0; a < 3; ++a) tris2[3 * (size_t)d + a] = (int)voff[tris[3 * (size_t)q + a]];
    }
}

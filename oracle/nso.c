/*
 * oracle/nso.c -- CPU restatement of the nice-slam-cpp render / map / track hot path.
 *
 * THIS FILE IS TEST INFRASTRUCTURE.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load it.  The product path (nice-slam-cpp_amd/csrc)
 * never links, includes or calls anything in oracle/.
 *
 * PARITY STATUS: "parity unpinned" for every row except A6.  The reference holds no tests,
 * golden vectors or fixtures and does not build in this image (Eigen,
 * OpenCV, yaml-cpp and the traced TorchScript decoders are absent), so the
 * only reference source that compiles here is src/models/GaussianFFT.cpp (oracle/_ref,
 * which pins A6).  Everything else in this file is cross-checked against an independent
 * restatement built from the very ATen ops the reference calls (oracle/torch_ref.py:
 * F.grid_sample, F.linear, torch.sort, torch.cumprod, autograd, torch.optim.Adam) and
 * against the golden vectors that restatement produced (tests/golden/).
 *
 * Where the reference source as written cannot execute or makes training a no-op the
 * *intended* semantics are implemented (SURVEY.md section 0.3 defect ledger D6,D7,D12-D16).
 * Each function cites the reference file:line it restates.
 *
 * Precision: compiled twice, REAL=float (libnso_f32.so, mirrors the reference's fp32
 * arithmetic) and REAL=double (libnso_f64.so, used to judge which fp32 result is closer).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#ifndef REAL
#define REAL float
#endif
typedef REAL real;

#define NSO_API __attribute__((visibility("default")))

#define E_DIM 93   /* src/models/MLP.cpp:21 embedding_size */
#define H_DIM 32   /* src/main.cpp:29 hidden_size */
#define MAX_S 64

static inline real r_sin(real x) { return sizeof(real) == 4 ? (real)sinf((float)x) : (real)sin((double)x); }
static inline real r_cos(real x) { return sizeof(real) == 4 ? (real)cosf((float)x) : (real)cos((double)x); }
static inline real r_exp(real x) { return sizeof(real) == 4 ? (real)expf((float)x) : (real)exp((double)x); }
static inline real r_sqrt(real x) { return sizeof(real) == 4 ? (real)sqrtf((float)x) : (real)sqrt((double)x); }
static inline real r_floor(real x) { return sizeof(real) == 4 ? (real)floorf((float)x) : (real)floor((double)x); }
/* torch::matmul on the CPU (MKL sgemm) accumulates a dot product with fused multiply-adds in k order: measured here for the K = 3 product of
 * GaussianFFT (tests/test_oracle.py::test_aten_matmul_k3_is_an_fma_chain: bit-equal on 100 % of 4.6 M elements; the unfused form on 65 %) */
static inline real r_fma(real a, real b, real c) { return sizeof(real) == 4 ? (real)fmaf((float)a, (float)b, (float)c) : (real)fma((double)a, (double)b, (double)c); }
static inline real r_abs(real x) { return x < 0 ? -x : x; }

/* ------------------------------------------------------------------------------------------
 * Decoder parameter packing (one flat array per decoder, torch::nn::Linear row-major [out,in]):
 *   MLP        (middle, fine, color; src/models/MLP.cpp:3-49):
 *       B[3][93], pts_linear[0..4].{w,b}, fc[0..4].{w,b}, output_linear.{w,b}
 *       pts_linear in-dims 93,32,32,125,32 (:24-41; input of [3] is cat(embedded,h) :96)
 *       fc in-dim = c_dim (32, fine: 64) (:14-20); output 32->1, color 32->4 (:43-46)
 *   MLP_no_xyz (coarse; src/models/MLP.cpp:104-138):
 *       pts_linear[0..4].{w,b} in-dims 32,32,32,64,32 (input of [3] is cat(c,h) :176), output.{w,b}
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int has_xyz, c_dim, out_dim;
    int in_dim[5];
    size_t oB, oW[5], ob[5], oFw[5], oFb[5], oWo, obo, total;
} dec_layout;

static void make_layout(int which, dec_layout* L)
{
    memset(L, 0, sizeof(*L));
    L->has_xyz = which != 0;
    L->c_dim = which == 2 ? 64 : 32;     /* src/models/NICE.cpp:4-7 (fine: c_dim*2) */
    L->out_dim = which == 3 ? 4 : 1;
    size_t o = 0;
    if (L->has_xyz) {
        int d[5] = { E_DIM, H_DIM, H_DIM, H_DIM + E_DIM, H_DIM };
        memcpy(L->in_dim, d, sizeof(d));
        L->oB = o; o += 3 * E_DIM;
    } else {
        int d[5] = { 32, H_DIM, H_DIM, H_DIM + 32, H_DIM };
        memcpy(L->in_dim, d, sizeof(d));
    }
    for (int i = 0; i < 5; ++i) { L->oW[i] = o; o += (size_t)H_DIM * L->in_dim[i]; L->ob[i] = o; o += H_DIM; }
    if (L->has_xyz)
        for (int i = 0; i < 5; ++i) { L->oFw[i] = o; o += (size_t)H_DIM * L->c_dim; L->oFb[i] = o; o += H_DIM; }
    L->oWo = o; o += (size_t)L->out_dim * H_DIM; L->obo = o; o += L->out_dim;
    L->total = o;
}

NSO_API int nso_real_size(void) { return (int)sizeof(real); }

NSO_API long nso_decoder_param_count(int which)
{
    dec_layout L; make_layout(which, &L); return (long)L.total;
}

/* ------------------------------------------------------------------------------------------ */
typedef struct {
    real bound[6];          /* [[x0,x1],[y0,y1],[z0,z1]]  src/Renderer.cpp:15 */
    int n_samples;          /* src/Renderer.cpp:9  */
    int n_surface;          /* src/Renderer.cpp:10 */
    int lindisp;            /* :7  */
    real perturb;           /* :8  */
    int occupancy;          /* :125 passes literal false (D9); 1 = alpha=sigmoid(10 sigma) */
    uint64_t seed;
} nso_opts;

typedef struct {
    int C, Z, Y, X;
    const real* v;          /* [C][Z][Y][X], the reference's [1,C,Z,Y,X] (src/main.cpp:39-44) */
} nso_grid;

/* counter-based uniform in [0,1) for the optional stratified perturbation (Renderer.cpp:115).
 * torch::rand's stream cannot be matched, so perturb>0 is "parity unpinned"; the HIP path uses
 * the same hash so that oracle and product agree with each other. */
static inline uint32_t hash_u32(uint64_t seed, uint32_t a, uint32_t b)
{
    uint64_t x = seed ^ (0x9E3779B97F4A7C15ull * ((uint64_t)a + 1)) ^ (0xC2B2AE3D27D4EB4Full * ((uint64_t)b + 1));
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return (uint32_t)(x >> 32);
}
static inline real hash_unit(uint64_t seed, uint32_t a, uint32_t b)
{
    return (real)(hash_u32(seed, a, b) >> 8) * (real)(1.0 / 16777216.0);
}

/* at::linspace (CPU kernel): step=(end-start)/(steps-1); first half start+i*step, second half
 * end-(steps-1-i)*step.  Used at src/Renderer.cpp:86,101. */
static inline real linspace01(int i, int steps)
{
    if (steps == 1) return 0;
    real step = (real)1 / (real)(steps - 1);
    return i < steps / 2 ? step * (real)i : (real)1 - step * (real)(steps - 1 - i);
}

/* src/Renderer.cpp:66-73 and src/Mapper.cpp:417-421, src/Tracker.cpp:49-53:
 * t = min_axis max_side (bound - o)/d   (detached, D6/D7) */
static real ray_box_far(const real* bound, const real* o, const real* d)
{
    real far = 0;
    for (int k = 0; k < 3; ++k) {
        real t0 = (bound[2 * k] - o[k]) / d[k];
        real t1 = (bound[2 * k + 1] - o[k]) / d[k];
        real m = t0 > t1 ? t0 : t1;
        if (k == 0 || m < far) far = m;
    }
    return far;
}

/* The inside-bbox pre-filter (src/Mapper.cpp:416-427, src/Tracker.cpp:48-58): t >= gt_depth with ATen's max / min, which hand a NaN on.
 * A NaN in any of the six quotients (0/0: an origin on a bound plane with no direction component across it) drops the ray, whichever
 * plane or axis it is; without one the comparisons are ATen's max and min.  ray_box_far above, what the sampling calls, keeps its text. */
static int ray_inside(const real* bound, const real* o, const real* d, real gt)
{
    real far = 0;
    int nan = 0;
    for (int k = 0; k < 3; ++k) {
        real t0 = (bound[2 * k] - o[k]) / d[k];
        real t1 = (bound[2 * k + 1] - o[k]) / d[k];
        nan = nan || t0 != t0 || t1 != t1;
        real m = t0 > t1 ? t0 : t1;
        if (k == 0 || m < far) far = m;
    }
    return !nan && far >= gt;
}

/* src/Renderer.cpp:44-119: z values of one ray, sorted ascending.  Returns S. */
static int ray_z_vals(const nso_opts* o, int n, const real* ro, const real* rd, int has_gt, real gt,
                      real gt_max, real* z)
{
    const int ns = o->n_samples;
    const int nsurf = has_gt ? o->n_surface : 0;            /* :54-57, D8 */
    real near = has_gt ? gt * (real)0.01 : (real)0.01;      /* :57,:63 */
    real far = ray_box_far(o->bound, ro, rd) + (real)0.01;  /* :69-73 */
    if (has_gt) {                                           /* :76 clamp(far_bb, 0, max(gt*1.2)) */
        real hi = gt_max * (real)1.2;
        if (far < 0) far = 0;
        if (far > hi) far = hi;
    }
    for (int j = 0; j < ns; ++j) {                          /* :101-108 */
        real t = linspace01(j, ns);
        if (!o->lindisp) z[j] = near * ((real)1 - t) + far * t;
        else z[j] = (real)1 / ((real)1 / near * ((real)1 - t) + (real)1 / far * t);
    }
    if (o->perturb > 0) {                                   /* :110-117 */
        real lo[MAX_S], up[MAX_S];
        for (int j = 0; j < ns; ++j) {
            lo[j] = j == 0 ? z[0] : (real)0.5 * (z[j] + z[j - 1]);
            up[j] = j == ns - 1 ? z[ns - 1] : (real)0.5 * (z[j + 1] + z[j]);
        }
        for (int j = 0; j < ns; ++j) z[j] = lo[j] + (up[j] - lo[j]) * hash_unit(o->seed, (uint32_t)n, (uint32_t)j);
    }
    for (int j = 0; j < nsurf; ++j) {                       /* :80-99 */
        real t = linspace01(j, nsurf);
        if (gt > 0) z[ns + j] = (real)0.95 * gt * ((real)1 - t) + (real)1.05 * gt * t;
        else z[ns + j] = (real)0.001 * ((real)1 - t) + gt_max * t;
    }
    int S = ns + nsurf;
    if (nsurf > 0) {                                        /* :119 sort(cat) -- insertion sort */
        for (int i = 1; i < S; ++i) {
            real v = z[i]; int j = i - 1;
            while (j >= 0 && z[j] > v) { z[j + 1] = z[j]; --j; }
            z[j + 1] = v;
        }
    }
    return S;
}

/* ------------------------------------------------------------------------------------------
 * Trilinear lookup = F::grid_sample(mode bilinear, padding border, align_corners=true) at
 * src/models/MLP.cpp:51-63,140-152 with normalize_3d_coordinate include/torchlib/utils.h:132-139
 * (intended form, D12/D13).  Semantics follow ATen/native/GridSampler.h:27-83 (unnormalize :31,
 * clip :58-60, clip gradient zero at/over the border :66-83).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int i0[3];       /* floor index along x,y,z */
    real t[3];       /* fractional part */
    real gmul[3];    /* d(index)/d(world coord), 0 when clipped */
} tri_coord;

static void tri_setup(const nso_grid* g, const real* bound, const real* p, tri_coord* tc)
{
    const int dims[3] = { g->X, g->Y, g->Z };
    for (int k = 0; k < 3; ++k) {
        real lo = bound[2 * k], hi = bound[2 * k + 1];
        real u = ((p[k] - lo) / (hi - lo)) * (real)2 - (real)1;          /* utils.h:135-137 */
        real x = ((u + (real)1) / (real)2) * (real)(dims[k] - 1);      /* GridSampler.h:31 */
        real mul = (real)(dims[k] - 1) / (real)2 * ((real)2 / (hi - lo));
        real mx = (real)(dims[k] - 1);
        if (x <= 0) { x = 0; mul = 0; }                                  /* :66-83 */
        else if (x >= mx) { x = mx; mul = 0; }
        real f = r_floor(x);
        tc->i0[k] = (int)f; tc->t[k] = x - f; tc->gmul[k] = mul;
    }
}

static inline int tri_inb(const nso_grid* g, int ix, int iy, int iz)
{
    return ix >= 0 && ix < g->X && iy >= 0 && iy < g->Y && iz >= 0 && iz < g->Z;
}

static void tri_sample(const nso_grid* g, const tri_coord* tc, real* feat /* [C] */)
{
    const size_t cs = (size_t)g->Z * g->Y * g->X;
    for (int c = 0; c < g->C; ++c) feat[c] = 0;
    for (int dz = 0; dz < 2; ++dz) for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx) {
        int ix = tc->i0[0] + dx, iy = tc->i0[1] + dy, iz = tc->i0[2] + dz;
        if (!tri_inb(g, ix, iy, iz)) continue;
        real w = (dx ? tc->t[0] : (real)1 - tc->t[0]) * (dy ? tc->t[1] : (real)1 - tc->t[1]) *
                 (dz ? tc->t[2] : (real)1 - tc->t[2]);
        size_t off = ((size_t)iz * g->Y + iy) * g->X + ix;
        for (int c = 0; c < g->C; ++c) feat[c] += w * g->v[c * cs + off];
    }
}

/* backward: scatter g_feat into g_grid (same layout as grid) and/or accumulate g_p[3].
 * r_grid (optional, [Z][Y][X]): += w(sample, voxel) * max_c |g_feat[c]|, the scale of what any fp32 evaluation of the sum
 * g_grid[v][c] = sum_samples w g_feat[c] may lose at voxel v (see nso_render_backward_scaled) */
static void tri_backward(const nso_grid* g, const tri_coord* tc, const real* g_feat, real* g_grid, real* g_p, real* r_grid)
{
    const size_t cs = (size_t)g->Z * g->Y * g->X;
    real gi[3] = { 0, 0, 0 };
    real gmax = 0;
    if (r_grid) for (int c = 0; c < g->C; ++c) if (r_abs(g_feat[c]) > gmax) gmax = r_abs(g_feat[c]);
    for (int dz = 0; dz < 2; ++dz) for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx) {
        int ix = tc->i0[0] + dx, iy = tc->i0[1] + dy, iz = tc->i0[2] + dz;
        if (!tri_inb(g, ix, iy, iz)) continue;
        real wx = dx ? tc->t[0] : (real)1 - tc->t[0];
        real wy = dy ? tc->t[1] : (real)1 - tc->t[1];
        real wz = dz ? tc->t[2] : (real)1 - tc->t[2];
        size_t off = ((size_t)iz * g->Y + iy) * g->X + ix;
        real dot = 0;
        if (r_grid) r_grid[off] += wx * wy * wz * gmax;
        for (int c = 0; c < g->C; ++c) {
            if (g_grid) g_grid[c * cs + off] += wx * wy * wz * g_feat[c];
            dot += g->v[c * cs + off] * g_feat[c];
        }
        gi[0] += (dx ? dot : -dot) * wy * wz;
        gi[1] += (dy ? dot : -dot) * wx * wz;
        gi[2] += (dz ? dot : -dot) * wx * wy;
    }
    if (g_p) for (int k = 0; k < 3; ++k) g_p[k] += gi[k] * tc->gmul[k];
}

/* ------------------------------------------------------------------------------------------
 * Decoders (intended loops, D14/D15):
 *   MLP::forward        src/models/MLP.cpp:76-102   GaussianFFT::forward src/models/GaussianFFT.cpp:10-15
 *   MLP_no_xyz::forward src/models/MLP.cpp:165-182
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    real e[E_DIM], ce[E_DIM];     /* sin(pB), cos(pB) */
    real c[64];
    real a[5][H_DIM];             /* pre-activation W_i x + b_i */
    unsigned char on[5][H_DIM];   /* a > 0: the branch torch::relu's backward takes (MLP.cpp:92,98); tests may force it */
    real h[5][H_DIM];             /* block output */
    real out[4];
} dec_act;

static void dec_forward(const dec_layout* L, const real* P, const real* p, dec_act* A)
{
    real x[E_DIM + H_DIM + 32];
    int nx;
    if (L->has_xyz) {
        const real* B = P + L->oB;
        for (int k = 0; k < E_DIM; ++k) {
            real s = r_fma(p[2], B[2 * E_DIM + k], r_fma(p[1], B[E_DIM + k], p[0] * B[k]));   /* GaussianFFT.cpp:13 matmul, see r_fma */
            A->e[k] = r_sin(s); A->ce[k] = r_cos(s);
            x[k] = A->e[k];
        }
        nx = E_DIM;
    } else {
        for (int k = 0; k < 32; ++k) x[k] = A->c[k];
        nx = 32;
    }
    for (int i = 0; i < 5; ++i) {
        const real* W = P + L->oW[i]; const real* b = P + L->ob[i];
        for (int o = 0; o < H_DIM; ++o) {
            real s = b[o];
            for (int k = 0; k < nx; ++k) s += W[(size_t)o * nx + k] * x[k];
            A->a[i][o] = s;
            A->on[i][o] = s > 0;
            real h = s > 0 ? s : 0;
            if (L->has_xyz) {
                const real* Fw = P + L->oFw[i]; const real* Fb = P + L->oFb[i];
                real f = Fb[o];
                for (int k = 0; k < L->c_dim; ++k) f += Fw[(size_t)o * L->c_dim + k] * A->c[k];
                h += f;
            }
            A->h[i][o] = h;
        }
        if (i == 2) {                       /* skips={2}: cat(embedded|c, h) */
            int pre = L->has_xyz ? E_DIM : 32;
            for (int k = 0; k < pre; ++k) x[k] = L->has_xyz ? A->e[k] : A->c[k];
            for (int k = 0; k < H_DIM; ++k) x[pre + k] = A->h[i][k];
            nx = pre + H_DIM;
        } else {
            for (int k = 0; k < H_DIM; ++k) x[k] = A->h[i][k];
            nx = H_DIM;
        }
    }
    const real* Wo = P + L->oWo; const real* bo = P + L->obo;
    for (int o = 0; o < L->out_dim; ++o) {
        real s = bo[o];
        for (int k = 0; k < H_DIM; ++k) s += Wo[o * H_DIM + k] * A->h[4][k];
        A->out[o] = s;
    }
}

/* backward of one decoder at one point.  g_out[out_dim] upstream.  Accumulates:
 *   gP (decoder parameter gradient, may be NULL), g_c[c_dim] (feature gradient, overwritten),
 *   g_p[3] (through the embedding only, accumulated, may be NULL). */
static void dec_backward(const dec_layout* L, const real* P, const real* p, const dec_act* A,
                         const real* g_out, real* gP, real* g_c, real* g_p, real* rP)
{
    real g_h[H_DIM], g_e[E_DIM];
    for (int k = 0; k < 64; ++k) g_c[k] = 0;
    for (int k = 0; k < E_DIM; ++k) g_e[k] = 0;
    const real* Wo = P + L->oWo;
    for (int k = 0; k < H_DIM; ++k) {
        real s = 0;
        for (int o = 0; o < L->out_dim; ++o) s += Wo[o * H_DIM + k] * g_out[o];
        g_h[k] = s;
    }
    if (gP) for (int o = 0; o < L->out_dim; ++o) {
        for (int k = 0; k < H_DIM; ++k) gP[L->oWo + o * H_DIM + k] += g_out[o] * A->h[4][k];
        gP[L->obo + o] += g_out[o];
    }
    if (rP) for (int o = 0; o < L->out_dim; ++o) {     /* rP: the same sums over |factor| |factor|, the running-error scale of each parameter's gradient */
        for (int k = 0; k < H_DIM; ++k) rP[L->oWo + o * H_DIM + k] += r_abs(g_out[o] * A->h[4][k]);
        rP[L->obo + o] += r_abs(g_out[o]);
    }
    for (int i = 4; i >= 0; --i) {
        const int nx = L->in_dim[i];
        const int pre = nx - H_DIM;         /* skip prefix length for i==3, else nx==H_DIM or first layer */
        real x[E_DIM + H_DIM + 32];
        if (i == 0) { for (int k = 0; k < nx; ++k) x[k] = L->has_xyz ? A->e[k] : A->c[k]; }
        else if (i == 3) {
            for (int k = 0; k < pre; ++k) x[k] = L->has_xyz ? A->e[k] : A->c[k];
            for (int k = 0; k < H_DIM; ++k) x[pre + k] = A->h[2][k];
        } else { for (int k = 0; k < H_DIM; ++k) x[k] = A->h[i - 1][k]; }
        real g_a[H_DIM];
        for (int o = 0; o < H_DIM; ++o) g_a[o] = A->on[i][o] ? g_h[o] : 0;
        if (L->has_xyz) {
            const real* Fw = P + L->oFw[i];
            for (int k = 0; k < L->c_dim; ++k) {
                real s = 0;
                for (int o = 0; o < H_DIM; ++o) s += Fw[(size_t)o * L->c_dim + k] * g_h[o];
                g_c[k] += s;
            }
            if (gP) for (int o = 0; o < H_DIM; ++o) {
                for (int k = 0; k < L->c_dim; ++k) gP[L->oFw[i] + (size_t)o * L->c_dim + k] += g_h[o] * A->c[k];
                gP[L->oFb[i] + o] += g_h[o];
            }
            if (rP) for (int o = 0; o < H_DIM; ++o) {
                for (int k = 0; k < L->c_dim; ++k) rP[L->oFw[i] + (size_t)o * L->c_dim + k] += r_abs(g_h[o] * A->c[k]);
                rP[L->oFb[i] + o] += r_abs(g_h[o]);
            }
        }
        if (gP) for (int o = 0; o < H_DIM; ++o) {
            for (int k = 0; k < nx; ++k) gP[L->oW[i] + (size_t)o * nx + k] += g_a[o] * x[k];
            gP[L->ob[i] + o] += g_a[o];
        }
        if (rP) for (int o = 0; o < H_DIM; ++o) {
            for (int k = 0; k < nx; ++k) rP[L->oW[i] + (size_t)o * nx + k] += r_abs(g_a[o] * x[k]);
            rP[L->ob[i] + o] += r_abs(g_a[o]);
        }
        const real* W = P + L->oW[i];
        real g_x[E_DIM + H_DIM + 32];
        for (int k = 0; k < nx; ++k) {
            real s = 0;
            for (int o = 0; o < H_DIM; ++o) s += W[(size_t)o * nx + k] * g_a[o];
            g_x[k] = s;
        }
        if (i == 0) {
            if (L->has_xyz) for (int k = 0; k < E_DIM; ++k) g_e[k] += g_x[k];
            else for (int k = 0; k < 32; ++k) g_c[k] += g_x[k];
        } else if (i == 3) {
            if (L->has_xyz) for (int k = 0; k < E_DIM; ++k) g_e[k] += g_x[k];
            else for (int k = 0; k < 32; ++k) g_c[k] += g_x[k];
            for (int k = 0; k < H_DIM; ++k) g_h[k] = g_x[pre + k];
        } else {
            for (int k = 0; k < H_DIM; ++k) g_h[k] = g_x[k];
        }
    }
    if (L->has_xyz) {
        const real* B = P + L->oB;
        for (int k = 0; k < E_DIM; ++k) {
            real gs = g_e[k] * A->ce[k];
            if (gP) for (int a = 0; a < 3; ++a) gP[L->oB + a * E_DIM + k] += p[a] * gs;
            if (rP) for (int a = 0; a < 3; ++a) rP[L->oB + a * E_DIM + k] += r_abs(p[a] * gs);
            if (g_p) for (int a = 0; a < 3; ++a) g_p[a] += gs * B[a * E_DIM + k];
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * NICE::forward stage composition (src/models/NICE.cpp:16-52) + Renderer::eval_points
 * (src/Renderer.cpp:19-42: strict in-bound mask, raw[~mask,3]=100).
 * stage: 0 coarse, 1 middle, 2 fine (fine+middle), 3 color (rgb=color, occ=fine+middle)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int inb;
    tri_coord tc[4];
    dec_act act[4];
    real raw[4];
} pt_state;

static const int STAGE_DECODERS[4][3] = { { 0, -1, -1 }, { 1, -1, -1 }, { 1, 2, -1 }, { 1, 2, 3 } };

static void point_forward(const nso_opts* o, const nso_grid* grids, const real* const* P, const dec_layout* L,
                          int stage, const real* p, pt_state* st)
{
    st->inb = p[0] < o->bound[1] && p[0] > o->bound[0] && p[1] < o->bound[3] && p[1] > o->bound[2] &&
              p[2] < o->bound[5] && p[2] > o->bound[4];                 /* Renderer.cpp:26-29 */
    real occ = 0;
    st->raw[0] = st->raw[1] = st->raw[2] = 0;                           /* NICE.cpp:22,30,37 */
    for (int q = 0; q < 3; ++q) {
        int w = STAGE_DECODERS[stage][q];
        if (w < 0) break;
        tri_setup(&grids[w], o->bound, p, &st->tc[w]);
        tri_sample(&grids[w], &st->tc[w], st->act[w].c);
        if (w == 2) {                                                   /* MLP.cpp:79-84 concat_feat (no grad) */
            tri_coord tcm; tri_setup(&grids[1], o->bound, p, &tcm);
            tri_sample(&grids[1], &tcm, st->act[w].c + 32);
        }
        dec_forward(&L[w], P[w], p, &st->act[w]);
        if (w == 3) { st->raw[0] = st->act[3].out[0]; st->raw[1] = st->act[3].out[1]; st->raw[2] = st->act[3].out[2]; }
        else occ += st->act[w].out[0];
    }
    st->raw[3] = st->inb ? occ : (real)100;                             /* Renderer.cpp:36 */
}

/* include/torchlib/utils.h:148-172 raw2outputs_nerf_color (occupancy=false branch is what the
 * reference executes, D9; occupancy=1 adds alpha=sigmoid(10*sigma)). */
static void composite_forward(const nso_opts* o, int S, const real* z, const real* rd, const real* raw /*[S][4]*/,
                              real* alpha, real* T, real* w, real* rgb, real* depth, real* var)
{
    real nrm = r_sqrt(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]);
    real Tacc = 1;
    rgb[0] = rgb[1] = rgb[2] = 0; *depth = 0;
    for (int s = 0; s < S; ++s) {
        real dist = (s + 1 < S ? z[s + 1] - z[s] : (real)1e10) * nrm;
        real sg = raw[4 * s + 3];
        if (o->occupancy) alpha[s] = (real)1 / ((real)1 + r_exp(-(real)10 * sg));
        else alpha[s] = (real)1 - r_exp(-(sg > 0 ? sg : 0) * dist);
        T[s] = Tacc;
        w[s] = alpha[s] * Tacc;
        Tacc *= ((real)1 - alpha[s] + (real)1e-10);
        for (int k = 0; k < 3; ++k) rgb[k] += w[s] * raw[4 * s + k];
        *depth += w[s] * z[s];
    }
    real v = 0;
    for (int s = 0; s < S; ++s) { real d = z[s] - *depth; v += w[s] * d * d; }
    *var = v;
}

NSO_API real nso_depth_max(int N, const real* gt_depth)
{
    real m = gt_depth[0];
    for (int i = 1; i < N; ++i) if (gt_depth[i] > m) m = gt_depth[i];
    return m;
}

/* Renderer::render_batch_ray forward.  gt_depth may be NULL (then n_surface=0, D8).
 * gt_depth_max < 0 -> computed over this batch (src/Renderer.cpp:76,93).
 * Optional outputs (may be NULL): weights [N][S], z_out [N][S], raw_out [N][S][4]. */
NSO_API int nso_render_forward(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int N,
                               const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max,
                               real* rgb, real* depth, real* var, real* weights, real* z_out, real* raw_out)
{
    dec_layout L[4]; for (int i = 0; i < 4; ++i) make_layout(i, &L[i]);
    if (o->n_samples + o->n_surface > MAX_S) return -1;
    if (gt_depth && gt_depth_max < 0) gt_depth_max = nso_depth_max(N, gt_depth);
    pt_state* st = (pt_state*)malloc(sizeof(pt_state));
#pragma omp parallel for schedule(dynamic, 4) if (N > 64)
    for (int n = 0; n < N; ++n) {
        pt_state stl; pt_state* sp = &stl;
        real z[MAX_S], raw[MAX_S * 4], al[MAX_S], T[MAX_S], w[MAX_S];
        int S = ray_z_vals(o, n, rays_o + 3 * n, rays_d + 3 * n, gt_depth != NULL, gt_depth ? gt_depth[n] : 0,
                           gt_depth_max, z);
        for (int s = 0; s < S; ++s) {
            real p[3];
            for (int k = 0; k < 3; ++k) p[k] = rays_o[3 * n + k] + rays_d[3 * n + k] * z[s];   /* :121 */
            point_forward(o, grids, P, L, stage, p, sp);
            memcpy(raw + 4 * s, sp->raw, 4 * sizeof(real));
        }
        composite_forward(o, S, z, rays_d + 3 * n, raw, al, T, w, rgb + 3 * n, depth + n, var + n);
        if (weights) memcpy(weights + (size_t)n * S, w, S * sizeof(real));
        if (z_out) memcpy(z_out + (size_t)n * S, z, S * sizeof(real));
        if (raw_out) memcpy(raw_out + (size_t)n * S * 4, raw, S * 4 * sizeof(real));
    }
    free(st);
    return 0;
}

/* Analytic backward of render_batch_ray (the reference relies on autograd: loss.backward() at
 * src/Mapper.cpp:444, src/Tracker.cpp:84; intended graph per D6/D7: z values and the in-bound mask
 * are constants, everything else differentiable).
 * Upstream: g_rgb [N][3], g_depth [N], g_var [N] (NULL = depth_var detached).
 * Accumulates into (each may be NULL): g_grids[l] ([C][Z][Y][X]), g_P[w] (packed decoder grads),
 * g_rays_o / g_rays_d [N][3] (overwritten).  Single-threaded when grads are accumulated. */
static int render_backward_impl(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int N,
                                const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max,
                                const real* g_rgb, const real* g_depth, const real* g_var,
                                real* const* g_grids, real* const* g_P, real* g_rays_o, real* g_rays_d,
                                const unsigned char* const* relu, const unsigned char* sigma_on,
                                real* const* r_grids, real* const* r_P, real* r_rays)
{
    dec_layout L[4]; for (int i = 0; i < 4; ++i) make_layout(i, &L[i]);
    if (o->n_samples + o->n_surface > MAX_S) return -1;
    if (gt_depth && gt_depth_max < 0) gt_depth_max = nso_depth_max(N, gt_depth);
    const int want_rays = g_rays_o != NULL || g_rays_d != NULL;
    /* rays are independent; each thread accumulates parameter gradients privately, then the partials are summed
     * (single-threaded when N is small so that the summation order is the plain ray order) */
#pragma omp parallel if (N > 64)
    {
    pt_state* st = (pt_state*)malloc(sizeof(pt_state) * MAX_S);
    real* tg[4] = { 0, 0, 0, 0 }; real* tp[4] = { 0, 0, 0, 0 };
    real* rg[4] = { 0, 0, 0, 0 }; real* rp[4] = { 0, 0, 0, 0 };
    int shared_acc = 1;
#ifdef _OPENMP
    shared_acc = omp_get_num_threads() == 1;
#endif
    for (int l = 0; l < 4; ++l) {
        size_t ng = (size_t)grids[l].C * grids[l].Z * grids[l].Y * grids[l].X;
        if (g_grids && g_grids[l]) tg[l] = shared_acc ? g_grids[l] : (real*)calloc(ng, sizeof(real));
        if (g_P && g_P[l]) tp[l] = shared_acc ? g_P[l] : (real*)calloc(L[l].total, sizeof(real));
        if (r_grids && r_grids[l]) rg[l] = shared_acc ? r_grids[l] : (real*)calloc(ng / (size_t)grids[l].C, sizeof(real));
        if (r_P && r_P[l] && tp[l]) rp[l] = shared_acc ? r_P[l] : (real*)calloc(L[l].total, sizeof(real));
    }
#pragma omp for schedule(dynamic, 4)
    for (int n = 0; n < N; ++n) {
        const real* ro = rays_o + 3 * n; const real* rd = rays_d + 3 * n;
        real z[MAX_S], raw[MAX_S * 4], al[MAX_S], T[MAX_S], w[MAX_S], rgb[3], D, V;
        int S = ray_z_vals(o, n, ro, rd, gt_depth != NULL, gt_depth ? gt_depth[n] : 0, gt_depth_max, z);
        for (int s = 0; s < S; ++s) {
            real p[3];
            for (int k = 0; k < 3; ++k) p[k] = ro[k] + rd[k] * z[s];
            point_forward(o, grids, P, L, stage, p, &st[s]);
            if (relu) for (int q = 0; q < 3; ++q) {               /* test aid: the backward takes the given ReLU branches */
                int wd = STAGE_DECODERS[stage][q];
                if (wd >= 0 && relu[wd]) memcpy(st[s].act[wd].on, relu[wd] + ((size_t)n * S + s) * 5 * H_DIM, 5 * H_DIM);
            }
            memcpy(raw + 4 * s, st[s].raw, 4 * sizeof(real));
        }
        composite_forward(o, S, z, rd, raw, al, T, w, rgb, &D, &V);
        /* d loss / d w_s */
        real gD = g_depth ? g_depth[n] : 0, gV = g_var ? g_var[n] : 0;
        real sw = 0; for (int s = 0; s < S; ++s) sw += w[s] * (z[s] - D);
        gD += gV * (real)(-2) * sw;
        real v[MAX_S];
        for (int s = 0; s < S; ++s) {
            real dz = z[s] - D;
            v[s] = gD * z[s] + gV * dz * dz;
            for (int k = 0; k < 3; ++k) v[s] += g_rgb[3 * n + k] * raw[4 * s + k];
        }
        real nrm = r_sqrt(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2]);
        real suffix = 0, g_nrm = 0, r_nrm = 0;
        real g_o[3] = { 0, 0, 0 }, g_d[3] = { 0, 0, 0 };
        real r_o = 0, r_d = 0;
        for (int s = S - 1; s >= 0; --s) {
            real g_alpha = v[s] * T[s] - suffix / ((real)1 - al[s] + (real)1e-10);
            suffix += v[s] * w[s];
            real sg = raw[4 * s + 3];
            real g_sigma;
            if (o->occupancy) g_sigma = g_alpha * (real)10 * al[s] * ((real)1 - al[s]);
            else {
                real dz = s + 1 < S ? z[s + 1] - z[s] : (real)1e10;
                real dist = dz * nrm;
                real rs = sg > 0 ? sg : 0;
                real ex = r_exp(-rs * dist);
                const int on = sigma_on ? sigma_on[(size_t)n * S + s] : (sg > 0);     /* relu(sigma), utils.h:160; tests may force the branch */
                g_sigma = on ? g_alpha * dist * ex : 0;
                g_nrm += g_alpha * rs * ex * dz;
                r_nrm += r_abs(g_alpha * rs * ex * dz);
            }
            if (!st[s].inb) g_sigma = 0;                      /* raw[~mask,3]=100 is a constant */
            real g_col[3];
            for (int k = 0; k < 3; ++k) g_col[k] = w[s] * g_rgb[3 * n + k];
            real p[3], g_p[3] = { 0, 0, 0 };
            for (int k = 0; k < 3; ++k) p[k] = ro[k] + rd[k] * z[s];
            for (int q = 0; q < 3; ++q) {
                int wd = STAGE_DECODERS[stage][q];
                if (wd < 0) break;
                real g_out[4] = { 0, 0, 0, 0 };
                if (wd == 3) { g_out[0] = g_col[0]; g_out[1] = g_col[1]; g_out[2] = g_col[2]; }
                else g_out[0] = g_sigma;
                real g_c[64];
                dec_backward(&L[wd], P[wd], p, &st[s].act[wd], g_out, tp[wd], g_c, want_rays ? g_p : NULL, rp[wd]);
                /* fine: only the first 32 features (grid_fine) carry gradient (MLP.cpp:81 NoGradGuard) */
                tri_backward(&grids[wd], &st[s].tc[wd], g_c, tg[wd], want_rays ? g_p : NULL, rg[wd]);
            }
            for (int k = 0; k < 3; ++k) { g_o[k] += g_p[k]; g_d[k] += g_p[k] * z[s]; }
            {
                real m = r_abs(g_p[0]); if (r_abs(g_p[1]) > m) m = r_abs(g_p[1]); if (r_abs(g_p[2]) > m) m = r_abs(g_p[2]);
                r_o += m; r_d += m * r_abs(z[s]);
            }
        }
        if (r_rays) { r_rays[2 * n] = r_o; r_rays[2 * n + 1] = r_d + r_nrm; }
        if (nrm > 0) for (int k = 0; k < 3; ++k) g_d[k] += g_nrm * rd[k] / nrm;      /* utils.h:153 norm(rays_d) */
        if (g_rays_o) memcpy(g_rays_o + 3 * n, g_o, sizeof(g_o));
        if (g_rays_d) memcpy(g_rays_d + 3 * n, g_d, sizeof(g_d));
    }
    if (!shared_acc) {
#pragma omp critical
        for (int l = 0; l < 4; ++l) {
            size_t ng = (size_t)grids[l].C * grids[l].Z * grids[l].Y * grids[l].X;
            if (tg[l]) { for (size_t i = 0; i < ng; ++i) g_grids[l][i] += tg[l][i]; free(tg[l]); }
            if (tp[l]) { for (size_t i = 0; i < L[l].total; ++i) g_P[l][i] += tp[l][i]; free(tp[l]); }
            if (rg[l]) { for (size_t i = 0; i < ng / (size_t)grids[l].C; ++i) r_grids[l][i] += rg[l][i]; free(rg[l]); }
            if (rp[l]) { for (size_t i = 0; i < L[l].total; ++i) r_P[l][i] += rp[l][i]; free(rp[l]); }
        }
    }
    free(st);
    }
    return 0;
}

NSO_API int nso_render_backward(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int N,
                                const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max,
                                const real* g_rgb, const real* g_depth, const real* g_var,
                                real* const* g_grids, real* const* g_P, real* g_rays_o, real* g_rays_d)
{
    return render_backward_impl(o, grids, P, stage, N, rays_o, rays_d, gt_depth, gt_depth_max, g_rgb, g_depth, g_var,
                                g_grids, g_P, g_rays_o, g_rays_d, NULL, NULL, NULL, NULL, NULL);
}

/* Test aid (not in the reference): the same backward with the branch of every hidden ReLU GIVEN instead of taken from
 * this evaluation's own pre-activations.  relu[w] (w = decoder 0..3, NULL = own branches): [N*S][5][32] bytes, 1 = "input > 0".
 * sigma_on[N*S] (or NULL): likewise the branch of relu(sigma) in the density compositing (utils.h:160).
 * The forward values are untouched.  With the branches another fp32 evaluation took (the HIP path's saved bits), the gradient
 * is one smooth function of the inputs for both, so ALL rays can be compared at the contract's tolerance. */
NSO_API int nso_render_backward_forced(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int N,
                                       const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max,
                                       const real* g_rgb, const real* g_depth, const real* g_var,
                                       real* const* g_grids, real* const* g_P, real* g_rays_o, real* g_rays_d,
                                       const unsigned char* const* relu, const unsigned char* sigma_on)
{
    return render_backward_impl(o, grids, P, stage, N, rays_o, rays_d, gt_depth, gt_depth_max, g_rgb, g_depth, g_var,
                                g_grids, g_P, g_rays_o, g_rays_d, relu, sigma_on, NULL, NULL, NULL);
}

/* Test aid: the forced backward (relu / sigma_on may be NULL) that also returns the SCALE of the rounding error any fp32 evaluation of its
 * sums may commit, so that a comparison can be made per voxel row, per weight and per ray instead of over a whole array:
 *   r_grids[l] [Z][Y][X]   R = sum_samples w(sample, voxel) max_c |g_feat(sample)[c]|: the running-error scale of g_grid[v][c] = sum w g_feat[c],
 *                          operand error of the chain that made g_feat included (it is relative to the size of g_feat, not to the possibly
 *                          cancelled sum).  R == 0 exactly where no sample touches the voxel with a non-zero weight and gradient.
 *   r_P[w] (packed)        sum |activation| |g| per decoder parameter (needs g_P[w])
 *   r_rays [N][2]          sum_samples max_k |g_p(sample)[k]| (for g_rays_o) and the same times |z| plus the sum over the samples of the
 *                          absolute terms of d loss / d |d| (for g_rays_d; the terms of a ray whose samples are all masked cancel)
 * Each may be NULL.  Buffers are accumulated into (the caller zeroes them). */
NSO_API int nso_render_backward_scaled(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int N,
                                       const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max,
                                       const real* g_rgb, const real* g_depth, const real* g_var,
                                       real* const* g_grids, real* const* g_P, real* g_rays_o, real* g_rays_d,
                                       const unsigned char* const* relu, const unsigned char* sigma_on,
                                       real* const* r_grids, real* const* r_P, real* r_rays)
{
    return render_backward_impl(o, grids, P, stage, N, rays_o, rays_d, gt_depth, gt_depth_max, g_rgb, g_depth, g_var,
                                g_grids, g_P, g_rays_o, g_rays_d, relu, sigma_on, r_grids, r_P, r_rays);
}

/* Test aid: the hidden ReLU inputs of decoder `which` at every sample, a_out[N*S][5][32] (tools/relu_flips.py counts the
 * branches on which two evaluations disagree), and optionally raw_out[N*S][4]. */
NSO_API int nso_preacts(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int which, int N,
                        const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max, real* a_out)
{
    dec_layout L[4]; for (int i = 0; i < 4; ++i) make_layout(i, &L[i]);
    if (gt_depth && gt_depth_max < 0) gt_depth_max = nso_depth_max(N, gt_depth);
#pragma omp parallel for schedule(dynamic, 4) if (N > 64)
    for (int n = 0; n < N; ++n) {
        pt_state st; real z[MAX_S];
        int S = ray_z_vals(o, n, rays_o + 3 * n, rays_d + 3 * n, gt_depth != NULL, gt_depth ? gt_depth[n] : 0,
                           gt_depth_max, z);
        for (int s = 0; s < S; ++s) {
            real p[3];
            for (int k = 0; k < 3; ++k) p[k] = rays_o[3 * n + k] + rays_d[3 * n + k] * z[s];
            point_forward(o, grids, P, L, stage, p, &st);
            memcpy(a_out + ((size_t)n * S + s) * 5 * H_DIM, st.act[which].a, sizeof(real) * 5 * H_DIM);
        }
    }
    return 0;
}

/* Test aid: how far the ReLU inputs of ANY fp32 evaluation of this path can lie from the exact ones -- a first-order error bound,
 * tau_out[N*S][5][32] for decoder `which`, evaluated at the samples with want[n*S+s] != 0 (want == NULL: all; the rest is left untouched).
 * Error sources, u = 2^-24 per fp32 operation:
 *   z      a handful of roundings of magnitudes <= the ray's largest z:                      dz  = 8 u z_max
 *   p      = fl(o + fl(d z)) (src/Renderer.cpp:121):                                        dp_i = |d_i| dz + u (|d_i z| + |p_i|)
 *   s_k    = the K = 3 FMA chain of p.B (GaussianFFT.cpp:13):                               ds_k = sum_i |B_ik| dp_i + u (|t0| + |t0 + t1| + |s_k|)
 *   e_k    = sin(s_k) with a sine accurate to sin_err absolute (glibc: 6e-8; v_sin_f32 + reduction: 3.2e-7):   de_k = ds_k + sin_err
 *   c_k    the trilinear feature: moving the lookup by dp moves it by at most (cells moved) x (spread of the 8 corner values), plus its own sums
 *   r_l[o] the local rounding of block l: a_l = b + sum_k W[o,k] x_k with every product in two fp16 / three bf16 pieces (2^-22 relative)
 *          summed in any order (K u), likewise fc_l c, and the sums that join them:
 *                                                      r = (K u + 2^-21) sum_k |W[o,k] x_k| + u |b| + the same for fc_l c + sum_k |F[o,k]| dc_k + 2 u |h|
 * The sources are carried through the network by the EXACT first-order map of this sample (the Jacobians d a_l / d source with this
 * sample's ReLU branches, so that paths that cancel do cancel), and only their signs are taken worst-case:
 *                                                      tau_l[o] = sum_src |d a_l[o] / d src| mag(src) + (local part of r_l[o]).
 * geometry_err = 0 leaves out dz, dp and ds: the bound between two fp32 evaluations that form z, p and p.B with the SAME operations (the HIP
 * kernels and the fp32 build of this file since round 4: bit-identical arguments) and differ in the sine and in the order of the sums.
 * quadrature = 1 turns the worst-case bound into the STANDARD DEVIATION of the probabilistic rounding model (Higham & Mary 2019: rounding errors
 * as independent zero-mean variables): every source enters with its rms (a uniform error of half-width e has rms e / sqrt 3; a sum of K rounded
 * additions u / sqrt 3 times the root-sum-square of the running sums) and the contributions add in quadrature instead of in absolute value.  The
 * caller multiplies by the number of sigmas it wants (6: one exceedance expected in 10^9 inputs).
 * tau_raw0 (optional, [N*S]): the same bound for the decoder's first output (the occupancy that enters relu(sigma), utils.h:160).
 * A branch of an fp32 evaluation that differs from this (exact) evaluation's must have |a| <= tau (to first order in u);
 * tests/test_gpu_relu.py asserts it for every ReLU of the HIP forward that took the other branch.  Worst-case signs over 93 + 128 sources:
 * ~10x above the rms error, three orders below a typical |a|. */
#define NSRC (E_DIM + 4 * H_DIM)
NSO_API int nso_preact_bounds(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int which, int N,
                              const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max, real sin_err,
                              int geometry_err, int quadrature, const unsigned char* want, real* tau_out, real* tau_raw0)
{
    dec_layout L[4]; for (int i = 0; i < 4; ++i) make_layout(i, &L[i]);
    if (which < 1 || which > 3) return -1;
    if (gt_depth && gt_depth_max < 0) gt_depth_max = nso_depth_max(N, gt_depth);
    const real u = (real)5.9604644775390625e-08, u22 = (real)4.76837158203125e-07;
    const dec_layout* Lw = &L[which];
    const real* Pw = P[which];
#pragma omp parallel for schedule(dynamic, 1) if (N > 8)
    for (int n = 0; n < N; ++n) {
        pt_state st; real z[MAX_S];
        const real* ro = rays_o + 3 * n; const real* rd = rays_d + 3 * n;
        int S = ray_z_vals(o, n, ro, rd, gt_depth != NULL, gt_depth ? gt_depth[n] : 0, gt_depth_max, z);
        int any = want == NULL;
        for (int s = 0; s < S && !any; ++s) any = want[(size_t)n * S + s] != 0;
        if (!any) continue;
        real (*Jh)[NSRC] = (real (*)[NSRC])malloc(sizeof(real) * H_DIM * NSRC);      /* d h_{l-1} / d source */
        real (*Jh2)[NSRC] = (real (*)[NSRC])malloc(sizeof(real) * H_DIM * NSRC);     /* d h_2 / d source (skip connection of block 3) */
        real (*Ja)[NSRC] = (real (*)[NSRC])malloc(sizeof(real) * H_DIM * NSRC);
        const real dz = geometry_err ? 8 * u * r_abs(z[S - 1]) : 0;
        for (int s = 0; s < S; ++s) {
            if (want && !want[(size_t)n * S + s]) continue;
            real p[3], dp[3];
            for (int k = 0; k < 3; ++k) {
                p[k] = ro[k] + rd[k] * z[s];
                dp[k] = geometry_err ? r_abs(rd[k]) * dz + u * (r_abs(rd[k] * z[s]) + r_abs(p[k])) : 0;
            }
            point_forward(o, grids, P, L, stage, p, &st);
            const dec_act* A = &st.act[which];
            real mag[NSRC], dc[64], loc4[H_DIM];
            const real* B = Pw + Lw->oB;
            for (int k = 0; k < E_DIM; ++k) {
                real t0 = p[0] * B[k], t1 = p[1] * B[E_DIM + k], t2 = p[2] * B[2 * E_DIM + k];
                real ds = r_abs(B[k]) * dp[0] + r_abs(B[E_DIM + k]) * dp[1] + r_abs(B[2 * E_DIM + k]) * dp[2] +
                          u * (r_abs(t0) + r_abs(t0 + t1) + r_abs(t0 + t1 + t2));
                mag[k] = quadrature ? r_sqrt((geometry_err ? ds * ds : 0) + sin_err * sin_err) * (real)0.57735 : (geometry_err ? ds : 0) + sin_err;
            }
            for (int half = 0; half < (which == 2 ? 2 : 1); ++half) {          /* fine: its own level, then the middle level (MLP.cpp:79-84) */
                const nso_grid* g = &grids[half == 0 ? which : 1];
                tri_coord tc; tri_setup(g, o->bound, p, &tc);
                const size_t cs = (size_t)g->Z * g->Y * g->X;
                real shift = tc.gmul[0] * dp[0] + tc.gmul[1] * dp[1] + tc.gmul[2] * dp[2] + 6 * u * (real)(g->X + g->Y + g->Z);
                for (int c = 0; c < g->C; ++c) {
                    real lo = 0, hi = 0, am = 0; int first = 1;
                    for (int q = 0; q < 8; ++q) {
                        int ix = tc.i0[0] + (q & 1), iy = tc.i0[1] + ((q >> 1) & 1), iz = tc.i0[2] + (q >> 2);
                        real v = tri_inb(g, ix, iy, iz) ? g->v[c * cs + ((size_t)iz * g->Y + iy) * g->X + ix] : 0;
                        if (first || v < lo) lo = v;
                        if (first || v > hi) hi = v;
                        if (r_abs(v) > am) am = r_abs(v);
                        first = 0;
                    }
                    dc[32 * half + c] = shift * (hi - lo) * 3 + 16 * u * am;     /* three axes: each lerp moves by at most shift x spread */
                }
            }
            real* tau = tau_out + ((size_t)n * S + s) * 5 * H_DIM;
            for (int i = 0; i < 5; ++i) {
                const int nx = Lw->in_dim[i];
                const real* W = Pw + Lw->oW[i]; const real* b = Pw + Lw->ob[i];
                const real* Fw = Pw + Lw->oFw[i]; const real* Fb = Pw + Lw->oFb[i];
                const int nsrc = E_DIM + (i < 4 ? i : 4) * H_DIM;               /* sources that exist before block i */
                for (int q = 0; q < H_DIM; ++q) {
                    const real* w = W + (size_t)q * nx;
                    real loc = 0;                                                /* local rounding of a_i[q] */
                    for (int c = 0; c < NSRC; ++c) Ja[q][c] = 0;
                    if (i == 0 || i == 3) {
                        for (int k = 0; k < E_DIM; ++k) { Ja[q][k] = w[k]; loc += r_abs(w[k] * A->e[k]); }
                        if (i == 3) for (int k = 0; k < H_DIM; ++k) {
                            const real wk = w[E_DIM + k];
                            loc += r_abs(wk * A->h[2][k]);
                            for (int c = 0; c < nsrc; ++c) Ja[q][c] += wk * Jh2[k][c];
                        }
                    } else {
                        for (int k = 0; k < H_DIM; ++k) {
                            const real wk = w[k];
                            loc += r_abs(wk * A->h[i - 1][k]);
                            for (int c = 0; c < nsrc; ++c) Ja[q][c] += wk * Jh[k][c];
                        }
                    }
                    if (quadrature) {                                            /* rms of K rounded terms + the pieces' 2^-22: sqrt(K) u / sqrt 3 x rss of the terms */
                        real ss = 0;
                        if (i == 0 || i == 3) for (int k = 0; k < E_DIM; ++k) ss += (w[k] * A->e[k]) * (w[k] * A->e[k]);
                        if (i == 3) for (int k = 0; k < H_DIM; ++k) ss += (w[E_DIM + k] * A->h[2][k]) * (w[E_DIM + k] * A->h[2][k]);
                        if (i != 0 && i != 3) for (int k = 0; k < H_DIM; ++k) ss += (w[k] * A->h[i - 1][k]) * (w[k] * A->h[i - 1][k]);
                        /* K rounded additions, each of the size of the running sum (a random walk from the bias to a: mean square a^2 / 3 + ss / 2) */
                        loc = r_sqrt((u * u / 3) * (real)nx * (A->a[i][q] * A->a[i][q] / 3 + ss / 2) + (u22 * u22 / 3) * ss);
                    } else loc = ((real)nx * u + 2 * u22) * loc + u * r_abs(b[q]);
                    real t = quadrature ? loc * loc : loc;
                    for (int c = 0; c < nsrc; ++c) { const real v = r_abs(Ja[q][c]) * mag[c]; t += quadrature ? v * v : v; }
                    if (quadrature) t = r_sqrt(t);
                    tau[i * H_DIM + q] = t;
                    {                                                            /* block output: relu(a) + fc c + bc; its local error becomes source (i, q) */
                        real flin = 0, fmag = 0;
                        for (int k = 0; k < Lw->c_dim; ++k) { flin += r_abs(Fw[(size_t)q * Lw->c_dim + k]) * dc[k]; fmag += r_abs(Fw[(size_t)q * Lw->c_dim + k] * A->c[k]); }
                        real m = loc + flin + ((real)Lw->c_dim * u + 2 * u22) * fmag + u * r_abs(Fb[q]) + 2 * u * r_abs(A->h[i][q]);
                        if (quadrature) {
                            real fs = 0;
                            for (int k = 0; k < Lw->c_dim; ++k) fs += (Fw[(size_t)q * Lw->c_dim + k] * A->c[k]) * (Fw[(size_t)q * Lw->c_dim + k] * A->c[k]);
                            const real f1 = (r_sqrt((real)Lw->c_dim) * u + u22) * (real)0.57735 * r_sqrt(fs), f2 = u * (real)0.57735 * r_abs(A->h[i][q]);
                            m = r_sqrt(loc * loc + flin * flin * (real)0.3333 + f1 * f1 + 2 * f2 * f2);
                        }
                        if (i < 4) mag[E_DIM + i * H_DIM + q] = m; else loc4[q] = m;
                    }
                }
                if (i == 4 && tau_raw0) {                                        /* out[0] = bo + Wo[0] . h4 (fp32 dot product in the kernels) */
                    const real* Wo = Pw + Lw->oWo;
                    real t = u * r_abs(Pw[Lw->obo]), mg = 0;
                    real col[NSRC];
                    for (int c = 0; c < NSRC; ++c) col[c] = 0;
                    for (int q = 0; q < H_DIM; ++q) {
                        const int on = A->a[4][q] > 0;
                        mg += r_abs(Wo[q] * A->h[4][q]);
                        t += r_abs(Wo[q]) * loc4[q];
                        if (on) for (int c = 0; c < NSRC; ++c) col[c] += Wo[q] * Ja[q][c];
                    }
                    if (quadrature) {
                        real t2 = 0, m2 = 0;
                        for (int q = 0; q < H_DIM; ++q) { t2 += (Wo[q] * loc4[q]) * (Wo[q] * loc4[q]); m2 += (Wo[q] * A->h[4][q]) * (Wo[q] * A->h[4][q]); }
                        for (int c = 0; c < NSRC; ++c) t2 += (col[c] * mag[c]) * (col[c] * mag[c]);
                        tau_raw0[(size_t)n * S + s] = r_sqrt(t2 + (real)H_DIM * u * u * (real)0.3333 * m2);
                    } else {
                    for (int c = 0; c < NSRC; ++c) t += r_abs(col[c]) * mag[c];
                    tau_raw0[(size_t)n * S + s] = t + (real)(H_DIM + 2) * u * mg;
                    }
                }
                if (i < 4) {
                    for (int q = 0; q < H_DIM; ++q) {
                        const int on = A->a[i][q] > 0;
                        for (int c = 0; c < NSRC; ++c) Jh[q][c] = on ? Ja[q][c] : 0;
                        Jh[q][E_DIM + i * H_DIM + q] = 1;
                    }
                    if (i == 2) memcpy(Jh2, Jh, sizeof(real) * H_DIM * NSRC);
                }
            }
        }
        free(Jh); free(Jh2); free(Ja);
    }
    return 0;
}

/* Test aid (not in the reference): per-ray fragility = min |x| over every ReLU input on the ray (hidden
 * pre-activations of the decoders the stage uses, and sigma of in-bound samples in density mode).
 * ReLU's derivative jumps at 0, so two fp32 evaluations whose pre-activations differ by rounding can
 * legitimately disagree on the gradient of such a ray; parity tests mask rays below a threshold. */
NSO_API int nso_ray_fragility(const nso_opts* o, const nso_grid* grids, const real* const* P, int stage, int N,
                              const real* rays_o, const real* rays_d, const real* gt_depth, real gt_depth_max,
                              real* frag)
{
    dec_layout L[4]; for (int i = 0; i < 4; ++i) make_layout(i, &L[i]);
    if (gt_depth && gt_depth_max < 0) gt_depth_max = nso_depth_max(N, gt_depth);
#pragma omp parallel for schedule(dynamic, 4) if (N > 64)
    for (int n = 0; n < N; ++n) {
        pt_state st; real z[MAX_S];
        int S = ray_z_vals(o, n, rays_o + 3 * n, rays_d + 3 * n, gt_depth != NULL, gt_depth ? gt_depth[n] : 0,
                           gt_depth_max, z);
        real m = (real)1e30;
        for (int s = 0; s < S; ++s) {
            real p[3];
            for (int k = 0; k < 3; ++k) p[k] = rays_o[3 * n + k] + rays_d[3 * n + k] * z[s];
            point_forward(o, grids, P, L, stage, p, &st);
            for (int q = 0; q < 3; ++q) {
                int w = STAGE_DECODERS[stage][q];
                if (w < 0) break;
                for (int i = 0; i < 5; ++i) for (int u = 0; u < H_DIM; ++u) {
                    real a = r_abs(st.act[w].a[i][u]); if (a < m) m = a;
                }
            }
            if (st.inb && !o->occupancy) { real a = r_abs(st.raw[3]); if (a < m) m = a; }
        }
        frag[n] = m;
    }
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * Losses.  Mapper: src/Mapper.cpp:435-442.  Tracker: src/Tracker.cpp:67-82.
 * Both return the loss and the seed gradients d loss / d depth, d loss / d rgb (, d loss / d var).
 * torch: d|x|/dx = sign(x) with sign(0)=0.
 * ------------------------------------------------------------------------------------------ */
static inline real sgn(real x) { return x > 0 ? (real)1 : (x < 0 ? (real)-1 : (real)0); }

NSO_API real nso_loss_map(int N, const real* depth, const real* rgb, const real* gt_depth, const real* gt_color,
                          real w_color, int use_color, real* g_depth, real* g_rgb)
{
    real loss = 0, closs = 0;
    for (int n = 0; n < N; ++n) {
        real g = 0;
        if (gt_depth[n] > 0) { real r = gt_depth[n] - depth[n]; loss += r_abs(r); g = -sgn(r); }
        g_depth[n] = g;
        for (int k = 0; k < 3; ++k) {
            real r = gt_color[3 * n + k] - rgb[3 * n + k];
            if (use_color) { closs += r_abs(r); g_rgb[3 * n + k] = -w_color * sgn(r); }
            else g_rgb[3 * n + k] = 0;
        }
    }
    return use_color ? loss + w_color * closs : loss;
}

static int cmp_real(const void* a, const void* b) { real x = *(const real*)a, y = *(const real*)b; return (x > y) - (x < y); }

/* torch.median of n elements = element (n-1)/2 of the sorted order (lower median) */
NSO_API real nso_loss_track(int N, const real* depth, const real* rgb, const real* var, const real* gt_depth,
                            const real* gt_color, real w_color, int use_color, int handle_dynamic, int detach_var,
                            real* g_depth, real* g_rgb, real* g_var)
{
    real thr = 0;
    if (handle_dynamic) {
        real* tmp = (real*)malloc(sizeof(real) * N);
        for (int n = 0; n < N; ++n) tmp[n] = r_abs(gt_depth[n] - depth[n]);
        qsort(tmp, N, sizeof(real), cmp_real);
        thr = (real)10 * tmp[(N - 1) / 2];
        free(tmp);
    }
    real loss = 0, closs = 0;
    for (int n = 0; n < N; ++n) {
        real r = gt_depth[n] - depth[n];
        int m = gt_depth[n] > 0 && (!handle_dynamic || r_abs(r) < thr);
        real u = r_sqrt(var[n] + (real)1e-10);
        g_depth[n] = 0; if (g_var) g_var[n] = 0;
        for (int k = 0; k < 3; ++k) g_rgb[3 * n + k] = 0;
        if (!m) continue;
        loss += r_abs(r) / u;
        g_depth[n] = -sgn(r) / u;
        if (g_var && !detach_var) g_var[n] = -r_abs(r) / ((real)2 * u * u * u);
        if (use_color) for (int k = 0; k < 3; ++k) {
            real rc = gt_color[3 * n + k] - rgb[3 * n + k];
            closs += r_abs(rc); g_rgb[3 * n + k] = -w_color * sgn(rc);
        }
    }
    return use_color ? loss + w_color * closs : loss;
}

/* torch::optim::Adam defaults (src/Mapper.cpp:330, src/Tracker.cpp:103): amsgrad off, no weight decay.
 * mask may be NULL; mask[i]==0 freezes element i (frustum feature selection, Mapper.cpp:254-290,333-350:
 * only masked voxels are optimiser parameters). step is the 1-based step count of this group. */
NSO_API void nso_adam_step(long n, real* p, const real* g, real* m, real* v, const unsigned char* mask,
                           real lr, real b1, real b2, real eps, int step)
{
    real bc1 = (real)1 - (real)pow((double)b1, step);
    real bc2 = (real)1 - (real)pow((double)b2, step);
    real step_size = lr / bc1;
    real bc2s = r_sqrt(bc2);
    for (long i = 0; i < n; ++i) {
        if (mask && !mask[i]) continue;
        m[i] = b1 * m[i] + ((real)1 - b1) * g[i];
        v[i] = b2 * v[i] + ((real)1 - b2) * g[i] * g[i];
        real denom = r_sqrt(v[i]) / bc2s + eps;
        p[i] -= step_size * (m[i] / denom);
    }
}

/* ------------------------------------------------------------------------------------------
 * Pose helpers.  quad2rotation include/torchlib/utils.h:174-195, get_camera_from_tensor :198-210.
 * cam = (qw,qx,qy,qz,tx,ty,tz) -> c2w [3][4] row-major.
 * ------------------------------------------------------------------------------------------ */
NSO_API void nso_camera_from_tensor(const real* cam, real* c2w /*[12]*/)
{
    real qr = cam[0], qi = cam[1], qj = cam[2], qk = cam[3];
    real two_s = (real)2 / (qr * qr + qi * qi + qj * qj + qk * qk);
    real R[9] = {
        (real)1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
        two_s * (qi * qj + qk * qr), (real)1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), (real)1 - two_s * (qi * qi + qj * qj) };
    for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) c2w[4 * a + b] = R[3 * a + b]; c2w[4 * a + 3] = cam[4 + a]; }
}

/* d loss / d cam from d loss / d c2w (g_c2w [12]) -- numerically exact chain rule of the above */
NSO_API void nso_camera_backward(const real* cam, const real* g_c2w, real* g_cam /*[7]*/)
{
    real q[4] = { cam[0], cam[1], cam[2], cam[3] };
    real n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    real two_s = (real)2 / n2;
    real qr = q[0], qi = q[1], qj = q[2], qk = q[3];
    /* R_ab = delta_ab*1 + two_s * M_ab(q);  dR/dq_c = dtwo_s/dq_c * M + two_s * dM/dq_c */
    real M[9] = { -(qj * qj + qk * qk), qi * qj - qk * qr, qi * qk + qj * qr,
                  qi * qj + qk * qr, -(qi * qi + qk * qk), qj * qk - qi * qr,
                  qi * qk - qj * qr, qj * qk + qi * qr, -(qi * qi + qj * qj) };
    /* dM/dq: rows = element, cols = (qr,qi,qj,qk) */
    real dM[9][4] = {
        { 0, 0, -2 * qj, -2 * qk }, { -qk, qj, qi, -qr }, { qj, qk, qr, qi },
        { qk, qj, qi, qr }, { 0, -2 * qi, 0, -2 * qk }, { -qi, -qr, qk, qj },
        { -qj, qk, -qr, qi }, { qi, qr, qk, qj }, { 0, -2 * qi, -2 * qj, 0 } };
    for (int c = 0; c < 4; ++c) {
        real dts = -(real)2 * two_s * q[c] / n2;      /* d(2/n2)/dq_c = -4 q_c / n2^2 */
        real s = 0;
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b)
            s += g_c2w[4 * a + b] * (dts * M[3 * a + b] + two_s * dM[3 * a + b][c]);
        g_cam[c] = s;
    }
    for (int a = 0; a < 3; ++a) g_cam[4 + a] = g_c2w[4 * a + 3];
}

/* raySampler direction/origin part, include/torchlib/utils.h:44-52 (pixel indices are an INPUT:
 * torch::randint's stream cannot be matched).  mode bit0: as-written j_t=(i-cy)/fy without sign
 * flip (D11); bit1: truncate intrinsics to int (D10).  Default 0 = intended OpenGL camera
 * dirs=[(i-cx)/fx, -(j-cy)/fy, -1]; rays_d = R dir (:51), rays_o = t (:52). */
NSO_API void nso_rays_from_pixels(int n, const int* pix_i /*col*/, const int* pix_j /*row*/, real fx, real fy,
                                  real cx, real cy, const real* c2w /*[12]*/, int mode, real* rays_o, real* rays_d)
{
    if (mode & 2) { fx = (real)(int)fx; fy = (real)(int)fy; cx = (real)(int)cx; cy = (real)(int)cy; }
    for (int r = 0; r < n; ++r) {
        real i = (real)pix_i[r], j = (real)pix_j[r];
        real dir[3];
        dir[0] = (i - cx) / fx;
        dir[1] = (mode & 1) ? (i - cy) / fy : -(j - cy) / fy;
        dir[2] = -1;
        for (int a = 0; a < 3; ++a) {
            rays_d[3 * r + a] = dir[0] * c2w[4 * a] + dir[1] * c2w[4 * a + 1] + dir[2] * c2w[4 * a + 2];
            rays_o[3 * r + a] = c2w[4 * a + 3];
        }
    }
}

/* d loss / d c2w from per-ray gradients: g_R[a][b] = sum_n g_d[n][a] dir[n][b], g_t = sum_n g_o[n] */
NSO_API void nso_rays_backward(int n, const int* pix_i, const int* pix_j, real fx, real fy, real cx, real cy, int mode,
                               const real* g_rays_o, const real* g_rays_d, real* g_c2w /*[12]*/)
{
    if (mode & 2) { fx = (real)(int)fx; fy = (real)(int)fy; cx = (real)(int)cx; cy = (real)(int)cy; }
    for (int k = 0; k < 12; ++k) g_c2w[k] = 0;
    for (int r = 0; r < n; ++r) {
        real i = (real)pix_i[r], j = (real)pix_j[r];
        real dir[3] = { (i - cx) / fx, (mode & 1) ? (i - cy) / fy : -(j - cy) / fy, (real)-1 };
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) g_c2w[4 * a + b] += g_rays_d[3 * r + a] * dir[b];
            g_c2w[4 * a + 3] += g_rays_o[3 * r + a];
        }
    }
}

/* inside-bbox pre-filter, src/Mapper.cpp:416-427 / src/Tracker.cpp:48-58: keep[n] = t >= gt_depth */
NSO_API int nso_inside_filter(const real* bound, int N, const real* rays_o, const real* rays_d, const real* gt_depth,
                              unsigned char* keep)
{
    int c = 0;
    for (int n = 0; n < N; ++n) { keep[n] = (unsigned char)ray_inside(bound, rays_o + 3 * n, rays_d + 3 * n, gt_depth[n]); c += keep[n]; }
    return c;
}

/* bound the OpenMP team (bench.py: the GPU box shows 256 logical CPUs to a process whose share is 16; every thread of
 * nso_render_backward owns a private copy of the gradient buffers) */
NSO_API void nso_set_num_threads(int n)
{
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

NSO_API int nso_num_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* ------------------------------------------------------------------------------------------
 * Frustum voxel mask ("next" row N2), Mapper::get_mask_from_c2w src/Mapper.cpp:42-130, intended semantics:
 *   points = meshgrid(linspace(bound) per axis) (D21: float end points), w2c = inverse(c2w) (:62), cam.x *= -1 (:73),
 *   uv = K cam / (z + 1e-5) (:74-76), depth sampled bilinearly at uv (cv::remap INTER_LINEAR, zero border; :93 --
 *   D22: the four memcpy's are reversed as written), zero depths replaced by the maximum sampled depth (:104-105),
 *   mask = 0<u<W & 0<v<H & 0 <= -z <= depth + 0.5 (:102,:109-111; the upstream Python tests -z, the C++ text z),
 *   OR |p - cam centre|^2 < 0.25 (:121-123).  grid_coarse: all ones (:54-59).
 * mask layout [Z][Y][X] (the permute of :261).  c2w: 16 floats row-major [4][4].
 * ------------------------------------------------------------------------------------------ */
static real bilinear_zero(const real* img, int H, int W, real u, real v)
{
    real x0 = r_floor(u), y0 = r_floor(v);
    real ax = u - x0, ay = v - y0;
    int ix = (int)x0, iy = (int)y0;
    real s = 0;
    for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx) {
        int x = ix + dx, y = iy + dy;
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        s += (dx ? ax : (real)1 - ax) * (dy ? ay : (real)1 - ay) * img[(size_t)y * W + x];
    }
    return s;
}

static void invert_rigid4(const real* m, real* inv)      /* general 4x4 inverse by Gauss-Jordan (c2w need not be orthonormal) */
{
    double a[4][8];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { a[i][j] = m[4 * i + j]; a[i][4 + j] = i == j; }
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r) if (fabs(a[r][c]) > fabs(a[p][c])) p = r;
        for (int j = 0; j < 8; ++j) { double t = a[c][j]; a[c][j] = a[p][j]; a[p][j] = t; }
        double d = a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] /= d;
        for (int r = 0; r < 4; ++r) if (r != c) { double f = a[r][c]; for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j]; }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) inv[4 * i + j] = (real)a[i][4 + j];
}

NSO_API void nso_world_to_camera(const real* c2w, real* w2c) { invert_rigid4(c2w, w2c); }

NSO_API int nso_frustum_mask(const real* bound, int Z, int Y, int X, const real* depth_img, int H, int W, real fx, real fy,
                             real cx, real cy, const real* c2w, int is_coarse, unsigned char* mask /*[Z][Y][X]*/)
{
    size_t n = (size_t)Z * Y * X;
    if (is_coarse) { memset(mask, 1, n); return (int)n; }
    real w2c[16];
    invert_rigid4(c2w, w2c);
    real* dep = (real*)malloc(n * sizeof(real));
    real* zz = (real*)malloc(n * sizeof(real));
    unsigned char* inimg = (unsigned char*)malloc(n);
    real dmax = 0;                                          /* the floor: a zero depth is "no reading", and so is a negative sample */
    for (int iz = 0; iz < Z; ++iz) for (int iy = 0; iy < Y; ++iy) for (int ix = 0; ix < X; ++ix) {
        size_t v = ((size_t)iz * Y + iy) * X + ix;
        real p[3];
        p[0] = bound[0] + (bound[1] - bound[0]) * linspace01(ix, X);
        p[1] = bound[2] + (bound[3] - bound[2]) * linspace01(iy, Y);
        p[2] = bound[4] + (bound[5] - bound[4]) * linspace01(iz, Z);
        real cam[3];
        for (int a = 0; a < 3; ++a) cam[a] = w2c[4 * a] * p[0] + w2c[4 * a + 1] * p[1] + w2c[4 * a + 2] * p[2] + w2c[4 * a + 3];
        cam[0] = -cam[0];
        real z = cam[2] + (real)1e-5;
        real u = (fx * cam[0] + cx * cam[2]) / z, vv = (fy * cam[1] + cy * cam[2]) / z;
        real d = bilinear_zero(depth_img, H, W, u, vv);
        dep[v] = d; zz[v] = z;
        inimg[v] = u < (real)W && u > 0 && vv < (real)H && vv > 0;
        if (d > dmax) dmax = d;
    }
    int cnt = 0;
    for (int iz = 0; iz < Z; ++iz) for (int iy = 0; iy < Y; ++iy) for (int ix = 0; ix < X; ++ix) {
        size_t v = ((size_t)iz * Y + iy) * X + ix;
        real d = dep[v] == 0 ? dmax : dep[v];
        int m = inimg[v] && (0 <= -zz[v]) && (-zz[v] <= d + (real)0.5);
        real p[3];
        p[0] = bound[0] + (bound[1] - bound[0]) * linspace01(ix, X);
        p[1] = bound[2] + (bound[3] - bound[2]) * linspace01(iy, Y);
        p[2] = bound[4] + (bound[5] - bound[4]) * linspace01(iz, Z);
        real dx = p[0] - c2w[3], dy = p[1] - c2w[7], dz = p[2] - c2w[11];
        if (dx * dx + dy * dy + dz * dz < (real)0.25) m = 1;
        mask[v] = (unsigned char)m; cnt += m;
    }
    free(dep); free(zz); free(inimg);
    return cnt;
}

/* Mapper::keyframe_selection_overlap, reference src/Mapper.cpp:132-196 (next row N3; also include/torchlib/utils.h:58-130):
 * the rays of `N` pixels of the current frame are sampled at `ns` depths between 0.8*depth and depth+0.5 and projected into
 * every keyframe; percent[k] = fraction of those points that fall inside keyframe k's image (20-pixel edge) in front of its
 * camera.  The caller ranks the keyframes by percent (descending, stable) and keeps the first k_overlap with percent > 0
 * (the reference's `selected_kf.size()-k_overlap > 0` on size_t is read as size > k_overlap). */
NSO_API void nso_keyframe_overlap(int N, const real* rays_o, const real* rays_d, const real* gt_depth, int ns, int H, int W,
                                  real fx, real fy, real cx, real cy, int K, const real* c2w /*[K][16]*/, real* percent /*[K]*/)
{
    const int edge = 20;
    for (int k = 0; k < K; ++k) {
        real w2c[16];
        invert_rigid4(c2w + 16 * k, w2c);
        long count = 0;
        for (int n = 0; n < N; ++n) {
            const real nearv = gt_depth[n] * (real)0.8, farv = gt_depth[n] + (real)0.5;
            for (int s = 0; s < ns; ++s) {
                const real t = linspace01(s, ns);
                const real z = nearv * ((real)1 - t) + farv * t;
                real p[3], cam[3];
                for (int a = 0; a < 3; ++a) p[a] = rays_o[3 * n + a] + rays_d[3 * n + a] * z;
                for (int a = 0; a < 3; ++a) cam[a] = w2c[4 * a] * p[0] + w2c[4 * a + 1] * p[1] + w2c[4 * a + 2] * p[2] + w2c[4 * a + 3];
                cam[0] = -cam[0];
                const real zc = cam[2] + (real)1e-5;
                const real u = (fx * cam[0] + cx * cam[2]) / zc, v = (fy * cam[1] + cy * cam[2]) / zc;
                if (u < (real)(W - edge) && u > (real)edge && v < (real)(H - edge) && v > (real)edge && zc < 0) ++count;
            }
        }
        percent[k] = (real)count / (real)((long)N * ns);
    }
}

/* raySampler's pixel draw and ground-truth gather, reference include/torchlib/utils.h:13-43 (next row N1).  The reference draws
 * `n` indices with torch::randint over the cropped window [H0,H1) x [W0,W1) (row-major, utils.h:19-36); that stream cannot be
 * reproduced, so the draw is restated with this library's counter-based hash: ind = floor(u32 * total / 2^32). */
NSO_API void nso_sample_pixels(uint64_t seed, int n, int H0, int H1, int W0, int W1, int* pix_i /*col*/, int* pix_j /*row*/)
{
    const int Ww = W1 - W0;
    const uint64_t total = (uint64_t)(H1 - H0) * (uint64_t)Ww;
    for (int r = 0; r < n; ++r) {
        const uint64_t ind = ((uint64_t)hash_u32(seed, (uint32_t)r, 0x51u) * total) >> 32;
        pix_i[r] = W0 + (int)(ind % (uint64_t)Ww);
        pix_j[r] = H0 + (int)(ind / (uint64_t)Ww);
    }
}
NSO_API void nso_gather_pixels(int n, const int* pix_i, const int* pix_j, int W, const real* depth /*[H][W]*/, const real* color /*[H][W][3]*/,
                               real* gt_depth, real* gt_color)
{
    for (int r = 0; r < n; ++r) {
        const size_t p = (size_t)pix_j[r] * W + pix_i[r];
        gt_depth[r] = depth[p];
        for (int k = 0; k < 3; ++k) gt_color[3 * r + k] = color[3 * p + k];
    }
}

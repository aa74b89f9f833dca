// hull_plan_test FILE -- the host side of nsk_points_hull and nsk_lattice_in_hull (csrc/nsk_hull_plan.h: the face table, the insertion
// loop, the scaled planes) over a CPU stand-in for the device's answers, against the clouds and expected hulls tests/test_hull_cpu.py
// writes to FILE (no torch, no HIP; built with AddressSanitizer + UndefinedBehaviorSanitizer).  FILE, little endian:
//   int32 clouds; per cloud: int32 N, float32 [N][3], int64 info[8], int32 nv, int32 nf, int32 vertices[nv], int32 faces[nf][3],
//   float64 scale, float64 planes[nf][6], float64 box[6].
// Prints "hull_plan_test: ok" when every cloud gives the expected bytes.
#include "nsk_hull_plan.h"
#include <cstdio>
#include <cstdlib>

// what nsk_hull.h's kernels answer, one point at a time: face_of per point, the new faces' counts and apexes
struct CpuPoints {
    std::vector<int> q;                 // [N][3], q_x = INT_MIN: not finite
    std::vector<int> face_of;
    std::vector<HullFaceRec> all;
    int rehome(bool initial, int apex, const int* aq, int first_new, int n_new, const HullFaceRec* recs, long long outside, HullReport* out)
    {
        if ((size_t)first_new != all.size()) return 1;
        all.insert(all.end(), recs, recs + n_new);
        const int N = (int)face_of.size();
        std::vector<long long> best((size_t)n_new, 0);
        long long seen = 0;
        for (int k = 0; k < n_new; ++k) { out[k].count = 0; out[k].apex = -1; out[k].q[0] = out[k].q[1] = out[k].q[2] = 0; }
        for (int p = 0; p < N; ++p) {
            const int* qp = &q[3 * (size_t)p];
            bool move;
            if (initial) { move = qp[0] != INT32_MIN; if (!move) face_of[(size_t)p] = -1; }
            else {
                const int f = face_of[(size_t)p];
                if (f >= 0) ++seen;
                move = f >= 0 && hull_side(all[(size_t)f].n, all[(size_t)f].a, aq) > 0;
            }
            if (!move) continue;
            int g = -1;
            long long det = 0;
            if (p != apex)
                for (int k = 0; k < n_new; ++k) {
                    const long long d = hull_side(recs[k].n, recs[k].a, qp);
                    if (d > 0) { g = k; det = d; break; }
                }
            face_of[(size_t)p] = g < 0 ? -1 : first_new + g;
            if (g < 0) continue;
            ++out[g].count;
            if (det > best[(size_t)g]) { best[(size_t)g] = det; out[g].apex = p; memcpy(out[g].q, qp, 12); }      // (ascending p: a tie keeps the smaller)
        }
        if (!initial && seen != outside) return 2;          // the loop's count of outside points is the points' own
        return 0;
    }
};

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static int run_cloud(FILE* f, int ci)
{
    int N = 0;
    if (!rd(f, &N, 1) || N < 0) return 1;
    std::vector<float> pts((size_t)N * 3);
    long long want[8];
    int nv = 0, nf = 0;
    if (!rd(f, pts.data(), pts.size()) || !rd(f, want, 8) || !rd(f, &nv, 1) || !rd(f, &nf, 1) || nv < 0 || nf < 0) return 1;
    std::vector<int> wv((size_t)nv), wf((size_t)nf * 3);
    double scale = 0, wbox[6];
    std::vector<double> wplanes((size_t)nf * 6);
    if (!rd(f, wv.data(), wv.size()) || !rd(f, wf.data(), wf.size()) || !rd(f, &scale, 1) || !rd(f, wplanes.data(), wplanes.size()) || !rd(f, wbox, 6)) return 1;

    long long info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int> verts, tris;
    [&]() {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        std::vector<uint8_t> fin((size_t)N);
        for (int i = 0; i < N; ++i) {
            const float* p = &pts[3 * (size_t)i];
            fin[(size_t)i] = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
            if (!fin[(size_t)i]) continue;
            ++info[0];
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)p[a]); hi[a] = std::max(hi[a], (double)p[a]); }
        }
        info[1] = N - info[0];
        if (info[0] == 0) return;
        const double E = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
        if (!(E > 0.0)) return;
        const double quantum = E / (double)HULL_QMAX, s = hull_scale(E);
        memcpy(&info[6], &quantum, 8);
        CpuPoints B;
        B.q.resize((size_t)N * 3); B.face_of.assign((size_t)N, -1);
        for (int i = 0; i < N; ++i)
            for (int a = 0; a < 3; ++a) B.q[3 * (size_t)i + a] = fin[(size_t)i] ? hull_quantise(pts[3 * (size_t)i + a], lo[a], s) : (a == 0 ? INT32_MIN : 0);
        // step 4, as k_hull_select scores it
        int idx[4] = {-1, -1, -1, -1}, q[4][3];
        long long u[3] = {0, 0, 0};
        for (int mode = 0; mode < 4; ++mode) {
            long long best = -1;
            for (int i = 0; i < N; ++i) {
                if (!fin[(size_t)i]) continue;
                const int* p = &B.q[3 * (size_t)i];
                long long sc;
                if (mode == 0) sc = ((1ll << 60) - 1) - (((long long)p[0] << 40) | ((long long)p[1] << 20) | (long long)p[2]);
                else {
                    const long long dx = (long long)p[0] - q[0][0], dy = (long long)p[1] - q[0][1], dz = (long long)p[2] - q[0][2];
                    if (mode == 1) sc = dx * dx + dy * dy + dz * dz;
                    else if (mode == 2) {
                        const long long cx = u[1] * dz - u[2] * dy, cy = u[2] * dx - u[0] * dz, cz = u[0] * dy - u[1] * dx;
                        sc = std::max(std::max(std::llabs(cx), std::llabs(cy)), std::llabs(cz));
                    } else sc = std::llabs(u[0] * dx + u[1] * dy + u[2] * dz);
                }
                if (sc > best) { best = sc; idx[mode] = i; }
            }
            memcpy(q[mode], &B.q[3 * (size_t)idx[mode]], 12);
            if (mode > 0 && best == 0) return;
            info[2] = mode;
            if (mode == 1) for (int a = 0; a < 3; ++a) u[a] = (long long)q[1][a] - q[0][a];
            if (mode == 2) hull_normal(q[0], q[1], q[2], u);
        }
        HullPlan P;
        P.start(idx, q);
        const int r = hull_plan_run(P, B);
        if (r != 0) { printf("cloud %d: the loop returned %d\n", ci, r); info[2] = -1; return; }
        P.result(verts, tris);
        info[3] = (long long)verts.size(); info[4] = (long long)tris.size() / 3; info[5] = P.insertions;
    }();
    for (int k = 0; k < 7; ++k) if (info[k] != want[k]) { printf("cloud %d: info[%d] = %lld, expected %lld\n", ci, k, info[k], want[k]); return 2; }
    if (verts != wv || tris != wf) { printf("cloud %d: the vertices or faces differ\n", ci); return 2; }
    if (nf > 0) {
        std::vector<float> xyz((size_t)nv * 3);
        std::vector<int> local(tris.size());
        for (int k = 0; k < nv; ++k) memcpy(&xyz[3 * (size_t)k], &pts[3 * (size_t)verts[(size_t)k]], 12);
        for (size_t k = 0; k < tris.size(); ++k) local[k] = (int)(std::lower_bound(verts.begin(), verts.end(), tris[k]) - verts.begin());
        std::vector<double> planes;
        double box[6];
        hull_mask_planes(nv, xyz.data(), nf, local.data(), scale, planes, box);
        if (memcmp(planes.data(), wplanes.data(), planes.size() * 8) != 0 || memcmp(box, wbox, sizeof(box)) != 0) {
            printf("cloud %d: the scaled planes differ\n", ci);
            return 2;
        }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: hull_plan_test FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    int clouds = 0, bad = 0;
    if (!rd(f, &clouds, 1)) { fclose(f); printf("short file\n"); return 2; }
    for (int ci = 0; ci < clouds; ++ci) {
        const int r = run_cloud(f, ci);
        if (r == 1) { printf("cloud %d: short file\n", ci); bad = 1; break; }
        bad |= r;
    }
    fclose(f);
    if (bad) return 1;
    printf("hull_plan_test: ok (%d clouds)\n", clouds);
    return 0;
}

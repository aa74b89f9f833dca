// nsk_hull_plan.h -- the host side of nsk_points_hull and nsk_lattice_in_hull (include/nsk.h states the rule): the face table of the
// incremental convex hull (triples, live flags, the directed edge -> face map), the insertion loop over whatever answers for the points
// (the device in nsk_hull.h, a CPU stand-in in host/test/hull_plan_test.cpp), and the scaled planes of the inside test.  Nothing here
// needs HIP: nsk.hip includes it, and host/test/hull_plan_test.cpp runs it alone under the sanitizers.
//
// Every decision is taken on the quantised integer coordinates (below 2^20 per axis): differences stay below 2^20, the components of a
// cross product below 2^41, a determinant below 3 * 2^61, so int64 never overflows.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

#define HULL_QMAX ((1 << 20) - 1)       // the largest quantised coordinate

// a face as the points' side needs it: the integer normal (b - a) x (c - a) and the corner a; det(face, p) = n . (q_p - a)
struct HullFaceRec { long long n[3]; int a[3]; int pad; };
// what the points' side reports for a new face: the size of its outside set, its apex (largest det, ties to the smallest index; -1 with
// an empty set) and the apex's quantised coordinates
struct HullReport { long long count; int apex; int q[3]; };

inline void hull_normal(const int a[3], const int b[3], const int c[3], long long n[3])
{
    const long long ux = (long long)b[0] - a[0], uy = (long long)b[1] - a[1], uz = (long long)b[2] - a[2];
    const long long vx = (long long)c[0] - a[0], vy = (long long)c[1] - a[1], vz = (long long)c[2] - a[2];
    n[0] = uy * vz - uz * vy; n[1] = uz * vx - ux * vz; n[2] = ux * vy - uy * vx;
}
inline long long hull_side(const long long n[3], const int a[3], const int p[3])
{
    return n[0] * ((long long)p[0] - a[0]) + n[1] * ((long long)p[1] - a[1]) + n[2] * ((long long)p[2] - a[2]);
}
// the quantisation of one coordinate: every operation an fp64 operation of its own, rint to nearest even (the default rounding mode)
inline int hull_quantise(float p, double lo, double s) { const double d = (double)p - lo; const double t = d * s; return (int)std::nearbyint(t); }
// s = (2^20 - 1) / E
inline double hull_scale(double E) { return (double)HULL_QMAX / E; }

struct HullPlan {
    struct Face {
        int v[3]; int q[3][3];          // the corners' indices and quantised coordinates
        long long n[3];
        long long count; int apex; int aq[3];       // its outside set, as reported
        bool live;
    };
    std::vector<Face> faces;
    std::unordered_map<unsigned long long, int> edge;       // directed edge (u, v) -> the live face it belongs to
    std::vector<HullFaceRec> recs;      // the faces created last (start, insert), for the points' side
    std::vector<int> visible, fresh;    // scratch of insert: the visible faces; (u, v) pairs and their corner slots
    std::vector<uint8_t> vis;
    int first_new = 0;                  // the number of the first of `recs`
    size_t cursor = 0;                  // no face below it has an outside point (counts only ever fall, new faces come behind)
    long long outside = 0;              // points in the outside sets of the live faces
    long long insertions = 0;

    static unsigned long long key(int u, int v) { return ((unsigned long long)(unsigned)u << 32) | (unsigned)v; }

    void add_face(int u, int v, int w, const int* qu, const int* qv, const int* qw)
    {
        Face f;
        f.v[0] = u; f.v[1] = v; f.v[2] = w;
        memcpy(f.q[0], qu, 12); memcpy(f.q[1], qv, 12); memcpy(f.q[2], qw, 12);
        hull_normal(f.q[0], f.q[1], f.q[2], f.n);
        f.count = 0; f.apex = -1; f.aq[0] = f.aq[1] = f.aq[2] = 0; f.live = true;
        const int id = (int)faces.size();
        edge[key(u, v)] = id; edge[key(v, w)] = id; edge[key(w, u)] = id;
        faces.push_back(f);
        HullFaceRec r;
        memcpy(r.n, f.n, sizeof(r.n)); memcpy(r.a, f.q[0], 12); r.pad = 0;
        recs.push_back(r);
    }

    // step 4's last two lines: the first simplex from i0..i3 (idx, q), wound so that the fourth point is not outside face 0
    void start(const int idx[4], const int q[4][3])
    {
        faces.clear(); edge.clear(); recs.clear(); cursor = 0; outside = 0; insertions = 0; first_new = 0;
        int i[4] = {idx[0], idx[1], idx[2], idx[3]};
        const int* p[4] = {q[0], q[1], q[2], q[3]};
        long long n[3];
        hull_normal(p[0], p[1], p[2], n);
        if (hull_side(n, p[0], p[3]) > 0) { std::swap(i[1], i[2]); std::swap(p[1], p[2]); }
        add_face(i[0], i[1], i[2], p[0], p[1], p[2]);
        add_face(i[0], i[3], i[1], p[0], p[3], p[1]);
        add_face(i[1], i[3], i[2], p[1], p[3], p[2]);
        add_face(i[2], i[3], i[0], p[2], p[3], p[0]);
    }

    // the reports for `recs`, in their order
    void report(const HullReport* r)
    {
        for (size_t k = 0; k < recs.size(); ++k) {
            Face& f = faces[(size_t)first_new + k];
            f.count = r[k].count; f.apex = r[k].apex; memcpy(f.aq, r[k].q, 12);
            outside += f.count;
        }
    }

    // step 6.1: the lowest-numbered live face with an outside point; false when there is none
    bool next(int& F)
    {
        while (cursor < faces.size() && !(faces[cursor].live && faces[cursor].count > 0)) ++cursor;
        if (cursor == faces.size()) return false;
        F = (int)cursor;
        return true;
    }

    // steps 6.3 .. 6.6 for the apex of face F: fills `recs` / `first_new` with the new faces.  Returns 0, or -1 when the table is not the
    // closed surface it must be (a directed edge without a twin, a face its own apex does not see: cannot happen with honest reports)
    int insert(int F)
    {
        const int apex = faces[(size_t)F].apex;
        int aq[3];
        memcpy(aq, faces[(size_t)F].aq, 12);
        visible.clear();
        vis.assign(faces.size(), 0);
        for (size_t f = 0; f < faces.size(); ++f)
            if (faces[f].live && hull_side(faces[f].n, faces[f].q[0], aq) > 0) { visible.push_back((int)f); vis[f] = 1; }
        if (apex < 0 || !vis[(size_t)F]) return -1;         // (its own apex is outside F: anything else is a broken report)
        fresh.clear();
        for (int f : visible)
            for (int sl = 0; sl < 3; ++sl) {
                const int u = faces[(size_t)f].v[sl], v = faces[(size_t)f].v[(sl + 1) % 3];
                const auto it = edge.find(key(v, u));
                if (it == edge.end()) return -1;
                if (!vis[(size_t)it->second]) { fresh.push_back(f); fresh.push_back(sl); }
            }
        // the horizon's corner coordinates are copied before the table grows (add_face may move the faces)
        std::vector<int> hq(fresh.size() / 2 * 8);
        for (size_t k = 0; k < fresh.size() / 2; ++k) {
            const Face& f = faces[(size_t)fresh[2 * k]];
            const int sl = fresh[2 * k + 1], s1 = (sl + 1) % 3;
            hq[8 * k] = f.v[sl]; hq[8 * k + 1] = f.v[s1];
            memcpy(&hq[8 * k + 2], f.q[sl], 12); memcpy(&hq[8 * k + 5], f.q[s1], 12);
        }
        for (int f : visible) {
            Face& d = faces[(size_t)f];
            d.live = false; outside -= d.count; d.count = 0;
            for (int sl = 0; sl < 3; ++sl) edge.erase(key(d.v[sl], d.v[(sl + 1) % 3]));
        }
        recs.clear();
        first_new = (int)faces.size();
        for (size_t k = 0; k < hq.size() / 8; ++k) add_face(hq[8 * k], hq[8 * k + 1], apex, &hq[8 * k + 2], &hq[8 * k + 5], aq);
        ++insertions;
        return 0;
    }

    // step 7: the live faces in ascending number [faces][3], the ascending list of the indices they name
    void result(std::vector<int>& verts, std::vector<int>& tris) const
    {
        verts.clear(); tris.clear();
        for (const Face& f : faces) if (f.live) { tris.push_back(f.v[0]); tris.push_back(f.v[1]); tris.push_back(f.v[2]); }
        verts = tris;
        std::sort(verts.begin(), verts.end());
        verts.erase(std::unique(verts.begin(), verts.end()), verts.end());
    }
};

// Steps 5 and 6 over a points' side B:
//   int B.rehome(initial, apex, aq, first_new, n_new, recs, outside, reports)
// initial: every finite point is placed on the lowest-numbered of the faces recs[0 .. n_new) it is outside of (step 5); otherwise the points
// of the faces the apex (index, quantised coordinates aq) sees are placed on the new faces, the apex itself leaves (step 6.7).  outside: the
// points in outside sets before the call.  It fills reports[0 .. n_new) and returns 0, or an error the loop hands on.
// The loop itself returns -2 when the face table lost an edge's twin.
template <class Backend>
int hull_plan_run(HullPlan& P, Backend& B)
{
    std::vector<HullReport> rep(P.recs.size());
    const int none[3] = {0, 0, 0};
    int r = B.rehome(true, -1, none, 0, (int)P.recs.size(), P.recs.data(), 0ll, rep.data());
    if (r != 0) return r;
    P.report(rep.data());
    int F;
    while (P.next(F)) {
        const int apex = P.faces[(size_t)F].apex;
        int aq[3];
        memcpy(aq, P.faces[(size_t)F].aq, 12);
        const long long before = P.outside;
        if (P.insert(F) != 0) return -2;
        rep.resize(P.recs.size());
        r = B.rehome(false, apex, aq, P.first_new, (int)P.recs.size(), P.recs.data(), before, rep.data());
        if (r != 0) return r;
        P.report(rep.data());
    }
    return 0;
}

// ---- the inside test's planes (nsk_lattice_in_hull) --------------------------------------------------------------------------------
// xyz [nv][3] the hull vertices' fp32 coordinates in ascending index order, tris [nf][3] positions in that list.  c: the sum of the
// widened coordinates in that order, left to right, divided by the count; V' = c + scale * (V - c); per face u = B' - A', v = C' - A',
// n = u x v, each product and each difference rounded on its own.  planes [nf][6] = (n, A'); box [6] = the V's lower and upper corner.
// Contraction is switched off for this function alone (a pragma at file scope would reach every kernel that follows in nsk.hip).
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
inline void hull_mask_planes(int nv, const float* xyz, int nf, const int* tris, double scale, std::vector<double>& planes, double box[6])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    std::vector<double> V((size_t)nv * 3);
    double c[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < nv; ++i) for (int a = 0; a < 3; ++a) c[a] = c[a] + (double)xyz[3 * (size_t)i + a];
    for (int a = 0; a < 3; ++a) {
        c[a] = c[a] / (double)nv;
        box[a] = std::numeric_limits<double>::infinity(); box[3 + a] = -std::numeric_limits<double>::infinity();
    }
    for (int i = 0; i < nv; ++i) for (int a = 0; a < 3; ++a) {
        const double d = (double)xyz[3 * (size_t)i + a] - c[a];
        const double t = scale * d;
        const double w = c[a] + t;
        V[3 * (size_t)i + a] = w;
        box[a] = std::min(box[a], w); box[3 + a] = std::max(box[3 + a], w);
    }
    planes.assign((size_t)nf * 6, 0.0);
    for (int f = 0; f < nf; ++f) {
        const double* A = &V[3 * (size_t)tris[3 * f]]; const double* Bv = &V[3 * (size_t)tris[3 * f + 1]]; const double* C = &V[3 * (size_t)tris[3 * f + 2]];
        const double u[3] = {Bv[0] - A[0], Bv[1] - A[1], Bv[2] - A[2]}, v[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
        double* p = &planes[6 * (size_t)f];
        const double a0 = u[1] * v[2], a1 = u[2] * v[1], b0 = u[2] * v[0], b1 = u[0] * v[2], c0 = u[0] * v[1], c1 = u[1] * v[0];
        p[0] = a0 - a1; p[1] = b0 - b1; p[2] = c0 - c1;
        p[3] = A[0]; p[4] = A[1]; p[5] = A[2];
    }
}

// rigid_test -- csrc/nsk_rigid.h alone (no torch, no HIP): the rigid solve from pair sums on clouds under known motions, a planar cloud whose
// plain SVD answer would be a reflection, collinear and single-point sums, no pair at all, and the 4x4 product.  Built with AddressSanitizer
// + UndefinedBehaviorSanitizer; exit 0 when every case holds (tests/test_icp_cpu.py).
#include <cmath>
#include <cstdio>
#include <vector>

#include "nsk_rigid.h"

static int g_bad = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_bad; std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static unsigned long long g_state = 0x243F6A8885A308D3ull;
static double uni()           // [0, 1)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) * (1.0 / 9007199254740992.0);
}

static void rodrigues(double deg, const double* axis, const double* trans, double* M)
{
    const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    const double a[3] = {axis[0] / n, axis[1] / n, axis[2] / n}, th = deg * 3.14159265358979323846 / 180.0, c = std::cos(th), s = std::sin(th);
    nsk_rigid::identity4(M);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[4 * i + j] = (i == j ? c : 0.0) + (1 - c) * a[i] * a[j];
    M[1] -= s * a[2]; M[2] += s * a[1]; M[4] += s * a[2]; M[6] -= s * a[0]; M[8] -= s * a[1]; M[9] += s * a[0];
    for (int i = 0; i < 3; ++i) M[4 * i + 3] = trans[i];
}

static void add_pair(std::vector<double>& sums, const double* s, const double* t)
{
    sums[0] += 1.0;
    for (int a = 0; a < 3; ++a) {
        sums[1] += (s[a] - t[a]) * (s[a] - t[a]); sums[2 + a] += s[a]; sums[5 + a] += t[a];
        for (int b = 0; b < 3; ++b) sums[8 + 3 * a + b] += s[a] * t[b];
    }
}
// the sums of n points spread(k) under the motion M: t = M s exactly in double
template <class F> static std::vector<double> sums_under(const double* M, int n, F spread)
{
    std::vector<double> sums(17, 0.0);
    for (int k = 0; k < n; ++k) {
        double s[3], t[3];
        spread(s);
        for (int a = 0; a < 3; ++a) t[a] = M[4 * a] * s[0] + M[4 * a + 1] * s[1] + M[4 * a + 2] * s[2] + M[4 * a + 3];
        add_pair(sums, s, t);
    }
    return sums;
}

static double proper(const double* U)        // the largest of |R^T R - I| and |det - 1|, inf when an entry is not finite
{
    double R[9], worst = 0;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[3 * i + j] = U[4 * i + j];
    for (int k = 0; k < 16; ++k) if (!(std::fabs(U[k]) < INFINITY)) return INFINITY;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0;
            for (int k = 0; k < 3; ++k) d += R[3 * k + i] * R[3 * k + j];
            worst = std::fmax(worst, std::fabs(d - (i == j ? 1.0 : 0.0)));
        }
    return std::fmax(worst, std::fabs(nsk_rigid::det3(R) - 1.0));
}
static double differ(const double* A, const double* B)
{
    double w = 0;
    for (int k = 0; k < 16; ++k) w = std::fmax(w, std::fabs(A[k] - B[k]));
    return w;
}

int main()
{
    double U[16], M[16], I[16];
    int rank = -1;
    nsk_rigid::identity4(I);
    // known motions, small and large, on full clouds
    const double motions[][7] = {{1.5, 0.5, -0.3, 0.8, 0.012, -0.011, 0.012}, {30, 1, 2, -1, 0.3, -0.2, 0.5}, {179, -1, 0.2, 0.1, -1, 2, 0.25},
                                 {0, 0, 0, 1, 0, 0, 0}, {90, 0, 0, 1, 0, 0, 0}, {120, 1, 1, 1, 0.1, 0.1, 0.1}};
    for (const auto& m : motions) {
        rodrigues(m[0], m + 1, m + 4, M);
        const std::vector<double> sums = sums_under(M, 1000, [](double* s) { for (int a = 0; a < 3; ++a) s[a] = 2 * uni() - 1; });
        EXPECT(nsk_rigid::from_sums(sums.data(), U, &rank) == 0, "rc");
        EXPECT(rank == 3, "rank %d", rank);
        EXPECT(differ(U, M) < 1e-12, "motion of %g degrees off by %.3g", m[0], differ(U, M));
        EXPECT(proper(U) < 1e-14, "not a rotation: %.3g", proper(U));
    }
    // a planar cloud: rank 2, and the sign of the third direction comes from the determinant, not from the data
    for (const auto& m : motions) {
        rodrigues(m[0], m + 1, m + 4, M);
        const std::vector<double> sums = sums_under(M, 500, [](double* s) { s[0] = 2 * uni() - 1; s[1] = uni(); s[2] = 0.25 * s[0] - 0.5 * s[1] + 0.1; });
        EXPECT(nsk_rigid::from_sums(sums.data(), U, &rank) == 0, "rc");
        EXPECT(rank == 2, "planar rank %d", rank);
        EXPECT(differ(U, M) < 1e-12, "planar motion of %g degrees off by %.3g", m[0], differ(U, M));
        EXPECT(proper(U) < 1e-14, "planar: not a rotation: %.3g", proper(U));
    }
    // a mirrored planar cloud: the best orthogonal map is a reflection, the answer must still be a rotation
    {
        std::vector<double> sums(17, 0.0);
        for (int k = 0; k < 500; ++k) {
            const double s[3] = {2 * uni() - 1, uni(), 0.0}, t[3] = {-s[0], s[1], 0.0};
            add_pair(sums, s, t);
        }
        EXPECT(nsk_rigid::from_sums(sums.data(), U, &rank) == 0, "rc");
        EXPECT(rank == 2 && proper(U) < 1e-14, "mirrored: rank %d, %.3g", rank, proper(U));
    }
    // collinear, and a single point: rank <= 1, a finite proper rotation all the same, and the means still map onto each other
    {
        rodrigues(20, motions[1] + 1, motions[1] + 4, M);
        const std::vector<double> line = sums_under(M, 300, [](double* s) { const double u = uni(); s[0] = u; s[1] = 1 - 2 * u; s[2] = 0.5 * u; });
        EXPECT(nsk_rigid::from_sums(line.data(), U, &rank) == 0, "rc");
        EXPECT(rank == 1 && proper(U) < 1e-14, "collinear: rank %d, %.3g", rank, proper(U));
        const std::vector<double> one = sums_under(M, 1, [](double* s) { s[0] = 0.3; s[1] = -0.2; s[2] = 0.9; });
        EXPECT(nsk_rigid::from_sums(one.data(), U, &rank) == 0, "rc");
        EXPECT(rank == 0 && proper(U) < 1e-14, "one point: rank %d, %.3g", rank, proper(U));
        double moved = 0;
        for (int a = 0; a < 3; ++a) moved = std::fmax(moved, std::fabs(U[4 * a] * 0.3 + U[4 * a + 1] * -0.2 + U[4 * a + 2] * 0.9 + U[4 * a + 3] - one[5 + a]));
        EXPECT(moved < 1e-14, "one point lands %.3g off", moved);
        // the same point many times: the covariance is rounding noise or zero
        const std::vector<double> same = sums_under(M, 1000, [](double* s) { s[0] = 0.3; s[1] = -0.2; s[2] = 0.9; });
        EXPECT(nsk_rigid::from_sums(same.data(), U, &rank) == 0 && proper(U) < 1e-14, "repeated point: %.3g", proper(U));
    }
    // no pair: the identity; a sum that is not finite: refused
    {
        std::vector<double> none(17, 0.0);
        EXPECT(nsk_rigid::from_sums(none.data(), U, &rank) == 0 && rank == 0 && differ(U, I) == 0.0, "count 0");
        none[0] = 5; none[9] = NAN;
        EXPECT(nsk_rigid::from_sums(none.data(), U, &rank) == -1 && differ(U, I) == 0.0, "a NaN sum");
    }
    // the 4x4 product: against the identity, and the composition of two motions applied to a point
    {
        double A[16], B[16], AB[16];
        rodrigues(30, motions[1] + 1, motions[1] + 4, A); rodrigues(77, motions[2] + 1, motions[2] + 4, B);
        nsk_rigid::mul4(A, I, AB); EXPECT(differ(AB, A) == 0.0, "A I");
        nsk_rigid::mul4(I, A, AB); EXPECT(differ(AB, A) == 0.0, "I A");
        nsk_rigid::mul4(A, B, AB);
        const double p[4] = {0.3, -0.7, 0.2, 1.0};
        double q[4], r[4], w = 0;
        for (int i = 0; i < 4; ++i) q[i] = B[4 * i] * p[0] + B[4 * i + 1] * p[1] + B[4 * i + 2] * p[2] + B[4 * i + 3] * p[3];
        for (int i = 0; i < 4; ++i) r[i] = A[4 * i] * q[0] + A[4 * i + 1] * q[1] + A[4 * i + 2] * q[2] + A[4 * i + 3] * q[3];
        for (int i = 0; i < 4; ++i) w = std::fmax(w, std::fabs(AB[4 * i] * p[0] + AB[4 * i + 1] * p[1] + AB[4 * i + 2] * p[2] + AB[4 * i + 3] * p[3] - r[i]));
        EXPECT(w < 1e-15 && AB[15] == 1.0 && AB[12] == 0.0, "(A B) p off by %.3g", w);
    }
    std::printf(g_bad ? "rigid_test: %d checks failed\n" : "rigid_test: ok\n", g_bad);
    return g_bad ? 1 : 0;
}

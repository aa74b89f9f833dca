// nsk_rigid.h -- the rigid motion that best maps one point set onto another, from their pair sums (Umeyama / Kabsch without scaling), and
// the 4x4 product the ICP loop accumulates it with.  Host only, double, no HIP and no torch: host/test/rigid_test.cpp compiles it alone.
// (include/nsk.h states the rule: nsk_rigid_from_sums, nsk_cloud_icp.)
#pragma once
#include <cmath>

namespace nsk_rigid {

// out = A B for row-major 4x4 matrices: out[i][j] = ((A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]) + A[i][3] B[3][j], every product
// and sum an operation of its own, k ascending.  out may be neither A nor B.
inline void mul4(const double* A, const double* B, double* out)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            volatile double acc = A[4 * i] * B[j];               // (volatile: the compiler may not contract the product into the next sum)
            for (int k = 1; k < 4; ++k) { volatile double p = A[4 * i + k] * B[4 * k + j]; acc = acc + p; }
            out[4 * i + j] = acc;
        }
}

inline void identity4(double* M)
{
    for (int k = 0; k < 16; ++k) M[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

inline double det3(const double* A)          // row-major 3x3
{
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// The singular value decomposition C = U diag(sig) V^T of a row-major 3x3 by one-sided cyclic Jacobi: plane rotations from the right make
// the columns of C V orthogonal; their lengths are the singular values, sorted to descend.  V is orthogonal to rounding whatever C is.
// The columns of U that belong to singular values at or below tol sig[0] carry no direction of their own and are completed to a
// right-handed orthonormal basis.  Returns the numerical rank: the singular values above tol sig[0] that are also above `floor`, the size
// below which the caller knows C to be the rounding of its own formation (0 for the zero matrix).
inline int svd3(const double* C, double* U, double* sig, double* V, double floor = 0.0, double tol = 1e-12)
{
    double A[9], W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) A[k] = C[k];
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool turned = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) { al += A[3 * i + p] * A[3 * i + p]; be += A[3 * i + q] * A[3 * i + q]; ga += A[3 * i + p] * A[3 * i + q]; }
                if (ga == 0.0 || std::fabs(ga) <= 1e-17 * std::sqrt(al * be)) continue;
                turned = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[3 * i + p], aq = A[3 * i + q];
                    A[3 * i + p] = cs * ap - sn * aq; A[3 * i + q] = sn * ap + cs * aq;
                    const double wp = W[3 * i + p], wq = W[3 * i + q];
                    W[3 * i + p] = cs * wp - sn * wq; W[3 * i + q] = sn * wp + cs * wq;
                }
            }
        if (!turned) break;
    }
    double len[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) len[j] = std::sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2 - a; ++b)
            if (len[ord[b]] < len[ord[b + 1]]) { const int t = ord[b]; ord[b] = ord[b + 1]; ord[b + 1] = t; }
    int rank = 0;
    for (int j = 0; j < 3; ++j) {
        sig[j] = len[ord[j]];
        for (int i = 0; i < 3; ++i) V[3 * i + j] = W[3 * i + ord[j]];
        if (sig[j] > floor && sig[j] > tol * sig[0]) ++rank;       // (descending: the counted ones come first)
    }
    for (int j = 0; j < rank; ++j)
        for (int i = 0; i < 3; ++i) U[3 * i + j] = A[3 * i + ord[j]] / sig[j];
    if (rank == 0) { for (int k = 0; k < 9; ++k) U[k] = (k % 4 == 0) ? 1.0 : 0.0; return 0; }
    if (rank == 1) {
        // a unit vector orthogonal to u0: the axis on which u0 is smallest, its part along u0 removed
        int m = 0;
        for (int i = 1; i < 3; ++i) if (std::fabs(U[3 * i]) < std::fabs(U[3 * m])) m = i;
        double v[3] = {0, 0, 0}, n2 = 0;
        v[m] = 1.0;
        const double d = U[3 * m];
        for (int i = 0; i < 3; ++i) { v[i] -= d * U[3 * i]; n2 += v[i] * v[i]; }
        for (int i = 0; i < 3; ++i) U[3 * i + 1] = v[i] / std::sqrt(n2);
    }
    // u2 = +-(u0 x u1): with three singular values the sign of the third column, whose own direction carries the rounding of the two larger
    // ones magnified by sig[0] / sig[2]; without a third, a right-handed basis
    const double x[3] = {U[3] * U[7] - U[6] * U[4], U[6] * U[1] - U[0] * U[7], U[0] * U[4] - U[3] * U[1]};
    const double sgn = rank == 3 && x[0] * U[2] + x[1] * U[5] + x[2] * U[8] < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i) U[3 * i + 2] = sgn * x[i];
    return rank;
}

// sums[17] as nsk_cloud_pair_sums leaves them: [0] the count n, [1] sum d^2 (not read), [2..4] sum s, [5..7] sum t, [8..16] sum s_a t_b row-major.
// C = sum s t^T / n - mu_s mu_t^T = Us diag(sig) V^T;  R = V diag(1, 1, det(V Us^T)) Us^T maps s onto t;  trans = mu_t - R mu_s.
// U4 (row-major 4x4) = [R trans; 0 0 0 1].  *rank = the numerical rank of C: 2 or 3 determine R, 0 or 1 still give a proper rotation (the
// caller's `degenerate`).  A count that is not positive gives the identity and rank 0.  Returns 0, or -1 when a sum is not finite.
inline int from_sums(const double* sums, double* U4, int* rank)
{
    identity4(U4);
    if (rank) *rank = 0;
    for (int k = 0; k < 17; ++k) if (!(std::fabs(sums[k]) < INFINITY)) return -1;
    const double n = sums[0];
    if (!(n > 0.0)) return 0;
    double ms[3], mt[3], C[9], Us[9], sig[3], V[9], R[9];
    for (int a = 0; a < 3; ++a) { ms[a] = sums[2 + a] / n; mt[a] = sums[5 + a] / n; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[3 * a + b] = sums[8 + 3 * a + b] / n - ms[a] * mt[b];
    double scale = 0.0;                                         // C is a difference of terms of this size: below 1e-14 of it, it is rounding
    for (int k = 0; k < 9; ++k) scale = std::fmax(scale, std::fabs(sums[8 + k] / n));
    const int rk = svd3(C, Us, sig, V, 1e-14 * scale);
    if (rank) *rank = rk;
    double VUt[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) VUt[3 * i + j] = V[3 * i] * Us[3 * j] + V[3 * i + 1] * Us[3 * j + 1] + V[3 * i + 2] * Us[3 * j + 2];
    const double d = det3(VUt) < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = V[3 * i] * Us[3 * j] + V[3 * i + 1] * Us[3 * j + 1] + d * V[3 * i + 2] * Us[3 * j + 2];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) U4[4 * i + j] = R[3 * i + j];
        U4[4 * i + 3] = mt[i] - (R[3 * i] * ms[0] + R[3 * i + 1] * ms[1] + R[3 * i + 2] * ms[2]);
    }
    return 0;
}

}  // namespace nsk_rigid

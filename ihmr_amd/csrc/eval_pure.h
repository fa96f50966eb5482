// Pure arithmetic of the Procrustes-aligned metrics (csrc/evaluate.h inlines it) -- compilable for the HOST as well, like render_pure.h
// and augment_pure.h: under hipcc `__host__ __device__`, under g++ ordinary inline functions (tests/test_pa_metrics_cpu.py builds
// tests/eval_pure_driver.cpp with -fsanitize=address,undefined and compares the aligned points with the float64 SVD statement of
// tests/pa_cases.py).  Reference: utils/metric_utils.py:59-104 (calc_transform), read with the points in ROWS.  float64 throughout,
// every operation a single IEEE binary64 +, -, *, / or sqrt (compile with -ffp-contract=off).
//
//   statement  x1 = p - mean1, x2 = g - mean2 over the n valid points;  M[a][b] = sum x1_a * x2_b;  var1 = sum |x1|^2.
//              R = the proper rotation (det +1) that maximises sum x2 . (R x1) = trace(R K), K = M;  scale = trace(R K) / var1;
//              t = mean2 - scale * R * mean1;  the aligned point is scale * R * p + t.
//   route      Horn's closed form (J. Opt. Soc. Am. A 4, 1987): trace(R K) = q^T N q for the unit quaternion q of R, N the symmetric
//              4 x 4 matrix below, so q is the eigenvector of N's largest eigenvalue lambda and scale = lambda / var1.  The search runs
//              over rotations only, so the reflection branch of the SVD form (det(U V^T) < 0) needs no special case, and a
//              rank-deficient M (3, 2 or 1 points, a planar set) yields a rotation like any other: where the largest eigenvalue is
//              multiple, every eigenvector of it gives the same aligned points wherever var1 > 0 of them are spanned.
//   solver     cyclic Jacobi, EVP_SWEEPS sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair whose off-diagonal entry is
//              exactly 0 is skipped.  Every index is a compile-time constant and no entry is chosen by a run-time select: the two
//              4 x 4 arrays live in registers (tests/test_pa_metrics_cpu.py reads private_segment_fixed_size == 0 of both kernels).
//   degenerate M = 0 leaves N = 0: q = (1,0,0,0), R = I, scale = 0.  var1 = 0 returns scale = 0 (the caller leaves such a set out).
// Nothing here touches memory other than its arguments.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define EVP_PURE __host__ __device__ __forceinline__
#else
#define EVP_PURE static inline
#endif

#define EVP_SWEEPS 12

// the SET RULES shared by host and device: a point is valid when its weight is > 0; a set is left out when the sum of its weights is
// < 2.0 (metric_utils.py:131 takes the sum, not the count) or when var1 == 0 (the reference divides by zero there)
#define EVP_MIN_WEIGHT_SUM 2.0

typedef struct evp_transform { double R[3][3]; double scale; double t[3]; } evp_transform;

// row K of one Jacobi rotation of the pair (P, Q): the entries of A outside the 2 x 2 block, and V
template <int P, int Q, int K>
EVP_PURE void evp_rotate_row(double (&A)[4][4], double (&V)[4][4], double c, double s) {
    if (K != P && K != Q) {
        const double akp = A[K][P], akq = A[K][Q];
        A[K][P] = c * akp - s * akq;
        A[P][K] = A[K][P];
        A[K][Q] = s * akp + c * akq;
        A[Q][K] = A[K][Q];
    }
    const double vkp = V[K][P], vkq = V[K][Q];
    V[K][P] = c * vkp - s * vkq;
    V[K][Q] = s * vkp + c * vkq;
}

// one Jacobi rotation of the pair (P, Q): A <- J^T A J, V <- V J
template <int P, int Q>
EVP_PURE void evp_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double mag = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double t = theta < 0.0 ? -mag : mag;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
    evp_rotate_row<P, Q, 0>(A, V, c, s);
    evp_rotate_row<P, Q, 1>(A, V, c, s);
    evp_rotate_row<P, Q, 2>(A, V, c, s);
    evp_rotate_row<P, Q, 3>(A, V, c, s);
}

EVP_PURE evp_transform procrustes_from_moments(double n, const double* mean1, const double* mean2, const double (*M)[3], double var1) {
    (void)n;
    const double Sxx = M[0][0], Sxy = M[0][1], Sxz = M[0][2], Syx = M[1][0], Syy = M[1][1], Syz = M[1][2], Szx = M[2][0], Szy = M[2][1],
                 Szz = M[2][2];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
#if defined(__HIPCC__)
#pragma nounroll
#endif
    for (int sweep = 0; sweep < EVP_SWEEPS; ++sweep) {
        evp_rotate<0, 1>(A, V);
        evp_rotate<0, 2>(A, V);
        evp_rotate<0, 3>(A, V);
        evp_rotate<1, 2>(A, V);
        evp_rotate<1, 3>(A, V);
        evp_rotate<2, 3>(A, V);
    }
    // the largest eigenvalue, ties to the lowest index.  Its column of V is blended with factors that are exactly 1 and 0 (V is an
    // orthogonal matrix: every entry is finite, so x * 1 + y * 0 is x): a select between two entries of V would be compiled into one
    // load at a run-time address, which puts the whole array into scratch memory on the device
    int best = 0;
    double lam = A[0][0];
    if (A[1][1] > lam) { lam = A[1][1]; best = 1; }
    if (A[2][2] > lam) { lam = A[2][2]; best = 2; }
    if (A[3][3] > lam) { lam = A[3][3]; best = 3; }
    const double b0 = best == 0 ? 1.0 : 0.0, b1 = best == 1 ? 1.0 : 0.0, b2 = best == 2 ? 1.0 : 0.0, b3 = best == 3 ? 1.0 : 0.0;
    double q0 = ((V[0][0] * b0 + V[0][1] * b1) + V[0][2] * b2) + V[0][3] * b3;
    double q1 = ((V[1][0] * b0 + V[1][1] * b1) + V[1][2] * b2) + V[1][3] * b3;
    double q2 = ((V[2][0] * b0 + V[2][1] * b1) + V[2][2] * b2) + V[2][3] * b3;
    double q3 = ((V[3][0] * b0 + V[3][1] * b1) + V[3][2] * b2) + V[3][3] * b3;
    const double nq = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    if (nq > 0.0) { q0 = q0 / nq; q1 = q1 / nq; q2 = q2 / nq; q3 = q3 / nq; } else { q0 = 1.0; q1 = 0.0; q2 = 0.0; q3 = 0.0; }
    evp_transform T;
    T.R[0][0] = 1.0 - 2.0 * (q2 * q2 + q3 * q3); T.R[0][1] = 2.0 * (q1 * q2 - q3 * q0);       T.R[0][2] = 2.0 * (q1 * q3 + q2 * q0);
    T.R[1][0] = 2.0 * (q1 * q2 + q3 * q0);       T.R[1][1] = 1.0 - 2.0 * (q1 * q1 + q3 * q3); T.R[1][2] = 2.0 * (q2 * q3 - q1 * q0);
    T.R[2][0] = 2.0 * (q1 * q3 - q2 * q0);       T.R[2][1] = 2.0 * (q2 * q3 + q1 * q0);       T.R[2][2] = 1.0 - 2.0 * (q1 * q1 + q2 * q2);
    T.scale = var1 > 0.0 ? lam / var1 : 0.0;
    T.t[0] = mean2[0] - T.scale * ((T.R[0][0] * mean1[0] + T.R[0][1] * mean1[1]) + T.R[0][2] * mean1[2]);
    T.t[1] = mean2[1] - T.scale * ((T.R[1][0] * mean1[0] + T.R[1][1] * mean1[1]) + T.R[1][2] * mean1[2]);
    T.t[2] = mean2[2] - T.scale * ((T.R[2][0] * mean1[0] + T.R[2][1] * mean1[1]) + T.R[2][2] * mean1[2]);
    return T;
}

// |scale * R * p + t - g|
EVP_PURE double evp_aligned_error(const evp_transform& T, const double* p, const double* g) {
    const double dx = (T.scale * ((T.R[0][0] * p[0] + T.R[0][1] * p[1]) + T.R[0][2] * p[2]) + T.t[0]) - g[0];
    const double dy = (T.scale * ((T.R[1][0] * p[0] + T.R[1][1] * p[1]) + T.R[1][2] * p[2]) + T.t[1]) - g[1];
    const double dz = (T.scale * ((T.R[2][0] * p[0] + T.R[2][1] * p[1]) + T.R[2][2] * p[2]) + T.t[2]) - g[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// scale * R * p + t, the operations of evp_aligned_error in the same order
EVP_PURE void evp_aligned_point(const evp_transform& T, const double* p, double* out) {
    out[0] = T.scale * ((T.R[0][0] * p[0] + T.R[0][1] * p[1]) + T.R[0][2] * p[2]) + T.t[0];
    out[1] = T.scale * ((T.R[1][0] * p[0] + T.R[1][1] * p[1]) + T.R[1][2] * p[2]) + T.t[1];
    out[2] = T.scale * ((T.R[2][0] * p[0] + T.R[2][1] * p[1]) + T.R[2][2] * p[2]) + T.t[2];
}

// ------------------------------------------------------------------------------------------ curve metrics: PCK counts and F-scores
// The THRESHOLD INDEX of a value v in an ascending table t[0..T): the number of thresholds that v exceeds.  Thresholds ascend, so
// the exceeded ones are t[0..idx) and the comparison holds for every k >= idx: a histogram over idx, summed from the left, is the
// count per threshold.  Two forms:
//   evp_threshold_index         idx = #{k : !(v <= t[k])}     v <= t[k] for k >= idx     (PCK: the comparison is non-strict)
//   evp_threshold_index_strict  idx = #{k : !(v <  t[k])}     v <  t[k] for k >= idx     (F-score, collision AUC: strict)
// A NaN satisfies no comparison and gets idx = T.  Binary search over memory (at most 9 probes for T <= 256): `t` is a pointer into
// LDS or global memory on the device, never a register array that a run-time index would push into scratch memory.
EVP_PURE int evp_threshold_index(double v, const double* t, int T) {
    int lo = 0, hi = T;                       // t[0..lo) exceeded, t[hi..T) not
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v <= t[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

EVP_PURE int evp_threshold_index_strict(double v, const double* t, int T) {
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v < t[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// |a - b|^2 in the one bracketed order that host and device share: (dx * dx + dy * dy) + dz * dz.  The nearest-neighbour search
// takes the minimum of these (exact, so the order of the search cannot change a bit) and the root once
EVP_PURE double evp_sq_dist(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// F = 2 P R / (P + R) of one hand from its two counts, P = n_pg / n and R = n_gp / n; 0 when P + R = 0
EVP_PURE double evp_fscore(double n_pg, double n_gp, double n) {
    const double P = n_pg / n, R = n_gp / n;
    return P + R > 0.0 ? 2.0 * P * R / (P + R) : 0.0;
}

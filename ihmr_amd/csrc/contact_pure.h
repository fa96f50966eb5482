// Pure arithmetic of the interacting-hand metrics -- MRRPE and contact consistency (csrc/evaluate.h inlines it) -- compilable for the
// HOST as well, like eval_pure.h and volume_pure.h: under hipcc `__host__ __device__`, under g++ ordinary inline functions
// (tests/test_contact_metrics_cpu.py builds tests/contact_host_driver.cpp with -fsanitize=address,undefined and compares every word with
// the float64 statement of tests/contact_cases.py).  float64 throughout on the float32 inputs, every operation a single IEEE binary64
// +, -, *, / or sqrt (compile with -ffp-contract=off).
//
//   statement    Every squared distance is evp_sq_dist, every distance one root, divided by the
//              sample's scale before it is compared or summed.
//              MRRPE    e = |(P[21] - P[0]) - (G[21] - G[0])| / scale, counted when the weights of both wrists are > 0.
//              pairs    d_X(i, j) = sqrt(sq_dist(R_X[i], L_X[j])) / scale for X in {pred, gt};  C = {(i, j) : d_gt(i, j) < tau_c}
//                       (strict);  a sample leaves [sum over C of d_pred, |C|].
//              maps     near_X(right, i) = min_j d_X(i, j), near_X(left, j) = min_i d_X(i, j): the minimum on the squares, one root;
//                       a NaN never replaces the running minimum, a vertex without a comparable partner keeps +inf.  A vertex is in
//                       contact at tau_k when near < tau_k (strict); per threshold tp = in contact in both, pp = in pred, gp = in gt.
//   order      The float64 pair sum has one order: a thread owns the query vertices tid, tid + 256, tid + 512, tid + 768 (its slots);
//              each slot adds its d_pred over j ascending, the thread adds its slots ascending, ((s0 + s1) + s2) + s3, and the 256
//              thread sums go through block_sum_f64 (csrc/evaluate.h): xor butterfly 32, 16, .. 1 over each wave of 64, then the four
//              waves ((w0 + w1) + w2) + w3.  ctp_block_sum restates that for the host.
// Nothing here touches memory other than its arguments.
#pragma once
#include "eval_pure.h"

#define CTP_NV 778
#define CTP_THREADS 256
#define CTP_SLOTS 4                       // 778 = 3 * 256 + 10: the fourth slot exists for the first 10 threads only
#define CTP_MAX_K 8                       // IHMR_EVAL_MAX_CONTACT_THRESHOLDS
// LDS of eval_contact_kernel: the other hand of both mesh pairs (six arrays of 778 doubles), the threshold table, the partial sums of
// block_sum_f64, three histograms over the threshold index and the pair count
#define CTP_LDS_BYTES (6 * CTP_NV * 8 + CTP_MAX_K * 8 + 4 * 10 * 8 + 3 * (CTP_MAX_K + 1) * 4 + 4)      // 37 840

// The MRRPE of one sample: the error of the vector from the right wrist (joint 0) to the left wrist (joint 21).  p0, p21, g0, g21 are
// xyz; false (e = 0) when a wrist weight is not > 0.  A non-finite input gives a non-finite e, which is counted.
EVP_PURE bool ctp_mrrpe(const double* p0, const double* p21, const double* g0, const double* g21, double w0, double w21, double sc,
                        double& e) {
    e = 0.0;
    if (!(w0 > 0.0 && w21 > 0.0)) return false;
    e = sqrt(evp_sq_dist(p21[0] - p0[0], p21[1] - p0[1], p21[2] - p0[2], g21[0] - g0[0], g21[1] - g0[1], g21[2] - g0[2])) / sc;
    return true;
}

// A distance from its square: one root, then the division by the sample's scale.
EVP_PURE double ctp_dist(double sq, double sc) { return sqrt(sq) / sc; }

// The pair predicate, literally: d_gt(i, j) < tau_c.  A NaN distance is never in contact.
EVP_PURE bool ctp_pair_in_contact(double sq_gt, double sc, double tau) { return ctp_dist(sq_gt, sc) < tau; }

// The kernel's filter on SQUARES in front of the predicate: a limit L with   sq > L  ==>  !(sqrt(sq) / sc < tau),   so a pair above
// it needs neither root nor division.  +inf (nothing is filtered, every pair takes the literal expression) wherever the proof below
// does not hold: a scale that is not a positive finite number, a threshold that is not positive, t = tau * sc below 1e-100 (t * t
// would lose its relative accuracy) or a limit that is not finite.
//   proof   t = fl(tau * sc) = tau sc (1 + a), |a| <= 2^-53.  L = fl(fl(t * t) * (1 + 2^-20)) >= t^2 (1 + 2^-20)(1 - 2^-52).  For
//           sq > L: sqrt(sq) > t (1 + 2^-22), so fl(sqrt(sq)) >= t (1 + 2^-22)(1 - 2^-53), and the exact quotient by sc is
//           >= tau (1 + a)(1 + 2^-22)(1 - 2^-53) > tau.  tau is a double and rounding is monotone: fl(quotient) >= tau.
//   The margin 2^-20 costs nothing: the pairs between the threshold and the limit take the literal expression.  A NaN square fails
//   `sq > L` and takes the literal expression too, which is false for it.
EVP_PURE double ctp_pair_limit(double tau, double sc) {
    const double inf = (double)INFINITY;
    if (!(sc > 0.0) || !(sc <= 1.7976931348623157e308) || !(tau > 0.0) || !(tau <= 1.7976931348623157e308)) return inf;
    const double t = tau * sc;
    if (!(t >= 1e-100)) return inf;
    const double L = (t * t) * (1.0 + 9.5367431640625e-07);        // 2^-20
    return L <= 1.7976931348623157e308 ? L : inf;
}

// The filtered predicate the kernel evaluates: the same decision as ctp_pair_in_contact for every input.
EVP_PURE bool ctp_pair_in_contact_filtered(double sq_gt, double sc, double tau, double limit) {
    if (sq_gt > limit) return false;
    return ctp_pair_in_contact(sq_gt, sc, tau);
}

// The running minimum over squared distances: a NaN satisfies no comparison and never replaces it.  Starts at +inf.
EVP_PURE double ctp_min_update(double best, double sq) { return sq < best ? sq : best; }

// The contact decision of one vertex against the ascending table thr[0..K): idx = the number of thresholds that `near` does not lie
// below, so the vertex is in contact (near < thr[k], strict) exactly for k >= idx.  NaN: idx = K, never in contact.
EVP_PURE int ctp_contact_index(double near, const double* thr, int K) { return evp_threshold_index_strict(near, thr, K); }

// A vertex is in contact in both mesh pairs at tau_k exactly for k >= max(idx_pred, idx_gt).
EVP_PURE int ctp_both_index(int idx_pred, int idx_gt) { return idx_pred > idx_gt ? idx_pred : idx_gt; }

// The sum of a workgroup's 256 thread values in the order of block_sum_f64 (host restatement; the device uses block_sum_f64 itself).
EVP_PURE double ctp_block_sum(const double* v) {
    double w[4];
    for (int wave = 0; wave < 4; ++wave) {
        double a[64];
        for (int l = 0; l < 64; ++l) a[l] = v[wave * 64 + l];
        for (int o = 32; o > 0; o >>= 1) {
            double b[64];
            for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ o];
            for (int l = 0; l < 64; ++l) a[l] = b[l];
        }
        w[wave] = a[0];
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}

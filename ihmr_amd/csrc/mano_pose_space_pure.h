// Pure arithmetic of the MANO layer's pose space and output stage (csrc/mano_pose_space.h inlines it) -- compilable for the HOST as well,
// like surface_pure.h: under hipcc `__host__ __device__`, under g++ ordinary inline functions (tests/test_mano_space_cpu.py builds
// tests/mano_space_driver.cpp with -fsanitize=address,undefined).  float32 unless stated, every operation a single IEEE operation
// (compile with -ffp-contract=off; the fused multiply-adds below are written as fmaf and are meant).
//
//   PCA forward   pose45[n][i] = sum_k coeffs[n][k] C[k][i], C = hands_components[:K] (K,45): ONE fmaf chain per element, k ascending
//                 from 0.0f -- acc = fmaf(c_k, C_ki, acc) -- so an element's bits depend on its own hand's K coefficients and on
//                 nothing else  (mps_fma_chain with a = the hand's coefficients, b = column i of C).
//   PCA backward  d_coeffs[n][k] = sum_i d_pose45[n][i] C[k][i]: the same chain, i ascending over 45  (a = the hand's d_pose45 row,
//                 b = row k of C).
//   translation   out = in + transl[n][c]: one float32 addition per coordinate; without a translation the value passes through
//                 unchanged (no addition: -0.0f stays -0.0f)  (mps_shift).
//   tips          joints_out[n][16 + t] = the translated vertex tip_ids[t]; a tip id outside [0, 778) gives a row of zeros forward and
//                 adds nothing backward  (mps_tip_ok).
//   d_transl      d_transl[n][c] = sum over the hand's MPS_ROWS(J) = 778 + J rows -- the 778 rows of d_verts_out, then the J = 16 or 21
//                 rows of d_joints_out -- in float64 in ONE order: thread t of 256 adds its rows t, t + 256, .. ascending from 0.0
//                 (mps_thread_rows), the 256 thread sums go through block_sum_f64 (csrc/evaluate.h; ctp_block_sum of contact_pure.h
//                 restates it for the host), one rounding to float32 at the end.
// Nothing here touches memory other than its arguments.
#pragma once
#include "eval_pure.h"

#define MPS_POSE 45                       // hand-pose parameters = columns of hands_components
#define MPS_VERTS 778
#define MPS_JOINTS 16
#define MPS_TIPS 5
#define MPS_THREADS 256
#define MPS_TILE 16                       // hands per workgroup of the two PCA kernels
#define MPS_C_STRIDE 45                   // floats per row of C in LDS: odd, so the backward's walk along k-rows visits 32 distinct banks
// LDS of mano_pca_fwd_kernel / mano_pca_bwd_kernel: C (45 rows of MPS_C_STRIDE floats) and the tile's (16 hands x 45) input rows
#define MPS_PCA_LDS_BYTES (MPS_POSE * MPS_C_STRIDE * 4 + MPS_TILE * MPS_POSE * 4)                    // 10 980
// LDS of mano_post_bwd_kernel: the four waves' partial sums of block_sum_f64 (rows of 10 doubles, its own layout)
#define MPS_POST_BWD_LDS_BYTES (4 * 10 * 8)                                                          // 320

#define MPS_ROWS(J) (MPS_VERTS + (J))     // rows of a hand that d_transl sums: 794 without tips, 799 with

// sum_{j < n} a[j * sa] * b[j * sb] as one fmaf chain, j ascending from 0.0f.
EVP_PURE float mps_fma_chain(const float* a, int sa, const float* b, int sb, int n) {
    float acc = 0.0f;
    for (int j = 0; j < n; ++j) acc = fmaf(a[j * sa], b[j * sb], acc);
    return acc;
}

// One coordinate through the output stage: with a translation one float32 addition, without one the value itself.
EVP_PURE float mps_shift(float x, bool has_transl, float t) { return has_transl ? x + t : x; }

EVP_PURE bool mps_tip_ok(int id) { return id >= 0 && id < MPS_VERTS; }

// Thread `tid`'s float64 partial sums of d_transl over its rows tid, tid + 256, .. < 778 + J (ascending): rows below 778 come from
// d_verts_out (778,3), the others from d_joints_out (J,3), both of ONE hand.
EVP_PURE void mps_thread_rows(const float* d_verts_out, const float* d_joints_out, int J, int tid, double* acc) {
    acc[0] = 0.0; acc[1] = 0.0; acc[2] = 0.0;
    for (int r = tid; r < MPS_ROWS(J); r += MPS_THREADS) {
        const float* row = r < MPS_VERTS ? d_verts_out + 3 * r : d_joints_out + 3 * (r - MPS_VERTS);
        acc[0] += (double)row[0]; acc[1] += (double)row[1]; acc[2] += (double)row[2];
    }
}

/*
 * ihmr_mano_ext.h -- C ABI of libihmr_hip.so, second header: the pose space and the output stage of the MANO layer (seam A).
 *
 * ihmr_hip.h declares the one call the reference makes of its MANO layer (smplx.create(..., use_pca=False) and
 * mano_model(global_orient, hand_pose (N,45), betas): models/optimize_model.py:105-106, 194-198).  The four entry points below are what
 * the published smplx MANO.forward does around that call for every other caller: the PCA pose space (use_pca=True, num_pca_comps), the
 * translation (transl) and the fingertip vertices the reference appends itself (optimize_model.py:99, 201-202).  Parity with smplx is
 * unpinned, as for the rest of seam A.  They run before and after ihmr_mano_lbs_fwd / ihmr_mano_lbs_bwd, which do
 * not change; the arithmetic is stated in ihmr_amd/csrc/mano_pose_space_pure.h.
 *
 * Conventions: those of ihmr_hip.h.  extern "C", returns int: 0 = ok, -1 and nothing launched for a bad argument (a NULL required
 * pointer, N < 1, K outside 1..45), otherwise a hipError_t value.  Every pointer is a DEVICE pointer owned by the caller, row-major
 * contiguous fp32 (ids int32); asynchronous on the given hipStream_t (passed as void*); no allocation, no synchronisation,
 * graph-capture safe.  A hand's words do not depend on N or on its place in the batch, and two runs give the same bits.
 */
#ifndef IHMR_MANO_EXT_H
#define IHMR_MANO_EXT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IHMR_MANO_POSE_DIM 45   /* hand-pose parameters: the most PCA components, the columns of `comps` */

/* ------------------------------------------------------------------ seam A: the PCA pose space */
/* smplx MANO.forward with use_pca=True: hand_pose (N,K) coefficients -> pose45 (N,45) = coeffs . comps, comps = hands_components[:K]
 * (K,45), 1 <= K <= 45.  One fmaf chain per element, k ascending from 0.  The hand mean is added by ihmr_mano_lbs_fwd, as ever. */
int ihmr_mano_pca_fwd(const float* coeffs, const float* comps, int N, int K, float* pose45, void* stream);
/* backward of the above: d_pose45 (N,45) -> d_coeffs (N,K) = d_pose45 . comps^T, one fmaf chain per element, i ascending. */
int ihmr_mano_pca_bwd(const float* d_pose45, const float* comps, int N, int K, float* d_coeffs, void* stream);

/* ------------------------------------------------------------------ seam A: translation and fingertips */
/* smplx `transl` and the reference's tip append (optimize_model.py:201-202): verts_in (N,778,3), joints16_in (N,16,3) ->
 * verts_out (N,778,3) = verts_in + transl[n], joints_out (N,J,3) = the 16 joints + transl[n], then -- with tip_ids (5) -- the five
 * translated vertices tip_ids[t]: J = 21 with tip_ids, 16 with NULL.  transl (N,3) NULL: no addition, the values pass through bit for
 * bit.  A tip id outside [0, 778) gives a row of zeros.  verts_out == verts_in (in place) is allowed; joints_out must not overlap
 * joints16_in. */
int ihmr_mano_post_fwd(const float* verts_in, const float* joints16_in, const float* transl, const int32_t* tip_ids, int N,
                       float* verts_out, float* joints_out, void* stream);
/* backward of the above: d_verts_out (N,778,3), d_joints_out (N,J,3) (J as in the forward: tip_ids decides) -> d_verts_in (N,778,3)
 * = d_verts_out with every tip row of d_joints_out added at its vertex, d_joints16 (N,16,3) = the first 16 rows of d_joints_out, and
 * -- unless d_transl is NULL -- d_transl (N,3) = the sum of the hand's 778 + J rows, accumulated in float64 in one fixed order and
 * rounded once. */
int ihmr_mano_post_bwd(const float* d_verts_out, const float* d_joints_out, const int32_t* tip_ids, int N, float* d_verts_in,
                       float* d_joints16, float* d_transl, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* IHMR_MANO_EXT_H */

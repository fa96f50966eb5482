// Evaluation metrics on the device: the four numbers the reference prints after a run (optimize.py:98-102) --
// mpjpe_3d, inter_mpjpe_3d, collision_ave, collision_max -- as per-sample partial results that the host adds up
// in float64 (and all-reduces over ranks, ihmr_amd/dist.py) -- and, at the end of this file, the Procrustes-aligned errors
// (PA-MPJPE / PA-MPVPE, utils/metric_utils.py:59-104) that the reference carries as calc_transform.
//
// Reference: utils/metric_utils.py:23-38 (get_single_joints_error: per-hand MPJPE with the root subtraction
// applied CUMULATIVELY to the same copies), :107-117 (calc_transform_no_rot: per-axis mean / std alignment),
// :120-143 (get_single_pa_inter_joints_error, use_rot=False), utils/evaluator.py:149-181 (collision_ave / _max =
// mean / max of the 1556 per-vertex depths x 1000, over samples whose hand_type is 'interacting').
#pragma once
#include "ihmr_common.h"
#include "eval_pure.h"
#include "contact_pure.h"

// ------------------------------------------------------------------------------------------ what the kernels of this file share
// Every sum has one fixed order (lane-strided partials, xor butterfly over the wave, waves in index order), so a sample's result does
// not depend on its place in the batch.
__device__ __forceinline__ double wave_reduce_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Joint j of sample b in the arithmetic type T of the caller: prediction, target and weight; zeros for the lanes j >= 42.
template <typename T>
__device__ __forceinline__ void load_joint(const float* __restrict__ pred, const float* __restrict__ gt, int b, int j,
                                           T (&p)[3], T (&g)[3], T& w) {
    p[0] = p[1] = p[2] = g[0] = g[1] = g[2] = w = (T)0;
    if (j < 42) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = (T)pred[((size_t)b * 42 + j) * 3 + k]; g[k] = (T)gt[((size_t)b * 42 + j) * 4 + k]; }
        w = (T)gt[((size_t)b * 42 + j) * 4 + 3];
    }
}

// Per-hand root-relative joint error (metric_utils.py:23-38), one wave, lane j: root 0 is subtracted for joints 0..20, then -- on the
// already shifted copies a, g, which the caller gives up -- root 21.  Lane j counts (true, err = |a - g| / sc) when its hand's root and
// its own weight are > 0; err is 0 otherwise.
template <typename T>
__device__ __forceinline__ bool root_relative_joint_error(int j, T w, T (&a)[3], T (&g)[3], T sc, T& err) {
    bool counted = false;
    err = (T)0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int root = 21 * h;
        if (__shfl(w, root) > (T)0) {     // uniform over the wave
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[k] -= __shfl(a[k], root); g[k] -= __shfl(g[k], root); }
            if (j >= root && j < root + 21 && w > (T)0) {
                const T dx = a[0] - g[0], dy = a[1] - g[1], dz = a[2] - g[2];
                err = sqrt((dx * dx + dy * dy) + dz * dz) / sc;
                counted = true;
            }
        }
    }
    return counted;
}

// Sums over a workgroup of 256 (four waves) of the first K of a thread's float64 accumulators: butterfly over the wave, lane 0 to
// part[wave][k], one barrier, the waves added as ((p0 + p1) + p2) + p3; every thread gets every sum.  The caller keeps a barrier
// between these reads of `part` and its next write.
template <int K, int N>
__device__ __forceinline__ void block_sum_f64(const double (&acc)[N], double (*part)[10], double (&sum)[N]) {
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_reduce_sum_f64(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) sum[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
}

// Hand h of sample b in the vertex kernels (grid = (B, 2)): its predicted and target mesh; true when the hand counts, i.e. a GT mesh
// exists (mano_params_weight[b][h] > 0).
__device__ __forceinline__ bool eval_hand(const float* __restrict__ pred_r, const float* __restrict__ pred_l, const float* __restrict__ gt_r,
                                          const float* __restrict__ gt_l, const float* __restrict__ params_weight, int b, int h,
                                          const float*& P, const float*& G) {
    P = (h ? pred_l : pred_r) + (size_t)b * NV3;
    G = (h ? gt_l : gt_r) + (size_t)b * NV3;
    return params_weight[b * 2 + h] > 0.f;
}

// grid = B, block = 64: lane j < 42 owns joint j.  out (B,6) doubles:
//   [0] sum of per-joint errors, [1] number of them, [2] sum of aligned ("inter") errors, [3] number of them,
//   [4] mean penetration depth [mm], [5] max penetration depth [mm]  ([4],[5] = 0 and not counted unless interacting)
// The rules are the reference's, literally (statement and case classes: tests/metric_cases.py): a joint counts when its weight is > 0,
// a hand when its root does; the aligned error is left out when the SUM of the 42 weights is < 2.0, else [3] = the number of w > 0
// joints and [2] is NaN where the reference divides 0 / 0 (one joint, or no spread of the prediction on an axis); a NaN depth makes
// both [4] and [5] NaN.  Float32 arithmetic, sums in butterfly order: a sample's six words do not depend on its place in the batch.
__global__ __launch_bounds__(64) void eval_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const float* __restrict__ coll, const float* __restrict__ scale,
                                                          const unsigned char* __restrict__ interacting, int B,
                                                          double* __restrict__ out) {
    const int b = blockIdx.x, j = threadIdx.x;
    const bool act = j < 42;
    float a[3], g[3], w;
    load_joint(pred, gt, b, j, a, g, w);
    const float sc = scale ? scale[b] : 1.0f;
    const float p0[3] = {a[0], a[1], a[2]}, g0[3] = {g[0], g[1], g[2]};   // un-shifted copies for the aligned error

    // ---- per-hand MPJPE (metric_utils.py:23-38)
    float err;
    const bool counted = root_relative_joint_error(j, w, a, g, sc, err);
    const double err_sum = (double)wave_reduce_sum(err), err_n = (double)wave_reduce_sum(counted ? 1.f : 0.f);

    // ---- aligned error over all valid joints (metric_utils.py:107-143, no rotation): p' = (p - mean p) / std p * std g + mean g
    // The sample is left out when the SUM of its 42 weights is < 2.0 (metric_utils.py:131; EVP_MIN_WEIGHT_SUM), not by the number n of
    // its w > 0 joints.  A kept set without spread on an axis (n = 1; equal predicted coordinates) divides 0 / 0 like the reference:
    // every joint of the set gets NaN and the set still counts.
    const bool valid = act && w > 0.f;
    const float n = wave_reduce_sum(valid ? 1.f : 0.f);
    const bool kept = wave_reduce_sum(act ? w : 0.f) >= (float)EVP_MIN_WEIGHT_SUM;     // uniform over the wave; implies n >= 1
    float ierr = 0.f;
    if (kept) {
        float d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float mp = wave_reduce_sum(valid ? p0[k] : 0.f) / n, mg = wave_reduce_sum(valid ? g0[k] : 0.f) / n;
            const float dp = p0[k] - mp, dg = g0[k] - mg;
            const float sp = sqrtf(wave_reduce_sum(valid ? dp * dp : 0.f) / n), sg = sqrtf(wave_reduce_sum(valid ? dg * dg : 0.f) / n);
            d[k] = (dp / sp * sg + mg) - g0[k];
        }
        if (valid) ierr = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / sc;
    }
    const double ierr_sum = (double)wave_reduce_sum(ierr);

    // ---- penetration depth statistics of the 1556 per-vertex values [mm]
    double csum = 0.0;
    float cmax = -INFINITY;
    bool cnan = false;          // fmaxf drops a NaN, np.max (evaluator.py:173) returns it: a NaN depth makes the maximum NaN
    const bool inter = interacting ? interacting[b] != 0 : true;
    if (inter) {
        for (int v = j; v < 2 * NV; v += 64) {
            const float x = coll[(size_t)b * 2 * NV + v];
            csum += (double)x;
            cmax = fmaxf(cmax, x);
            cnan |= x != x;
        }
    }
    const double cs = wave_reduce_sum_f64(csum);
    const float cm = __ballot(cnan) != 0ull ? NAN : wave_reduce_max(cmax);
    if (j == 0) {
        double* o = out + (size_t)b * 6;
        o[0] = err_sum; o[1] = err_n;
        o[2] = kept ? ierr_sum : 0.0; o[3] = kept ? (double)n : 0.0;
        o[4] = inter ? cs / (double)(2 * NV) * 1000.0 : 0.0;
        o[5] = inter ? (double)cm * 1000.0 : 0.0;
    }
}

// MPVPE partial sums (BASELINE.json's metric list; the reference exports the meshes -- baseline_model.py:365-368,
// mlp_model.py:708-711 -- and has no vertex metric of its own).  Same convention as the MPJPE above: per hand,
// root-relative, L2 per point, / scale; the root of a mesh is its wrist regressed with row 0 of the MANO joint
// regressor (root_w (2,778): right, left).  A hand counts when mano_params_weight[b][h] > 0 (a GT mesh exists).
// grid = (B, 2), block = 256.  out (B,2,2) doubles: per hand [sum of the per-vertex errors, number of them].
__global__ __launch_bounds__(256) void eval_mpvpe_kernel(const float* __restrict__ pred_r, const float* __restrict__ pred_l,
                                                         const float* __restrict__ gt_r, const float* __restrict__ gt_l,
                                                         const float* __restrict__ root_w, const float* __restrict__ params_weight,
                                                         const float* __restrict__ scale, int B, double* __restrict__ hand_out) {
    __shared__ float part[4][8];
    __shared__ float root[6];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    double* o = hand_out + ((size_t)b * 2 + h) * 2;
    const float *P, *G;
    if (!eval_hand(pred_r, pred_l, gt_r, gt_l, params_weight, b, h, P, G)) {
        if (tid == 0) { o[0] = 0.0; o[1] = 0.0; }
        return;
    }
    const float* W = root_w + (size_t)h * NV;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int v = tid; v < NV; v += 256) {
        const float w = W[v];
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[k] += w * P[3 * v + k]; acc[3 + k] += w * G[3 * v + k]; }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float s = wave_reduce_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (tid < 6) root[tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    __syncthreads();
    const float sc = scale ? scale[b] : 1.0f;
    float err = 0.f;
    for (int v = tid; v < NV; v += 256) {
        const float dx = (P[3 * v] - root[0]) - (G[3 * v] - root[3]);
        const float dy = (P[3 * v + 1] - root[1]) - (G[3 * v + 1] - root[4]);
        const float dz = (P[3 * v + 2] - root[2]) - (G[3 * v + 2] - root[5]);
        err += sqrtf(dx * dx + dy * dy + dz * dz) / sc;
    }
    const float s = wave_reduce_sum(err);
    __syncthreads();
    if (lane == 0) part[wave][0] = s;
    __syncthreads();
    if (tid == 0) { o[0] = ((double)part[0][0] + (double)part[1][0]) + ((double)part[2][0] + (double)part[3][0]); o[1] = (double)NV; }
}

// ------------------------------------------------------------------------------------------ Procrustes-aligned errors (PA-MPJPE / PA-MPVPE)
// utils/metric_utils.py:59-104 (calc_transform) and :120-143 (get_single_pa_inter_joints_error, use_rot=True), read with the points
// in rows; the arithmetic and the set rules are csrc/eval_pure.h.  Inputs float32, every operation float64, no atomics.

// One joint set of one sample, one wave: `in_set` marks the lanes whose joint belongs to the set, a member is one of them with w > 0.
// Returns the lane's aligned error / sc (0 for a non-member and for a set left out), n = the number of members, kept = the set counts.
__device__ __forceinline__ double pa_joint_set_error(bool in_set, double w, const double (&p)[3], const double (&g)[3], double sc,
                                                     double& n, bool& kept) {
    const bool member = in_set && w > 0.0;
    const double wsum = wave_reduce_sum_f64(in_set ? w : 0.0);
    n = wave_reduce_sum_f64(member ? 1.0 : 0.0);
    double err = 0.0;
    kept = false;
    if (wsum >= EVP_MIN_WEIGHT_SUM && n > 0.0) {          // uniform over the wave
        double m1[3], m2[3], x1[3], x2[3], M[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            m1[k] = wave_reduce_sum_f64(member ? p[k] : 0.0) / n;
            m2[k] = wave_reduce_sum_f64(member ? g[k] : 0.0) / n;
            x1[k] = member ? p[k] - m1[k] : 0.0;
            x2[k] = member ? g[k] - m2[k] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[a][c] = wave_reduce_sum_f64(x1[a] * x2[c]);
        const double var1 = wave_reduce_sum_f64((x1[0] * x1[0] + x1[1] * x1[1]) + x1[2] * x1[2]);
        if (var1 > 0.0) {
            kept = true;
            const evp_transform T = procrustes_from_moments(n, m1, m2, M, var1);
            if (member) err = evp_aligned_error(T, p, g) / sc;
        }
    }
    return err;
}

// grid = B, block = 64: lane j < 42 owns joint j.  Three sets per sample: 0 = all valid joints (the reference's call), 1 = the valid
// joints of the right hand (0..20), 2 = those of the left hand (21..41).  out (B,3,2) doubles [sum of errors, count];
// point_err (B,3,42) doubles or NULL: the aligned error of a set's member, 0 for every other joint and for a set left out.
__global__ __launch_bounds__(64) void eval_pa_joints_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                            const float* __restrict__ scale, int B, double* __restrict__ out,
                                                            double* __restrict__ point_err) {
    const int b = blockIdx.x, j = threadIdx.x;
    const bool act = j < 42;
    double p[3], g[3], w;
    load_joint(pred, gt, b, j, p, g, w);
    const double sc = scale ? (double)scale[b] : 1.0;
#pragma nounroll
    for (int s = 0; s < 3; ++s) {
        const int lo = s == 2 ? 21 : 0, hi = s == 1 ? 21 : 42;
        double n;
        bool kept;
        const double err = pa_joint_set_error(act && j >= lo && j < hi, w, p, g, sc, n, kept);
        const double esum = wave_reduce_sum_f64(err);
        if (point_err && act) point_err[((size_t)b * 3 + s) * 42 + j] = err;
        if (j == 0) {
            double* o = out + ((size_t)b * 3 + s) * 2;
            o[0] = kept ? esum : 0.0;
            o[1] = kept ? n : 0.0;
        }
    }
}

// The transform of one hand's 778 vertices, all valid, by one workgroup of 256: two passes over the mesh (means, centred moments) with
// `part` (4,10) doubles of LDS between them.  False when var1 == 0 (the set is left out); every thread returns the same T.
__device__ __forceinline__ bool pa_verts_transform(const float* __restrict__ P, const float* __restrict__ G, double (*part)[10],
                                                   evp_transform& T) {
    const int tid = threadIdx.x;
    double acc[10], sum[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int v = tid; v < NV; v += 256) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[k] += (double)P[3 * v + k]; acc[3 + k] += (double)G[3 * v + k]; }
    }
    block_sum_f64<6>(acc, part, sum);
    double m1[3], m2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { m1[k] = sum[k] / (double)NV; m2[k] = sum[3 + k] / (double)NV; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int v = tid; v < NV; v += 256) {
        double x1[3], x2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { x1[k] = (double)P[3 * v + k] - m1[k]; x2[k] = (double)G[3 * v + k] - m2[k]; }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[3 * a + c] += x1[a] * x2[c];
        acc[9] += (x1[0] * x1[0] + x1[1] * x1[1]) + x1[2] * x1[2];
    }
    block_sum_f64<10>(acc, part, sum);
    double M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[a][c] = sum[3 * a + c];
    const double var1 = sum[9];
    __syncthreads();
    if (!(var1 > 0.0)) return false;
    T = procrustes_from_moments((double)NV, m1, m2, M, var1);
    return true;
}

// grid = (B, 2), block = 256: one hand's 778 vertices, all valid; the hand counts when mano_params_weight[b][h] > 0.  Three passes over
// the mesh: means, centred moments, errors.  out (B,2,2) doubles [sum of errors, count]; point_err (B,2,778) doubles or NULL.
__global__ __launch_bounds__(256) void eval_pa_verts_kernel(const float* __restrict__ pred_r, const float* __restrict__ pred_l,
                                                            const float* __restrict__ gt_r, const float* __restrict__ gt_l,
                                                            const float* __restrict__ params_weight, const float* __restrict__ scale,
                                                            int B, double* __restrict__ out, double* __restrict__ point_err) {
    __shared__ double part[4][10];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    double* o = out + ((size_t)b * 2 + h) * 2;
    double* pe = point_err ? point_err + ((size_t)b * 2 + h) * NV : nullptr;
    const float *P, *G;
    evp_transform T;
    const bool kept = eval_hand(pred_r, pred_l, gt_r, gt_l, params_weight, b, h, P, G) && pa_verts_transform(P, G, part, T);      // uniform over the block
    if (!kept) {
        if (pe) for (int v = tid; v < NV; v += 256) pe[v] = 0.0;
        if (tid == 0) { o[0] = 0.0; o[1] = 0.0; }
        return;
    }
    const double sc = scale ? (double)scale[b] : 1.0;
    double esum[1] = {0.0}, total[1];
    for (int v = tid; v < NV; v += 256) {
        const double p[3] = {(double)P[3 * v], (double)P[3 * v + 1], (double)P[3 * v + 2]};
        const double g[3] = {(double)G[3 * v], (double)G[3 * v + 1], (double)G[3 * v + 2]};
        const double e = evp_aligned_error(T, p, g) / sc;
        esum[0] += e;
        if (pe) pe[v] = e;
    }
    block_sum_f64<1>(esum, part, total);
    if (tid == 0) { o[0] = total[0]; o[1] = (double)NV; }
}

// ------------------------------------------------------------------------------------------ curve metrics: PCK counts, F-score counts
// The other half of a hand-mesh result table: per threshold tau_k the NUMBER of points whose error is <= tau_k (the host divides and
// integrates: PCK curve and its AUC), and per hand the number of nearest-neighbour distances < tau (precision / recall of the F-score).
// A point's thresholds are found once -- its threshold index (csrc/eval_pure.h), a binary search over the table in LDS -- and
// counted into an integer histogram in LDS (integer atomics: the result has no order); the histogram summed from the left is the
// count per threshold.  Inputs float32, every operation float64, no float atomics, every float sum in one fixed order; a sample's
// (hand's) result does not depend on its place in the batch.  Counts are written as doubles: they add over batches and ranks with the
// other metric sums.
#define EVAL_MAX_T IHMR_EVAL_MAX_THRESHOLDS        // 256
#define EVAL_MAX_F IHMR_EVAL_MAX_F_THRESHOLDS      // 8

// hist[0..T) in LDS -> out[k] = hist[0] + ... + hist[k] for k < T, out[T] = n.  One whole wave: lane l sums its run of
// ceil(T / 64) consecutive entries, the runs are scanned over the wave.
__device__ __forceinline__ void curve_emit_counts(const int* hist, int T, double n, double* __restrict__ out) {
    const int lane = threadIdx.x % WAVE, per = (T + WAVE - 1) / WAVE, base = lane * per;
    int local = 0;
    for (int i = 0; i < per; ++i)
        if (base + i < T) local += hist[base + i];
    int incl = local;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    int run = incl - local;
    for (int i = 0; i < per; ++i)
        if (base + i < T) { run += hist[base + i]; out[base + i] = (double)run; }
    if (lane == 0) out[T] = n;
}

// grid = B, block = 64: lane j < 42 owns joint j.  Three populations per sample:
//   0  j3d           the valid joints of a hand whose wrist is valid: get_single_joints_error in float64 (root 0 subtracted for the
//                    right hand, then -- on the already shifted copies -- root 21 for the left)
//   1  pa_inter_j3d  all valid joints, one alignment (the set 0 of eval_pa_joints_kernel)
//   2  pa_j3d        the valid joints, one alignment per hand (sets 1 + 2)
// counts (B,3,T+1) doubles: [#err <= tau_0 .. #err <= tau_{T-1}, number of points].  1 <= T <= EVAL_MAX_T, thresholds ascending.
__global__ __launch_bounds__(64) void eval_curve_joints_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               const float* __restrict__ scale, int B,
                                                               const double* __restrict__ thresholds, int T,
                                                               double* __restrict__ counts) {
    __shared__ double thr[EVAL_MAX_T];
    __shared__ int hist[3][EVAL_MAX_T + 1];
    const int b = blockIdx.x, j = threadIdx.x;
    const bool act = j < 42;
    for (int k = j; k < T; k += 64) thr[k] = thresholds[k];
    for (int k = j; k < 3 * (EVAL_MAX_T + 1); k += 64) (&hist[0][0])[k] = 0;
    double p[3], g[3], w;
    load_joint(pred, gt, b, j, p, g, w);
    const double sc = scale ? (double)scale[b] : 1.0;
    __syncthreads();

    double n[3] = {0.0, 0.0, 0.0};
    {   // ---- population 0
        double a[3] = {p[0], p[1], p[2]}, c[3] = {g[0], g[1], g[2]}, err;
        const bool counted = root_relative_joint_error(j, w, a, c, sc, err);
        if (counted) atomicAdd(&hist[0][evp_threshold_index(err, thr, T)], 1);
        n[0] = wave_reduce_sum_f64(counted ? 1.0 : 0.0);
    }
    // ---- populations 1 and 2: the three sets of eval_pa_joints_kernel
#pragma nounroll
    for (int s = 0; s < 3; ++s) {
        const int lo = s == 2 ? 21 : 0, hi = s == 1 ? 21 : 42;
        const bool in_set = act && j >= lo && j < hi;
        double ns;
        bool kept;
        const double err = pa_joint_set_error(in_set, w, p, g, sc, ns, kept);
        if (kept) {
            if (in_set && w > 0.0) atomicAdd(&hist[s == 0 ? 1 : 2][evp_threshold_index(err, thr, T)], 1);
            if (s == 0) n[1] += ns; else n[2] += ns;
        }
    }
    __syncthreads();
    double* o = counts + (size_t)b * 3 * (T + 1);
    curve_emit_counts(hist[0], T, n[0], o);
    curve_emit_counts(hist[1], T, n[1], o + (T + 1));
    curve_emit_counts(hist[2], T, n[2], o + 2 * (T + 1));
}

// The minimum squared distance from each of a thread's query points (slot s = vertex tid + 256 s) to the 778 targets held as three
// arrays in LDS.  Every lane reads the same target at the same time (a broadcast, no bank conflict) and one read serves all slots.
// 778 = 3 * 256 + 10: slot 3 exists for tid < 10 only, so only wave 0 walks it (`slot3` is uniform over a wave).
__device__ __forceinline__ void nn_min_sq(const double (&q)[4][3], const double* tx, const double* ty, const double* tz, bool slot3,
                                          double (&best)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) best[s] = INFINITY;
    for (int j = 0; j < NV; ++j) {
        const double x = tx[j], y = ty[j], z = tz[j];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const double d = evp_sq_dist(q[s][0], q[s][1], q[s][2], x, y, z);
            best[s] = d < best[s] ? d : best[s];
        }
        if (slot3) {
            const double d = evp_sq_dist(q[3][0], q[3][1], q[3][2], x, y, z);
            best[3] = d < best[3] ? d : best[3];
        }
    }
}

// grid = (B, 2), block = 256: one hand per workgroup; the hand counts when mano_params_weight[b][h] > 0.
//   counts   (B,2,2,T+1)    hand, then v3d (root-relative, the root = root_w . mesh, as get_single_verts_error) / pa_v3d (aligned, as
//                           eval_pa_verts_kernel): [#err <= tau_k ..., number of points]
//   f_counts (B,2,2,2,F)    hand, raw / pa, p->g / g->p, tau: the number of nearest-neighbour distances < tau  (NULL with F = 0)
//   nn_dist  (B,2,2,2,778)  the distances themselves, or NULL
// raw: p = P - root(P), g = G - root(G); pa: p = scale R P + t, g = G.  d_pg[i] = min_j |p_i - g_j| / sc, d_gp[j] = min_i |p_i - g_j| / sc:
// the minimum over squared distances, one root.  Four passes (raw p->g, raw g->p, pa p->g, pa g->p): the target set of a pass lies in
// LDS (3 x 778 doubles), each thread keeps its up to four query points in registers; between passes the roles swap.
// A hand that does not count writes zeros everywhere; a hand the PA rules leave out (var1 == 0) writes zeros in its pa halves.
__global__ __launch_bounds__(256) void eval_curve_verts_kernel(const float* __restrict__ pred_r, const float* __restrict__ pred_l,
                                                               const float* __restrict__ gt_r, const float* __restrict__ gt_l,
                                                               const float* __restrict__ root_w, const float* __restrict__ params_weight,
                                                               const float* __restrict__ scale, int B,
                                                               const double* __restrict__ thresholds, int T,
                                                               const double* __restrict__ f_thresholds, int F,
                                                               double* __restrict__ counts, double* __restrict__ f_counts,
                                                               double* __restrict__ nn_dist) {
    __shared__ double tx[NV], ty[NV], tz[NV];
    __shared__ double thr[EVAL_MAX_T], fthr[EVAL_MAX_F];
    __shared__ double part[4][10];
    __shared__ int hist[2][EVAL_MAX_T + 1];
    __shared__ int fhist[4][EVAL_MAX_F + 1];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, wave = tid / WAVE;
    const size_t hand = (size_t)b * 2 + h;
    double* o = counts + hand * 2 * (T + 1);
    double* fo = F > 0 ? f_counts + hand * 4 * F : nullptr;
    double* nd = nn_dist ? nn_dist + hand * 4 * NV : nullptr;
    const float *P, *G;
    if (!eval_hand(pred_r, pred_l, gt_r, gt_l, params_weight, b, h, P, G)) {         // uniform over the block
        for (int k = tid; k < 2 * (T + 1); k += 256) o[k] = 0.0;
        for (int k = tid; k < 4 * F; k += 256) fo[k] = 0.0;
        if (nd) for (int k = tid; k < 4 * NV; k += 256) nd[k] = 0.0;
        return;
    }
    for (int k = tid; k < T; k += 256) thr[k] = thresholds[k];
    for (int k = tid; k < F; k += 256) fthr[k] = f_thresholds[k];
    for (int k = tid; k < 2 * (EVAL_MAX_T + 1); k += 256) (&hist[0][0])[k] = 0;
    for (int k = tid; k < 4 * (EVAL_MAX_F + 1); k += 256) (&fhist[0][0])[k] = 0;
    const float* W = root_w + (size_t)h * NV;
    const double sc = scale ? (double)scale[b] : 1.0;

    // ---- the two roots, float64
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, root[6];
    for (int v = tid; v < NV; v += 256) {
        const double w = (double)W[v];
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[k] += w * (double)P[3 * v + k]; acc[3 + k] += w * (double)G[3 * v + k]; }
    }
    block_sum_f64<6>(acc, part, root);
    const double rootP[3] = {root[0], root[1], root[2]}, rootG[3] = {root[3], root[4], root[5]};
    __syncthreads();
    evp_transform T_pa;
    const bool kept_pa = pa_verts_transform(P, G, part, T_pa);      // uniform over the block

    // ---- the two error populations
    for (int v = tid; v < NV; v += 256) {
        const double p[3] = {(double)P[3 * v], (double)P[3 * v + 1], (double)P[3 * v + 2]};
        const double g[3] = {(double)G[3 * v], (double)G[3 * v + 1], (double)G[3 * v + 2]};
        const double e = sqrt(evp_sq_dist(p[0] - rootP[0], p[1] - rootP[1], p[2] - rootP[2], g[0] - rootG[0], g[1] - rootG[1], g[2] - rootG[2])) / sc;
        atomicAdd(&hist[0][evp_threshold_index(e, thr, T)], 1);
        if (kept_pa) atomicAdd(&hist[1][evp_threshold_index(evp_aligned_error(T_pa, p, g) / sc, thr, T)], 1);
    }

    // ---- the four nearest-neighbour passes
    if (F > 0 || nd) {
        // point v of the predicted (which = 0) or the target (which = 1) set of a variant (0 = raw, 1 = pa)
        auto point = [&](int variant, int which, int v, double* out) {
            const float* S = which ? G : P;
            const double x[3] = {(double)S[3 * v], (double)S[3 * v + 1], (double)S[3 * v + 2]};
            if (variant == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out[k] = x[k] - (which ? rootG[k] : rootP[k]);
            } else if (which == 0) {
                evp_aligned_point(T_pa, x, out);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) out[k] = x[k];
            }
        };
#pragma nounroll
        for (int pass = 0; pass < 4; ++pass) {
            const int variant = pass >> 1, dir = pass & 1;       // dir 0: the queries are p, the targets g; dir 1: the reverse
            if (variant == 1 && !kept_pa) {
                if (nd) for (int v = tid; v < NV; v += 256) nd[(size_t)pass * NV + v] = 0.0;
                continue;
            }
            __syncthreads();                                     // the pass before has read its targets
            for (int v = tid; v < NV; v += 256) {
                double t[3];
                point(variant, 1 - dir, v, t);
                tx[v] = t[0]; ty[v] = t[1]; tz[v] = t[2];
            }
            double q[4][3], best[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int v = tid + 256 * s;
                q[s][0] = 0.0; q[s][1] = 0.0; q[s][2] = 0.0;
                if (v < NV) point(variant, dir, v, q[s]);
            }
            __syncthreads();
            nn_min_sq(q, tx, ty, tz, wave == 0, best);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int v = tid + 256 * s;
                if (v < NV) {
                    const double d = sqrt(best[s]) / sc;
                    if (nd) nd[(size_t)pass * NV + v] = d;
                    if (F > 0) atomicAdd(&fhist[pass][evp_threshold_index_strict(d, fthr, F)], 1);
                }
            }
        }
    }
    __syncthreads();
    if (wave == 0) curve_emit_counts(hist[0], T, (double)NV, o);
    if (wave == 1) curve_emit_counts(hist[1], T, kept_pa ? (double)NV : 0.0, o + (T + 1));
    if (tid < 4 * F) {
        const int pass = tid / F, k = tid % F;
        int c = 0;
        for (int i = 0; i <= k; ++i) c += fhist[pass][i];
        fo[(size_t)pass * F + k] = (double)c;
    }
}

// ------------------------------------------------------------------------------------------ interacting-hand metrics: MRRPE, contact consistency
// How the two hands sit RELATIVE TO EACH OTHER, compared with the ground truth (there is no reference
// call site).  The arithmetic and the rules are csrc/contact_pure.h.  Inputs float32, every operation float64, no float atomics, every
// float sum in one fixed order: a sample's words do not depend on its place in the batch.

// grid = ceil(B / 64), block = 64: one thread per sample.  out (B,2) doubles [e, counted]: the error of the vector from the right
// wrist (joint 0) to the left wrist (joint 21), counted when both wrist weights are > 0 and the sample is interacting.
__global__ __launch_bounds__(64) void eval_mrrpe_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ scale, const unsigned char* __restrict__ interacting,
                                                        int B, double* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float* P = pred + (size_t)b * 42 * 3;
    const float* G = gt + (size_t)b * 42 * 4;
    double p0[3], p21[3], g0[3], g21[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { p0[k] = (double)P[k]; p21[k] = (double)P[21 * 3 + k]; g0[k] = (double)G[k]; g21[k] = (double)G[21 * 4 + k]; }
    const double sc = scale ? (double)scale[b] : 1.0;
    double e;
    const bool wrists = ctp_mrrpe(p0, p21, g0, g21, (double)G[3], (double)G[21 * 4 + 3], sc, e);
    const bool counted = wrists && (interacting ? interacting[b] != 0 : true);
    out[(size_t)b * 2] = counted ? e : 0.0;
    out[(size_t)b * 2 + 1] = counted ? 1.0 : 0.0;
}

struct ContactLds {
    double t[6][CTP_NV];                 // the OTHER hand: x, y, z of the predicted mesh, then of the target mesh
    double thr[CTP_MAX_K];
    double part[4][10];
    int hist[3][CTP_MAX_K + 1];          // over the threshold index: in contact in both, in pred, in gt
    int pairs;
};
static_assert(sizeof(ContactLds) == CTP_LDS_BYTES, "contact_pure.h names the LDS of eval_contact_kernel");

// One step of the walk: target j against slot s of the thread.  The squared distance is always sq_dist(right, left).
template <bool PAIRS>
__device__ __forceinline__ void contact_step(const double (&qp)[3], const double (&qg)[3], const double (&t)[6], bool valid, double sc,
                                             double tau, double limit, double& bp, double& bg, double& acc, int& npairs) {
    const double sp = PAIRS ? evp_sq_dist(qp[0], qp[1], qp[2], t[0], t[1], t[2]) : evp_sq_dist(t[0], t[1], t[2], qp[0], qp[1], qp[2]);
    const double sg = PAIRS ? evp_sq_dist(qg[0], qg[1], qg[2], t[3], t[4], t[5]) : evp_sq_dist(t[3], t[4], t[5], qg[0], qg[1], qg[2]);
    bp = ctp_min_update(bp, sp);
    bg = ctp_min_update(bg, sg);
    if (PAIRS && valid && ctp_pair_in_contact_filtered(sg, sc, tau, limit)) {
        acc += ctp_dist(sp, sc);
        ++npairs;
    }
}

// One walk over the 778 targets in LDS, j ascending.  Every lane reads the same target at the same time (a broadcast, no bank
// conflict) and one read serves all slots; slot 3 exists for tid < 10 only, so only wave 0 walks it (`slot3` is uniform over a wave).
template <bool PAIRS>
__device__ __forceinline__ void contact_walk(const ContactLds& s, const double (&qp)[CTP_SLOTS][3], const double (&qg)[CTP_SLOTS][3],
                                             bool slot3, bool valid3, double sc, double tau, double limit, double (&bp)[CTP_SLOTS],
                                             double (&bg)[CTP_SLOTS], double (&acc)[CTP_SLOTS], int& npairs) {
    for (int j = 0; j < NV; ++j) {
        const double t[6] = {s.t[0][j], s.t[1][j], s.t[2][j], s.t[3][j], s.t[4][j], s.t[5][j]};
#pragma unroll
        for (int k = 0; k < 3; ++k) contact_step<PAIRS>(qp[k], qg[k], t, true, sc, tau, limit, bp[k], bg[k], acc[k], npairs);
        if (slot3) contact_step<PAIRS>(qp[3], qg[3], t, valid3, sc, tau, limit, bp[3], bg[3], acc[3], npairs);
    }
}

// grid = (B, 2), block = 256: workgroup (b, h) owns the vertices of hand h (0 = right, 1 = left) as queries and holds the OTHER hand
// of both mesh pairs as targets in LDS.  A sample is counted when both mano_params_weight are > 0 and use[b] != 0 (use NULL: every row).
//   pair_out  (B,2,2)      [sum over C of d_pred, |C|] in the h = 0 row, zeros in the h = 1 row
//   count_out (B,2,K,3)    of hand h's 778 vertices per threshold: [in contact in both, in pred, in gt]
//   near      (B,2,2,778)  hand, pred / gt, vertex: the distance to the nearest vertex of the other hand; or NULL
// A sample that is not counted writes zeros everywhere and does no pair work.  1 <= K <= CTP_MAX_K, thresholds ascending;
// tau_c = thresholds[0].
__global__ __launch_bounds__(256) void eval_contact_kernel(const float* __restrict__ pred_r, const float* __restrict__ pred_l,
                                                           const float* __restrict__ gt_r, const float* __restrict__ gt_l,
                                                           const float* __restrict__ params_weight, const float* __restrict__ scale,
                                                           const unsigned char* __restrict__ use, int B,
                                                           const double* __restrict__ thresholds, int K, double* __restrict__ pair_out,
                                                           double* __restrict__ count_out, double* __restrict__ near) {
    __shared__ ContactLds s;
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, wave = tid / WAVE;
    const size_t hand = (size_t)b * 2 + h;
    double* po = pair_out + hand * 2;
    double* co = count_out + hand * 3 * K;
    double* nr = near ? near + hand * 2 * NV : nullptr;
    const bool counted = params_weight[b * 2] > 0.f && params_weight[b * 2 + 1] > 0.f && (use ? use[b] != 0 : true);   // uniform over the block
    if (!counted) {
        if (tid < 2) po[tid] = 0.0;
        if (tid < 3 * K) co[tid] = 0.0;
        if (nr) for (int k = tid; k < 2 * NV; k += 256) nr[k] = 0.0;
        return;
    }
    const float* Qp = (h ? pred_l : pred_r) + (size_t)b * NV3;
    const float* Qg = (h ? gt_l : gt_r) + (size_t)b * NV3;
    const float* Tp = (h ? pred_r : pred_l) + (size_t)b * NV3;
    const float* Tg = (h ? gt_r : gt_l) + (size_t)b * NV3;
    if (tid < K) s.thr[tid] = thresholds[tid];
    if (tid < 3 * (CTP_MAX_K + 1)) (&s.hist[0][0])[tid] = 0;
    if (tid == 0) s.pairs = 0;
    for (int v = tid; v < NV; v += 256) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { s.t[k][v] = (double)Tp[3 * v + k]; s.t[3 + k][v] = (double)Tg[3 * v + k]; }
    }
    double qp[CTP_SLOTS][3], qg[CTP_SLOTS][3], bp[CTP_SLOTS], bg[CTP_SLOTS], acc[CTP_SLOTS];
#pragma unroll
    for (int k = 0; k < CTP_SLOTS; ++k) {
        const int v = tid + 256 * k;
        bp[k] = INFINITY; bg[k] = INFINITY; acc[k] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { qp[k][c] = v < NV ? (double)Qp[3 * v + c] : 0.0; qg[k][c] = v < NV ? (double)Qg[3 * v + c] : 0.0; }
    }
    const double sc = scale ? (double)scale[b] : 1.0;
    const double tau = thresholds[0], limit = ctp_pair_limit(tau, sc);
    int npairs = 0;
    __syncthreads();
    if (h == 0) contact_walk<true>(s, qp, qg, wave == 0, tid + 768 < NV, sc, tau, limit, bp, bg, acc, npairs);
    else contact_walk<false>(s, qp, qg, wave == 0, tid + 768 < NV, sc, tau, limit, bp, bg, acc, npairs);
#pragma unroll
    for (int k = 0; k < CTP_SLOTS; ++k) {
        const int v = tid + 256 * k;
        if (v < NV) {
            const double np = ctp_dist(bp[k], sc), ng = ctp_dist(bg[k], sc);
            if (nr) { nr[v] = np; nr[NV + v] = ng; }
            const int ip = ctp_contact_index(np, s.thr, K), ig = ctp_contact_index(ng, s.thr, K);
            atomicAdd(&s.hist[0][ctp_both_index(ip, ig)], 1);
            atomicAdd(&s.hist[1][ip], 1);
            atomicAdd(&s.hist[2][ig], 1);
        }
    }
    if (npairs) atomicAdd(&s.pairs, npairs);
    const double mine[1] = {((acc[0] + acc[1]) + acc[2]) + acc[3]};
    double total[1];
    block_sum_f64<1>(mine, s.part, total);            // its barrier also orders the integer atomics above
    if (tid == 0) { po[0] = h == 0 ? total[0] : 0.0; po[1] = h == 0 ? (double)s.pairs : 0.0; }
    if (tid < 3 * K) {
        const int k = tid / 3, c = tid % 3;
        int n = 0;
        for (int i = 0; i <= k; ++i) n += s.hist[c][i];
        co[tid] = (double)n;
    }
}

// The MANO layer's pose space and output stage: four small kernels that run before and after the skinning launches of mano_lbs.h,
// which they leave alone (statement and arithmetic: mano_pose_space_pure.h; the entry points: include/ihmr_mano_ext.h).
//
//   mano_pca_fwd_kernel   coefficients (N,K) -> pose45 (N,45).  One workgroup per tile of MPS_TILE = 16 hands; C = comps (K,45) and the
//                         tile's coefficient rows are loaded into LDS once, then thread e of the tile's 16 x 45 outputs (whole waves up to
//                         the tile's end, the loop bound is the guard: no thread leaves before the barrier) forms ONE fmaf chain, k
//                         ascending.  Lanes read C along i: consecutive dwords (a row has 45 > 32 of them, so the two ends of a 32-lane
//                         group can meet on a bank, 2-way at the most); lanes of one hand read the same coefficient (a broadcast).
//   mano_pca_bwd_kernel   d_pose45 (N,45) -> d_coeffs (N,K), the same tiles; thread e of the tile's 16 x K outputs walks row k of C, i
//                         ascending.  Rows of C are MPS_C_STRIDE = 45 floats apart: odd, so lanes on consecutive k-rows hit distinct banks.
//   mano_post_fwd_kernel  one workgroup per hand, one pass over its 2334 vertex floats (coalesced dwords) and 48 joint floats: adds
//                         transl[n] (transl == NULL: the values pass through bit for bit), writes verts_out (N,778,3) and joints_out
//                         (N,J,3), J = 16, or 21 with tip_ids: the thread that owns a vertex float also writes it to the tip row that
//                         names its vertex, so a tip is the translated vertex's bits.  IN PLACE on the vertex buffer (verts_out ==
//                         verts_in) is allowed: every float is read and written by its one owning thread, and the tips are taken from
//                         that thread's value, not read back.  joints_out must not overlap joints16_in.
//   mano_post_bwd_kernel  one workgroup per hand.  d_verts_in = d_verts_out with each tip's d_joints_out[16 + t] added at its vertex by the
//                         owning thread (tips ascending; the asset's five ids are distinct); d_joints16 = d_joints_out[:, :16]; d_transl[n]
//                         = the float64 sum of the hand's 794 (799) rows in one fixed order (mps_thread_rows, then block_sum_f64), rounded
//                         once.  No float atomics; two runs give the same bits.
// No scratch, nothing passes from one workgroup to another, a hand's words do not depend on its place in the batch.
#pragma once
#include "ihmr_common.h"
#include "evaluate.h"
#include "mano_pose_space_pure.h"

static_assert(MPS_VERTS == NV && MPS_JOINTS == NJ && MPS_TIPS == IHMR_NUM_TIPS, "mano_pose_space_pure.h and ihmr_hip.h name one hand");
static_assert(MPS_C_STRIDE >= MPS_POSE && MPS_C_STRIDE % 2 == 1, "rows of C in LDS: whole and an odd number of banks apart");

struct MpsPcaLds {
    float C[MPS_POSE * MPS_C_STRIDE];           // rows k < K are filled
    float in[MPS_TILE * MPS_POSE];              // forward: the tile's coefficients, rows of K; backward: its d_pose45, rows of 45
};
static_assert(sizeof(MpsPcaLds) == MPS_PCA_LDS_BYTES, "mano_pose_space_pure.h names the LDS of the PCA kernels");

__device__ __forceinline__ void mps_load_tile(MpsPcaLds& L, const float* __restrict__ comps, int K, const float* __restrict__ rows, int n_in) {
    for (int e = threadIdx.x; e < K * MPS_POSE; e += MPS_THREADS) L.C[(e / MPS_POSE) * MPS_C_STRIDE + e % MPS_POSE] = comps[e];
    for (int e = threadIdx.x; e < n_in; e += MPS_THREADS) L.in[e] = rows[e];
    __syncthreads();
}

__global__ __launch_bounds__(MPS_THREADS) void mano_pca_fwd_kernel(const float* __restrict__ coeffs, const float* __restrict__ comps, int N,
                                                                    int K, float* __restrict__ pose45) {
    __shared__ MpsPcaLds L;
    const int n0 = blockIdx.x * MPS_TILE, hands = min(MPS_TILE, N - n0);
    mps_load_tile(L, comps, K, coeffs + (size_t)n0 * K, hands * K);
    float* out = pose45 + (size_t)n0 * MPS_POSE;
    for (int e = threadIdx.x; e < hands * MPS_POSE; e += MPS_THREADS) {
        const int h = e / MPS_POSE, i = e % MPS_POSE;
        out[e] = mps_fma_chain(L.in + h * K, 1, L.C + i, MPS_C_STRIDE, K);
    }
}

__global__ __launch_bounds__(MPS_THREADS) void mano_pca_bwd_kernel(const float* __restrict__ d_pose45, const float* __restrict__ comps, int N,
                                                                    int K, float* __restrict__ d_coeffs) {
    __shared__ MpsPcaLds L;
    const int n0 = blockIdx.x * MPS_TILE, hands = min(MPS_TILE, N - n0);
    mps_load_tile(L, comps, K, d_pose45 + (size_t)n0 * MPS_POSE, hands * MPS_POSE);
    float* out = d_coeffs + (size_t)n0 * K;
    for (int e = threadIdx.x; e < hands * K; e += MPS_THREADS) {
        const int h = e / K, k = e % K;
        out[e] = mps_fma_chain(L.in + h * MPS_POSE, 1, L.C + k * MPS_C_STRIDE, 1, MPS_POSE);
    }
}

// The five tip ids as named values (-1: no tips).  Neither they nor the translation sit in an indexed local array or struct: the compiler
// turns a select over neighbouring members into an indexed load and moves the object into LDS.
#define MPS_LOAD_TIPS(tip_ids)                                                                                               \
    const int tip0 = tip_ids ? tip_ids[0] : -1, tip1 = tip_ids ? tip_ids[1] : -1, tip2 = tip_ids ? tip_ids[2] : -1, \
              tip3 = tip_ids ? tip_ids[3] : -1, tip4 = tip_ids ? tip_ids[4] : -1
static_assert(MPS_TIPS == 5, "MPS_LOAD_TIPS names five tips");

__global__ __launch_bounds__(MPS_THREADS) void mano_post_fwd_kernel(const float* verts_in, const float* __restrict__ joints16_in,
                                                                     const float* __restrict__ transl, const int32_t* __restrict__ tip_ids,
                                                                     float* verts_out, float* __restrict__ joints_out) {
    const int n = blockIdx.x, tid = threadIdx.x;
    const int J = tip_ids ? MPS_JOINTS + MPS_TIPS : MPS_JOINTS;
    const bool has_transl = transl != nullptr;
    const float* t = has_transl ? transl + 3 * (size_t)n : nullptr;
    MPS_LOAD_TIPS(tip_ids);
    const float* vi = verts_in + (size_t)n * NV3;
    float* vo = verts_out + (size_t)n * NV3;
    float* jo = joints_out + (size_t)n * J * 3;
    float* jt = jo + MPS_JOINTS * 3;            // the tip rows
    for (int e = tid; e < NV3; e += MPS_THREADS) {
        const int v = e / 3, c = e - 3 * v;
        const float x = mps_shift(vi[e], has_transl, has_transl ? t[c] : 0.f);
        vo[e] = x;
        if (tip0 == v) jt[c] = x;
        if (tip1 == v) jt[3 + c] = x;
        if (tip2 == v) jt[6 + c] = x;
        if (tip3 == v) jt[9 + c] = x;
        if (tip4 == v) jt[12 + c] = x;
    }
    if (tid < MPS_JOINTS * 3) jo[tid] = mps_shift(joints16_in[(size_t)n * MPS_JOINTS * 3 + tid], has_transl, has_transl ? t[tid % 3] : 0.f);
    if (tip_ids && tid < MPS_TIPS * 3 && !mps_tip_ok(tip_ids[tid / 3])) jt[tid] = 0.f;
}

__global__ __launch_bounds__(MPS_THREADS) void mano_post_bwd_kernel(const float* __restrict__ d_verts_out, const float* __restrict__ d_joints_out,
                                                                     const int32_t* __restrict__ tip_ids, float* __restrict__ d_verts_in,
                                                                     float* __restrict__ d_joints16, float* __restrict__ d_transl) {
    __shared__ double part[4][10];
    static_assert(sizeof(part) == MPS_POST_BWD_LDS_BYTES, "mano_pose_space_pure.h names the LDS of mano_post_bwd_kernel");
    const int n = blockIdx.x, tid = threadIdx.x;
    const int J = tip_ids ? MPS_JOINTS + MPS_TIPS : MPS_JOINTS;
    MPS_LOAD_TIPS(tip_ids);
    const float* dvo = d_verts_out + (size_t)n * NV3;
    const float* djo = d_joints_out + (size_t)n * J * 3;
    const float* djt = djo + MPS_JOINTS * 3;    // the tip rows (read only where a tip id matched, i.e. with tip_ids)
    float* dvi = d_verts_in + (size_t)n * NV3;
    for (int e = tid; e < NV3; e += MPS_THREADS) {
        const int v = e / 3, c = e - 3 * v;
        float g = dvo[e];
        if (tip0 == v) g += djt[c];
        if (tip1 == v) g += djt[3 + c];
        if (tip2 == v) g += djt[6 + c];
        if (tip3 == v) g += djt[9 + c];
        if (tip4 == v) g += djt[12 + c];
        dvi[e] = g;
    }
    if (tid < MPS_JOINTS * 3) d_joints16[(size_t)n * MPS_JOINTS * 3 + tid] = djo[tid];
    if (d_transl) {                             // (uniform)
        double acc[3], sum[3];
        mps_thread_rows(dvo, djo, J, tid, acc);
        block_sum_f64<3>(acc, part, sum);
        if (tid == 0) {
            float* dt = d_transl + 3 * (size_t)n;
            dt[0] = (float)sum[0]; dt[1] = (float)sum[1]; dt[2] = (float)sum[2];
        }
    }
}

static bool mps_pca_ok(int N, int K) { return N >= 1 && K >= 1 && K <= MPS_POSE; }

static int mps_pca_fwd_launch(const float* coeffs, const float* comps, int N, int K, float* pose45, hipStream_t stream) {
    if (!coeffs || !comps || !pose45 || !mps_pca_ok(N, K)) return -1;
    hipLaunchKernelGGL(mano_pca_fwd_kernel, dim3((N + MPS_TILE - 1) / MPS_TILE), dim3(MPS_THREADS), 0, stream, coeffs, comps, N, K, pose45);
    return (int)hipGetLastError();
}

static int mps_pca_bwd_launch(const float* d_pose45, const float* comps, int N, int K, float* d_coeffs, hipStream_t stream) {
    if (!d_pose45 || !comps || !d_coeffs || !mps_pca_ok(N, K)) return -1;
    hipLaunchKernelGGL(mano_pca_bwd_kernel, dim3((N + MPS_TILE - 1) / MPS_TILE), dim3(MPS_THREADS), 0, stream, d_pose45, comps, N, K, d_coeffs);
    return (int)hipGetLastError();
}

static int mps_post_fwd_launch(const float* verts_in, const float* joints16_in, const float* transl, const int32_t* tip_ids, int N,
                               float* verts_out, float* joints_out, hipStream_t stream) {
    if (!verts_in || !joints16_in || !verts_out || !joints_out || N < 1) return -1;
    hipLaunchKernelGGL(mano_post_fwd_kernel, dim3(N), dim3(MPS_THREADS), 0, stream, verts_in, joints16_in, transl, tip_ids, verts_out,
                       joints_out);
    return (int)hipGetLastError();
}

static int mps_post_bwd_launch(const float* d_verts_out, const float* d_joints_out, const int32_t* tip_ids, int N, float* d_verts_in,
                               float* d_joints16, float* d_transl, hipStream_t stream) {
    if (!d_verts_out || !d_joints_out || !d_verts_in || !d_joints16 || N < 1) return -1;
    hipLaunchKernelGGL(mano_post_bwd_kernel, dim3(N), dim3(MPS_THREADS), 0, stream, d_verts_out, d_joints_out, tip_ids, d_verts_in,
                       d_joints16, d_transl);
    return (int)hipGetLastError();
}

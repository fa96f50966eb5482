// libihmr_hip.so -- C ABI (include/ihmr_hip.h) over the gfx950 kernels.  Single translation unit.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC ihmr_hip.hip -o libihmr_hip.so
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "ihmr_common.h"
#include "../../include/ihmr_mano_ext.h"
#include "mano_lbs.h"
#include "sdf_collision.h"
#include "preprocess.h"
#include "augment.h"
#include "render.h"
#include "mlp_infer.h"
#include "refine.h"
#include "encoder.h"
#include "encoder_bf16.h"
#include "evaluate.h"
#include "volume.h"
#include "surface.h"
#include "mano_pose_space.h"
#include "train.h"
#include "train_conv.h"
#include "copy_pack.h"
#include "launch_plan.h"
#include "stage_plan.h"

// bench.py's per-kernel timer -- the library's ONE piece of process-global state (include/ihmr_hip.h says so): the pointer and the
// list of pending event pairs are shared by every stream and thread of the process, guarded by g_timer_mutex; while no timer is set
// (the default) nothing here is touched.  (a,b) brackets one in-loop launch of kernel slot `k` (k < 0: an EMPTY pair, the cost of
// two event records)
static ihmr_kernel_timer* g_timer = nullptr;
static std::mutex g_timer_mutex;
struct TimedPair { hipEvent_t a, b; int k; };
static std::vector<TimedPair> g_pending;
static int timed_mark(hipEvent_t* ev, hipStream_t st) {
    HIP_TRY(hipEventCreate(ev));
    HIP_TRY(hipEventRecord(*ev, st));
    return 0;
}
// events around a group of back-to-back launches: timed_begin (empty pair + first mark), timed_next(k) after each launch
static int timed_begin(hipEvent_t* cur, hipStream_t st) {
    hipEvent_t e0, e1;
    if (int rc = timed_mark(&e0, st)) return rc;
    if (int rc = timed_mark(&e1, st)) return rc;
    { std::lock_guard<std::mutex> lk(g_timer_mutex); g_pending.push_back(TimedPair{e0, e1, -1}); }
    return timed_mark(cur, st);
}
static int timed_next(hipEvent_t* cur, int k, hipStream_t st) {
    hipEvent_t e;
    if (int rc = timed_mark(&e, st)) return rc;
    { std::lock_guard<std::mutex> lk(g_timer_mutex); g_pending.push_back(TimedPair{*cur, e, k}); }
    return timed_mark(cur, st);      // (a fresh start mark: every event belongs to exactly one pair)
}

// ------------------------------------------------------------------------------------------ model
// Every device buffer of ihmr_mano with the host table it is filled from (mano_tables.h): the ONE list that create, destroy and
// nothing else walk.  f(device pointer, host data, bytes) -> 0 or an error, which ends the walk.
template <typename F>
static int mano_buffers(ihmr_mano& m, const ManoTables& t, F f) {
    int rc = 0;
    auto go = [&](auto*& dev, const auto& host) { if (!rc) rc = f((void**)&dev, (const void*)host.data(), host.size() * sizeof(host[0])); };
    go(m.pd4, t.pd4); go(m.sd4, t.sd4); go(m.vt4, t.vt4);
    go(m.v_template, t.v_template); go(m.shapedirs_t, t.shapedirs_t); go(m.posedirs, t.posedirs);
    go(m.J_template, t.J_template); go(m.J_shapedirs, t.J_shapedirs); go(m.weights, t.weights);
    go(m.w4_w, t.w4_w); go(m.w4_j, t.w4_j);
    go(m.pose_mean, t.pose_mean); go(m.parents, t.parents); go(m.depth, t.depth);
    go(m.tip_ids, t.tip_ids); go(m.wj_start, t.wj_start); go(m.wj_vert, t.wj_vert);
    go(m.wj_w, t.wj_w); go(m.seg_q, t.seg_q); go(m.jseg_start, t.jseg_start);
    go(m.faces, t.faces); go(m.faces_pk, t.faces_pk); go(m.J_regressor, t.J_regressor);
    return rc;
}

// lbs_bwd1 keeps the per-segment partial sums in dynamic LDS (48 B per segment on top of ~36 KB static): dense
// weight matrices (up to ~960 segments) go past the default 64 KB per workgroup, so raise the cap to what is needed --
// for every instantiation that is launched with dynamic LDS, and checked: a kernel whose static + dynamic LDS does not fit
// the device is never launched (m->tail_fits = 0: ihmr_opt_run_stage falls back to the three separate launches)
static int mano_lds_fit(ihmr_mano* m) {
    const int dyn = m->nseg * 12 * (int)sizeof(float);
    hipError_t e1 = hipFuncSetAttribute((const void*)lbs_bwd1_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    hipError_t e2 = hipFuncSetAttribute((const void*)lbs_bwd1_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
    if (e1 != hipSuccess || e2 != hipSuccess) return (int)(e1 != hipSuccess ? e1 : e2);
    int dev = 0, lds_max = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    // (opt_tail_kernel_trans has no dynamic LDS: it is checked like the others and asks for none)
    const void* tails[4] = {(const void*)opt_tail_kernel<true, true>, (const void*)opt_tail_kernel<true>, (const void*)opt_tail_kernel<false>,
                            (const void*)opt_tail_kernel_trans};
    m->tail_fits = 1;
    const int tail_dyn = opt_tail_dynamic_lds(m->nseg);
    for (const void* k : tails) {
        hipFuncAttributes fa;
        const int dyn_k = k == (const void*)opt_tail_kernel_trans ? 0 : tail_dyn;
        if (hipFuncGetAttributes(&fa, k) != hipSuccess || (long)fa.sharedSizeBytes + dyn_k > (long)lds_max ||
            (dyn_k && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, dyn_k) != hipSuccess))
            m->tail_fits = 0;
    }
    (void)hipGetLastError();
    return 0;
}

// build the tables, upload them, fit the LDS; any failure frees what was allocated and leaves *out alone
extern "C" int ihmr_mano_create(const ihmr_mano_arrays* h, ihmr_mano** out) {
    if (!h || !out) return -1;
    ManoTables t;
    if (build_mano_tables(*h, t)) return -1;
    ihmr_mano* m = new ihmr_mano();
    memset(m, 0, sizeof(*m));
    m->sparse4 = t.sparse4;
    m->max_depth = t.max_depth;
    m->nnz = t.nnz;
    m->nseg = t.nseg;
    int rc = mano_buffers(*m, t, [](void** dev, const void* host, size_t bytes) {
        HIP_TRY(hipMalloc(dev, bytes));
        HIP_TRY(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
        return 0;
    });
    if (!rc) rc = mano_lds_fit(m);
    if (rc) { ihmr_mano_destroy(m); return rc; }
    *out = m;
    return 0;
}

extern "C" int ihmr_mano_destroy(ihmr_mano* m) {
    if (!m) return 0;
    mano_buffers(*m, ManoTables(), [](void** dev, const void*, size_t) {
        if (*dev) (void)hipFree(*dev);
        return 0;
    });
    delete m;
    return 0;
}

extern "C" int ihmr_mano_update_shapedirs(ihmr_mano* m, const float* shapedirs_host) {
    if (!m || !shapedirs_host) return -1;
    ManoTables t;
    t.J_regressor.resize((size_t)NJ * NV);
    t.v_template.resize(NV3);
    HIP_TRY(hipMemcpy(t.J_regressor.data(), m->J_regressor, t.J_regressor.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(t.v_template.data(), m->v_template, t.v_template.size() * 4, hipMemcpyDeviceToHost));
    build_shape_tables(shapedirs_host, t);
    HIP_TRY(hipMemcpy(m->shapedirs_t, t.shapedirs_t.data(), t.shapedirs_t.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->J_shapedirs, t.J_shapedirs.data(), t.J_shapedirs.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->sd4, t.sd4.data(), t.sd4.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// ------------------------------------------------------------------------------------------ seam A
extern "C" size_t ihmr_mano_workspace_bytes(int N) { return lbs_ws_bytes(N); }

// the skinning launch (REUSE: the workspace holds v_posed of the current pose and shape parameters, see lbs_skin_kernel)
static_assert(plan::SKIN_SMALL_MAX_HANDS == LBS_SMALL_MAX_HANDS && plan::BWD2_LDS_MIN_HANDS == LBS_B2_MIN_HANDS &&
              plan::PREP_SMALL_MAX_HANDS == SDF_PREP_SMALL_MAX_HANDS, "stage_plan.h restates the launch-form thresholds of the kernel headers");
template <bool TWO_HAND, int MODE>
static void lbs_skin_launch_mode(const ihmr_mano* m, int N, int B, float* verts, float* joints, const LbsWork& wk, float* pose_off, hipStream_t st) {
    const bool small = plan::skin_small(N);
    const int hg8 = 8 * (small ? LBS_HG_SMALL : LBS_HG);
    const dim3 skin_grid(8, 4 * ((N + hg8 - 1) / hg8));
    if (small) hipLaunchKernelGGL((lbs_skin_kernel<TWO_HAND, MODE, LBS_HG_SMALL>), skin_grid, dim3(LBS_THREADS), 0, st, *m, (const float*)wk.skel, N, B,
                                  verts, joints, wk.v_posed, pose_off);
    else hipLaunchKernelGGL((lbs_skin_kernel<TWO_HAND, MODE, LBS_HG>), skin_grid, dim3(LBS_THREADS), 0, st, *m, (const float*)wk.skel, N, B, verts,
                            joints, wk.v_posed, pose_off);
}
// skin modes of the callers: plan::Skin (stage_plan.h)
#define LBS_SKIN_FULL 0
#define LBS_SKIN_REUSE 1
#define LBS_SKIN_KEEP_P 2
#define LBS_SKIN_FULL_STORE_P 3
static_assert(plan::SKIN_FULL == LBS_SKIN_FULL && plan::SKIN_REUSE == LBS_SKIN_REUSE && plan::SKIN_KEEP_P == LBS_SKIN_KEEP_P &&
              plan::SKIN_FULL_STORE_P == LBS_SKIN_FULL_STORE_P, "stage_plan.h restates the skin modes");
static int g_force_full_skin = 0;    // checker switch: ihmr_debug_force_full_skin
template <bool TWO_HAND>
static void lbs_skin_launch(const ihmr_mano* m, int mode, int N, int B, float* verts, float* joints, const LbsWork& wk, hipStream_t st) {
    if (g_force_full_skin && (mode == LBS_SKIN_KEEP_P || mode == LBS_SKIN_FULL_STORE_P)) mode = LBS_SKIN_FULL;
    if (mode == LBS_SKIN_REUSE) lbs_skin_launch_mode<TWO_HAND, LBS_MODE_REUSE>(m, N, B, verts, joints, wk, nullptr, st);
    else if (mode == LBS_SKIN_KEEP_P) lbs_skin_launch_mode<TWO_HAND, LBS_MODE_KEEP_P>(m, N, B, verts, joints, wk, wk.pose_off, st);
    else lbs_skin_launch_mode<TWO_HAND, LBS_MODE_FULL>(m, N, B, verts, joints, wk, mode == LBS_SKIN_FULL_STORE_P ? wk.pose_off : nullptr, st);
}
extern "C" int ihmr_debug_force_full_skin(int force) {
    const int prev = g_force_full_skin;
    g_force_full_skin = force ? 1 : 0;
    return prev;
}
// checker switch: ihmr_opt_run_stage launches the three generic forms of opt_tail_kernel only -- no opt_tail_kernel_trans, no kept rotations
static int g_force_generic_tail = 0;
extern "C" int ihmr_debug_force_generic_tail(int force) {
    const int prev = g_force_generic_tail;
    g_force_generic_tail = force ? 1 : 0;
    return prev;
}

static void lbs_forward_launch(const ihmr_mano* m, bool two_hand, const float* orient, const float* pose, const float* betas,
                               const float* trans, int N, int B, float* verts, float* joints, const LbsWork& wk, hipStream_t st) {
    if (two_hand) {
        hipLaunchKernelGGL(lbs_skel_kernel<true>, dim3(N), dim3(192), 0, st, *m, orient, pose, betas, trans, B, wk.skel, joints);
        lbs_skin_launch<true>(m, LBS_SKIN_FULL, N, B, verts, joints, wk, st);
    } else {
        hipLaunchKernelGGL(lbs_skel_kernel<false>, dim3(N), dim3(192), 0, st, *m, orient, pose, betas, trans, B, wk.skel, joints);
        lbs_skin_launch<false>(m, LBS_SKIN_FULL, N, B, verts, joints, wk, st);
    }
}

static int g_bwd2_streaming = 0;     // checker switch: ihmr_debug_force_lbs_bwd2_streaming
extern "C" int ihmr_debug_force_lbs_bwd2_streaming(int force) {
    const int prev = g_bwd2_streaming;
    g_bwd2_streaming = force ? 1 : 0;
    return prev;
}

static void lbs_backward_launch(const ihmr_mano* m, bool two_hand, int N, int B, const float* d_verts, const float* d_joints,
                                float* d_orient, float* d_pose, float* d_betas, float* d_trans, int need_mask, const LbsWork& wk,
                                hipStream_t st, bool bwd1_done = false) {
    const size_t part_lds = (size_t)m->nseg * 12 * sizeof(float);
    if (bwd1_done) {}        // (the per-hand part ran inside opt_tail_kernel)
    else if (two_hand)
        hipLaunchKernelGGL(lbs_bwd1_kernel<true>, dim3(N), dim3(LBS_THREADS), part_lds, st, *m, wk, B, d_verts, d_joints, d_orient,
                           d_betas, d_trans, need_mask);
    else
        hipLaunchKernelGGL(lbs_bwd1_kernel<false>, dim3(N), dim3(LBS_THREADS), part_lds, st, *m, wk, B, d_verts, d_joints, d_orient,
                           d_betas, d_trans, need_mask);
    if (need_mask & 2) {
        if (plan::bwd2_lds(N, g_bwd2_streaming)) hipLaunchKernelGGL(lbs_bwd2_lds_kernel, dim3((N + LBS_B2_HANDS - 1) / LBS_B2_HANDS, LBS_KG), dim3(256), 0, st, *m, wk, N);
        else hipLaunchKernelGGL(lbs_bwd2_kernel, dim3(5, (N + 31) / 32, LBS_KG), dim3(64), 0, st, *m, wk, N);
        if (two_hand) hipLaunchKernelGGL(lbs_bwd3_kernel<true>, dim3(N), dim3(64), 0, st, wk, N, B, d_pose);
        else hipLaunchKernelGGL(lbs_bwd3_kernel<false>, dim3(N), dim3(64), 0, st, wk, N, B, d_pose);
    }
}

extern "C" int ihmr_mano_lbs_fwd(const ihmr_mano* m, const float* orient, const float* pose, const float* betas, int N,
                                 float* verts, float* joints, void* workspace, void* stream) {
    if (!m || N <= 0 || !workspace) return -1;
    lbs_forward_launch(m, false, orient, pose, betas, nullptr, N, 0, verts, joints, lbs_carve(workspace, N), (hipStream_t)stream);
    return (int)hipGetLastError();
}

extern "C" int ihmr_mano_lbs_bwd(const ihmr_mano* m, int N, const void* workspace, const float* d_verts, const float* d_joints,
                                 float* d_orient, float* d_pose, float* d_betas, int need_mask, void* stream) {
    if (!m || N <= 0 || !workspace) return -1;
    lbs_backward_launch(m, false, N, 0, d_verts, d_joints, d_orient, d_pose, d_betas, nullptr, need_mask,
                        lbs_carve(const_cast<void*>(workspace), N), (hipStream_t)stream);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ seam B
// (tail: the SoA and the packed copies of the caller's two face arrays)
// Compute units of the CURRENT device, cached per device id in relaxed atomics (concurrent first calls store the same value: no lock, no
// data race).  The persistent grid of sdf_dist_kernel and the Stream-K worker count of ihmr_conv_igemm derive from it; the latter fixes
// the K partition, so results are bit-stable per device MODEL (same CU count), not across models.
static int device_cu_count(int* cus_out) {
    static std::atomic<int> cache[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int cus = cache[dev & 63].load(std::memory_order_relaxed);
    if (cus == 0) {
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (cus <= 0) cus = 256;
        cache[dev & 63].store(cus, std::memory_order_relaxed);
    }
    *cus_out = cus;
    return 0;
}

extern "C" size_t ihmr_sdf_workspace_bytes(int B) { return sdf_ws_bytes(2 * B) + (size_t)2 * NFP * 4 * 4 + 256; }

static int g_collect_stats = 0;
// checker switch: sdf_prep_kernel neither fills nor reads its LDS copy of the packed face table -- every (triangle, column) pair of the
// ray-parity phase gathers its face word from global memory.  The same bits and the same work either way (tests/test_gpu_prep_faces.py);
// never set in the product path.  Read when a launch is issued: a captured graph keeps what it was captured with.
static int g_prep_global_faces = 0;
extern "C" int ihmr_debug_prep_global_faces(int force) {
    const int prev = g_prep_global_faces;
    g_prep_global_faces = force ? 1 : 0;
    return prev;
}

static int sdf_launch(const VertLayout& vl, const int32_t* faces_r_soa, const int32_t* faces_l_soa, const uint32_t* fpk_r,
                      const uint32_t* fpk_l, int B, SdfWorkspace ws, float robustifier, float* loss, float* per_vert, float* origin, float* dval, bool dense, hipStream_t st) {
    // the inside-voxel counter is zero on entry (faces_to_soa_kernel on seam B, the skeleton kernel of the iteration
    // on seam C); the prep kernel appends to it
    // an inside-list entry is (hand << 16) | voxel with bit 31 reserved (SDF_ENT_REFUSED): hand ids stay below 32768
    if (B <= 0 || 2 * B > SDF_MAX_HANDS) return -1;
    const int prep = plan::prep_form(2 * B, dense);      // (see sdf_collision.h)
    ws.fpk[0] = fpk_r; ws.fpk[1] = fpk_l; ws.B = B;
    const bool timed = g_timer != nullptr;
    hipEvent_t tcur;
    if (timed) { if (int rc = timed_begin(&tcur, st)) return rc; }
    if (prep == plan::PREP_DENSE)
        hipLaunchKernelGGL((sdf_prep_kernel<true, SDF_PREP_THREADS_LARGE>), dim3(2 * B), dim3(SDF_PREP_THREADS_LARGE), 0, st, vl, B, faces_r_soa,
                           faces_l_soa, ws, g_collect_stats, g_prep_global_faces);
    else if (prep == plan::PREP_SMALL)
        hipLaunchKernelGGL((sdf_prep_kernel<false, SDF_PREP_THREADS_SMALL>), dim3(2 * B), dim3(SDF_PREP_THREADS_SMALL), 0, st, vl, B, faces_r_soa,
                           faces_l_soa, ws, g_collect_stats, g_prep_global_faces);
    else
        hipLaunchKernelGGL((sdf_prep_kernel<false, SDF_PREP_THREADS_LARGE>), dim3(2 * B), dim3(SDF_PREP_THREADS_LARGE), 0, st, vl, B, faces_r_soa,
                           faces_l_soa, ws, g_collect_stats, g_prep_global_faces);
    // persistent grid: as many workgroups as the GPU holds at once; they pull work units from a queue (sdf_collision.h)
    int cus = 0;
    if (int rc = device_cu_count(&cus)) return rc;
    const int dist_blocks = SDF_DIST_WG_PER_CU * cus;
    if (timed) { if (int rc = timed_next(&tcur, IHMR_TIMED_SDF_PREP, st)) return rc; }
    int nblk = dist_blocks;
#ifdef IHMR_TUNING_BUILD
    if (const char* e = getenv("IHMR_DIST_BLOCKS_PER_SAMPLE")) nblk = std::max(64, std::min(dist_blocks, atoi(e) * B));
#endif
    if (g_collect_stats) hipLaunchKernelGGL(sdf_dist_kernel<true>, dim3(nblk), dim3(SDF_THREADS), 0, st, ws);
    else hipLaunchKernelGGL(sdf_dist_kernel<false>, dim3(nblk), dim3(SDF_THREADS), 0, st, ws);
    // (the launch the refinement really runs is the one that is timed: a second launch would find the work cursor spent)
    if (timed) { if (int rc = timed_next(&tcur, IHMR_TIMED_SDF_DIST, st)) return rc; (void)hipEventDestroy(tcur); }
    if (loss)
        hipLaunchKernelGGL(sdf_sample_kernel, dim3(B), dim3(SDF_SAMPLE_THREADS), 0, st, vl, ws, robustifier, loss, per_vert, origin,
                           dval, B);
    return (int)hipGetLastError();
}

// seam-B callers hand over (F,3) int32 AoS faces on the device; the SoA copy lives in the workspace tail
__global__ void faces_to_soa_kernel(const int32_t* __restrict__ aos, int32_t* __restrict__ soa, uint32_t* __restrict__ packed, int* zero8) {
    if (zero8 && blockIdx.x == 0 && threadIdx.x < SDF_NZERO) sdf_zero_counter(zero8, (int)threadIdx.x);  // inside-voxel counters, work cursors
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= NFP) return;
    const int s = f < NF ? f : 0;
    uint32_t pk = 0;
    for (int k = 0; k < 3; ++k) {
        const int32_t id = min(max(aos[s * 3 + k], 0), NV - 1);      // (an out-of-range id of the caller cannot leave the vertex array)
        soa[k * NFP + f] = id;
        pk |= (uint32_t)id << (10 * k);
    }
    packed[f] = pk;
}
// both hands' SoA and packed copies, carved from the tail of the caller's workspace (the first launch also zeroes the counters of `ws`)
struct FaceCopies { const int32_t *soa_r, *soa_l; const uint32_t *pk_r, *pk_l; };
static FaceCopies faces_to_workspace(const int32_t* faces_right, const int32_t* faces_left, void* workspace, int B, const SdfWorkspace& ws, hipStream_t st) {
    int32_t* soa = (int32_t*)((char*)workspace + sdf_ws_bytes(2 * B));
    uint32_t* pk = (uint32_t*)(soa + 6 * NFP);
    hipLaunchKernelGGL(faces_to_soa_kernel, dim3((NFP + 255) / 256), dim3(256), 0, st, faces_right, soa, pk, ws.inside_count);
    hipLaunchKernelGGL(faces_to_soa_kernel, dim3((NFP + 255) / 256), dim3(256), 0, st, faces_left, soa + 3 * NFP, pk + NFP, (int*)nullptr);
    return FaceCopies{soa, soa + 3 * NFP, pk, pk + NFP};
}

extern "C" int ihmr_sdf_collision_ex(const int32_t* faces_right, const int32_t* faces_left, const float* hand_verts, int B,
                                     float robustifier, const ihmr_sdf_options* options, float* loss, float* per_vert,
                                     float* origin_scale, float* dval, void* workspace, void* stream) {
    if (!workspace || B <= 0 || 2 * B > SDF_MAX_HANDS) return -1;
    hipStream_t st = (hipStream_t)stream;
    SdfWorkspace ws = sdf_carve(workspace, 2 * B);
    if (options) {
        ws.align_corners = options->align_corners ? 1 : 0;
        if (options->loss_divisor > 0.f) ws.loss_div = options->loss_divisor;
        ws.swap_xz = options->swap_xz ? 1 : 0;
    }
    const FaceCopies f = faces_to_workspace(faces_right, faces_left, workspace, B, ws, st);
    VertLayout vl{hand_verts, (long)2 * NV3, (long)NV3};
    return sdf_launch(vl, f.soa_r, f.soa_l, f.pk_r, f.pk_l, B, ws, robustifier, loss, per_vert, origin_scale, dval, false, st);
}

extern "C" int ihmr_sdf_collision(const int32_t* faces_right, const int32_t* faces_left, const float* hand_verts, int B,
                                  float robustifier, float* loss, float* per_vert, float* origin_scale, float* dval,
                                  void* workspace, void* stream) {
    return ihmr_sdf_collision_ex(faces_right, faces_left, hand_verts, B, robustifier, nullptr, loss, per_vert, origin_scale, dval,
                                 workspace, stream);
}

extern "C" int ihmr_sdf_dense_grid(const int32_t* faces_right, const int32_t* faces_left, const float* hand_verts, int B,
                                   float* phi, void* workspace, void* stream) {
    if (!workspace || B <= 0 || 2 * B > SDF_MAX_HANDS) return -1;
    hipStream_t st = (hipStream_t)stream;
    SdfWorkspace ws = sdf_carve(workspace, 2 * B);
    const FaceCopies f = faces_to_workspace(faces_right, faces_left, workspace, B, ws, st);
    VertLayout vl{hand_verts, (long)2 * NV3, (long)NV3};
    int rc = sdf_launch(vl, f.soa_r, f.soa_l, f.pk_r, f.pk_l, B, ws, 0.f, nullptr, nullptr, nullptr, nullptr, true, st);
    if (rc) return rc;
    // workspace order is hand = hnd*B + b; the caller's grid is (B,2,...)
    for (int b = 0; b < B; ++b)
        for (int hnd = 0; hnd < 2; ++hnd)
            HIP_TRY(hipMemcpyAsync(phi + ((size_t)b * 2 + hnd) * SDF_NVOX, ws.phi + ((size_t)hnd * B + b) * SDF_NVOX,
                                   (size_t)SDF_NVOX * 4, hipMemcpyDeviceToDevice, st));
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ seam C
extern "C" size_t ihmr_opt_workspace_bytes(int B) { return opt_ws_bytes(B); }

// `prev` = the Adam step of the previous iteration (group < 0: none), applied at the head of the skeleton kernel
static const ParamStep kNoStep{0, 0.f, 0.f, 1.f, -1, 0, 0};
// the collision workspace of one iteration with the switches of this call (plan::plan_sdf_flags)
static SdfWorkspace opt_sdf_ws(const ihmr_opt_io* io, const OptWork& wk, int B, int lists, int static_mask) {
    SdfWorkspace ws = sdf_carve(wk.sdf_ws, 2 * B, true);
    const plan::SdfFlags f = plan::plan_sdf_flags(lists, static_mask, io->sdf_no_candidate_lists, io->sdf_no_static_reuse);
    ws.list_mode = f.list_mode;
    ws.force_rebuild = f.force_rebuild;
    ws.static_stage = f.static_stage;
    ws.static_mask = f.static_mask;
    ws.moving_box = f.moving_box;
    ws.align_corners = io->sdf_align_corners ? 1 : 0;
    if (io->sdf_loss_divisor > 0.f) ws.loss_div = io->sdf_loss_divisor;
    ws.swap_xz = io->sdf_swap_xz ? 1 : 0;
    return ws;
}

// what every launch of the refinement loop is handed; sel: the accept / reject step of an IHMR-MLP evaluation, or none
struct OptCtx {
    const ihmr_mano *m, *m_left;
    const ihmr_opt_io* io;
    OptWork wk;
    int B;
    const ihmr_opt_weights* w;
    hipStream_t st;
    const MlpSelect* sel;
};

// The launches of one iteration, exactly as `q` lists them (plan::IterPlan): head = the Adam + skeleton launch applying `prev`, skin = the
// skinning launch, the collision prep + distance launches, the tail -- which in its stepping forms applies `next` -- and the LBS backward
static int run_iteration(const OptCtx& c, const plan::IterPlan& q, const ParamStep& prev, const ParamStep& next) {
    const ihmr_mano* m = c.m;
    const ihmr_opt_io* io = c.io;
    const OptWork& wk = c.wk;
    const int B = c.B;
    hipStream_t st = c.st;
    const SdfWorkspace ws = opt_sdf_ws(io, wk, B, q.lists, q.static_mask);
    if (q.head) hipLaunchKernelGGL(opt_adam_skel_kernel, dim3(B), dim3(384), 0, st, *m, *io, wk, B, prev, ws.inside_count);
    if (q.skin != plan::SKIN_NONE) lbs_skin_launch<true>(m, q.skin, 2 * B, B, io->verts, wk.joints_raw, wk.lbs, st);
    if (q.tail == plan::TAIL_NONE) return (int)hipGetLastError();
    VertLayout vl{io->verts, (long)NV3, (long)B * NV3};
    int rc = sdf_launch(vl, m->faces, c.m_left ? c.m_left->faces : m->faces, m->faces_pk, c.m_left ? c.m_left->faces_pk : m->faces_pk, B, ws, 0.f,
                        nullptr, nullptr, nullptr, nullptr, false, st);
    if (rc) return rc;
    if (q.tail == plan::TAIL_SEPARATE) {
        // collision sampling (loss_batch[2], masked by hand type; gradient -> g_verts) and the joint losses in one launch
        MlpSelect no_sel;
        memset(&no_sel, 0, sizeof(no_sel));
        hipLaunchKernelGGL(opt_sample_loss_kernel, dim3(B), dim3(SDF_SAMPLE_THREADS), 0, st, *io, wk, B, *c.w, vl, ws, q.need_cam, c.sel ? *c.sel : no_sel);
    } else {
        const size_t tail_lds = (size_t)opt_tail_dynamic_lds(m->nseg);
        hipEvent_t tcur;
        const bool timed = g_timer != nullptr;
        if (timed) { if (int rc2 = timed_begin(&tcur, st)) return rc2; }
        const TailArgs ta{*m, *io, wk, B, *c.w, vl, ws, q.need_cam, q.need_mask, next, ws.inside_count, q.keep_rot, q.first};
        if (q.tail == plan::TAIL_TRANS)
            hipLaunchKernelGGL(opt_tail_kernel_trans, dim3(B), dim3(SDF_SAMPLE_THREADS), 0, st, ta);
        else if (q.tail == plan::TAIL_STEP_SKIN)
            hipLaunchKernelGGL((opt_tail_kernel<true, true>), dim3(B), dim3(SDF_SAMPLE_THREADS), tail_lds, st, ta);
        else if (q.tail == plan::TAIL_STEP)
            hipLaunchKernelGGL(opt_tail_kernel<true>, dim3(B), dim3(SDF_SAMPLE_THREADS), tail_lds, st, ta);
        else
            hipLaunchKernelGGL(opt_tail_kernel<false>, dim3(B), dim3(SDF_SAMPLE_THREADS), tail_lds, st, ta);
        if (timed) { if (int rc2 = timed_next(&tcur, IHMR_TIMED_OPT_TAIL, st)) return rc2; (void)hipEventDestroy(tcur); }
    }
    if (q.after != plan::AFTER_NONE)
        lbs_backward_launch(m, true, 2 * B, B, wk.g_verts, wk.g_joints, wk.g_orient, wk.g_pose, wk.g_shape, wk.g_trans, q.need_mask, wk.lbs, st,
                            /*bwd1_done=*/q.after == plan::AFTER_BWD23);
    return (int)hipGetLastError();
}

extern "C" int ihmr_opt_forward_losses(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B,
                                       const ihmr_opt_weights* w, void* stream) {
    if (!m || !io || !w || B <= 0 || 2 * B > SDF_MAX_HANDS) return -1;
    return run_iteration(OptCtx{m, m_left, io, opt_carve(io->workspace, B), B, w, (hipStream_t)stream, nullptr}, plan::kForwardLosses, kNoStep, kNoStep);
}

static_assert(plan::PB_CAM == IHMR_PB_CAM && plan::PB_TRANS == IHMR_PB_TRANS && plan::PB_ORIENT_R == IHMR_PB_ORIENT_R &&
              plan::PB_ORIENT_L == IHMR_PB_ORIENT_L && plan::PB_POSE_R == IHMR_PB_POSE_R && plan::PB_POSE_L == IHMR_PB_POSE_L &&
              plan::PB_SHAPE_R == IHMR_PB_SHAPE_R && plan::PB_SHAPE_L == IHMR_PB_SHAPE_L, "stage_plan.h restates the parameter-block bits");
static_assert(plan::OPTIM_ADAM == IHMR_OPTIM_ADAM && plan::OPTIM_SGD == IHMR_OPTIM_SGD, "stage_plan.h restates the optimizers");

extern "C" int ihmr_opt_run_stage(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B,
                                  const ihmr_opt_weights* w, const ihmr_opt_stage* sg, void* stream) {
    if (!m || !io || !w || !sg || B <= 0 || 2 * B > SDF_MAX_HANDS) return -1;
    if (!plan::stage_ok(sg->param_mask, sg->optimizer, sg->n_iters, sg->save_freq, sg->select_loss)) return -1;
    const OptCtx c{m, m_left, io, opt_carve(io->workspace, B), B, w, (hipStream_t)stream, nullptr};
    const plan::StagePlan p = plan::plan_stage(sg->param_mask, io->no_fused_tail, m->tail_fits, io->sdf_no_static_reuse, g_force_generic_tail, sg->keep_lists);
    const int sgd = sg->optimizer == IHMR_OPTIM_SGD;
    ParamStep step{0, 0.f, 0.f, 1.f, -1, 1, 0};   // iteration 0: no step yet, zero the optimizer state
    for (int it = 0; it < sg->n_iters; ++it) {
        const plan::StepPlan s = plan::plan_step(sg->lr, sgd, it, sg->save_freq);
        const ParamStep next{sg->param_mask, w->shape_reg, s.step_size, s.bc2_sqrt, s.snap_idx, 0, sgd};
        if (int rc = run_iteration(c, plan::plan_iter(p, it, sg->n_iters), step, next)) return rc;
        step = next;
    }
    hipLaunchKernelGGL(opt_adam_kernel, dim3(B), dim3(128), 0, c.st, *io, c.wk, B, step);
    hipLaunchKernelGGL(opt_select_kernel, dim3((B + 63) / 64), dim3(64), 0, c.st, *io, B, plan::snapshot_count(sg->n_iters, sg->save_freq), *sg);
    return (int)hipGetLastError();
}

extern "C" int ihmr_opt_set_params(const ihmr_opt_io* io, const float* final_params, int B, void* stream) {
    if (!io || !final_params || B <= 0) return -1;
    hipLaunchKernelGGL(opt_unpack_params_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, *io, final_params, B);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ IHMR-MLP inference glue (mlp_infer.h)
// [256 B header | hidden activations (B, 512 + 256 + 128) | raw joints of every sample's accepted state (B, 42, 3)]
extern "C" size_t ihmr_mlp_workspace_bytes(int B) { return ((size_t)B * (512 + 256 + 128 + 126) * sizeof(float) + 256 + 255) & ~(size_t)255; }
static float* mlp_acc_joints(void* workspace, int B) { return (float*)((char*)workspace + 256) + (size_t)B * (512 + 256 + 128); }

static int mlp_fill_select(MlpSelect& s, const ihmr_mlp_tables* t, const ihmr_mlp_stage* stage, int mode, void* workspace) {
    memset(&s, 0, sizeof(s));
    s.mode = mode;
    if (mode == 2) {
        if (!stage || stage->n_filter < 0 || stage->n_filter > 4 || stage->select_loss < 0 || stage->select_loss > 2) return -1;
        s.n_filter = stage->n_filter;
        for (int f = 0; f < stage->n_filter; ++f) {
            if (stage->filter_loss[f] < 0 || stage->filter_loss[f] > 2) return -1;
            s.filter_loss[f] = stage->filter_loss[f];
            s.filter_factor[f] = stage->filter_factor[f];
        }
        s.select_loss = stage->select_loss;
    }
    s.idx = (const long long*)t->idx; s.new_params = t->new_params; s.img_feat = t->img_feat;
    s.data_idxs_all = t->data_idxs_all; s.img_feat_all = t->img_feat_all; s.prev_final = t->prev_final; s.prev_loss = t->prev_loss;
    s.final_out = t->final_params; s.kept = t->kept;
    return 0;
}

extern "C" int ihmr_mlp_stage_head(const ihmr_mlp_net* net, const ihmr_mlp_tables* t, const ihmr_opt_io* io, int B, void* workspace,
                                   void* stream) {
    if (!net || !t || !io || !workspace || B <= 0 || net->k_out <= 0 || net->k_out > 122) return -1;
    MlpHeadArgs a;
    memset(&a, 0, sizeof(a));
    a.feat = t->img_feat; a.prev = t->final_params;
    for (int l = 0; l < 4; ++l) { a.w[l] = net->w[l]; a.b[l] = net->b[l]; a.ldw[l] = net->ldw[l]; if (!a.w[l] || !a.b[l]) return -1; }
    if (a.ldw[0] < 512 || a.ldw[1] < 256 || a.ldw[2] < 128 || a.ldw[3] < ((net->k_out + 15) & ~15)) return -1;
    a.kout = net->k_out;
    for (int j = 0; j < net->k_out; ++j) {
        if (net->col[j] < 0 || net->col[j] >= 122) return -1;
        a.col[j] = (unsigned char)net->col[j];
    }
    float* h = (float*)((char*)workspace + 256);
    a.h[0] = h; a.h[1] = h + (size_t)B * 512; a.h[2] = a.h[1] + (size_t)B * 256;
    a.new_params = t->new_params;
    a.B = B;
    const int tr = (B + 15) / 16;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_layer_kernel<0>, dim3(std::min(tr * 32, MLPI_MAX_WG)), dim3(MLPI_THREADS), 0, st, a, *io);
    hipLaunchKernelGGL(mlp_layer_kernel<1>, dim3(std::min(tr * 16, MLPI_MAX_WG)), dim3(MLPI_THREADS), 0, st, a, *io);
    hipLaunchKernelGGL(mlp_layer_kernel<2>, dim3(std::min(tr * 8, MLPI_MAX_WG)), dim3(MLPI_THREADS), 0, st, a, *io);
    hipLaunchKernelGGL(mlp_layer_kernel<3>, dim3(std::min(tr * ((a.kout + 15) / 16), MLPI_MAX_WG)), dim3(MLPI_THREADS), 0, st, a, *io);
    return (int)hipGetLastError();
}

extern "C" int ihmr_mlp_forward_select(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B, const ihmr_opt_weights* w,
                                       const ihmr_mlp_tables* t, const ihmr_mlp_stage* stage, int mode, void* workspace, void* stream) {
    if (!m || !io || !w || !workspace || B <= 0 || 2 * B > SDF_MAX_HANDS || mode < 0 || mode > 3 || (mode && !t)) return -1;
    MlpSelect sel;
    memset(&sel, 0, sizeof(sel));
    // mode 3 (round 6): the caller's bookkeeping (ihmr_amd/mlp_model.py) says the workspace holds v_posed of these parameters (plan_mlp_eval)
    const plan::IterPlan q = plan::plan_mlp_eval(mode);
    if (mode == 3) mode = 2;
    if (mode) { if (int rc = mlp_fill_select(sel, t, stage, mode, workspace)) return rc; }
    OptWork wk = opt_carve(io->workspace, B);
    if (mode) { sel.joints_now = wk.joints_raw; sel.acc_joints = mlp_acc_joints(workspace, B); }
    return run_iteration(OptCtx{m, m_left, io, wk, B, w, (hipStream_t)stream, mode ? &sel : nullptr}, q, kNoStep, kNoStep);
}

// the evaluation of a stage that moved ONLY the camera: one small launch (mlp_camera_select_kernel, refine.h)
extern "C" int ihmr_mlp_camera_select(const ihmr_opt_io* io, int B, const ihmr_opt_weights* w, const ihmr_mlp_tables* t,
                                      const ihmr_mlp_stage* stage, void* workspace, void* stream) {
    if (!io || !w || !t || !stage || !workspace || B <= 0) return -1;
    MlpSelect sel;
    if (int rc = mlp_fill_select(sel, t, stage, 2, workspace)) return rc;
    OptWork wk = opt_carve(io->workspace, B);
    sel.joints_now = nullptr; sel.acc_joints = nullptr;          // (the accepted joints do not change: the camera moves no joint)
    wk.joints_raw = mlp_acc_joints(workspace, B);                 // the loss wave reads the accepted state's raw joints
    hipLaunchKernelGGL(mlp_camera_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, *io, wk, B, *w, sel);
    return (int)hipGetLastError();
}

// skeletons + skinning of the parameters in `io` only (no collision term, no losses): the annotation's meshes of the export
extern "C" int ihmr_opt_forward_verts(const ihmr_mano* m, const ihmr_opt_io* io, int B, void* stream) {
    if (!m || !io || B <= 0) return -1;
    return run_iteration(OptCtx{m, nullptr, io, opt_carve(io->workspace, B), B, nullptr, (hipStream_t)stream, nullptr}, plan::kForwardVerts, kNoStep, kNoStep);
}

// ------------------------------------------------------------------------------------------ stage graphs
// A stage is ~8 launches x n_iters with no host decision inside: capture it once into a hipGraph (per model
// instance and stage -- the io pointers and the per-iteration Adam constants are baked into the nodes) and
// replay it, so the host cost per stage drops from ~n_iters x 8 launches to one graph launch.
struct ihmr_graph {
    hipGraph_t graph;
    hipGraphExec_t exec;
};

template <typename F>
static int capture_graph(F&& enqueue, ihmr_graph** out) {
    hipStream_t cs;
    HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    ihmr_kernel_timer* keep = g_timer;
    g_timer = nullptr;  // no event records inside a capture
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    int rc = e == hipSuccess ? enqueue(cs) : (int)e;
    hipGraph_t g = nullptr;
    hipError_t e2 = hipStreamEndCapture(cs, &g);
    g_timer = keep;
    (void)hipStreamDestroy(cs);
    if (rc) return rc;
    if (e2 != hipSuccess) return (int)e2;
    ihmr_graph* h = new ihmr_graph();
    h->graph = g;
    hipError_t e3 = hipGraphInstantiate(&h->exec, g, nullptr, nullptr, 0);
    if (e3 != hipSuccess) { (void)hipGraphDestroy(g); delete h; return (int)e3; }
    *out = h;
    return 0;
}

extern "C" int ihmr_opt_stage_graph_create(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B,
                                           const ihmr_opt_weights* w, const ihmr_opt_stage* stage, ihmr_graph** out) {
    if (!out) return -1;
    return capture_graph([&](hipStream_t cs) { return ihmr_opt_run_stage(m, m_left, io, B, w, stage, (void*)cs); }, out);
}

extern "C" int ihmr_opt_forward_graph_create(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B,
                                             const ihmr_opt_weights* w, ihmr_graph** out) {
    if (!out) return -1;
    return capture_graph([&](hipStream_t cs) { return ihmr_opt_forward_losses(m, m_left, io, B, w, (void*)cs); }, out);
}

extern "C" int ihmr_graph_launch(ihmr_graph* g, void* stream) {
    if (!g) return -1;
    return (int)hipGraphLaunch(g->exec, (hipStream_t)stream);
}

extern "C" int ihmr_graph_destroy(ihmr_graph* g) {
    if (!g) return 0;
    (void)hipGraphExecDestroy(g->exec);
    (void)hipGraphDestroy(g->graph);
    delete g;
    return 0;
}

// diagnostics (synchronises): one forward + losses with the SDF work counters switched on.
// out[0] = (voxel, triangle) ray tests, out[1] = exact point-triangle distances, out[2] = inside voxels,
// out[3] = needed voxels -- totals of ONE sdf_prep_kernel + sdf_dist_kernel launch pair.
extern "C" int ihmr_opt_sdf_stats(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B,
                                  const ihmr_opt_weights* w, unsigned long long* out4, void* stream) {
    if (!m || !io || !w || !out4 || B <= 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    OptWork wk = opt_carve(io->workspace, B);
    SdfWorkspace ws = sdf_carve(wk.sdf_ws, 2 * B, true);
    HIP_TRY(hipMemsetAsync(ws.stats, 0, 128, st));
    ihmr_kernel_timer* keep = g_timer;
    g_timer = nullptr;
    g_collect_stats = 1;
    int rc = run_iteration(OptCtx{m, m_left, io, wk, B, w, st, nullptr}, plan::kForwardLosses, kNoStep, kNoStep);
    g_collect_stats = 0;
    g_timer = keep;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(out4, ws.stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

// diagnostics of the fused loop: enable = 1 zeroes the SDF work counters and switches them on for every launch recorded or issued
// afterwards (a stage graph captured while they are on keeps counting); enable = 0 synchronises, copies the sixteen counter slots out
// (ray tests, exact distances, inside voxels, needed voxels, bounding-sphere tests, voxels answered from candidate lists, voxels
// of such hands handed to the full search, voxels whose lists were rebuilt, plane + circle tests; the rest unused) and switches them off.
extern "C" int ihmr_opt_sdf_counters(const ihmr_opt_io* io, int B, unsigned long long* out16, int enable) {
    if (!io || B <= 0) return -1;
    SdfWorkspace ws = sdf_carve(opt_carve(io->workspace, B).sdf_ws, 2 * B, true);
    HIP_TRY(hipDeviceSynchronize());
    if (enable) {
        HIP_TRY(hipMemset(ws.stats, 0, 128));
        g_collect_stats = 1;
        return 0;
    }
    g_collect_stats = 0;
    if (!out16) return -1;
    HIP_TRY(hipMemcpy(out16, ws.stats, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ihmr_opt_sdf_inside_bits(const ihmr_opt_io* io, int B, unsigned* out, float* box) {
    if (!io || B <= 0 || 2 * B > SDF_MAX_HANDS || (!out && !box)) return -1;
    SdfWorkspace ws = sdf_carve(opt_carve(io->workspace, B).sdf_ws, 2 * B, true);
    HIP_TRY(hipDeviceSynchronize());
    if (out) HIP_TRY(hipMemcpy(out, ws.inside_bits, (size_t)2 * B * SDF_NCOL * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (box) HIP_TRY(hipMemcpy(box, ws.box, (size_t)2 * B * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ encoder
// The tile kernels of a launcher, looked up by what its planner (csrc/launch_plan.h) chose; a plan without an entry is an error
template <typename Args>
struct TileKernel { int bm, bn, mode; void (*kernel)(Args); };
template <typename Args, size_t n>
static void (*tile_kernel(const TileKernel<Args> (&table)[n], int bm, int bn, int mode))(Args) {
    for (const TileKernel<Args>& e : table)
        if (e.bm == bm && e.bn == bn && e.mode == mode) return e.kernel;
    return nullptr;
}
static_assert(plan::CONV_BK_F32 == CONV_BK && plan::CONV_BK_BF16 == CONVB_BK, "launch_plan.h restates the K steps of the conv kernels");
static_assert(plan::GENERIC == CONV_GENERIC && plan::FAST == CONV_FAST && plan::C4 == CONV_C4, "launch_plan.h restates the gather modes");
static_assert(plan::GENERIC == CONVB_GENERIC && plan::FAST == CONVB_FAST && plan::C4 == CONVB_C4, "launch_plan.h restates the gather modes");

static const TileKernel<ConvArgs> kConvKernels[] = {
    {128, 128, CONV_FAST, conv_igemm_kernel<128, 128, CONV_FAST>},       {64, 128, CONV_FAST, conv_igemm_kernel<64, 128, CONV_FAST>},
    {128, 64, CONV_FAST, conv_igemm_kernel<128, 64, CONV_FAST>},         {64, 64, CONV_FAST, conv_igemm_kernel<64, 64, CONV_FAST>},
    {128, 64, CONV_C4, conv_igemm_kernel<128, 64, CONV_C4>},             {64, 64, CONV_C4, conv_igemm_kernel<64, 64, CONV_C4>},
    {128, 128, CONV_GENERIC, conv_igemm_kernel<128, 128, CONV_GENERIC>}, {64, 128, CONV_GENERIC, conv_igemm_kernel<64, 128, CONV_GENERIC>},
    {128, 64, CONV_GENERIC, conv_igemm_kernel<128, 64, CONV_GENERIC>},   {64, 64, CONV_GENERIC, conv_igemm_kernel<64, 64, CONV_GENERIC>}};

extern "C" int ihmr_conv_igemm(const float* x, const float* w, const float* bias, const float* residual, float* y, int N, int H,
                               int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int ldx, int ldw,
                               int ldy, int ldr, int act, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return -1;
    hipStream_t st = (hipStream_t)stream;
    int cus = 0;
    if (int rc = device_cu_count(&cus)) return rc;
    plan::ConvTuning tuning;
#ifdef IHMR_TUNING_BUILD   // per-layer tile / split measurements (scripts/prof_encoder.py builds its own library with this macro)
    if (const char* force = getenv("IHMR_CONV_FORCE")) sscanf(force, "%d %d", &tuning.force_tile, &tuning.force_ksplit);   // "<tile 0-3> <ksplit>"
    if (const char* f = getenv("IHMR_CONV_SK")) {   // "<max tiles> <min K steps> <workers>"
        tuning.sk_workers = plan::streamk_workers(cus);
        sscanf(f, "%d %d %d", &tuning.sk_max_tiles, &tuning.sk_min_nk, &tuning.sk_workers);
        if (tuning.sk_workers < 8 || tuning.sk_workers % 8 != 0) return -1;
    }
#endif
    const plan::ConvPlan p = plan::plan_conv_fp32(N, Cin, Ho, Wo, Cout, kh, kw, ldx, ldw, ldy, cus, workspace ? workspace_bytes : 0,
                                                  ((uintptr_t)y % 16) == 0, tuning);
    if (!p.ok) return -1;
    ConvArgs a{x, w, bias, residual, y, N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, ldx, ldw, ldy, ldr, act, (float*)workspace, p.ksplit};
    if (p.streamk) {
        const int total = p.sk_tiles * p.nk;
        hipLaunchKernelGGL(conv_streamk_kernel, dim3(p.sk_workers), dim3(512), 0, st, a, p.tiles_m, p.nk, total);
        hipLaunchKernelGGL(conv_streamk_fixup_kernel, dim3((unsigned)p.sk_tiles, 8), dim3(256), 0, st, a, p.tiles_m, p.nk, total, p.sk_workers);
        return (int)hipGetLastError();
    }
    void (*kernel)(ConvArgs) = tile_kernel(kConvKernels, p.bm, p.bn, p.mode);
    if (!kernel) return -1;
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(p.threads), 0, st, a);
    const long M = (long)N * Ho * Wo;
    if (p.reduce == 4) hipLaunchKernelGGL(conv_splitk_reduce_kernel<4>, dim3((unsigned)((M * (Cout / 4) + 255) / 256)), dim3(256), 0, st, a);
    else if (p.reduce == 1) hipLaunchKernelGGL(conv_splitk_reduce_kernel<1>, dim3((unsigned)((M * Cout + 255) / 256)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int ihmr_maxpool3x3s2(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, void* stream) {
    if (C % 4) return -1;
    const long total = (long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C, Ho, Wo);
    return (int)hipGetLastError();
}

extern "C" int ihmr_avgpool_relu(const float* x, float* y, int N, int HW, int C, int ldy, void* stream) {
    hipLaunchKernelGGL(avgpool_relu_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y, N, HW, C, ldy);
    return (int)hipGetLastError();
}

// ---- bf16 encoder path (csrc/encoder_bf16.h)
static const TileKernel<ConvArgsBF16> kConvKernelsBF16[] = {
    {128, 128, CONVB_FAST, conv_igemm_bf16_kernel<128, CONVB_FAST>}, {128, 128, CONVB_C4, conv_igemm_bf16_kernel<128, CONVB_C4>},
    {128, 128, CONVB_GENERIC, conv_igemm_bf16_kernel<128, CONVB_GENERIC>},
    {128, 64, CONVB_FAST, conv_igemm_bf16_kernel<64, CONVB_FAST>},   {128, 64, CONVB_C4, conv_igemm_bf16_kernel<64, CONVB_C4>},
    {128, 64, CONVB_GENERIC, conv_igemm_bf16_kernel<64, CONVB_GENERIC>}};

extern "C" int ihmr_conv_igemm_bf16(const uint16_t* x, const uint16_t* w, const float* bias, const uint16_t* residual, uint16_t* y, int N,
                                    int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int ldx,
                                    int ldw, int ldy, int ldr, int act, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !y) return -1;
    if (((uintptr_t)w % 16) != 0 || (bias && ((uintptr_t)bias % 16) != 0)) return -1;
    hipStream_t st = (hipStream_t)stream;
    int cus = 0;
    if (int rc = device_cu_count(&cus)) return rc;
    const plan::ConvPlanBF16 p = plan::plan_conv_bf16(N, Cin, Ho, Wo, Cout, kh, kw, ldx, ldw, ldy, ldr, act, cus, workspace ? workspace_bytes : 0,
                                                      ((uintptr_t)x % 16) == 0, ((uintptr_t)x % 8) == 0, ((uintptr_t)y % 8) == 0,
                                                      residual != nullptr, ((uintptr_t)residual % 8) == 0);
    if (!p.ok) return -1;
    ConvArgsBF16 a{x, w, bias, residual, y, N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, ldx, ldw, ldy, ldr, act, (float*)workspace, p.ksplit, p.vec};
    void (*kernel)(ConvArgsBF16) = tile_kernel(kConvKernelsBF16, 128, p.bn, p.mode);
    if (!kernel) return -1;
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(256), 0, st, a);
    if (p.ksplit > 1) {
        const long total = (long)N * Ho * Wo * ((Cout + 3) / 4);
        hipLaunchKernelGGL(conv_splitk_reduce_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    }
    return (int)hipGetLastError();
}

extern "C" int ihmr_pack_image_bf16(const float* img, uint16_t* y, int N, int H, int W, void* stream) {
    if (!img || !y || N <= 0 || H <= 0 || W <= 0 || ((uintptr_t)y % 8) != 0) return -1;
    const long total = (long)N * H * W;
    hipLaunchKernelGGL(image_to_nhwc4_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, y, N, H * W);
    return (int)hipGetLastError();
}

extern "C" int ihmr_maxpool3x3s2_bf16(const uint16_t* x, uint16_t* y, int N, int H, int W, int C, int Ho, int Wo, void* stream) {
    if (!x || !y || C % 8 || ((uintptr_t)x % 16) != 0 || ((uintptr_t)y % 16) != 0) return -1;
    const long total = (long)N * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(maxpool3x3s2_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, H, W, C, Ho, Wo);
    return (int)hipGetLastError();
}

extern "C" int ihmr_avgpool_relu_bf16(const uint16_t* x, float* y, int N, int HW, int C, int ldy, void* stream) {
    if (!x || !y || C % 8 || ((uintptr_t)x % 16) != 0) return -1;
    hipLaunchKernelGGL(avgpool_relu_bf16_kernel, dim3((N * (C / 8) + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y, N, HW, C, ldy);
    return (int)hipGetLastError();
}

extern "C" int ihmr_cast_f32_bf16(const float* x, uint16_t* y, size_t n, void* stream) {
    if (!x || !y) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ evaluator
extern "C" int ihmr_eval_metrics(const float* pred_joints_3d, const float* gt_joints_3d, const float* coll_origin_scale,
                                 const float* sample_scale, const unsigned char* interacting, int B, double* out6, void* stream) {
    if (!pred_joints_3d || !gt_joints_3d || !coll_origin_scale || !out6 || B <= 0) return -1;
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pred_joints_3d, gt_joints_3d, coll_origin_scale,
                       sample_scale, interacting, B, out6);
    return (int)hipGetLastError();
}

extern "C" int ihmr_eval_mpvpe(const float* pred_right, const float* pred_left, const float* gt_right, const float* gt_left,
                               const float* root_weights, const float* mano_params_weight, const float* sample_scale, int B,
                               double* out4, void* stream) {
    if (!pred_right || !pred_left || !gt_right || !gt_left || !root_weights || !mano_params_weight || !out4 || B <= 0) return -1;
    hipLaunchKernelGGL(eval_mpvpe_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, pred_right, pred_left, gt_right, gt_left,
                       root_weights, mano_params_weight, sample_scale, B, out4);
    return (int)hipGetLastError();
}

extern "C" int ihmr_eval_pa_joints(const float* pred_joints_3d, const float* gt_joints_3d, const float* sample_scale, int B, double* out,
                                   double* point_err, void* stream) {
    if (!pred_joints_3d || !gt_joints_3d || !out || B <= 0) return -1;
    hipLaunchKernelGGL(eval_pa_joints_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pred_joints_3d, gt_joints_3d, sample_scale, B,
                       out, point_err);
    return (int)hipGetLastError();
}

extern "C" int ihmr_eval_pa_verts(const float* pred_right, const float* pred_left, const float* gt_right, const float* gt_left,
                                  const float* mano_params_weight, const float* sample_scale, int B, double* out, double* point_err,
                                  void* stream) {
    if (!pred_right || !pred_left || !gt_right || !gt_left || !mano_params_weight || !out || B <= 0) return -1;
    hipLaunchKernelGGL(eval_pa_verts_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, pred_right, pred_left, gt_right, gt_left,
                       mano_params_weight, sample_scale, B, out, point_err);
    return (int)hipGetLastError();
}

extern "C" int ihmr_eval_curve_joints(const float* pred_joints_3d, const float* gt_joints_3d, const float* sample_scale, int B,
                                      const double* thresholds, int T, double* counts, void* stream) {
    if (!pred_joints_3d || !gt_joints_3d || !thresholds || !counts || B <= 0 || T < 1 || T > IHMR_EVAL_MAX_THRESHOLDS) return -1;
    hipLaunchKernelGGL(eval_curve_joints_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pred_joints_3d, gt_joints_3d, sample_scale,
                       B, thresholds, T, counts);
    return (int)hipGetLastError();
}

extern "C" int ihmr_eval_curve_verts(const float* pred_right, const float* pred_left, const float* gt_right, const float* gt_left,
                                     const float* root_weights, const float* mano_params_weight, const float* sample_scale, int B,
                                     const double* thresholds, int T, const double* f_thresholds, int F, double* counts,
                                     double* f_counts, double* nn_dist, void* stream) {
    if (!pred_right || !pred_left || !gt_right || !gt_left || !root_weights || !mano_params_weight || !thresholds || !counts || B <= 0)
        return -1;
    if (T < 1 || T > IHMR_EVAL_MAX_THRESHOLDS || F < 0 || F > IHMR_EVAL_MAX_F_THRESHOLDS || (F > 0 && (!f_thresholds || !f_counts))) return -1;
    hipLaunchKernelGGL(eval_curve_verts_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, pred_right, pred_left, gt_right, gt_left,
                       root_weights, mano_params_weight, sample_scale, B, thresholds, T, f_thresholds, F, counts, f_counts, nn_dist);
    return (int)hipGetLastError();
}

extern "C" int ihmr_eval_mrrpe(const float* pred_joints_3d, const float* gt_joints_3d, const float* sample_scale,
                               const unsigned char* interacting, int B, double* out, void* stream) {
    if (!pred_joints_3d || !gt_joints_3d || !out || B < 1) return -1;
    hipLaunchKernelGGL(eval_mrrpe_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred_joints_3d, gt_joints_3d, sample_scale,
                       interacting, B, out);
    return (int)hipGetLastError();
}

static_assert(CTP_MAX_K == IHMR_EVAL_MAX_CONTACT_THRESHOLDS, "contact_pure.h and ihmr_hip.h name one limit");
extern "C" int ihmr_eval_contact(const float* pred_right, const float* pred_left, const float* gt_right, const float* gt_left,
                                 const float* mano_params_weight, const float* sample_scale, const unsigned char* use, int B,
                                 const double* thresholds, int K, double* pair_out, double* count_out, double* near, void* stream) {
    if (!pred_right || !pred_left || !gt_right || !gt_left || !mano_params_weight || !thresholds || !pair_out || !count_out || B < 1)
        return -1;
    if (K < 1 || K > IHMR_EVAL_MAX_CONTACT_THRESHOLDS) return -1;
    hipLaunchKernelGGL(eval_contact_kernel, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, pred_right, pred_left, gt_right, gt_left,
                       mano_params_weight, sample_scale, use, B, thresholds, K, pair_out, count_out, near);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ IHMR-MLP training step
extern "C" int ihmr_sdf_volume(const float* verts_a, const int32_t* faces_a, int n_verts_a, int n_faces_a, const float* verts_b,
                               const int32_t* faces_b, int n_verts_b, int n_faces_b, int B, int subdiv, const uint8_t* keep, float* box,
                               int32_t* status, uint32_t* counts, uint32_t* bits, void* stream) {
    return vol_launch(verts_a, faces_a, n_verts_a, n_faces_a, verts_b, faces_b, n_verts_b, n_faces_b, B, subdiv, keep, box, status,
                      counts, bits, (hipStream_t)stream);
}

extern "C" int ihmr_surface_distance(const float* points, int P, const float* verts, int V, const int32_t* faces, int F_dist, int F_total,
                                     const uint8_t* use, int B, int is_signed, double* dist, int32_t* face, double* bary, void* stream) {
    return srf_launch(points, P, verts, V, faces, F_dist, F_total, use, B, is_signed, dist, face, bary, (hipStream_t)stream);
}

extern "C" int ihmr_surface_distance_bwd(const float* points, int P, const float* verts, int V, const int32_t* faces, int F_dist,
                                         int F_total, const uint8_t* use, int B, const double* dist, const int32_t* face,
                                         const double* bary, const double* g_dist, float* d_points, float* d_verts, void* stream) {
    return srf_launch_bwd(points, P, verts, V, faces, F_dist, F_total, use, B, dist, face, bary, g_dist, d_points, d_verts,
                          (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ MANO layer: pose space and output stage
// (include/ihmr_mano_ext.h)
extern "C" int ihmr_mano_pca_fwd(const float* coeffs, const float* comps, int N, int K, float* pose45, void* stream) {
    return mps_pca_fwd_launch(coeffs, comps, N, K, pose45, (hipStream_t)stream);
}

extern "C" int ihmr_mano_pca_bwd(const float* d_pose45, const float* comps, int N, int K, float* d_coeffs, void* stream) {
    return mps_pca_bwd_launch(d_pose45, comps, N, K, d_coeffs, (hipStream_t)stream);
}

extern "C" int ihmr_mano_post_fwd(const float* verts_in, const float* joints16_in, const float* transl, const int32_t* tip_ids, int N,
                                  float* verts_out, float* joints_out, void* stream) {
    return mps_post_fwd_launch(verts_in, joints16_in, transl, tip_ids, N, verts_out, joints_out, (hipStream_t)stream);
}

extern "C" int ihmr_mano_post_bwd(const float* d_verts_out, const float* d_joints_out, const int32_t* tip_ids, int N, float* d_verts_in,
                                  float* d_joints16, float* d_transl, void* stream) {
    return mps_post_bwd_launch(d_verts_out, d_joints_out, tip_ids, N, d_verts_in, d_joints16, d_transl, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ IHMR-MLP training gradient
extern "C" int ihmr_mlp_train_grad(const ihmr_mano* m, const ihmr_mano* m_left, const ihmr_opt_io* io, int B,
                                   const ihmr_opt_weights* w, const ihmr_train_weights* tw, const float* gt_pose,
                                   const float* gt_shape, const float* params_weight, const float* init_shape,
                                   const float* trans_weight_mean, float* grad122, float* terms5, const int32_t* out_cols,
                                   int n_out, float* d_out, int ld_out, void* stream) {
    if (!m || !io || !w || !tw || !gt_pose || !gt_shape || !params_weight || !init_shape || !grad122 || !terms5 || B <= 0 ||
        (d_out && (!out_cols || n_out <= 0 || ld_out < n_out)))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    OptWork wk = opt_carve(io->workspace, B);
    int rc = run_iteration(OptCtx{m, m_left, io, wk, B, w, st, nullptr}, plan::kForwardBackward, kNoStep, kNoStep);
    if (rc) return rc;
    hipLaunchKernelGGL(mlp_train_grad_kernel, dim3(B), dim3(128), 0, st, *io, wk, B, *tw, gt_pose, gt_shape, params_weight, init_shape,
                       trans_weight_mean, grad122, terms5, out_cols, n_out, d_out, ld_out);
    return (int)hipGetLastError();
}

extern "C" int ihmr_transpose(const float* x, float* y, int rows, int cols, int ldx, int ldy, void* stream) {
    if (!x || !y || rows <= 0 || cols <= 0 || ldx < cols || ldy < rows) return -1;
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, (hipStream_t)stream, x, y, rows, cols, ldx,
                       ldy);
    return (int)hipGetLastError();
}

extern "C" int ihmr_relu_backward(float* dx, const float* y, int rows, int cols, int ld_dx, int ld_y, void* stream) {
    if (!dx || !y || rows <= 0 || cols <= 0) return -1;
    const long total = (long)rows * cols;
    if (ld_dx == cols && ld_y == cols && total % 4 == 0 && ((uintptr_t)dx % 16) == 0 && ((uintptr_t)y % 16) == 0)
        hipLaunchKernelGGL(relu_backward4_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float4*)dx,
                           (const float4*)y, total / 4);
    else
        hipLaunchKernelGGL(relu_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, y, rows, cols, ld_dx,
                           ld_y);
    return (int)hipGetLastError();
}

extern "C" int ihmr_colsum(const float* x, float* out, int rows, int cols, int ldx, void* stream) {
    if (!x || !out || rows <= 0 || cols <= 0) return -1;
    hipLaunchKernelGGL(colsum_kernel, dim3((cols + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, out, rows, cols, ldx);
    return (int)hipGetLastError();
}

extern "C" int ihmr_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, float grad_scale,
                              float lr, float beta1, float beta2, float eps, int step, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n == 0 || step <= 0) return -1;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, n, grad_scale, beta1, beta2, eps, (float)((double)lr / bc1), (float)sqrt(bc2));
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ encoder training kernels
static dim3 bn_grid(int C, int S) { return dim3((unsigned)((C / 4 + 255) / 256), (unsigned)S); }

extern "C" size_t ihmr_bn_workspace_bytes(int C) { return (size_t)BN_MAX_CHUNKS * 2 * C * sizeof(float) + (size_t)2 * C * sizeof(float); }

extern "C" int ihmr_bn_train_forward(const float* z, long M, int C, const float* gamma, const float* beta, const float* residual,
                                     int relu, float eps, float* y, float* mean, float* var, float* invstd, float* running_mean,
                                     float* running_var, float momentum, void* workspace, void* stream) {
    if (!z || !gamma || !beta || !y || !mean || !var || !invstd || !workspace || M <= 0 || C <= 0 || C % 4) return -1;
    hipStream_t st = (hipStream_t)stream;
    const plan::BnChunks ch = plan::plan_bn_chunks(M);
    const int S = ch.chunks, rows_per = ch.rows_per;
    float* part = (float*)workspace;
    const dim3 grid = bn_grid(C, S);
    // two passes over z: sum z -> mean (chunks added in double), then sum (z - mean)^2 -> biased variance / invstd / running statistics
    hipLaunchKernelGGL(bn_partial_kernel<0>, grid, dim3(256), 0, st, z, (const float*)nullptr, (int)M, C, C, C, rows_per,
                       (const float*)nullptr, (const float*)nullptr, part, (const float*)nullptr);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((C + 15) / 16), dim3(256), 0, st, (const float*)part, S, 1, C, 1.0 / (double)M, mean,
                       (float*)nullptr, 0.f, (float*)nullptr);
    hipLaunchKernelGGL(bn_partial_kernel<1>, grid, dim3(256), 0, st, z, (const float*)nullptr, (int)M, C, C, C, rows_per,
                       (const float*)mean, (const float*)nullptr, part, (const float*)nullptr);
    hipLaunchKernelGGL(bn_finish_stats_kernel, dim3((C + 15) / 16), dim3(256), 0, st, (const float*)part, S, C, M, (const float*)mean, var,
                       invstd, eps, running_mean, running_var, momentum);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((M * (C / 4) + 255) / 256)), dim3(256), 0, st, z, (const float*)mean,
                       (const float*)invstd, gamma, beta, residual, y, M, C, relu);
    return (int)hipGetLastError();
}

extern "C" int ihmr_bn_train_backward(const float* z, const float* g, long M, int C, const float* mean, const float* invstd,
                                      const float* gamma, const float* relu_y, float* dz, float* dgamma, float* dbeta, void* workspace,
                                      void* stream) {
    if (!z || !g || !mean || !invstd || !gamma || !dz || !dgamma || !dbeta || !workspace || M <= 0 || C <= 0 || C % 4) return -1;
    hipStream_t st = (hipStream_t)stream;
    const plan::BnChunks ch = plan::plan_bn_chunks(M);
    const int S = ch.chunks, rows_per = ch.rows_per;
    float* part = (float*)workspace;
    // sum g -> dbeta, sum g * xhat -> dgamma (written by the finish kernel itself, read back by the apply kernel)
    hipLaunchKernelGGL(bn_partial_kernel<2>, bn_grid(C, S), dim3(256), 0, st, z, g, (int)M, C, C, C, rows_per, mean, invstd, part, relu_y);
    hipLaunchKernelGGL(bn_finish_kernel, dim3((2 * C + 15) / 16), dim3(256), 0, st, (const float*)part, S, 2, C, 1.0, dbeta,
                       (float*)nullptr, 0.f, dgamma);
    hipLaunchKernelGGL(bn_backward_apply_kernel, dim3((unsigned)((M * (C / 4) + 255) / 256)), dim3(256), 0, st, z, g, mean, invstd, gamma,
                       (const float*)dbeta, (const float*)dgamma, dz, M, C, relu_y);
    return (int)hipGetLastError();
}

static const TileKernel<WgradArgs> kWgradKernels[] = {{128, 128, 0, conv_wgrad_kernel<128, 128>}, {128, 64, 0, conv_wgrad_kernel<128, 64>},
                                                      {64, 128, 0, conv_wgrad_kernel<64, 128>},   {64, 64, 0, conv_wgrad_kernel<64, 64>}};

extern "C" int ihmr_conv_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                               int kh, int kw, int stride, int pad, int ldx, int lddy, int ldw, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!x || !dy || !dw || !workspace) return -1;
    hipStream_t st = (hipStream_t)stream;
    const plan::WgradPlan p = plan::plan_conv_wgrad(N, Cin, Ho, Wo, Cout, kh, kw, ldx, lddy, ldw, workspace_bytes);
    if (!p.ok) return -1;
    const int K = kh * kw * Cin;
    WgradArgs a{x, dy, (float*)workspace, N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, ldx, lddy, p.chunks_per};
    void (*kernel)(WgradArgs) = tile_kernel(kWgradKernels, p.bm, p.bn, 0);
    if (!kernel) return -1;
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(p.threads), 0, st, a);
    // fixed-order sum of the pixel-range partials into dw [K][ldw]
    ConvArgs r{nullptr, nullptr, nullptr, nullptr, dw, K, 1, 1, 0, 1, 1, Cout, 1, 1, 1, 0, 0, 0, ldw, 0, 0, (float*)workspace, p.msplit};
    if (p.reduce == plan::WGRAD_REDUCE)
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(((long)K * (Cout / 4) + 15) / 16)), dim3(256), 0, st, (const float*)workspace, dw, K,
                           Cout, ldw, p.msplit);
    else if (p.reduce == plan::WGRAD_SPLITK4) hipLaunchKernelGGL(conv_splitk_reduce_kernel<4>, dim3((unsigned)(((long)K * (Cout / 4) + 255) / 256)), dim3(256), 0, st, r);
    else hipLaunchKernelGGL(conv_splitk_reduce_kernel<1>, dim3((unsigned)(((long)K * Cout + 255) / 256)), dim3(256), 0, st, r);
    return (int)hipGetLastError();
}

extern "C" int ihmr_pack_dgrad_weight(const float* w, float* out, int kh, int kw, int Cin, int Cout, int ldw, int ldo, void* stream) {
    if (!w || !out || ldw < Cout || ldo < Cin) return -1;
    const long total = (long)kh * kw * Cout * Cin;
    hipLaunchKernelGGL(pack_dgrad_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, out, kh, kw, Cin,
                       Cout, ldw, ldo);
    return (int)hipGetLastError();
}

extern "C" int ihmr_interleave2(const float* p00, const float* p01, const float* p10, const float* p11, float* dx, int N, int Ho, int Wo,
                                int C, void* stream) {
    if (!p00 || !p01 || !p10 || !p11 || !dx || C % 4) return -1;
    const long total = (long)N * 2 * Ho * 2 * Wo * (C / 4);
    hipLaunchKernelGGL(interleave2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p00, p01, p10, p11, dx, N,
                       Ho, Wo, C);
    return (int)hipGetLastError();
}

extern "C" int ihmr_dilate2(const float* dy, float* out, int N, int Ho, int Wo, int C, void* stream) {
    if (!dy || !out || C % 4) return -1;
    const long total = (long)N * 2 * Ho * 2 * Wo * (C / 4);
    hipLaunchKernelGGL(dilate2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, out, N, Ho, Wo, C);
    return (int)hipGetLastError();
}

extern "C" int ihmr_maxpool3x3s2_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int Ho, int Wo,
                                          void* stream) {
    if (!x || !dy || !dx || C % 4) return -1;
    const long total = (long)N * H * W * (C / 4);
    hipLaunchKernelGGL(maxpool3x3s2_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, N, H,
                       W, C, Ho, Wo);
    return (int)hipGetLastError();
}

extern "C" int ihmr_avgpool_relu_backward(const float* y, const float* dy, float* dx, int N, int HW, int C, int ldy, void* stream) {
    if (!y || !dy || !dx) return -1;
    const long total = (long)N * HW * C;
    hipLaunchKernelGGL(avgpool_relu_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, dy, dx, N, HW,
                       C, ldy);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ image preprocessing
extern "C" int ihmr_preprocess_images(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const uint8_t* do_flip,
                                      int B, int final_size, float* img_out, uint8_t* img_u8, const float* joints_in,
                                      float* joints_out, void* stream) {
    if (!pixels || !offsets || !sizes || !img_out || B <= 0 || final_size <= 0 || final_size % PRE_PPT || (joints_in && !joints_out))
        return -1;
    hipLaunchKernelGGL(preprocess_kernel, dim3((final_size * final_size / PRE_PPT + PRE_THREADS - 1) / PRE_THREADS, B), dim3(PRE_THREADS), 0,
                       (hipStream_t)stream, pixels, offsets, sizes, do_flip, final_size, img_out, img_u8, joints_in, joints_out, 1);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ training-time augmentation
extern "C" int ihmr_augment_images(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, const ihmr_aug_params* params,
                                   int B, int final_size, int steps, const float* blur_bank, const int32_t* blur_dims, int n_blur,
                                   uint8_t* buf0, uint8_t* buf1, uint32_t* gray_sums, float* img_out, int* final_buffer, void* stream) {
    const int S = final_size;
    if (!pixels || !offsets || !sizes || !params || !buf0 || !buf1 || !img_out || !final_buffer || B <= 0 || S <= 0 || S % PRE_PPT || S > 4096)
        return -1;
    if ((steps & IHMR_AUG_COLOR) && !gray_sums) return -1;
    if ((steps & IHMR_AUG_BLUR) && (!blur_bank || !blur_dims || n_blur <= 0)) return -1;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((S * S / PRE_PPT + AUG_THREADS - 1) / AUG_THREADS, B), block(AUG_THREADS);
    int left = !!(steps & IHMR_AUG_RESCALE) + !!(steps & IHMR_AUG_ROTATE) + !!(steps & IHMR_AUG_COLOR) + !!(steps & IHMR_AUG_BLUR);
    uint8_t *cur = buf0, *nxt = buf1;
    // pad, resize, flip: the test-time kernel through its uint8 output; it writes the float planes itself when no step follows
    hipLaunchKernelGGL(preprocess_kernel, grid, block, 0, st, pixels, offsets, sizes, reinterpret_cast<const uint8_t*>(&params->flip), S,
                       left ? (float*)nullptr : img_out, cur, (const float*)nullptr, (float*)nullptr, (int)sizeof(ihmr_aug_params));
    if (steps & IHMR_AUG_RESCALE) {
        hipLaunchKernelGGL(aug_rescale_kernel, grid, block, 0, st, cur, nxt, --left ? (float*)nullptr : img_out, params, S);
        std::swap(cur, nxt);
    }
    if (steps & IHMR_AUG_ROTATE) {
        hipLaunchKernelGGL(aug_rotate_kernel, grid, block, 0, st, cur, nxt, --left ? (float*)nullptr : img_out, params, S);
        std::swap(cur, nxt);
    }
    if (steps & IHMR_AUG_COLOR) {
        if (hipMemsetAsync(gray_sums, 0, sizeof(uint32_t) * (size_t)B, st) != hipSuccess) return (int)hipGetLastError();
        hipLaunchKernelGGL(aug_gray_sum_kernel, grid, block, 0, st, cur, params, S, gray_sums);
        hipLaunchKernelGGL(aug_color_kernel, grid, block, 0, st, cur, nxt, --left ? (float*)nullptr : img_out, params, S, gray_sums);
        std::swap(cur, nxt);
    }
    if (steps & IHMR_AUG_BLUR) {
        const int tiles = (S + AUG_BLUR_TILE - 1) / AUG_BLUR_TILE;
        hipLaunchKernelGGL(aug_blur_kernel, dim3(tiles * tiles, B), block, 0, st, cur, nxt, --left ? (float*)nullptr : img_out, params, S,
                           blur_bank, blur_dims, n_blur);
        std::swap(cur, nxt);
    }
    *final_buffer = cur == buf0 ? 0 : 1;
    return (int)hipGetLastError();
}

extern "C" int ihmr_augment_labels(const int32_t* sizes, const ihmr_aug_params* params, int B, int final_size, const float* joints_2d,
                                   const float* joints_3d, const float* mano_pose, const float* mano_betas, const float* mano_params_weight,
                                   const float* hand_type_array, float* out_joints_2d, float* out_joints_3d, float* out_mano_pose,
                                   float* out_mano_betas, float* out_mano_params_weight, float* out_hand_type_array, float* out_do_flip,
                                   float* out_hand_trans, void* stream) {
    if (!sizes || !params || B <= 0 || final_size <= 0 || !joints_2d || !joints_3d || !mano_pose || !mano_betas || !mano_params_weight ||
        !hand_type_array || !out_joints_2d || !out_joints_3d || !out_mano_pose || !out_mano_betas || !out_mano_params_weight ||
        !out_hand_type_array || !out_do_flip || !out_hand_trans)
        return -1;
    hipLaunchKernelGGL(aug_labels_kernel, dim3(B), dim3(AUG_LABEL_THREADS), 0, (hipStream_t)stream, sizes, params, final_size, joints_2d,
                       joints_3d, mano_pose, mano_betas, mano_params_weight, hand_type_array, out_joints_2d, out_joints_3d, out_mano_pose,
                       out_mano_betas, out_mano_params_weight, out_hand_type_array, out_do_flip, out_hand_trans);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ visualisation: mesh renderer
extern "C" size_t ihmr_render_workspace_bytes(int B, int n_verts) {
    return B > 0 && n_verts > 0 ? sizeof(rnd_vertex) * (size_t)B * (size_t)n_verts : 0;
}

// both forms of the render: `albedo` per hand (B,2,3) or per vertex (B,n_verts,3)
static int render_launch(bool per_vertex, const float* verts, const int32_t* faces, const int32_t* csr_offsets, const int32_t* csr_ids,
                         int n_verts, int n_faces, int face_split, const uint8_t* present, const float* albedo, const float* cam,
                         const ihmr_render_lights* lights, const uint8_t* background, int S, uint8_t* out_img, int32_t* out_face_ids,
                         void* workspace, int B, void* stream) {
    if (!verts || !faces || !csr_offsets || !csr_ids || !albedo || !cam || !lights || !out_img || !workspace) return -1;
    if (B <= 0 || B > 65535 || n_verts <= 0 || n_faces <= 0 || n_faces > (1 << 24) || n_verts > (1 << 24) || face_split < 0 ||
        face_split > n_faces || S < 16 || S > 2048)
        return -1;
    if ((uintptr_t)workspace & 3u) return -1;
    const hipStream_t st = (hipStream_t)stream;
    rnd_vertex* ws = static_cast<rnd_vertex*>(workspace);
    const dim3 vgrid((n_verts + RND_THREADS - 1) / RND_THREADS, B);
    if (per_vertex)
        hipLaunchKernelGGL(paint_vertex_kernel, vgrid, dim3(RND_THREADS), 0, st, verts, faces, csr_offsets, csr_ids, n_verts, n_faces,
                           face_split, albedo, cam, *lights, S, ws);
    else
        hipLaunchKernelGGL(render_vertex_kernel, vgrid, dim3(RND_THREADS), 0, st, verts, faces, csr_offsets, csr_ids, n_verts, n_faces,
                           face_split, albedo, cam, *lights, S, ws);
    const int tiles = (S + RND_TILE - 1) / RND_TILE;
    // whole 12-byte runs as three dwords when every run is complete and aligned
    const int vec = S % RND_PPT == 0 && !((uintptr_t)out_img & 3u) && !((uintptr_t)background & 3u);
    hipLaunchKernelGGL(render_raster_kernel, dim3(tiles * tiles, B), dim3(RND_THREADS), 0, st, ws, faces, n_verts, n_faces, face_split,
                       present, background, S, vec, out_img, out_face_ids);
    return (int)hipGetLastError();
}

extern "C" int ihmr_render_meshes(const float* verts, const int32_t* faces, const int32_t* csr_offsets, const int32_t* csr_ids, int n_verts,
                                  int n_faces, int face_split, const uint8_t* present, const float* albedo, const float* cam,
                                  const ihmr_render_lights* lights, const uint8_t* background, int S, uint8_t* out_img,
                                  int32_t* out_face_ids, void* workspace, int B, void* stream) {
    return render_launch(false, verts, faces, csr_offsets, csr_ids, n_verts, n_faces, face_split, present, albedo, cam, lights, background, S,
                         out_img, out_face_ids, workspace, B, stream);
}

extern "C" int ihmr_paint_meshes(const float* verts, const int32_t* faces, const int32_t* csr_offsets, const int32_t* csr_ids, int n_verts,
                                 int n_faces, int face_split, const uint8_t* present, const float* vertex_albedo, const float* cam,
                                 const ihmr_render_lights* lights, const uint8_t* background, int S, uint8_t* out_img,
                                 int32_t* out_face_ids, void* workspace, int B, void* stream) {
    return render_launch(true, verts, faces, csr_offsets, csr_ids, n_verts, n_faces, face_split, present, vertex_albedo, cam, lights,
                         background, S, out_img, out_face_ids, workspace, B, stream);
}

extern "C" int ihmr_view_vertices(const float* verts, const uint8_t* present, int n_verts, int n_split, const float* rot, int rot_per_sample,
                                  const float* pivot, float* out, int B, void* stream) {
    if (!verts || !rot || !out) return -1;
    if (B <= 0 || B > 65535 || n_verts <= 0 || n_verts > (1 << 24) || n_split < 0 || n_split > n_verts || (rot_per_sample != 0 && rot_per_sample != 1))
        return -1;
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)n_verts * 12u, a = (uintptr_t)verts, o = (uintptr_t)out;
    if (a < o + bytes && o < a + bytes) return -1;                              // in place or overlapping: a vertex would be read after it was written
    hipLaunchKernelGGL(view_vertices_kernel, dim3(B), dim3(RND_THREADS), 0, (hipStream_t)stream, verts, present, n_verts, n_split, rot,
                       rot_per_sample, pivot, out);
    return (int)hipGetLastError();
}

extern "C" int ihmr_heat_colours(const float* depth, const float* albedo, const float* hot, float lo, float hi, int n_verts, int n_split,
                                 int layout, float* out, int B, void* stream) {
    if (!depth || !albedo || !hot || !out) return -1;
    if (B <= 0 || B > 65535 || n_verts <= 0 || n_verts > (1 << 24) || n_split < 0 || n_split > n_verts) return -1;
    if (!rnd_finite(lo) || !rnd_finite(hi) || !(hi > lo)) return -1;
    if (layout != 0 && layout != 1) return -1;
    if (layout == 1 && n_verts != 2 * n_split) return -1;
    hipLaunchKernelGGL(heat_colours_kernel, dim3((n_verts + RND_THREADS - 1) / RND_THREADS, B), dim3(RND_THREADS), 0, (hipStream_t)stream,
                       depth, albedo, hot[0], hot[1], hot[2], lo, hi, n_verts, n_split, layout, out);
    return (int)hipGetLastError();
}

extern "C" int ihmr_draw_keypoints(uint8_t* img, const float* kps, const float* weight, const uint8_t* colour, int B, int S, int K,
                                   void* stream) {
    if (!img || !kps || !weight || !colour || B <= 0 || S <= 0 || S > 4096 || K <= 0) return -1;
    hipLaunchKernelGGL(draw_keypoints_kernel, dim3(B), dim3(RND_KP_THREADS), 0, (hipStream_t)stream, img, kps, weight, (int)colour[0],
                       (int)colour[1], (int)colour[2], S, K);
    return (int)hipGetLastError();
}

extern "C" int ihmr_copy_segments(const ihmr_copy_seg* segs, int n, void* stream) {
    if (!segs || n <= 0 || n > IHMR_COPY_MAX_SEGS) return -1;
    CopySegTable t;
    memset(&t, 0, sizeof(t));
    long biggest = 0;
    for (int i = 0; i < n; ++i) {
        const ihmr_copy_seg& g = segs[i];
        if (!g.src || !g.dst || g.rows <= 0 || g.width <= 0 || g.src_ld < g.width || g.dst_ld < g.width) return -1;
        if (((uintptr_t)g.src | (uintptr_t)g.dst) & 3u) return -1;
        t.s[i] = g;
        biggest = std::max(biggest, (long)g.rows * g.width);
    }
    const unsigned bx = (unsigned)std::max<long>(1, std::min<long>(64, (biggest + 1023) / 1024));
    hipLaunchKernelGGL(copy_segments_kernel, dim3(bx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, t);
    return (int)hipGetLastError();
}

extern "C" int ihmr_root_align_joints(const float* joints4, float* out4, int B, void* stream) {
    if (!joints4 || !out4 || B <= 0) return -1;
    hipLaunchKernelGGL(root_align_joints_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, joints4, out4, B);
    return (int)hipGetLastError();
}

extern "C" int ihmr_set_kernel_timer(ihmr_kernel_timer* t) {
    std::lock_guard<std::mutex> lk(g_timer_mutex);
    g_timer = t;
    return 0;
}

extern "C" int ihmr_flush_kernel_timer(void) {
    std::lock_guard<std::mutex> lk(g_timer_mutex);
    for (auto& p : g_pending) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(p.b));
        HIP_TRY(hipEventElapsedTime(&ms, p.a, p.b));
        if (g_timer) {
            if (p.k < 0) { g_timer->ms_event_pair += ms; g_timer->n_event_pair += 1; }
            else if (p.k < IHMR_TIMED_KERNELS) { g_timer->ms[p.k] += ms; g_timer->n[p.k] += 1; }
        }
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    g_pending.clear();
    return 0;
}


#ifdef SDF_STAMPS
// experiment builds only (scripts/sdf_stamps.py): zero = 1 clears the per-wave phase sums, zero = 0 copies them to the host (4096 * (4 * 12 + 8 + 4) int64: g_sdf_stamps, g_sdf_span, g_sdf_prep, g_sdf_prep2)
extern "C" int ihmr_debug_stamps(long long* host, int zero) {
    HIP_TRY(hipDeviceSynchronize());
    if (zero) {
        void* p; HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_sdf_stamps))); HIP_TRY(hipMemset(p, 0, sizeof(long long) * 4096 * 4 * 8));
        HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_sdf_prep))); HIP_TRY(hipMemset(p, 0, sizeof(long long) * 4096 * 8));
        HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_sdf_prep2))); HIP_TRY(hipMemset(p, 0, sizeof(long long) * 4096 * 4));
        return 0;
    }
    HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_sdf_stamps), sizeof(long long) * 4096 * 4 * 8));
    HIP_TRY(hipMemcpyFromSymbol(host + 4096 * 4 * 8, HIP_SYMBOL(g_sdf_span), sizeof(long long) * 4096 * 4 * 4));
    HIP_TRY(hipMemcpyFromSymbol(host + 4096 * 4 * 12, HIP_SYMBOL(g_sdf_prep), sizeof(long long) * 4096 * 8));
    HIP_TRY(hipMemcpyFromSymbol(host + 4096 * 4 * 12 + 4096 * 8, HIP_SYMBOL(g_sdf_prep2), sizeof(long long) * 4096 * 4));
    return 0;
}
#endif

#ifdef SDF_QMASK_CHECK
// device pointers of the collision workspace of a fused-loop io: qcell, inside_bits, box, phi
extern "C" int ihmr_debug_sdf_ptrs(const ihmr_opt_io* io, int B, void** out4) {
    SdfWorkspace ws = sdf_carve(opt_carve(io->workspace, B).sdf_ws, 2 * B, true);
    out4[0] = ws.qcell; out4[1] = ws.inside_bits; out4[2] = ws.box; out4[3] = ws.phi;
    return 0;
}
extern "C" int ihmr_debug_qmask(unsigned* host8) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return (int)hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_qmask_bad), 32);
}
#endif

#ifdef SDF_HANDLOG
// experiment builds only: cap > 0 -- allocate a log of `cap` records and start; cap == 0 -- copy the records out ([n][4] uint32: hand,
// voxels with a candidate list, voxels for the full search, bit 0 lists reused | bit 1 static hand), n = return value
extern "C" long ihmr_debug_handlog(unsigned* host, long cap) {
    static uint4* buf = nullptr;
    static unsigned cap_now = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (cap > 0) {
        if (buf) (void)hipFree(buf);
        if (hipMalloc(&buf, (size_t)cap * 16) != hipSuccess) return -1;
        cap_now = (unsigned)cap;
        const unsigned zero = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_handlog_n), &zero, 4) != hipSuccess) return -1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_handlog_cap), &cap_now, 4) != hipSuccess) return -1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_handlog), &buf, 8) != hipSuccess) return -1;
        return 0;
    }
    unsigned n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_handlog_n), 4) != hipSuccess) return -1;
    if (n > cap_now) n = cap_now;
    if (n && hipMemcpy(host, buf, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    uint4* null = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_handlog), &null, 8);
    return (long)n;
}
#endif

#ifdef CONV_STAMPS
// experiment builds only (scripts/experiments/conv_stamps.py): zero = 1 clears, zero = 0 copies the 1024 x 10 phase sums of conv_streamk_kernel out
extern "C" int ihmr_debug_conv_stamps(long long* host, int zero) {
    HIP_TRY(hipDeviceSynchronize());
    void* p;
    HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_conv_stamps)));
    if (zero) { HIP_TRY(hipMemset(p, 0, sizeof(long long) * 1024 * 10)); return 0; }
    HIP_TRY(hipMemcpy(host, p, sizeof(long long) * 1024 * 10, hipMemcpyDeviceToHost));
    return 0;
}
#endif

#ifdef TAIL_STAMPS
// experiment builds only (scripts/tail_stamps.py): zero = 1 clears, zero = 0 copies the 3 x 4096 x 8 phase sums of opt_tail_kernel out
extern "C" int ihmr_debug_tail_stamps(long long* host, int zero) {
    HIP_TRY(hipDeviceSynchronize());
    void *p, *q;
    HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_tail_stamps)));
    HIP_TRY(hipGetSymbolAddress(&q, HIP_SYMBOL(g_samp_stamps)));
    if (zero) { HIP_TRY(hipMemset(p, 0, sizeof(long long) * 3 * 4096 * 8)); HIP_TRY(hipMemset(q, 0, sizeof(long long) * 4096 * 8)); return 0; }
    HIP_TRY(hipMemcpy(host, p, sizeof(long long) * 3 * 4096 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host + 3 * 4096 * 8, q, sizeof(long long) * 4096 * 8, hipMemcpyDeviceToHost));      // the sampler's own phases
    return 0;
}
#endif

#ifdef BWD2_STAMPS
// experiment builds only (scripts/bwd2_stamps.py): zero = 1 clears, zero = 0 copies the 1024 x 8 phase sums of lbs_bwd2_lds_kernel out
extern "C" int ihmr_debug_bwd2_stamps(long long* host, int zero) {
    HIP_TRY(hipDeviceSynchronize());
    void* p;
    HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(g_bwd2_stamps)));
    if (zero) { HIP_TRY(hipMemset(p, 0, sizeof(long long) * 1024 * 8)); return 0; }
    HIP_TRY(hipMemcpy(host, p, sizeof(long long) * 1024 * 8, hipMemcpyDeviceToHost));
    return 0;
}
#endif

#ifdef IHMR_TIMELINE
// experiment builds only (scripts/timeline_wg.py): cap > 0 -- allocate a ring of `cap` workgroup records (256 segments) and start
// recording; cap == 0 -- copy the records out (host: [n][3] uint64, n = return value) and stop
extern "C" long ihmr_debug_timeline(unsigned long long* host, long cap) {
    static unsigned long long* ring = nullptr;
    static unsigned seg_cap = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    void* cur = nullptr;
    if (hipGetSymbolAddress(&cur, HIP_SYMBOL(g_tl_cursor)) != hipSuccess) return -1;
    if (cap > 0) {
        if (ring) (void)hipFree(ring);
        seg_cap = (unsigned)(cap / 256);
        if (hipMalloc(&ring, (size_t)seg_cap * 256 * 24) != hipSuccess) return -1;
        if (hipMemset(cur, 0, 256 * 32 * 4) != hipSuccess) return -1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_tl_cap), &seg_cap, 4) != hipSuccess) return -1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_tl_ring), &ring, 8) != hipSuccess) return -1;
        return 0;
    }
    static unsigned counts[256 * 32];
    if (hipMemcpy(counts, cur, sizeof(counts), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    long n = 0;
    for (int s = 0; s < 256; ++s) {
        const unsigned c = counts[s * 32] < seg_cap ? counts[s * 32] : seg_cap;
        if (c && hipMemcpy(host + 3 * n, ring + 3 * (size_t)s * seg_cap, (size_t)c * 24, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        n += c;
    }
    unsigned long long* null = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tl_ring), &null, 8);
    return n;
}
#endif

extern "C" const char* ihmr_version(void) { return "ihmr_hip 0.2 (gfx950)"; }

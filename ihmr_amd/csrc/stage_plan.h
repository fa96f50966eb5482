// Launch plan of the refinement loop of ihmr_hip.hip -- what a stage derives from `param_mask` and the checker switches, which launches
// one iteration makes, the per-iteration optimizer constants, the integer half of the collision workspace and the size-dependent launch
// forms next to them -- as pure functions of plain numbers: no HIP header, no pointer, no getenv, no globals, so the GPU-less container
// compiles them with g++ under AddressSanitizer / UBSan and compares them field for field with the Python restatement the stage tests
// choose their cases from (tests/test_stage_plan_cpu.py builds tests/stage_plan_driver.cpp; tests/stage_cases.py).  ihmr_opt_run_stage
// validates with stage_ok, calls plan_stage, and per iteration plan_iter + plan_step; run_iteration only launches what the IterPlan says.
#pragma once
#include <math.h>

namespace plan {

// the values of IHMR_PB_* and IHMR_OPTIM_* (include/ihmr_hip.h) and of LBS_SKIN_* (ihmr_hip.hip asserts they agree)
enum ParamBlock { PB_CAM = 1, PB_TRANS = 2, PB_ORIENT_R = 4, PB_ORIENT_L = 8, PB_POSE_R = 16, PB_POSE_L = 32, PB_SHAPE_R = 64, PB_SHAPE_L = 128 };
enum Optimizer { OPTIM_ADAM = 0, OPTIM_SGD = 1 };
// skin modes: FULL (both blends), REUSE (v_posed kept: lbs_skin_kernel), FULL_STORE_P (both blends + the pose offsets P stored: the first
// iteration of a stage that moves the shape but not the finger pose), KEEP_P (the later iterations of such a stage: no pose rows read);
// NONE: no skin launch -- the tail launch of the previous iteration has skinned the stored v_posed with the new skeletons
enum Skin { SKIN_FULL = 0, SKIN_REUSE = 1, SKIN_KEEP_P = 2, SKIN_FULL_STORE_P = 3, SKIN_NONE = 4 };
// temporal candidate lists of the collision kernels: off (single-shot callers), reuse while valid, rebuild now, KEEP = the first iteration
// of a stage whose caller vouches for the lists of the previous stage (ihmr_opt_stage::keep_lists): the static-hand bookkeeping starts
// over, a hand's lists stay while its own displacement test passes
enum Lists { LISTS_OFF = 0, LISTS_REUSE = 1, LISTS_REBUILD = 2, LISTS_KEEP = 3 };
// what closes an iteration.  NONE: nothing after the skinning (no collision term, no losses); SEPARATE: opt_sample_loss_kernel; the fused
// forms are ONE launch per sample: PLAIN opt_tail_kernel<false> (sampling + losses + LBS backward of both hands), STEP opt_tail_kernel<true>
// (+ optimizer step + next skeletons), STEP_SKIN opt_tail_kernel<true, true> (+ skinning of the next vertices), TRANS opt_tail_kernel_trans
enum Tail { TAIL_NONE = 0, TAIL_SEPARATE = 1, TAIL_PLAIN = 2, TAIL_STEP = 3, TAIL_STEP_SKIN = 4, TAIL_TRANS = 5 };
// what follows the tail: nothing, the whole LBS backward, or only lbs_bwd2 + lbs_bwd3 (the per-hand part ran inside opt_tail_kernel)
enum After { AFTER_NONE = 0, AFTER_LBS_BWD = 1, AFTER_BWD23 = 2 };

// ------------------------------------------------------------------------------------------ ihmr_opt_run_stage
// the refusal conditions on the stage struct
inline bool stage_ok(int param_mask, int optimizer, int n_iters, int save_freq, int select_loss) {
    if (n_iters <= 0 || save_freq <= 0) return false;
    if (param_mask <= 0 || param_mask > 255 || select_loss < 0 || select_loss > 2) return false;
    return optimizer == OPTIM_ADAM || optimizer == OPTIM_SGD;
}

struct StagePlan {
    int need_mask;              // what the LBS backward has to deliver (bit0 orient, bit1 pose, bit2 betas, bit3 trans)
    int need_cam;
    int vposed_fixed, pose_fixed, pose_stage;
    int first_skin, later_skin; // Skin of the first / of the later iterations
    int static_mask;            // SdfWorkspace::static_mask, and bits 2-3: sides that only translate
    int fused_tail, trans_tail, keep_rot;
    int lists_first;            // Lists of the first iteration
};

// switches: io->no_fused_tail, m->tail_fits, io->sdf_no_static_reuse (0, 1, 2), ihmr_debug_force_generic_tail; the stage's keep_lists
inline StagePlan plan_stage(int pm, int no_fused_tail, int tail_fits, int sdf_no_static_reuse, int force_generic_tail, int keep_lists) {
    StagePlan p{};
    p.need_mask = ((pm & (PB_ORIENT_R | PB_ORIENT_L)) ? 1 : 0) | ((pm & (PB_POSE_R | PB_POSE_L)) ? 2 : 0) |
                  ((pm & (PB_SHAPE_R | PB_SHAPE_L)) ? 4 : 0) | ((pm & PB_TRANS) ? 8 : 0);
    p.need_cam = (pm & PB_CAM) ? 1 : 0;
    // a stage that moves neither the finger pose nor the shape keeps v_posed: computed in its first iteration, reused after
    p.vposed_fixed = (pm & (PB_POSE_R | PB_POSE_L | PB_SHAPE_R | PB_SHAPE_L)) == 0;
    // ... and a stage that moves the shape but not the finger pose keeps the pose offsets P: stored by its first iteration's skinning, reused
    // after (lbs_skin_kernel MODE KEEP_P: the 1.8 MB pose basis is not read again; the same bits, test_skin_keeps_pose_offsets_bit_identically)
    p.pose_fixed = (pm & (PB_POSE_R | PB_POSE_L)) == 0;
    p.later_skin = p.vposed_fixed ? SKIN_REUSE : (p.pose_fixed ? SKIN_KEEP_P : SKIN_FULL);
    p.first_skin = (!p.vposed_fixed && p.pose_fixed) ? SKIN_FULL_STORE_P : SKIN_FULL;
    // The tail of an iteration -- sampling + losses, LBS backward of both hands, and in the stages that do not move the finger pose also the
    // optimizer step + next skeletons -- is ONE launch per sample (opt_tail_kernel): 4 launches per iteration instead of 6 (finger-pose
    // stage, whose backward continues with a batch-wide GEMM: 7 instead of 8); in a stage that keeps v_posed the same launch also skins
    // the next iteration's vertices: 3 launches (SKIN_NONE in plan_iter).  A tail whose LDS does not fit the device is never launched
    p.fused_tail = p.need_mask != 0 && !no_fused_tail && tail_fits;
    // Hands whose vertices cannot change during this stage (SdfWorkspace::static_mask): the right hand when none of its own blocks is
    // refined; the left hand when neither its own blocks, nor the translation, nor the right hand's shape (the left hand is shifted by
    // trans + J_r[0] - J_l[0], optimize_model.py:217-224) is.  opt_default's translation stage: the right hands.
    p.static_mask = ((pm & (PB_ORIENT_R | PB_POSE_R | PB_SHAPE_R)) ? 0 : 1) | ((pm & (PB_ORIENT_L | PB_POSE_L | PB_SHAPE_L | PB_TRANS | PB_SHAPE_R)) ? 0 : 2);
    // Round 5: a left hand that the stage only TRANSLATES (the translation stage of opt_default: trans alone moves) is static in its own
    // normalised frame -- its box follows it, everything inside the box stays: treated as static with a moving box (SdfWorkspace::moving_box;
    // bits 2-3 of the mask).  The kept grid is the first iteration's; a recomputation would differ by the rounding of the translated
    // vertices, so unlike the static reuse this is not bit-identical to the from-scratch path (sdf_no_static_reuse = 2 switches it off).
    if ((pm & PB_TRANS) && !(pm & (PB_ORIENT_L | PB_POSE_L | PB_SHAPE_L | PB_SHAPE_R)) && sdf_no_static_reuse == 0) p.static_mask |= 2 | (2 << 2);
    p.pose_stage = (p.need_mask & 2) != 0;
    // Each stage's tail does only what that stage can move (ihmr_debug_force_generic_tail switches both off):
    //   * only the translation (and the camera) moves: opt_tail_kernel_trans -- the right hand is left alone, the left hand's vertices are
    //     the kept pre-shift values plus the new shift;
    //   * a hand none of whose axis-angles is refined keeps the rotations and the pose feature of its skeleton record in the STEP tails
    //     (lbs_skel_hand: keep_rot; the record is in LDS whenever the LBS backward runs, need_mask & 7).  opt_default: the shape stage
    p.trans_tail = p.vposed_fixed && p.need_mask == 8 && !force_generic_tail;
    p.keep_rot = ((p.need_mask & 7) == 0 || force_generic_tail) ? 0
                 : (((pm & (PB_ORIENT_R | PB_POSE_R)) ? 0 : 1) | ((pm & (PB_ORIENT_L | PB_POSE_L)) ? 0 : 2));
    // the first iteration of a stage starts the candidate lists over (the workspace is the caller's memory: whatever it holds, a stage
    // is self-contained) -- unless the caller vouches for them (keep_lists): then a hand keeps its lists while the prep kernel's
    // displacement test against the reference pose they were built at passes, whether an optimizer step or the previous stage's
    // select step moved the hand
    p.lists_first = keep_lists ? LISTS_KEEP : LISTS_REBUILD;
    return p;
}

// The launches of one iteration, in order: head (opt_adam_skel_kernel: the optimizer step of the previous iteration + skeletons), skin,
// the collision prep + distance launches with `lists`, the tail, and what follows it.  The last four fields are the stage's, copied
// so that an IterPlan alone says what is launched (the single-shot entry points have constant ones, below).
struct IterPlan {
    int head, skin, lists, tail, after;
    int first;                  // the tail's `first` flag: the stage's first iteration
    int need_cam, need_mask, static_mask, keep_rot;
};

inline IterPlan plan_iter(const StagePlan& p, int it, int n_iters) {
    IterPlan q{};
    const bool last = it + 1 >= n_iters;
    q.lists = it == 0 ? p.lists_first : LISTS_REUSE;
    q.first = it == 0 ? 1 : 0;
    q.need_cam = p.need_cam; q.need_mask = p.need_mask; q.static_mask = p.static_mask; q.keep_rot = p.keep_rot;
    if (p.fused_tail) {
        // head: stand-alone in the first iteration (zero the optimizer state, first skeletons) and in the finger-pose stage; otherwise the
        // tail of iteration it - 1 has done it
        // ... and in a stage that keeps v_posed (translation, orientation) the tail has skinned the next vertices as well: 3 launches
        q.head = it == 0 || p.pose_stage;
        q.skin = it == 0 ? p.first_skin : (p.vposed_fixed ? SKIN_NONE : p.later_skin);
        q.tail = last ? TAIL_PLAIN : p.trans_tail ? TAIL_TRANS : p.vposed_fixed ? TAIL_STEP_SKIN : !p.pose_stage ? TAIL_STEP : TAIL_PLAIN;
        q.after = p.pose_stage ? AFTER_BWD23 : AFTER_NONE;
    } else {
        q.head = 1;             // applies the step of iteration it - 1 first
        q.skin = it == 0 ? p.first_skin : p.later_skin;
        q.tail = TAIL_SEPARATE;
        q.after = p.need_mask ? AFTER_LBS_BWD : AFTER_NONE;
    }
    return q;
}

// The constant plans of the single-shot entry points: head + FULL skin unless said otherwise, no camera, nothing static
//   forward + losses, lists off (ihmr_opt_forward_losses, ihmr_opt_sdf_stats)
constexpr IterPlan kForwardLosses{1, SKIN_FULL, LISTS_OFF, TAIL_SEPARATE, AFTER_NONE, 0, 0, 0, 0, 0};
//   ... + the whole LBS backward of every block (ihmr_mlp_train_grad)
constexpr IterPlan kForwardBackward{1, SKIN_FULL, LISTS_OFF, TAIL_SEPARATE, AFTER_LBS_BWD, 0, 0, 15, 0, 0};
//   skeletons + skinning only (ihmr_opt_forward_verts)
constexpr IterPlan kForwardVerts{1, SKIN_FULL, LISTS_OFF, TAIL_NONE, AFTER_NONE, 0, 0, 0, 0, 0};
// An IHMR-MLP evaluation (ihmr_mlp_forward_select).  The evaluations of one test() call move the hands by a stage's residual at a time:
// the collision kernels keep their per-voxel candidate lists from one evaluation to the next (valid while a hand stays within the slack
// of the pose its lists were built at, checked per hand and evaluation; rebuilt otherwise) -- started over by the evaluation that opens
// the batch (mode 1).  No static-hand reuse here: a rejected update falls back to parameters the vertex buffers no longer hold.
// mode 3 = mode 2 for a stage that moves neither finger pose nor shape while the workspace still holds v_posed of exactly these finger
// poses and shapes: the skinning launch skips both blends (lbs_skin_kernel MODE REUSE: the stored values are the bits a recomputation gives)
inline IterPlan plan_mlp_eval(int mode) {
    IterPlan q = kForwardLosses;
    q.skin = mode == 3 ? SKIN_REUSE : SKIN_FULL;
    q.lists = mode == 1 ? LISTS_REBUILD : LISTS_REUSE;
    return q;
}

// the per-iteration optimizer constants of iteration `it` (Adam: lr / (1 - beta1^t), sqrt(1 - beta2^t); SGD: step_size = lr) and the
// snapshot slot: before the step at iterations 0, f, 2f, ... (-1: no snapshot)
struct StepPlan { float step_size, bc2_sqrt; int snap_idx; };
inline StepPlan plan_step(float lr, int sgd, int it, int save_freq) {
    const double t = (double)(it + 1);
    const double bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
    return StepPlan{sgd ? lr : (float)((double)lr / bc1), (float)sqrt(bc2), (it % save_freq == 0) ? it / save_freq : -1};
}
inline int snapshot_count(int n_iters, int save_freq) { return (n_iters + save_freq - 1) / save_freq; }

// ------------------------------------------------------------------------------------------ collision workspace
// The switches of SdfWorkspace for one launch pair.  static_mask in: bit 0 / 1 = the right / left hands have had bit-identical vertices
// since the stage's first iteration, bits 2-3: sides that only translate
struct SdfFlags { int list_mode, force_rebuild, static_stage, static_mask, moving_box; };
inline SdfFlags plan_sdf_flags(int lists, int static_mask, int sdf_no_candidate_lists, int sdf_no_static_reuse) {
    SdfFlags f{};
    f.list_mode = (lists != LISTS_OFF && !sdf_no_candidate_lists) ? 1 : 0;
    f.force_rebuild = lists == LISTS_REBUILD ? 1 : 0;
    f.static_stage = (f.list_mode && sdf_no_static_reuse != 1) ? (static_mask & 3) : 0;
    f.static_mask = lists >= LISTS_REBUILD ? 0 : f.static_stage;
    f.moving_box = (static_mask >> 2) & f.static_stage;
    return f;
}

// ------------------------------------------------------------------------------------------ size-dependent launch forms
// thresholds of csrc/mano_lbs.h and csrc/sdf_collision.h (ihmr_hip.hip asserts they agree)
constexpr int SKIN_SMALL_MAX_HANDS = 256, PREP_SMALL_MAX_HANDS = 128, BWD2_LDS_MIN_HANDS = 256;
// small skin launches: four instead of eight hands per skin workgroup (half the chain per thread)
inline bool skin_small(int hands) { return hands <= SKIN_SMALL_MAX_HANDS; }
// sdf_prep_kernel: the dense-grid form, or for small launches the 1024-thread form (half the chain per thread), else the 512-thread form
enum PrepForm { PREP_LARGE = 0, PREP_SMALL = 1, PREP_DENSE = 2 };
inline int prep_form(int hands, int dense) { return dense ? PREP_DENSE : (hands <= PREP_SMALL_MAX_HANDS ? PREP_SMALL : PREP_LARGE); }
// lbs_bwd2: the LDS-tiled form from 256 hands on (one batch of 64 samples = 128 hands: 2 x 25 workgroups are too few; the streaming form
// stays there, and everywhere under ihmr_debug_force_lbs_bwd2_streaming); the same bits either way
inline bool bwd2_lds(int hands, int force_streaming) { return hands >= BWD2_LDS_MIN_HANDS && !force_streaming; }

}  // namespace plan

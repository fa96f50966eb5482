"""Which parameter subsets of a refinement stage launch something different, and the inputs the stage tests run them on.  Host only.

`ihmr_opt_run_stage` (csrc/ihmr_hip.hip, csrc/stage_plan.h) derives a stage's whole launch plan from `param_mask`.  `plan` restates that derivation so
that the tests can pick ONE mask per distinct plan instead of all 255 (`CLASSES`, `REPRESENTATIVES`); `stage_for` and `batch` build
the stage and the two B = 3 batches every case runs on; `oracle_gradients` is the float64 / float32 oracle gradient of the whole
loss over all eight parameter blocks at a given state."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

# include/ihmr_hip.h: IHMR_PB_* (ihmr_amd.hip.PARAM_BLOCKS carries the same bits; test_stage_cases_cpu.py compares them)
CAM, TRANS, ORIENT_R, ORIENT_L, POSE_R, POSE_L, SHAPE_R, SHAPE_L = (1 << i for i in range(8))
ALL_MASKS = tuple(range(1, 256))

# tail forms of one iteration
TAIL_SEPARATE = "separate launches"             # no fused tail: opt_sample_loss_kernel (+ the LBS backward when anything needs it)
TAIL_PLAIN = "opt_tail_kernel<false>"           # sampling + losses + LBS backward
TAIL_STEP = "opt_tail_kernel<true>"             # ... + optimizer step + next skeletons
TAIL_STEP_SKIN = "opt_tail_kernel<true,true>"   # ... + skinning of the next vertices
TAIL_TRANS = "opt_tail_kernel_trans"            # the translation stage's own tail

Plan = namedtuple("Plan", "need_mask need_cam vposed_fixed pose_fixed first_skin later_skin static_mask trans_tail keep_rot pose_stage "
                          "fused_tail step_tail last_tail lists_first")


def plan(mask, *, no_fused_tail=0, tail_fits=1, sdf_no_static_reuse=0, force_generic_tail=0, keep_lists=0):
    """The launch plan `ihmr_opt_run_stage` derives from `param_mask` and its switches (csrc/stage_plan.h: `plan_stage`, and the tail
    selection of `plan_iter`), restated.  The defaults are the product's: static reuse on, translated reuse on (`sdf_no_static_reuse`
    = 0), fused tail on (`no_fused_tail` = 0, the tail fits the device), generic tail not forced, candidate lists rebuilt by the
    stage's first iteration.  `step_tail` is the tail of every iteration but the stage's last, `last_tail` the last one's (`tail_form`).

    This restatement CHOOSES the cases -- one mask per distinct value -- that tests/test_gpu_stage_masks.py runs against the generic
    tail forms, the separate launches and the float64 oracle; tests/test_stage_plan_cpu.py compiles stage_plan.h for the host and
    compares it with this function field for field, at every mask, switch combination and iteration."""
    pm = int(mask)
    if not 1 <= pm <= 255:
        raise ValueError(f"param_mask {mask!r}: 1 .. 255")
    need_mask = (1 if pm & (ORIENT_R | ORIENT_L) else 0) | (2 if pm & (POSE_R | POSE_L) else 0) | (4 if pm & (SHAPE_R | SHAPE_L) else 0) | \
                (8 if pm & TRANS else 0)
    need_cam = 1 if pm & CAM else 0
    vposed_fixed = (pm & (POSE_R | POSE_L | SHAPE_R | SHAPE_L)) == 0
    pose_fixed = (pm & (POSE_R | POSE_L)) == 0
    later_skin = "REUSE" if vposed_fixed else ("KEEP_P" if pose_fixed else "FULL")
    first_skin = "FULL_STORE_P" if (not vposed_fixed and pose_fixed) else "FULL"
    fused_tail = need_mask != 0 and not no_fused_tail and bool(tail_fits)
    static_mask = (0 if pm & (ORIENT_R | POSE_R | SHAPE_R) else 1) | (0 if pm & (ORIENT_L | POSE_L | SHAPE_L | TRANS | SHAPE_R) else 2)
    if (pm & TRANS) and not (pm & (ORIENT_L | POSE_L | SHAPE_L | SHAPE_R)) and sdf_no_static_reuse == 0:
        static_mask |= 2 | (2 << 2)           # the left hand only translates: static in its own frame, with a moving box
    pose_stage = (need_mask & 2) != 0
    trans_tail = vposed_fixed and need_mask == 8 and not force_generic_tail
    keep_rot = 0 if ((need_mask & 7) == 0 or force_generic_tail) else ((0 if pm & (ORIENT_R | POSE_R) else 1) | (0 if pm & (ORIENT_L | POSE_L) else 2))
    if not fused_tail:
        step_tail = last_tail = TAIL_SEPARATE
    else:
        step_tail = TAIL_TRANS if trans_tail else (TAIL_STEP_SKIN if vposed_fixed else (TAIL_STEP if not pose_stage else TAIL_PLAIN))
        last_tail = TAIL_PLAIN
    # (the skinning launch of a later iteration is the tail's own fourth phase in the forms that skin)
    return Plan(need_mask, need_cam, vposed_fixed, pose_fixed, first_skin, later_skin, static_mask, trans_tail, keep_rot, pose_stage,
                fused_tail, step_tail, last_tail, "KEEP" if keep_lists else "REBUILD")


def tail_form(mask, it, n, **switches):
    """The tail of iteration `it` of an `n`-iteration stage."""
    if not 0 <= it < n:
        raise ValueError("0 <= it < n")
    p = plan(mask, **switches)
    return p.step_tail if it + 1 < n else p.last_tail


def moving_box(mask):
    """The stage treats the left hand as static with a moving box (the rounding-level acceleration, `sdf_no_translated_reuse`)."""
    return (plan(mask).static_mask >> 2) != 0


def _classes(key):
    out = OrderedDict()
    for m in ALL_MASKS:
        out.setdefault(key(plan(m)), []).append(m)
    return out


CLASSES = _classes(lambda p: p)                                   # plan -> its masks, ascending
CLASSES_NO_CAM = _classes(lambda p: p._replace(need_cam=0))
REPRESENTATIVES = tuple(v[0] for v in CLASSES.values())           # the lowest mask of each class, ascending
# the lowest mask of each class when the camera bit is ignored: 47 masks without the camera, and mask 1 -- the camera alone, the only
# way to differentiate nothing through MANO
REPRESENTATIVES_NO_CAM = tuple(v[0] for v in CLASSES_NO_CAM.values())


def block_names(mask):
    """The `update_params` names of a mask, in slot order."""
    from ihmr_amd import hip
    return [n for n, (bit, _, _) in sorted(hip.PARAM_BLOCKS.items(), key=lambda kv: kv[1][1]) if mask & bit]


def stage_for(mask, n_iters, lr=None):
    """A strategy entry that refines exactly the blocks of `mask` for `n_iters` iterations: every loss term weighted (the reporting
    weights, finger regulariser included, so every term reaches every block it can), the default strategy's learning rates (1e-4 for
    the camera and the translation, 1e-2 otherwise) and its filter and select criteria."""
    from ihmr_amd.strategies import OPT_DEFAULT_LOSS_WEIGHTS, make_opt_strategy
    default = make_opt_strategy(0)[0]
    if lr is None:
        lr = 1e-4 if mask & (CAM | TRANS) else 1e-2
    return dict(update_params=block_names(mask), loss_weights=dict(OPT_DEFAULT_LOSS_WEIGHTS), lr=lr, epoch=int(n_iters) - 1,
                filter_loss=list(default["filter_loss"]), select_loss=default["select_loss"])


_BATCHES = {}


def batch(mano_arrays, kind, B=3):
    """default: the synthetic batch (B = 3: control / right hand only / left hand only -- a (1, 0) sample, collision gradient scale 0);
    deep: the deep-overlap hands of the deep-interpenetration tests; far: the default batch with the left hands moved a metre away
    (no collision: only the fingertip gradients are non-zero).  Built once, handed out unchanged."""
    key = (kind, B)
    if key not in _BATCHES:
        from helpers import DEEP_SEED, oracle_two_hand_verts, ragged_opt_batch
        if kind == "deep":
            _, out = oracle_two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
        elif B == 3:
            _, out = oracle_two_hand_verts(mano_arrays, 8, 2608)
            out = {k: v[:B].clone() for k, v in ragged_opt_batch(out).items()}
            assert (out["hand_type_array"] == torch.tensor([1.0, 0.0])).all(dim=1).any()
        else:
            _, out = oracle_two_hand_verts(mano_arrays, B, 2604 if B == 1 else 1700 + B)
        if kind == "far":
            out = {k: v.clone() for k, v in out.items()}
            out["init_hand_trans"].reshape(B, -1)[:, 0] += 1.0
        _BATCHES[key] = out
    return _BATCHES[key]


ORACLE_BLOCKS = ("pred_cam_params", "pred_hand_trans", "pred_right_orient", "pred_left_orient", "pred_right_pose_params",
                 "pred_left_pose_params", "pred_right_shape_params", "pred_left_shape_params")
_ORACLES = {}


def oracle(mano_arrays, B, dtype):
    """One `OptimizeRef` per precision, shared (its state is set by every caller)."""
    from oracle.opt_ref import OptimizeRef
    if (B, dtype) not in _ORACLES:
        _ORACLES[B, dtype] = OptimizeRef(mano_arrays[0], mano_arrays[1], B, [], save_mid_freq=1, dtype=dtype)
    return _ORACLES[B, dtype]


def oracle_gradients(mano_arrays, data, weights, dtype, state=None):
    """d(whole loss) / d(each of the eight blocks) from autograd through the oracle in `dtype`, as (B, 122) float64 in the slot order of
    the product's parameter vector.  The state is the batch's initial one, with the blocks of `state` (name -> float32 values, converted
    exactly) replaced."""
    from ihmr_amd import hip
    B = data["init_cam"].shape[0]
    orc = oracle(mano_arrays, B, dtype)
    orc.set_input(data)
    orc.init_optimize()
    for name, value in (state or {}).items():
        assert name in ORACLE_BLOCKS
        cur = getattr(orc, name)
        setattr(orc, name, torch.as_tensor(np.asarray(value, np.float32)).to(dtype).reshape(cur.shape))
    leaves = []
    for name in ORACLE_BLOCKS:
        leaf = getattr(orc, name).detach().clone().requires_grad_(True)
        setattr(orc, name, leaf)
        leaves.append(leaf)
    orc.forward()
    orc.compute_loss(weights)
    grads = torch.autograd.grad(orc.loss, leaves, allow_unused=True)
    out = np.zeros((B, hip.OPT_NPARAM), np.float64)
    for name, g in zip(ORACLE_BLOCKS, grads):
        _, lo, size = hip.PARAM_BLOCKS[name]
        if g is not None:
            out[:, lo:lo + size] = g.detach().double().reshape(B, size).numpy()
    return out


def oracle_state_after(mano_arrays, data, stage, n_steps, dtype=torch.float32):
    """name -> float32 values of the stage's blocks after `n_steps` Adam iterations of the oracle's loop (no snapshot, no selection)."""
    B = data["init_cam"].shape[0]
    orc = oracle(mano_arrays, B, dtype)
    orc.set_input(data)
    orc.init_optimize()
    params = []
    for name in stage["update_params"]:
        leaf = getattr(orc, name).detach().clone().requires_grad_(True)
        setattr(orc, name, leaf)
        params.append(leaf)
    optimizer = torch.optim.Adam(params, lr=stage["lr"], betas=(0.9, 0.999))
    for _ in range(n_steps):
        orc.forward()
        orc.compute_loss(stage["loss_weights"])
        optimizer.zero_grad()
        orc.loss.backward()
        optimizer.step()
    return {name: p.detach().float().numpy().copy() for name, p in zip(stage["update_params"], params)}


def block_slices(mask=255):
    """name -> slice of the 122-vector, for the blocks of `mask`."""
    from ihmr_amd import hip
    return OrderedDict((n, slice(hip.PARAM_BLOCKS[n][1], hip.PARAM_BLOCKS[n][1] + hip.PARAM_BLOCKS[n][2])) for n in block_names(mask))


GRAD_FLOOR = 3e-4      # x max|g_64| of the block: the bar of the single-step gradient tests (tests/test_gpu_parity.py)
GRAD_RULE = 1.5        # x the float32 oracle's own distance from float64: the rule of tests/test_gpu_mano_layer.py


def gradient_bar(g32, g64, sl):
    """(bar, which): the larger of 1.5 x the float32 oracle's distance from float64 and the floor, over one block and the batch."""
    d32 = float(np.abs(g32[:, sl] - g64[:, sl]).max())
    floor = GRAD_FLOOR * float(np.abs(g64[:, sl]).max())
    return (GRAD_RULE * d32, "rule") if GRAD_RULE * d32 >= floor else (floor, "floor")

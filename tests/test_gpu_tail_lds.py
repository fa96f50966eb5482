"""The fused tail launch (`opt_tail_kernel`) against the three launches it replaces (`opt.no_fused_tail`) on stages opt_default never
runs, bit for bit.

In a stage that moves the shape the tail keeps `d v_posed` in LDS (it takes the place of the hand's dead `v_posed` record) instead of
sending it through the workspace; the stand-alone `lbs_bwd1_kernel` -- what `opt.no_fused_tail` runs -- keeps the workspace route and is
the checker.  The stage lists pick every route of the tail's backward: shape alone, shape with the general backward and the
translation gradient, shape together with the finger pose (`d v_posed` needed in LDS and in the workspace, which the pose GEMM reads),
and the two shortcuts (orientation only, translation only).  One sample and a ragged batch of three (both hands / right only / left
only: collision mask 0 for the single-hand samples)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPOCH, FREQ = 3, 1          # 4 iterations per stage, a snapshot at every one
EXPORT_KEYS = ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
               "pred_joints_3d", "collision_loss", "collision_loss_origin_scale")


def _stage_lists():
    from ihmr_amd.strategies import make_opt_strategy
    trans, orient, pose, shape = make_opt_strategy(EPOCH)
    shape_orient_trans = dict(shape, update_params=["pred_hand_trans", "pred_left_orient", "pred_right_orient",
                                                    "pred_left_shape_params", "pred_right_shape_params"])
    pose_shape = dict(pose, update_params=["pred_left_pose_params", "pred_right_pose_params", "pred_left_shape_params", "pred_right_shape_params"])
    return {"shape": [shape], "shape-orient-trans": [shape_orient_trans], "pose-shape": [pose_shape], "orient-then-trans": [orient, trans]}


_BATCHES = {}


def _batch(mano_arrays, B):
    """B = 1: the synthetic batch; B = 3: the first three samples of the ragged batch of eight (tests/helpers.py: control, right hand
    only, left hand only).  Built once, handed out unchanged.
    The seeds are chosen with the CPU oracle (oracle/opt_ref.py), not with the kernels under test: a stage ends with the reference's
    filter / select step, which puts the stage's input back when no snapshot passes the filter (the collision loss has to fall by 10 %
    within four iterations).  On these batches the oracle's shape stage selects a later snapshot for at least one sample with Adam and
    with SGD alike (B = 1, seeds 2601 - 2603: not with SGD), so the shape the stage returns is one that the backward produced."""
    if B not in _BATCHES:
        from helpers import oracle_two_hand_verts, ragged_opt_batch
        if B == 1:
            _, batch = oracle_two_hand_verts(mano_arrays, 1, 2604)
        else:
            _, batch = oracle_two_hand_verts(mano_arrays, 8, 2608)
            batch = {k: v[:B].clone() for k, v in ragged_opt_batch(batch).items()}
            assert batch["hand_type_array"].sum(dim=1).min() < 1.5      # (a single-hand sample: collision mask 0)
        _BATCHES[B] = batch
    return _BATCHES[B]


def _make_opt(B, optimizer, no_fused_tail):
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root="", strategy="opt_default", save_mid_freq=FREQ,
                                 optimizer=optimizer, opt_epoch=EPOCH, no_fused_tail=no_fused_tail)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("stages,optimizer", [("shape", "adam"), ("shape", "sgd"), ("shape-orient-trans", "adam"), ("pose-shape", "adam"),
                                              ("orient-then-trans", "adam")])
def test_fused_tail_matches_separate_launches_on_custom_stages(mano_arrays, B, stages, optimizer):
    from ihmr_amd.optimize_model import OptimizeModel
    batch = _batch(mano_arrays, B)
    outs = []
    for off in (False, True):
        m = OptimizeModel(_make_opt(B, optimizer, off))
        m.strategy = _stage_lists()[stages]
        for rep in range(2):        # (the first pass captures the stage graphs, the second replays them)
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
        outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["adam_m"].cpu().numpy(),
                     m.buf["snap_loss"].cpu().numpy()))
    (a, sa, ma, la), (b, sb, mb, lb) = outs
    if stages == "shape":           # (the comparison is not empty: the stage has moved the shape)
        assert not np.array_equal(a["pred_shape_params"], batch["init_shape_params"].numpy()), "the shape stage left the shape where it was"
    assert np.array_equal(sa, sb), "selected_history"
    assert np.array_equal(ma, mb), "adam_m"
    assert np.array_equal(la, lb), "snap_loss"
    for k in EXPORT_KEYS:
        assert np.array_equal(a[k], b[k]), f"{k}: the fused tail launch changed the result"

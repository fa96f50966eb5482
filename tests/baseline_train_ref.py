"""The IHMR-Baseline training objective as ONE plain-torch statement (CPU, any dtype), built from ``oracle/losses_ref.py`` and
``oracle/mano_ref.py`` only (and the oracle's collision module for the collision term): what ``InterHandModel.compute_loss_gradients()`` (``ihmr_amd/baseline_train.py``) has to compute.

Forward: the Baseline's own -- SEPARATE right / left MANO models (the left one with the ``shapedirs[:, 0, :]`` sign fix), 16 joints + the
five tips per hand, the left hand moved to the right wrist + the predicted translation, ``batch_orthogonal_project``
(``baseline_model.py:208-282``).  The product runs both hands through the mirrored right-hand model instead; that this statement does
not is the point.  Terms: ``backward_E`` (``baseline_model.py:285-338``), every one pinned to the reference's own ``LossUtil`` by
``tests/golden/baseline_loss.npz`` -- except the translation term, see :func:`baseline_loss_terms`.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses_ref as L
from oracle.mano_ref import ManoRef
from oracle.sdf_ref import SDFLossRef

TIP_IDS = [744, 320, 443, 554, 671]
TERMS = ("hand_type_loss", "joints_2d_loss", "joints_3d_loss", "mano_pose_loss", "mano_shape_loss", "hand_trans_loss", "shape_reg_loss",
         "collision_loss")
# term -> key of InterHandModel.loss_weights (the handedness term has no weight)
WEIGHT_KEY = dict(joints_2d_loss="joints_2d", joints_3d_loss="joints_3d", mano_pose_loss="mano_pose", mano_shape_loss="mano_shape",
                  hand_trans_loss="hand_trans", shape_reg_loss="shape_reg", collision_loss="collision")
DEFAULT_WEIGHTS = dict(joints_2d=10.0, joints_3d=10.0, mano_pose=10.0, mano_shape=10.0, hand_trans=10.0, shape_reg=0.1, collision=0.0)
BATCH_KEYS = ("joints_2d", "joints_3d", "mano_pose", "mano_betas", "mano_params_weight", "hand_trans", "hand_type_array", "hand_type_valid")
BATCH_SEED, PRED_SEED = 77, 6


def two_from_models(mr, ml):
    """``two(pose (B,96), shape (B,20), trans (B,3)) -> (right verts, left verts, joints (B,42,3))`` over a right and a left MANO layer
    (baseline_model.py:208-254)."""
    def two(pose, shape, trans):
        outs = {}
        for name, m, ps, bs in (("right", mr, 0, 0), ("left", ml, 48, 10)):
            o = m(global_orient=pose[:, ps:ps + 3], hand_pose=pose[:, ps + 3:ps + 48], betas=shape[:, bs:bs + 10])
            outs[name] = (o.vertices, torch.cat([o.joints, o.vertices[:, TIP_IDS]], 1))
        shift = trans.reshape(-1, 1, 3) + (outs["right"][1][:, 0:1] - outs["left"][1][:, 0:1])
        return outs["right"][0], outs["left"][0] + shift, torch.cat([outs["right"][1], outs["left"][1] + shift], 1)
    return two


def separate_two_hand_forward(mano_arrays, dtype=torch.float32):
    """:func:`two_from_models` over ``ManoRef(right)`` and ``ManoRef(left)`` with the reference's sign fix (baseline_model.py:145-149)."""
    right, left = mano_arrays
    l_arr = dict(left); l_arr["shapedirs"] = left["shapedirs"].copy(); l_arr["shapedirs"][:, 0, :] *= -1
    return two_from_models(ManoRef(right, dtype=dtype), ManoRef(l_arr, dtype=dtype))


def hand_type_loss(gt, pred, valid):
    """loss_utils.py:41-44: mean over (B,2) of BCE(pred, gt) * valid."""
    return (F.binary_cross_entropy(pred, gt, reduction="none") * valid).mean()


def hand_trans_loss_documented(gt, pred, w):
    """The ONE term with no reference counterpart (the reference's ``backward_E`` raises at this line): the form
    ``ihmr_amd/baseline_train.py`` documents and the MLP stage uses, ``mean_i(w_i) * mean_{b,k}((gt - pred)^2)``; gt, pred (B,3), w (B,)."""
    return w.mean() * ((gt - pred) ** 2).mean()


def baseline_loss_terms(two, batch, final_params, pred_hand_type, sdf=None):
    """The eight UNWEIGHTED terms of ``backward_E`` as scalars of ``final_params`` (B,122) = [cam 3 | pose 96 | shape 20 | trans 3] and
    ``pred_hand_type`` (B,2); ``two`` as from :func:`two_from_models`; ``batch`` in the dtype of the parameters.  The joint terms run on
    clones (the loss functions align in place): ONE root alignment, by the annotation's weights.  ``sdf``: the collision module, or None
    for a zero collision term.  Every function is looked up in its module at call time."""
    cam, pose, shape, trans = final_params[:, :3], final_params[:, 3:99], final_params[:, 99:119], final_params[:, 119:122]
    rv, lv, j3 = two(pose, shape, trans)
    j2 = L.batch_orthogonal_project(j3, cam)
    g2, g3, mw = batch["joints_2d"], batch["joints_3d"], batch["mano_params_weight"]
    gp, gs, ht = batch["mano_pose"], batch["mano_betas"], batch["hand_trans"]
    t = {}
    t["hand_type_loss"] = hand_type_loss(batch["hand_type_array"], pred_hand_type, batch["hand_type_valid"])
    t["joints_2d_loss"] = L.joints_2d_loss(g2[:, :, :2].clone(), j2.clone(), g2[:, :, 2:3])[0]
    t["joints_3d_loss"] = L.joints_3d_loss_(g3[:, :, :3].clone(), j3.clone(), g3[:, :, 3:4])[0]
    # use_hand_rotation off: the 15 finger joints of each hand (loss_utils.py:58-60)
    t["mano_pose_loss"] = L.mano_pose_loss(gp[:, 3:48], pose[:, 3:48], mw[:, 0:1]) + L.mano_pose_loss(gp[:, 51:], pose[:, 51:], mw[:, 1:2])
    t["mano_shape_loss"] = L.mano_shape_loss(gs[:, :10], shape[:, :10], mw[:, 0:1]) + L.mano_shape_loss(gs[:, 10:], shape[:, 10:], mw[:, 1:2])
    t["hand_trans_loss"] = hand_trans_loss_documented(ht[:, 0, :3], trans, ht[:, 0, 3])
    t["shape_reg_loss"] = L.shape_reg_loss(shape)
    t["collision_loss"] = L.collision_loss(sdf, rv, lv, batch["hand_type_array"])[0] if sdf is not None else final_params.sum() * 0.0
    return t


def baseline_loss_statement(mano_arrays, batch, final_params, pred_hand_type, weights, dtype=torch.float64):
    """-> (terms, d total / d final_params (B,122), d total / d pred_hand_type (B,2)): ``terms`` holds the eight WEIGHTED terms and
    ``total_loss`` as Python floats (``collision_loss`` is 0.0 at weight 0, where the module does not run), the gradients come from
    autograd, in ``dtype``.  float64 the way ``_oracle_param_grad(..., f64=True)`` of the MLP training test gets it: the float32 inputs
    and MANO arrays converted, every operation in double (the collision grid itself is the oracle's float32 grid)."""
    two = separate_two_hand_forward(mano_arrays, dtype)
    b = {k: batch[k].detach().clone().to(dtype) for k in BATCH_KEYS}
    fp = final_params.detach().clone().to(dtype).requires_grad_(True)
    ph = pred_hand_type.detach().clone().to(dtype).requires_grad_(True)
    right, left = mano_arrays
    sdf = SDFLossRef(right["faces"], left["faces"], robustifier=None) if weights["collision"] else None
    t = baseline_loss_terms(two, b, fp, ph, sdf)
    t = {n: t[n] * (weights[WEIGHT_KEY[n]] if n in WEIGHT_KEY else 1.0) for n in TERMS}
    total = sum(t.values())
    total.backward()
    terms = {n: float(v.detach()) for n, v in t.items()}
    terms["total_loss"] = float(total.detach())
    return terms, fp.grad.detach(), ph.grad.detach()


# ------------------------------------------------------------------------------------------------------------------------- inputs
def baseline_batch(mano_arrays, B, seed=BATCH_SEED):
    """The default synthetic batch over the Baseline's own forward, with a dummy image (the loss never reads it)."""
    from ihmr_amd.synthetic import synthetic_opt_batch
    two = separate_two_hand_forward(mano_arrays)
    batch = synthetic_opt_batch(B, lambda p, s, t: two(p, s, t)[2], seed=seed)
    batch["img"] = torch.zeros(B, 3, 8, 8)
    return batch


def ragged_baseline_batch(batch):
    """``helpers.ragged_opt_batch`` (B >= 8; in place) plus what only the Baseline's objective reads: ``mano_params_weight`` 0 for the hand
    a single-hand sample lacks (1: left, 2: right) and for the right hand of the two-hand sample 4; ``hand_type_valid`` 0 for the two-hand
    samples 3 and 6.  The translation weights then average to 6/8 and the valid handedness targets cover (1,1), (1,0) and (0,1)."""
    from helpers import ragged_opt_batch
    batch = ragged_opt_batch(batch)
    w = batch["mano_params_weight"]
    w[1, 1] = 0.0; w[2, 0] = 0.0; w[4, 0] = 0.0
    batch["hand_type_valid"][3] = 0.0
    batch["hand_type_valid"][6] = 0.0
    return batch


def seeded_predictions(batch, seed=PRED_SEED):
    """``final_params`` = [init_cam | init_pose | init_shape | init_trans] + seeded N(0, 0.02) (as ``_oracle_param_grad`` of the MLP training
    test draws them), ``pred_hand_type`` = seeded U(0.02, 0.98); float32."""
    B = batch["init_cam"].shape[0]
    rng = np.random.RandomState(seed)
    init = torch.cat([batch["init_cam"], batch["init_pose_params"], batch["init_shape_params"], batch["init_hand_trans"][:, 0, :3]], 1).float()
    final = init + torch.tensor(rng.normal(0, 0.02, size=(B, 122)), dtype=torch.float32)
    hand = torch.tensor(rng.uniform(0.02, 0.98, size=(B, 2)), dtype=torch.float32)
    return final.contiguous(), hand.contiguous()


# --------------------------------------------------------------------------------------------------------------------------- bars
def term_bar(ref):
    """What ``_close`` gives the MLP training terms (tests/test_gpu_mlp_train.py): 2e-6 + 2e-5 |ref|."""
    return 2e-6 + 2e-5 * abs(ref)


def gradient_blocks():
    """The ``COLS`` blocks of ``final_params`` the gradient is judged by, one after the other."""
    from ihmr_amd.mlp_model import COLS
    return COLS


def block_distance(got, ref64, sl):
    """(B,) per sample: max |got - ref64| over the block's columns, relative to the block's scale max |ref64| (1 where the block is 0)."""
    ref = ref64[:, sl].double()
    scale = float(ref.abs().max()) or 1.0
    return (got[:, sl].double() - ref).abs().max(1).values / scale


def block_bar(g32, ref64, sl):
    """The rule of ``test_param_gradient_matches_oracle_autograd``: 3 x (float32 statement vs float64) + 1e-6, relative to the block's scale."""
    return 3.0 * float(block_distance(g32, ref64, sl).max()) + 1e-6

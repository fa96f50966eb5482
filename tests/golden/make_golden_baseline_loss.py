#!/usr/bin/env python3
"""Writes ``tests/golden/baseline_loss.npz``: the terms of the IHMR-Baseline training objective as the reference's OWN functions give
them, run where the reference tree is present (imported with CPU stubs, ``_ref_import.py``).

What runs: ``LossUtil._hand_type_loss / _joints_2d_loss / _joints_3d_loss / _mano_pose_loss / _mano_shape_loss / _shape_reg_loss``
(models/loss_utils.py) called as ``backward_E`` calls them (models/baseline_model.py:285-330: the 48-d pose of each hand with
``use_hand_rotation`` off, ``mano_params_weight[:, h:h+1]``), and ``transform_utils.batch_orthogonal_project``.  The joints come from the
injected MANO seam (``smplx.create`` -> ``oracle/mano_ref.py``), one layer per hand, composed as the Baseline composes them
(``tests/baseline_train_ref.two_from_models``).  ``_hand_trans_loss`` is NOT run: ``backward_E`` raises at that line, the product's
translation term has no reference counterpart.  The collision term needs the third-party module and is pinned elsewhere.

Inputs: the ragged batch (``baseline_train_ref.ragged_baseline_batch``) at B = 8 and the seeded predictions
(``baseline_train_ref.seeded_predictions``).  Stored, float32: the inputs, each UNWEIGHTED term (``term_*``) and autograd's
``d term / d final_params`` (``dfp_*``, (8,122)) and, for the handedness term, ``d term / d pred_hand_type`` (``dht_*``, (8,2); no other
term reaches that leaf, which is asserted).
"""
import os
import os.path as osp
import sys

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, osp.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _ref_import import import_reference, make_opt  # noqa: E402

B = 8
REF_TERMS = ("hand_type_loss", "joints_2d_loss", "joints_3d_loss", "mano_pose_loss", "mano_shape_loss", "shape_reg_loss")


def generate():
    """-> dict of float32 arrays (what the file holds)."""
    import baseline_train_ref as R
    from ihmr_amd.assets import synthetic_mano
    ns = import_reference()
    import smplx
    models = {h: smplx.create("", "mano", use_pca=False, is_rhand=(h == "right"), batch_size=B) for h in ("left", "right")}
    if torch.mean(torch.abs(models["left"].shapedirs[:, 0, :] - models["right"].shapedirs[:, 0, :])) < 1e-7:
        models["left"].shapedirs[:, 0, :] *= -1
    two = R.two_from_models(models["right"], models["left"])
    lu = ns.loss_utils.LossUtil(make_opt(B, is_train=True), models)
    batch = R.ragged_baseline_batch(R.baseline_batch((synthetic_mano(True), synthetic_mano(False)), B))
    final, hand = R.seeded_predictions(batch)
    out = {f"in_{k}": batch[k].clone() for k in R.BATCH_KEYS}
    out.update(in_final_params=final.clone(), in_pred_hand_type=hand.clone())
    j2d, j3d, mw = batch["joints_2d"], batch["joints_3d"], batch["mano_params_weight"]
    gp, gs = batch["mano_pose"], batch["mano_betas"]

    def term(name, fp, ph):
        pose, shape = fp[:, 3:99], fp[:, 99:119]
        if name == "hand_type_loss":
            return lu._hand_type_loss(batch["hand_type_array"], ph, batch["hand_type_valid"])
        if name in ("joints_2d_loss", "joints_3d_loss"):
            j3 = two(pose, shape, fp[:, 119:122])[2]
            if name == "joints_2d_loss":
                return lu._joints_2d_loss(j2d[:, :, :2].clone(), ns.transform_utils.batch_orthogonal_project(j3, fp[:, :3]), j2d[:, :, 2:3])[0]
            return lu._joints_3d_loss(j3d[:, :, :3].clone(), j3.clone(), j3d[:, :, 3:4])[0]
        if name == "mano_pose_loss":
            return (lu._mano_pose_loss(gp[:, :48], pose[:, :48], mw[:, 0:1]) + lu._mano_pose_loss(gp[:, 48:], pose[:, 48:], mw[:, 1:2]))
        if name == "mano_shape_loss":
            return (lu._mano_shape_loss(gs[:, :10], shape[:, :10], mw[:, 0:1]) + lu._mano_shape_loss(gs[:, 10:], shape[:, 10:], mw[:, 1:2]))
        assert name == "shape_reg_loss"
        return lu._shape_reg_loss(shape)

    import contextlib
    torch.cuda.device = lambda *a, **k: contextlib.nullcontext()      # batch_rodrigues enters torch.cuda.device(get_device()): -1 on CPU
    for name in REF_TERMS:
        fp, ph = final.clone().requires_grad_(True), hand.clone().requires_grad_(True)
        l = term(name, fp, ph)
        l.backward()
        out[f"term_{name}"] = l.detach()
        if name == "hand_type_loss":
            assert fp.grad is None
            out[f"dht_{name}"] = ph.grad
        else:
            assert ph.grad is None
            out[f"dfp_{name}"] = fp.grad
    return {k: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, np.float32) for k, v in out.items()}


def main():
    out = generate()
    path = sys.argv[1] if len(sys.argv) > 1 else osp.join(HERE, "baseline_loss.npz")       # (another path: the regeneration test's)
    np.savez_compressed(path, **out)
    print("baseline_loss.npz", len(out), "arrays", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()

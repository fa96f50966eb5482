#!/usr/bin/env python3
"""Writes ``tests/golden/metrics_pa.npz``: the reference's Procrustes-aligned joint error, recorded IN THE BUILD CONTAINER (the
reference imported with CPU stubs, ``_ref_import.py``).

What runs: the reference's own ``utils/metric_utils.get_single_pa_inter_joints_error(..., use_rot=True)`` and ``calc_transform`` on
seeded cases of ``tests/pa_cases.py``.  Stored per case ``<name>``:

* ``<name>_pred`` (42,3), ``<name>_gt`` (42,4) float32, ``<name>_scale``: the inputs;
* ``<name>_ref32``: the per-joint errors of the call on the float32 arrays (the reference then works in float32 inside);
* ``<name>_ref64``: the same call on float64 casts of the same arrays;
* ``<name>_aligned32`` / ``<name>_aligned64``: what ``calc_transform`` returns for the valid joints.

``three_valid`` and ``two_valid`` pin the reference's reading of a (3,3) / (2,3) input as coordinates x points."""
import os.path as osp
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, osp.join(ROOT, "tests"))

import pa_cases as PC  # noqa: E402
from _ref_import import import_reference  # noqa: E402

CASES = ("all_42", "missing_wrist_41", "right_hand_only_21", "four_valid", "mirrored", "rotation_near_pi", "scale_half", "scale_two",
         "translated_metres", "fractional_weights", "three_valid", "two_valid")


def main():
    mu = import_reference().metric_utils
    cases = PC.joint_cases()
    out = dict(names=np.array(CASES))
    for name in CASES:
        pred, gt, scale = cases[name]
        valid = gt[:, 3] > 0
        out[f"{name}_pred"], out[f"{name}_gt"], out[f"{name}_scale"] = pred, gt, np.float64(scale)
        out[f"{name}_ref32"] = np.asarray(mu.get_single_pa_inter_joints_error(pred, gt[:, :3], gt[:, 3:], scale, True), np.float64)
        out[f"{name}_ref64"] = np.asarray(mu.get_single_pa_inter_joints_error(pred.astype(np.float64), gt[:, :3].astype(np.float64),
                                                                                gt[:, 3:].astype(np.float64), scale, True), np.float64)
        out[f"{name}_aligned32"] = np.asarray(mu.calc_transform(pred[valid].copy(), gt[valid, :3].copy()))
        out[f"{name}_aligned64"] = np.asarray(mu.calc_transform(pred[valid].astype(np.float64), gt[valid, :3].astype(np.float64)))
        print(f"{name:22s} n = {int(valid.sum()):2d}  mean ref64 {out[f'{name}_ref64'].mean():.6f}  "
              f"max |ref32 - ref64| {np.abs(out[f'{name}_ref32'] - out[f'{name}_ref64']).max():.2e}  dtype32 {out[f'{name}_aligned32'].dtype}")
    path = osp.join(HERE, "metrics_pa.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, osp.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes ``tests/golden/metrics_edges.npz``: the reference's joint error and its aligned ("inter") joint error at the edges of their
set rules, recorded IN THE BUILD CONTAINER (the reference imported with CPU stubs, ``_ref_import.py``).

What runs: the reference's own ``utils/metric_utils.get_single_joints_error`` and ``get_single_pa_inter_joints_error(...,
use_rot=False)`` on every sample of the classes ``fractional``, ``flat``, ``missing`` and ``scaled`` of ``tests/metric_cases.py``.
Stored per sample ``<i>`` (``names[i]`` is its name):

* ``<i>_pred`` (42,3), ``<i>_gt`` (42,4) float32, ``<i>_scale``: the inputs;
* ``<i>_j3d32`` / ``<i>_pa32``: the two lists of the calls on the float32 arrays (the reference then works in float32 inside);
* ``<i>_j3d64`` / ``<i>_pa64``: the same calls on float64 casts of the same arrays.

The lengths of the lists (0 for a sample the reference leaves out) and the positions of their NaN are part of the data."""
import os.path as osp
import sys
import warnings

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, osp.join(ROOT, "tests"))

import metric_cases as MC  # noqa: E402
from _ref_import import import_reference  # noqa: E402

CLASSES = ("fractional", "flat", "missing", "scaled")


def main():
    mu = import_reference().metric_utils
    classes = MC.joint_classes()
    samples = [s for c in CLASSES for s in classes[c]]
    out = dict(names=np.array([s["name"] for s in samples]))
    warnings.simplefilter("ignore", RuntimeWarning)          # the 0 / 0 of a set without spread is what is being recorded
    for i, s in enumerate(samples):
        pred, gt, scale = s["pred"], s["gt"], float(s["scale"])
        out[f"{i}_pred"], out[f"{i}_gt"], out[f"{i}_scale"] = pred, gt, np.float64(scale)
        for tag, cast in (("32", np.float32), ("64", np.float64)):
            p, g = pred.astype(cast), gt.astype(cast)
            out[f"{i}_j3d{tag}"] = np.asarray(mu.get_single_joints_error(p, g[:, :3], g[:, 3:], scale), np.float64)
            out[f"{i}_pa{tag}"] = np.asarray(mu.get_single_pa_inter_joints_error(p, g[:, :3], g[:, 3:], scale, use_rot=False), np.float64)
        print(f"{s['name']:40s} j3d n = {len(out[f'{i}_j3d64']):2d}  pa n = {len(out[f'{i}_pa64']):2d}  "
              f"NaN {int(np.isnan(out[f'{i}_pa64']).sum()):2d} / {int(np.isnan(out[f'{i}_pa32']).sum()):2d} (float64 / float32)")
    path = osp.join(HERE, "metrics_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, osp.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes ``tests/golden/metrics_curves.npz``: the reference's collision AUC, recorded IN THE BUILD CONTAINER (the reference imported
with CPU stubs, ``_ref_import.py``).

What runs: the reference's own ``utils/metric_utils.calc_collision_auc`` on the seeded arrays of ``tests/curve_cases.collision_cases``
(all below 0.5, all above 15, single elements, values EQUAL to thresholds of ``np.linspace(0.5, 15)`` -- which pins the strict
comparison --, realistic spreads).  Stored per case ``<name>``:

* ``<name>_in32`` / ``<name>_in64``: the input as float32 and as float64 (the float64 form is the float32 one cast back, except in
  ``on_thresholds``, whose float64 input holds the thresholds themselves);
* ``<name>_auc32`` / ``<name>_auc64``: what the call returns for each."""
import os.path as osp
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, osp.join(ROOT, "tests"))

import curve_cases as CC  # noqa: E402
from _ref_import import import_reference  # noqa: E402


def main():
    if not hasattr(np, "trapz"):            # the reference was written for numpy 1.x
        np.trapz = np.trapezoid
    mu = import_reference().metric_utils
    cases = CC.collision_cases()
    out = dict(names=np.array(list(cases)))
    for name, x in cases.items():
        x32 = x.astype(np.float32)
        x64 = x.astype(np.float64) if name == "on_thresholds" else x32.astype(np.float64)
        out[f"{name}_in32"], out[f"{name}_in64"] = x32, x64
        out[f"{name}_auc32"] = np.float64(mu.calc_collision_auc(x32))
        out[f"{name}_auc64"] = np.float64(mu.calc_collision_auc(x64))
        print(f"{name:18s} n = {len(x):3d}  auc32 {out[f'{name}_auc32']!r}  auc64 {out[f'{name}_auc64']!r}")
    path = osp.join(HERE, "metrics_curves.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, osp.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the MANO layer (``ihmr_amd.mano``) at N = 128 hands (a batch of 64 samples): today's call -- ``use_pca=False`` and none of
the newer arguments -- forward and forward + backward, the same with another build of the library (the parent commit's, built as a
library of its own) in alternating windows, and the wider call ``use_pca=True, num_pca_comps=6, transl, return_tips``.

Per configuration: the time per call from device events around a window of 50 calls that ends in a synchronise; five repetitions, one
window of every configuration per repetition (they alternate), median and min-max.  No bar is set on the wider call; for today's call
the claim is "no extra launch" (tests/test_gpu_mano_space.py proves it structurally), the parent's windows show the margin.

    python scripts/bench_mano_layer.py [--parent-library PATH] [--json PATH] [--hands N]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_cases as MC  # noqa: E402
from ihmr_amd import hip, mano  # noqa: E402
from ihmr_amd.assets import synthetic_mano  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-library", default=None, help="libihmr_hip.so of the parent commit, for the alternating windows")
ap.add_argument("--json", default=None)
ap.add_argument("--hands", type=int, default=128)
args = ap.parse_args()
N, WINDOW, REPS, K = args.hands, 50, 5, 6
hip.require_gpu()

libs = {"new": hip.lib()}
if args.parent_library:
    libs["parent"] = hip.bind(ctypes.CDLL(args.parent_library))      # it lacks the newer symbols: bind() skips them


def use(name):
    hip._LIB = libs[name]


up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
arrays = synthetic_mano(True)
orient, pose, betas = (up(a) for a in MC.inputs("mild", N, 17, arrays["hands_mean"]))
rng = np.random.RandomState(3)
coeffs, transl = up(MC._f32(0.6 * rng.standard_normal((N, K)))), up(MC._f32(0.3 * rng.standard_normal((N, 3))))
gv, gj16, gj21 = (up(MC._f32(rng.standard_normal(s))) for s in ((N, 778, 3), (N, 16, 3), (N, 21, 3)))

# one layer per library: its device tables belong to the library that made them
layers = {}
for name in libs:
    use(name)
    layers[name] = mano.create("", "mano", use_pca=False, is_rhand=True, batch_size=N).cuda()
    layers[name](global_orient=orient, hand_pose=pose, betas=betas)
use("new")
wide = mano.create("", "mano", use_pca=True, num_pca_comps=K, is_rhand=True, batch_size=N).cuda()


def plain(name, backward):
    def run():
        use(name)
        o, p, b = (t.detach().requires_grad_(backward) for t in (orient, pose, betas))
        out = layers[name](global_orient=o, hand_pose=p, betas=b)
        if backward:
            torch.autograd.backward([out.vertices, out.joints], [gv, gj16])
    return run


def wider(backward):
    def run():
        use("new")
        o, c, b, t = (x.detach().requires_grad_(backward) for x in (orient, coeffs, betas, transl))
        out = wide(global_orient=o, hand_pose=c, betas=b, transl=t, return_tips=True)
        if backward:
            torch.autograd.backward([out.vertices, out.joints], [gv, gj21])
    return run


runs = {}
for name in libs:
    runs[f"use_pca=False, {name} library, forward"] = plain(name, False)
    runs[f"use_pca=False, {name} library, forward + backward"] = plain(name, True)
runs[f"use_pca=True K={K} + transl + tips, forward"] = wider(False)
runs[f"use_pca=True K={K} + transl + tips, forward + backward"] = wider(True)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(WINDOW):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / WINDOW


for fn in runs.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(REPS):
    for k, fn in runs.items():                          # alternating: one window of every configuration per repetition
        times[k].append(window(fn))
use("new")

out = dict(hands=N, window=WINDOW, repetitions=REPS, num_pca_comps=K, parent_library=bool(args.parent_library), configs={})
for k, v in times.items():
    out["configs"][k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    print(f"{k:58s} {statistics.median(v):8.4f} ms per call of {N} hands [{min(v):.4f} - {max(v):.4f}]")
print(json.dumps(out))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(out, fh)

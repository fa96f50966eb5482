#!/usr/bin/env python3
"""Timing of the two-hand intersection volume (``ihmr_sdf_volume``: one box launch + one count launch of B * subdiv^3 workgroups) on a
batch of 64 hand pairs: the default synthetic batch and the deep-overlap batch, subdiv 1, 2 and 4, MANO faces with the wrist closed.

Reports, from ONE process (the six configurations alternate inside every repetition, five repetitions, median and min-max), the
time per call from device events around a window of calls that ends in a synchronise:
  * the C entry point alone (the two launches, preallocated outputs, no bits);
  * ``ihmr_amd.sdf.penetration_volume`` (the launches + the torch arithmetic that forms the volume).
With every row: the workgroups per launch (subdiv 1 puts only 64 workgroups on the 256 CUs), the batch's median volume in cm^3 and the
share of samples whose hands intersect.

    python scripts/bench_volume.py [batch] [json output path]
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ihmr_amd import hip, two_hand  # noqa: E402
from ihmr_amd import mano as mano_shim  # noqa: E402
from ihmr_amd.sdf import _volume_faces, penetration_volume  # noqa: E402
from ihmr_amd.synthetic import synthetic_opt_batch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
WINDOW, REPS = 50, 5
DEEP_SEED = 6475                   # the deep batch of the collision tests (tests/helpers.py)

right = mano_shim.create("MANO_RIGHT.pkl", "mano", use_pca=False, is_rhand=True, batch_size=2 * B).cuda()
left = mano_shim.create("MANO_LEFT.pkl", "mano", use_pca=False, is_rhand=False, batch_size=2 * B)
fwd = lambda p, s, t: two_hand.forward_from_packed(right, p.cuda(), s.cuda(), t.cuda())


def hands(seed, overlap):
    out = {}

    def joints_only(p, s, t):
        out["verts"] = fwd(p, s, t)
        return out["verts"][2]
    batch = synthetic_opt_batch(B, joints_only, seed=seed, overlap=overlap)
    with torch.no_grad():
        rv, lv, _ = fwd(batch["init_pose_params"], batch["init_shape_params"], batch["init_hand_trans"][:, 0, :3])
    return rv.contiguous(), lv.contiguous()


batches = {"default": hands(11, None), "deep": hands(DEEP_SEED, "deep")}
faces = (np.asarray(right.faces), np.asarray(left.faces))
dev = batches["default"][0].device
fa, fb = _volume_faces(faces[0], 778, True, dev), _volume_faces(faces[1], 778, True, dev)       # the closed tables: 1552 faces each
box = torch.empty(B, 4, device="cuda")
status = torch.empty(B, device="cuda", dtype=torch.int32)
counts = torch.empty(B, 64, device="cuda", dtype=torch.int32)


def entry_point(name, n):
    va, vb = batches[name]
    hip.check(hip.lib().ihmr_sdf_volume(va.data_ptr(), fa.data_ptr(), 778, len(fa), vb.data_ptr(), fb.data_ptr(), 778, len(fb), B, n, None,
                                        box.data_ptr(), status.data_ptr(), counts.data_ptr(), None, hip.stream_ptr()), "ihmr_sdf_volume")


def wrapper(name, n):
    penetration_volume(*batches[name], faces[0], faces[1], subdiv=n)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(WINDOW):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / WINDOW


runs = {}
for name in batches:
    for n in (1, 2, 4):
        runs[f"{name}, subdiv {n}, entry point"] = (lambda name=name, n=n: entry_point(name, n))
        runs[f"{name}, subdiv {n}, penetration_volume"] = (lambda name=name, n=n: wrapper(name, n))
for fn in runs.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(REPS):
    for k, fn in runs.items():                          # alternating: one window of every configuration per repetition
        times[k].append(window(fn))

out = dict(batch=B, window=WINDOW, repetitions=REPS, configs={}, volumes={})
for name in batches:
    for n in (1, 2, 4):
        vol, cnt, _, st = penetration_volume(*batches[name], faces[0], faces[1], subdiv=n)
        vol = vol.cpu().numpy() * 1e6
        out["volumes"][f"{name}, subdiv {n}"] = dict(median_cm3=float(np.median(vol)), mean_cm3=float(vol.mean()), pen_rate=float((vol > 0).mean()),
                                                     counted=int((st == 0).sum()), voxels=int(cnt.sum()))
for k, v in times.items():
    n = int(k.split("subdiv ")[1][0])
    out["configs"][k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), workgroups=B * n ** 3)
    vk = out["volumes"][k.rsplit(",", 1)[0]]
    print(f"{k:44s} {statistics.median(v):9.4f} ms per batch of {B} (min {min(v):.4f}, max {max(v):.4f}), {B * n ** 3:5d} workgroups, "
          f"median {vk['median_cm3']:.2f} cm^3, pen_rate {vk['pen_rate']:.2f}")
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(out, fh)

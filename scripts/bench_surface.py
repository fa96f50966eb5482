#!/usr/bin/env python3
"""Timing of the exact point-to-surface distance (``ihmr_surface_distance``: per call B * 4 workgroups, each lane one of a hand's 778
vertices against the other hand's 1552 triangles in float64) on a batch of 64 hand pairs -- the default synthetic batch and the
deep-overlap batch as ground truth, the prediction = ground truth + N(0, 2 mm) noise -- and the measurement that motivates it: how far
the vertex-to-vertex ``near`` of the contact metrics lies above the distance to the surface.

Reports, from ONE process (the configurations alternate inside every repetition, five repetitions, median and min-max), the time per
call from device events around a window of 50 calls that ends in a synchronise:
  * the C entry point alone: the two calls of one mesh pair (right on left, left on right; preallocated outputs);
  * the backward entry point, both gradients, the same two calls;
  * ``Evaluator.update_device_surface`` without and with GT meshes (2 and 4 calls + the torch arithmetic of the per-sample rows; the
    accumulator is cleared between windows);
and next to it the float64 numpy statement (tests/surface_ref.py) on the first samples of the batch, wall clock, scaled to the batch.
With every batch: the depth metrics, and ``near`` (vertex to nearest vertex) against the surface distance: the mean and the maximum of
``near - |dist|`` in mm and the vertices whose contact status at 3 mm and 5 mm differs.  No bar is set for any of these numbers.

    python scripts/bench_surface.py [batch] [json output path]
"""
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ihmr_amd import hip, sdf, two_hand  # noqa: E402
from ihmr_amd import mano as mano_shim  # noqa: E402
from ihmr_amd.assets import synthetic_mano  # noqa: E402
from ihmr_amd.evaluator import SURFACE_THRESHOLDS, Evaluator  # noqa: E402
from ihmr_amd.synthetic import synthetic_opt_batch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
WINDOW, REPS, HOST_SAMPLES = 50, 5, 2
DEEP_SEED = 6475                   # the deep batch of the collision tests (tests/helpers.py)
NV = 778

right = mano_shim.create("MANO_RIGHT.pkl", "mano", use_pca=False, is_rhand=True, batch_size=2 * B).cuda()
fwd = lambda p, s, t: two_hand.forward_from_packed(right, p.cuda(), s.cuda(), t.cuda())
models = dict(right=types.SimpleNamespace(faces=synthetic_mano(True)["faces"]), left=types.SimpleNamespace(faces=synthetic_mano(False)["faces"]))


def hands(seed, overlap):
    batch = synthetic_opt_batch(B, lambda p, s, t: fwd(p, s, t)[2], seed=seed, overlap=overlap)
    with torch.no_grad():
        rv, lv, _ = fwd(batch["init_pose_params"], batch["init_shape_params"], batch["init_hand_trans"][:, 0, :3])
    gen = torch.Generator(device="cuda").manual_seed(seed)
    noise = lambda v: v + 0.002 * torch.randn(v.shape, device=v.device, generator=gen)
    return noise(rv).contiguous(), noise(lv).contiguous(), rv.contiguous(), lv.contiguous()


batches = {"default": hands(11, None), "deep": hands(DEEP_SEED, "deep")}
weight = torch.ones(B, 2, device="cuda")
tables = {h: sdf._surface_faces(models[h].faces, NV, True, torch.device("cuda", torch.cuda.current_device())) for h in ("right", "left")}
dist = torch.empty(2, B, NV, device="cuda", dtype=torch.float64)
face = torch.empty(2, B, NV, device="cuda", dtype=torch.int32)
bary = torch.empty(2, B, NV, 3, device="cuda", dtype=torch.float64)
g_dist = torch.ones(B, NV, device="cuda", dtype=torch.float64)
d_points = torch.empty(B, NV, 3, device="cuda")
d_verts = torch.empty(B, NV, 3, device="cuda")
evaluator = Evaluator(models, surface_metrics=True)


def entry_point(name):
    pr, pl = batches[name][:2]
    for k, (q, v, h) in enumerate(((pr, pl, "left"), (pl, pr, "right"))):
        t, fd = tables[h]
        hip.check(hip.lib().ihmr_surface_distance(q.data_ptr(), NV, v.data_ptr(), NV, t.data_ptr(), fd, len(t), None, B, 1, dist[k].data_ptr(),
                                                  face[k].data_ptr(), bary[k].data_ptr(), hip.stream_ptr()), "ihmr_surface_distance")


def backward(name):
    pr, pl = batches[name][:2]
    for k, (q, v, h) in enumerate(((pr, pl, "left"), (pl, pr, "right"))):
        t, fd = tables[h]
        hip.check(hip.lib().ihmr_surface_distance_bwd(q.data_ptr(), NV, v.data_ptr(), NV, t.data_ptr(), fd, len(t), None, B, dist[k].data_ptr(),
                                                      face[k].data_ptr(), bary[k].data_ptr(), g_dist.data_ptr(), d_points.data_ptr(),
                                                      d_verts.data_ptr(), hip.stream_ptr()), "ihmr_surface_distance_bwd")


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(WINDOW):
        fn()
    e1.record()
    torch.cuda.synchronize()
    evaluator.clear()
    return e0.elapsed_time(e1) / WINDOW


def statement_ms(name):
    """Wall clock of the numpy statement on HOST_SAMPLES samples (both directions), scaled to the batch."""
    import surface_ref as SR
    pr, pl = (t[:HOST_SAMPLES].cpu().numpy() for t in batches[name][:2])
    fr, fl = SR.hand_faces("mitten")
    t0 = time.perf_counter()
    for b in range(HOST_SAMPLES):
        SR.surface_distance(pr[b], pl[b], fl, 1538)
        SR.surface_distance(pl[b], pr[b], fr, 1538)
    return (time.perf_counter() - t0) * 1e3 * B / HOST_SAMPLES


def near_against_surface(name):
    """``near`` (each vertex to the nearest VERTEX of the other hand, float64) against |dist| to the other hand's surface."""
    pr, pl = batches[name][:2]
    entry_point(name)
    d = torch.cdist(pr.double(), pl.double())
    near = torch.cat([d.min(dim=2).values, d.min(dim=1).values], dim=1)                    # (B,1556), right hand first
    sd = torch.cat([dist[0], dist[1]], dim=1)
    gap = near - sd.abs()
    close = near < 0.02                                                                    # where contact is decided: within 2 cm
    out = dict(mean_gap_mm=float(gap.mean() * 1e3), max_gap_mm=float(gap.max() * 1e3), mean_gap_within_2cm_mm=float(gap[close].mean() * 1e3),
               max_gap_within_2cm_mm=float(gap[close].max() * 1e3), vertices=int(gap.numel()), inside=int((sd < 0).sum()))
    for tau in SURFACE_THRESHOLDS:
        a, b = near < tau, sd < tau
        out[f"contact_{tau * 1e3:g}mm"] = dict(vertex_rule=int(a.sum()), surface_rule=int(b.sum()), changed=int((a != b).sum()))
    return out


runs = {}
for name in batches:
    runs[f"{name}, entry point (2 calls)"] = (lambda name=name: entry_point(name))
    runs[f"{name}, backward (2 calls)"] = (lambda name=name: backward(name))
    runs[f"{name}, update_device_surface"] = (lambda name=name: evaluator.update_device_surface(*batches[name][:2]))
    runs[f"{name}, update_device_surface + GT"] = (lambda name=name: evaluator.update_device_surface(*batches[name], weight))
for fn in runs.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
evaluator.clear()
times = {k: [] for k in runs}
for _ in range(REPS):
    for k, fn in runs.items():                          # alternating: one window of every configuration per repetition
        times[k].append(window(fn))

out = dict(batch=B, window=WINDOW, repetitions=REPS, thresholds=list(SURFACE_THRESHOLDS), configs={}, batches={}, host={})
for name in batches:
    evaluator.clear()
    evaluator.update_device_surface(*batches[name], weight)
    m = Evaluator.surface_metrics_from_sums(evaluator.surface_sums())
    out["batches"][name] = dict(pen_depth_max=m["pen_depth_max"], pen_depth_ave=m["pen_depth_ave"], pen_vertex_rate=m["pen_vertex_rate"],
                                surface_contact_f1=m["surface_contact_f1"].tolist(), near=near_against_surface(name))
    out["host"][name] = dict(ms_scaled_to_batch=statement_ms(name), samples_timed=HOST_SAMPLES)
evaluator.clear()
for k, v in times.items():
    out["configs"][k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    print(f"{k:44s} {statistics.median(v):9.4f} ms per batch of {B} (min {min(v):.4f}, max {max(v):.4f})")
for name, h in out["host"].items():
    print(f"{name + ', numpy statement':44s} {h['ms_scaled_to_batch']:9.0f} ms per batch of {B} (wall clock of {HOST_SAMPLES} samples, scaled)")
for name, bk in out["batches"].items():
    n = bk["near"]
    print(f"{name}: pen_depth_max {bk['pen_depth_max']:.3f} mm, pen_depth_ave {bk['pen_depth_ave']:.4f} mm, pen_vertex_rate {bk['pen_vertex_rate']:.4f}; "
          f"near - |dist|: mean {n['mean_gap_mm']:.3f} mm, max {n['max_gap_mm']:.3f} mm (within 2 cm: mean {n['mean_gap_within_2cm_mm']:.3f}, max "
          f"{n['max_gap_within_2cm_mm']:.3f}); contact at 3 mm {n['contact_3mm']}, at 5 mm {n['contact_5mm']} of {n['vertices']} vertices")
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(out, fh)

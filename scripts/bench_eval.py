#!/usr/bin/env python3
"""Timing of the evaluator with the Procrustes-aligned metrics on, one batch of 64 samples with GT meshes (the IHMR-Baseline / IHMR-MLP
case): the device path against the host loop.

Reports, from ONE process (the two sides alternate inside every repetition, five repetitions, median and min-max):
  * device: `Evaluator.update_device` + `update_device_verts` + `update_device_pa` + `update_device_pa_verts` on device tensors, per
    batch, from device events around a window of batches that ends in a synchronise; and the same window closed by `metric_sums()` +
    `pa_metric_sums()` (the one device-to-host copy of the run), in wall-clock time;
  * the PA part alone (`update_device_pa` + `update_device_pa_verts`), to show what the two new kernels add;
  * host: `Evaluator(pa_metrics=True).update` on the exported numpy arrays of the same batch (the per-sample loop, one LAPACK SVD per set),
    and the same with `pa_metrics=False`, in wall-clock time per batch.

    python scripts/bench_eval.py [--curves] [batch] [json output path]

``--curves`` adds the curve metrics (PCK counts of the five error populations, F-score counts, collision AUC) to the same alternation:
  * device: `update_device_curves` + `update_device_curve_verts` per batch from device events, the same window closed by `curve_sums()`
    in wall-clock time, `ihmr_eval_curve_verts` alone (the launch, no torch arithmetic around it), and everything together (the set of
    metrics above + the curves);
  * host: `Evaluator(curve_metrics=True).update` + `curve_sums()` on the exported arrays (the per-sample loop with four 778 x 778
    nearest-neighbour searches per hand).
Without the flag the output is what it was.
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
from ihmr_amd.evaluator import Evaluator  # noqa: E402

CURVES = "--curves" in sys.argv
sys.argv = [a for a in sys.argv if a != "--curves"]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
WINDOW, HOST_WINDOW, REPS = 50, 2, 5
rng = np.random.RandomState(0)
gt = rng.normal(0, 0.05, (B, 42, 3)).astype(np.float32)
res = dict(pred_cam_params=np.zeros((B, 3), np.float32), pred_shape_params=np.zeros((B, 20), np.float32), pred_pose_params=np.zeros((B, 96), np.float32),
           pred_hand_trans=np.zeros((B, 3), np.float32), pred_joints_3d=gt + rng.normal(0, 0.005, (B, 42, 3)).astype(np.float32),
           gt_joints_3d=np.concatenate([gt, np.ones((B, 42, 1), np.float32)], 2),
           collision_loss_origin_scale=np.abs(rng.normal(0, 1e-3, (B, 1556))).astype(np.float32), mano_params_weight=np.ones((B, 2), np.float32))
for side in ("right", "left"):
    res[f"gt_{side}_hand_verts"] = rng.normal(0, 0.04, (B, 778, 3)).astype(np.float32)
    res[f"pred_{side}_hand_verts"] = res[f"gt_{side}_hand_verts"] + rng.normal(0, 0.003, (B, 778, 3)).astype(np.float32)
one_hot = np.zeros(778, np.float32)
one_hot[0] = 1.0
mano = types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=np.stack([one_hot] * 16))
mano = dict(right=mano, left=mano)
dev = {k: torch.from_numpy(v).cuda() for k, v in res.items()}
meshes = [dev[f"{m}_{s}_hand_verts"] for m in ("pred", "gt") for s in ("right", "left")]      # pred right, pred left, gt right, gt left
ev = Evaluator(mano, curve_metrics=CURVES)


def device_all():
    ev.update_device(dev["pred_joints_3d"], dev["gt_joints_3d"], dev["collision_loss_origin_scale"])
    ev.update_device_verts(*meshes, dev["mano_params_weight"])
    device_pa()


def device_pa():
    ev.update_device_pa(dev["pred_joints_3d"], dev["gt_joints_3d"])
    ev.update_device_pa_verts(*meshes, dev["mano_params_weight"])


def device_window(fn, read_sums):
    ev.clear()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(WINDOW):
        fn()
    e1.record()
    if read_sums:
        ev.metric_sums(), ev.pa_metric_sums()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / WINDOW
    return wall if read_sums else e0.elapsed_time(e1) / WINDOW


def host_window(pa):
    h = Evaluator(mano, pa_metrics=pa)
    t0 = time.perf_counter()
    for _ in range(HOST_WINDOW):
        h.update(np.arange(B), res, save_verts=False)
    h.metric_sums(), h.pa_metric_sums()
    return (time.perf_counter() - t0) * 1e3 / HOST_WINDOW


runs = {"device, all metrics (events)": lambda: device_window(device_all, False),
        "device, all metrics + sums read back (wall)": lambda: device_window(device_all, True),
        "device, PA kernels alone (events)": lambda: device_window(device_pa, False),
        "host loop, PA metrics on (wall)": lambda: host_window(True),
        "host loop, PA metrics off (wall)": lambda: host_window(False)}
if CURVES:
    from ihmr_amd import hip

    def device_curves():
        ev.update_device_curves(dev["pred_joints_3d"], dev["gt_joints_3d"])
        ev.update_device_curve_verts(*meshes, dev["mano_params_weight"])

    def device_everything():
        device_all()
        device_curves()

    T, F = len(ev.thresholds), len(ev.f_thresholds)
    thr_d, fthr_d = torch.from_numpy(ev.thresholds).cuda(), torch.from_numpy(ev.f_thresholds).cuda()
    root_w = torch.from_numpy(ev.root_weights).cuda().contiguous()
    counts_d = torch.empty(B, 2, 2, T + 1, device="cuda", dtype=torch.float64)
    fc_d = torch.empty(B, 2, 2, 2, F, device="cuda", dtype=torch.float64)

    def vertex_kernel():
        hip.check(hip.lib().ihmr_eval_curve_verts(*[m.data_ptr() for m in meshes], root_w.data_ptr(), dev["mano_params_weight"].data_ptr(), None,
                                                  B, thr_d.data_ptr(), T, fthr_d.data_ptr(), F, counts_d.data_ptr(), fc_d.data_ptr(), None,
                                                  hip.stream_ptr()), "ihmr_eval_curve_verts")

    def curve_window(fn, read_sums):
        ev.clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(WINDOW):
            fn()
        e1.record()
        if read_sums:
            ev.curve_sums()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / WINDOW
        return wall if read_sums else e0.elapsed_time(e1) / WINDOW

    def host_curve_window():
        h = Evaluator(mano, curve_metrics=True)
        t0 = time.perf_counter()
        for _ in range(HOST_WINDOW):
            h.update(np.arange(B), res, save_verts=False)
        h.metric_sums(), h.pa_metric_sums(), h.curve_sums()
        return (time.perf_counter() - t0) * 1e3 / HOST_WINDOW

    runs.update({"device, curve metrics (events)": lambda: curve_window(device_curves, False),
                 "device, curve metrics + sums read back (wall)": lambda: curve_window(device_curves, True),
                 "device, curve vertex kernel alone (events)": lambda: curve_window(vertex_kernel, False),
                 "device, all metrics + curve metrics (events)": lambda: curve_window(device_everything, False),
                 "host loop, curve metrics on (wall)": host_curve_window})
    for _ in range(3):
        device_curves()
for _ in range(3):
    device_all()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(REPS):
    for k, fn in runs.items():                          # alternating: one window of every configuration per repetition
        times[k].append(fn())

# the two sides report the same numbers
ev.clear()
device_all()
h = Evaluator(mano, pa_metrics=True)
h.update(np.arange(B), res, save_verts=False)
agree = float(np.abs(ev.pa_metric_sums() / h.pa_metric_sums() - 1.0).max())
out = dict(batch=B, window=WINDOW, host_window=HOST_WINDOW, repetitions=REPS, pa_sums_max_relative_difference=agree, configs={})
for k, v in times.items():
    out["configs"][k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    print(f"{k:46s} {statistics.median(v):9.4f} ms per batch of {B} (min {min(v):.4f}, max {max(v):.4f})")
print(f"PA sums, device against host: max relative difference {agree:.1e}")
if CURVES:
    ev.clear()
    device_everything()
    h = Evaluator(mano, curve_metrics=True)
    h.update(np.arange(B), res, save_verts=False)
    out["curve_sums_entries_that_differ"] = int(np.sum(ev.curve_sums() != h.curve_sums()))
    print(f"curve sums, device against host: {out['curve_sums_entries_that_differ']} of {len(h.curve_sums())} entries differ")
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(out, fh)

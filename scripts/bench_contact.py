#!/usr/bin/env python3
"""Timing of the contact-consistency kernel (``ihmr_eval_contact``: one launch of B * 2 workgroups, each a 778 x 778 float64 distance
walk over both mesh pairs) on a batch of 64 hand pairs: the default synthetic batch and the deep-overlap batch as ground truth, the
prediction = ground truth + N(0, 2 mm) noise.

Reports, from ONE process (the configurations alternate inside every repetition, five repetitions, median and min-max), the time per
call from device events around a window of 50 calls that ends in a synchronise:
  * the C entry point alone (preallocated outputs, no ``near``);
  * ``Evaluator.update_device_contact`` (the launch + the torch arithmetic that forms the per-sample rows; the accumulator is cleared
    between windows);
and next to it the numpy host loop (``get_single_contact`` per sample) on the same batch, wall clock, three runs.  With every batch: the
mean number of GT contact pairs, ``contact_dev`` and ``contact_f1``.  No bar is set for any of these numbers.

    python scripts/bench_contact.py [batch] [json output path]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ihmr_amd import hip, two_hand  # noqa: E402
from ihmr_amd import mano as mano_shim  # noqa: E402
from ihmr_amd.evaluator import CONTACT_THRESHOLDS, Evaluator, get_single_contact  # noqa: E402
from ihmr_amd.synthetic import synthetic_opt_batch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
WINDOW, REPS, HOST_RUNS = 50, 5, 3
DEEP_SEED = 6475                   # the deep batch of the collision tests (tests/helpers.py)
K = len(CONTACT_THRESHOLDS)

right = mano_shim.create("MANO_RIGHT.pkl", "mano", use_pca=False, is_rhand=True, batch_size=2 * B).cuda()
fwd = lambda p, s, t: two_hand.forward_from_packed(right, p.cuda(), s.cuda(), t.cuda())


def hands(seed, overlap):
    batch = synthetic_opt_batch(B, lambda p, s, t: fwd(p, s, t)[2], seed=seed, overlap=overlap)
    with torch.no_grad():
        rv, lv, _ = fwd(batch["init_pose_params"], batch["init_shape_params"], batch["init_hand_trans"][:, 0, :3])
    gen = torch.Generator(device="cuda").manual_seed(seed)
    noise = lambda v: v + 0.002 * torch.randn(v.shape, device=v.device, generator=gen)
    return noise(rv).contiguous(), noise(lv).contiguous(), rv.contiguous(), lv.contiguous()


batches = {"default": hands(11, None), "deep": hands(DEEP_SEED, "deep")}
weight = torch.ones(B, 2, device="cuda")
thr = torch.tensor(CONTACT_THRESHOLDS, dtype=torch.float64, device="cuda")
pair = torch.empty(B, 2, 2, device="cuda", dtype=torch.float64)
counts = torch.empty(B, 2, K, 3, device="cuda", dtype=torch.float64)
evaluator = Evaluator(interaction_metrics=True)


def entry_point(name):
    pr, pl, gr, gl = batches[name]
    hip.check(hip.lib().ihmr_eval_contact(pr.data_ptr(), pl.data_ptr(), gr.data_ptr(), gl.data_ptr(), weight.data_ptr(), None, None, B,
                                          thr.data_ptr(), K, pair.data_ptr(), counts.data_ptr(), None, hip.stream_ptr()), "ihmr_eval_contact")


def wrapper(name):
    evaluator.update_device_contact(*batches[name], weight)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(WINDOW):
        fn()
    e1.record()
    torch.cuda.synchronize()
    evaluator.clear()
    return e0.elapsed_time(e1) / WINDOW


def host_loop(name):
    arrays = [t.cpu().numpy() for t in batches[name]]
    t0 = time.perf_counter()
    for b in range(B):
        get_single_contact(arrays[0][b], arrays[1][b], arrays[2][b], arrays[3][b], 1.0, CONTACT_THRESHOLDS)
    return (time.perf_counter() - t0) * 1e3


runs = {}
for name in batches:
    runs[f"{name}, entry point"] = (lambda name=name: entry_point(name))
    runs[f"{name}, update_device_contact"] = (lambda name=name: wrapper(name))
for fn in runs.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
evaluator.clear()
times = {k: [] for k in runs}
for _ in range(REPS):
    for k, fn in runs.items():                          # alternating: one window of every configuration per repetition
        times[k].append(window(fn))

out = dict(batch=B, window=WINDOW, repetitions=REPS, thresholds=list(CONTACT_THRESHOLDS), configs={}, batches={}, host={})
for name in batches:
    evaluator.clear()
    wrapper(name)
    s = evaluator.interaction_sums()
    m = Evaluator.interaction_metrics_from_sums(s)
    entry_point(name)
    torch.cuda.synchronize()
    out["batches"][name] = dict(mean_pairs=float(pair[:, 0, 1].mean()), samples_with_contact=int(s[3]), contact_dev=m["contact_dev"],
                                contact_rate=m["contact_rate"], contact_f1=m["contact_f1"].tolist())
    h = [host_loop(name) for _ in range(HOST_RUNS)]
    out["host"][name] = dict(median_ms=statistics.median(h), min_ms=min(h), max_ms=max(h))
evaluator.clear()
for k, v in times.items():
    out["configs"][k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), workgroups=2 * B)
    bk = out["batches"][k.split(",")[0]]
    print(f"{k:36s} {statistics.median(v):9.4f} ms per batch of {B} (min {min(v):.4f}, max {max(v):.4f}), {2 * B} workgroups, "
          f"mean |C| {bk['mean_pairs']:.1f}, contact_dev {bk['contact_dev'] * 1e3:.2f} mm")
for name, h in out["host"].items():
    print(f"{name + ', numpy host loop':36s} {h['median_ms']:9.1f} ms per batch of {B} (min {h['min_ms']:.1f}, max {h['max_ms']:.1f}), wall clock")
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(out, fh)

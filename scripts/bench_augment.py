#!/usr/bin/env python3
"""Timing of the training-time augmentation chain (ihmr_amd/augment.py) at the training batch: 64 crops -> (64,3,224,224).

Reports, from ONE process (the configurations alternate inside every repetition, device events around windows of launches that end
in a synchronise, five repetitions, median and min-max):
  * ms per batch with all six augmentations on (draws included: the host makes them per batch, as a training step would);
  * ms per batch with none on (the chain's pad / resize / flip kernel alone, through the same entry point);
  * the existing `ihmr_preprocess_images` (test-time preprocessing) for comparison;
  * every step switched on alone, and the bytes each step reads and writes (computed from the shapes).

    python scripts/bench_augment.py [batch] [json output path]
"""
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ihmr_amd import augment as G
from ihmr_amd.preprocess import DataProcessor

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
S, WINDOW, REPS = 224, 100, 5
FLAGS = ("use_random_flip", "use_random_rescale", "use_random_position", "use_random_rotation", "use_color_jittering", "use_motion_blur")
rng = np.random.RandomState(0)
shapes = [(int(rng.randint(200, 600)), int(rng.randint(200, 600))) for _ in range(B)]
images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in shapes]
types_host = np.ones((B, 2), np.float32)
labels = dict(joints_2d=rng.uniform(0, 200, (B, 42, 3)), joints_3d=rng.normal(0, 0.1, (B, 42, 4)), mano_pose=rng.normal(0, 0.5, (B, 96)),
              mano_betas=rng.normal(0, 0.5, (B, 20)), mano_params_weight=np.ones((B, 2)), hand_type_array=types_host)
labels = {k: torch.as_tensor(np.asarray(v, np.float32)).cuda() for k, v in labels.items()}
pre = DataProcessor(final_size=S)
buf, off, sz = pre.pack(images)
buf, off, sz = buf.cuda(), off.cuda(), sz.cuda()


def processor(**on):
    opt = types.SimpleNamespace(inputSize=S, motion_blur_prob=1.0, **{f: bool(on.get(f)) for f in FLAGS})
    return G.TrainDataProcessor(opt, G.line_blur_kernels(), seed=0)


configs = {
    "all six on": processor(**{f: True for f in FLAGS}),
    "none on": processor(),
    "rescale + position only": processor(use_random_rescale=True, use_random_position=True),
    "rotation only": processor(use_random_rotation=True),
    "colour only": processor(use_color_jittering=True),
    "blur only (every sample)": processor(use_motion_blur=True),
}
runs = {k: (lambda p=p: p.apply_packed(buf, off, sz, labels, p.draw(types_host))) for k, p in configs.items()}
fixed = configs["all six on"].draw(types_host)
runs["all six on, draws reused"] = lambda: configs["all six on"].apply_packed(buf, off, sz, labels, fixed)
runs["ihmr_preprocess_images"] = lambda: pre.preprocess_packed(buf, off, sz)

for fn in runs.values():                               # every shape and code object once
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(REPS):
    for k, fn in runs.items():                         # alternating: one window of every configuration per repetition
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(WINDOW):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / WINDOW)

img = B * S * S * 3
src = sum(im.size for im in images)
step_bytes = {                                         # bytes a step reads + writes (uint8 in, uint8 out; the last one adds the float planes)
    "pad / resize / flip": src + img,
    "rescale": 2 * img, "rotation": 2 * img, "grey sum": img, "colour": 2 * img, "blur": 2 * img, "float planes (last step)": 4 * img,
}
res = dict(batch=B, final_size=S, window=WINDOW, repetitions=REPS, step_bytes=step_bytes,
           ms_per_batch={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()})
for k, v in res["ms_per_batch"].items():
    print(f"{k:32s} {v['median']:.4f} ms per batch of {B} (min {v['min']:.4f}, max {v['max']:.4f})")
print("bytes per step (MB):", {k: round(v / 1e6, 1) for k, v in step_bytes.items()})
print(json.dumps(res))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as fh:
        json.dump(res, fh)

#!/usr/bin/env python3
"""Timing of the mesh renderer (ihmr_amd/render.py, `ihmr_render_meshes`): a batch of two-hand samples drawn over a background image.

Reports, from ONE process (the configurations alternate inside every repetition, device events around windows of launches that end in a
synchronise, five repetitions, median and min-max):
  * ms per batch at S = 448 (the evaluator's size) and S = 224 through `MeshRenderer.render` (with its per-call allocations and
    conversions on the host), with and without the face-id output, and of the entry point alone on buffers made once (the device's share);
  * the HBM bytes a launch pair must move (background read + image write + vertex and face tables + the vertex workspace written and
    read back), computed from the shapes, over the time, as a fraction of the 8 TB/s peak;
  * the numpy restatement (tests/render_ref.py) for ONE image of the same scene on the CPU, as the baseline.

With `--views N` the S = 448 batch is also drawn through `MeshRenderer.render_views` with N turned views next to the camera's (one
`ihmr_view_vertices` launch and one more render each); with `--collision_map` it is also drawn painted by a per-vertex penetration depth
(`penetration_colors` = one `ihmr_heat_colours` launch, then `ihmr_paint_meshes`).  Both alternate with the plain render in the same windows.

    python scripts/bench_render.py [batch] [json output path] [--views N] [--collision_map]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_cases as RC  # noqa: E402  (the deep-overlap synthetic hands of the tests)
import render_ref as R  # noqa: E402
from ihmr_amd import render  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=64)
ap.add_argument("json_path", nargs="?", default=None)
ap.add_argument("--views", type=int, default=0, help="number of turned views drawn next to the camera's view")
ap.add_argument("--collision_map", action="store_true", help="also draw the batch painted by a per-vertex penetration depth")
args = ap.parse_args()
B = args.batch
WINDOW, REPS, HBM_PEAK = 50, 5, 8.0e12
rng = np.random.RandomState(0)
base = RC.hand_verts()
verts = torch.from_numpy(base[np.arange(B) % base.shape[0]] + rng.normal(0, 0.0005, (B, 1556, 3)).astype(np.float32)).cuda()
cam_host = np.stack([rng.uniform(4.5, 6.5, B), rng.uniform(-0.1, -0.075, B), rng.uniform(-0.02, 0.02, B)], 1).astype(np.float32)
cam = torch.from_numpy(cam_host).cuda()
fr, fl = RC.hand_faces()
renderer = render.MeshRenderer(fr, fl)
bgs = {S: torch.from_numpy(rng.randint(0, 256, (B, S, S, 3)).astype(np.uint8)).cuda() for S in (448, 224)}

runs = {}
for S in (448, 224):
    runs[f"S = {S}"] = lambda S=S: renderer.render(verts[:, :778], verts[:, 778:], cam, bgs[S])
    runs[f"S = {S}, with face ids"] = lambda S=S: renderer.render(verts[:, :778], verts[:, 778:], cam, bgs[S], return_face_ids=True)
if args.views > 0:
    view_list = [None] + [("yxz"[k % 3], 90.0 + 35.0 * (k // 3)) for k in range(args.views)]
    runs[f"S = 448, {args.views} extra view(s)"] = lambda: renderer.render_views(verts[:, :778], verts[:, 778:], cam, view_list, bgs[448])
if args.collision_map:
    depth = torch.from_numpy(rng.uniform(-0.002, 0.008, (B, 1556)).astype(np.float32)).cuda()
    runs["S = 448, heat map"] = lambda: renderer.render(verts[:, :778], verts[:, 778:], cam, bgs[448],
                                                        vertex_colors=render.penetration_colors(depth))


def entry_point_alone(S):
    """The two launches of `ihmr_render_meshes` on buffers made once: what the device takes, without the Python wrapper's per-call
    allocations and conversions."""
    import ctypes as C
    from ihmr_amd import hip
    L = hip.lib()
    faces, off, ids = renderer._tables(verts.device)
    albedo = torch.tensor([render.COLORS["light_green"], render.COLORS["light_blue"]], dtype=torch.float32).repeat(B, 1, 1).cuda().contiguous()
    ws = torch.empty(L.ihmr_render_workspace_bytes(B, 1556), dtype=torch.uint8, device="cuda")
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    lights = render._lights_struct()
    keep = (faces, off, ids, albedo, ws, out, lights)
    args = (hip.ptr(verts), hip.ptr(faces), hip.ptr(off), hip.ptr(ids), 1556, 3076, 1538, None, hip.ptr(albedo), hip.ptr(cam), C.byref(lights),
            hip.ptr(bgs[S]), S, hip.ptr(out), None, hip.ptr(ws), B, hip.stream_ptr())
    return lambda keep=keep: hip.check(L.ihmr_render_meshes(*args), "ihmr_render_meshes")


for S in (448, 224):
    runs[f"S = {S}, entry point alone"] = entry_point_alone(S)

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

covered = {}
for S in (448, 224):
    _, ids = renderer.render(verts[:, :778], verts[:, 778:], cam, bgs[S], return_face_ids=True)
    covered[S] = float((ids >= 0).float().mean().item())


def launch_bytes(S, with_ids, views=0, heat=False):
    tables = B * 1556 * 12 + 3076 * 12 + 1557 * 4 + 3 * 3076 * 4 + B * (12 + 24 + 2)       # vertices, faces, CSR, camera / albedo / present
    workspace = 2 * B * 1556 * 24                                                          # written by the vertex launch, read by the raster launch
    one = 2 * B * S * S * 3 + (B * S * S * 4 if with_ids else 0) + tables + workspace
    turned = B * S * S * 3 + tables + workspace + 2 * B * 1556 * 12                        # on white: no background read; vertices read and written
    painted = B * 1556 * 4 + 2 * B * 1556 * 12                                             # depth read, colours written and read back
    return one + views * turned + (painted if heat else 0)


t0 = time.perf_counter()
R.render_sample(base[0], RC.faces(), cam_host[0], 448, RC.TWO_HAND, RC.SPLIT, (1, 1), bgs[448][0].cpu().numpy())
cpu_ms = (time.perf_counter() - t0) * 1e3

res = dict(batch=B, window=WINDOW, repetitions=REPS, covered_fraction=covered, cpu_restatement_ms_per_image_448=cpu_ms, configs={})
for k, v in times.items():
    S, with_ids = (448 if "448" in k else 224), "face ids" in k
    med = statistics.median(v)
    nbytes = launch_bytes(S, with_ids, args.views if "extra view" in k else 0, "heat map" in k)
    res["configs"][k] = dict(median_ms=med, min_ms=min(v), max_ms=max(v), hbm_bytes=nbytes, fraction_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK)
    print(f"{k:28s} {med:.4f} ms per batch of {B} (min {min(v):.4f}, max {max(v):.4f}); {nbytes / 1e6:.1f} MB -> "
          f"{nbytes / (med * 1e-3) / 1e12:.3f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s peak")
print(f"covered pixels: {covered};  numpy restatement, one 448 x 448 image on the CPU: {cpu_ms:.0f} ms")
print(json.dumps(res))
if args.json_path:
    with open(args.json_path, "w") as fh:
        json.dump(res, fh)

#!/usr/bin/env python3
"""Counterpart of the reference's ``src/train_baseline.py`` (main loop :60-108) on synthetic data:
``set_input -> forward -> optimize_parameters`` per batch, learning-rate update and checkpoint per epoch.  One process per GPU
(``python -m torch.distributed.run --nproc-per-node N -m ihmr_amd.run_train_baseline``); the encoder's flat gradient
(26 M floats) is averaged over the ranks in 25 MB buckets that are all-reduced while the backward pass is still running.

    python -m ihmr_amd.run_train_baseline --num_samples 256 --batchSize 64 --total_epoch 2

With any of the reference's augmentation flags (``bash/train_baseline.sh:35-41``: ``--use_random_flip --use_random_rescale
--use_random_position --use_random_rotation --use_color_jittering --use_motion_blur``) the loop keeps the raw uint8 crops and the
unaugmented labels on the device and augments every batch there each step (``ihmr_amd/augment.py``), as the reference's DataLoader
workers do per image on the CPU; motion blur draws from a small built-in bank of line kernels.  With none of them the loop is the
plain one: fixed images, no augmentation code runs.
"""
from __future__ import annotations

import argparse
import json
import time
import types

import numpy as np
import torch

from . import dist as D
from . import two_hand
from .baseline_model import InterHandModel
from .synthetic import synthetic_opt_batch


AUGMENT_FLAGS = ("use_random_flip", "use_random_rescale", "use_random_position", "use_random_rotation", "use_color_jittering",
                 "use_motion_blur")


def raw_batch(b, S):
    """A synthetic batch as a dataset would hold it before preprocessing: uint8 crops (packed as ``DataProcessor.pack`` lays them
    out) and 2-D joints in pixels, on the device."""
    B = b["img"].shape[0]
    u8 = ((b["img"].permute(0, 2, 3, 1) + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).contiguous()
    j2 = b["joints_2d"].clone()
    j2[:, :, :2] = (j2[:, :, :2] + 1.0) * (0.5 * S)
    raw = {k: v.cuda() for k, v in b.items() if k != "img"}
    raw.update(pixels=u8.reshape(-1).cuda(), offsets=(torch.arange(B, dtype=torch.int64) * (S * S * 3)).cuda(),
               sizes=torch.full((B, 2), S, dtype=torch.int32).cuda(), joints_2d=j2.cuda(), hand_types_host=b["hand_type_array"].numpy().copy())
    return raw


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_samples", type=int, default=128, help="samples per rank")
    ap.add_argument("--batchSize", type=int, default=64)
    ap.add_argument("--total_epoch", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--lr_decay_type", type=str, default="none", choices=["none", "cosine"])
    ap.add_argument("--use_collision_loss", action="store_true")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--save", action="store_true")
    for flag in AUGMENT_FLAGS:                                # options/train_options.py names
        ap.add_argument("--" + flag, action="store_true")
    ap.add_argument("--motion_blur_prob", type=float, default=0.5)
    ap.add_argument("--augment_seed", type=int, default=None, help="seed of the augmentation draws (default: --seed + rank)")
    args = ap.parse_args(argv)
    rank, world = D.init_dist()
    grouped = torch.distributed.is_available() and torch.distributed.is_initialized()   # (a one-rank group under torch.distributed.run too)
    if world == 1:
        torch.cuda.set_device(0)
    B = args.batchSize
    opt = types.SimpleNamespace(isTrain=True, dist=grouped, process_rank=rank if grouped else -1, batchSize=B, inputSize=224, input_nc=3,
                                num_joints=42, total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                trans_params_dim=3, model_root="", mean_param_file="mean_mano_params.pkl", checkpoints_dir="./checkpoints",
                                lr=args.lr, lr_decay_type=args.lr_decay_type, total_epoch=args.total_epoch,
                                use_collision_loss=args.use_collision_loss)
    torch.manual_seed(args.seed)                              # same initial weights on every rank (they are broadcast anyway)
    model = InterHandModel(opt)
    fwd = lambda p, s, t: two_hand.forward_from_packed(model.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    augmenter = None
    if any(getattr(args, f) for f in AUGMENT_FLAGS):
        from .augment import TrainDataProcessor, line_blur_kernels
        aopt = types.SimpleNamespace(inputSize=opt.inputSize, motion_blur_prob=args.motion_blur_prob, **{f: getattr(args, f) for f in AUGMENT_FLAGS})
        augmenter = TrainDataProcessor(aopt, line_blur_kernels() if args.use_motion_blur else None,
                                       seed=args.augment_seed if args.augment_seed is not None else args.seed + rank)
    data = []
    for i in range(max(1, args.num_samples // B)):
        b = synthetic_opt_batch(B, fwd, seed=args.seed + 1000 * rank + i, first_index=i * B, with_image=True)
        data.append(raw_batch(b, opt.inputSize) if augmenter else {k: v.cuda() for k, v in b.items()})
    log = []
    for epoch in range(1, args.total_epoch + 1):
        torch.cuda.synchronize()
        t0, first = time.time(), None
        for b in data:
            if augmenter:                                     # fresh draws for every batch and epoch, all work on the device
                aug = augmenter.apply_packed(b["pixels"], b["offsets"], b["sizes"], b, augmenter.draw(b["hand_types_host"]))
                b = {**b, **aug}
            model.set_input(b)
            model.forward_train()
            model.optimize_parameters()
            if first is None:
                first = model.get_current_errors()["total_loss"]
        last = model.get_current_errors()["total_loss"]
        torch.cuda.synchronize()
        dt = time.time() - t0
        model.update_learning_rate(epoch)
        if args.save and rank == 0:
            model.save("latest", epoch)
        log.append(dict(epoch=epoch, steps=len(data), ms_per_step=1e3 * dt / len(data), images_per_s=world * B * len(data) / dt,
                        loss_first=first, loss_last=last))
        if rank == 0:
            print(json.dumps(log[-1]))
    if torch.distributed.is_available() and torch.distributed.is_initialized():     # (also a one-rank group under torch.distributed.run)
        torch.distributed.destroy_process_group()
    return log


if __name__ == "__main__":
    main()

"""Seam A -- drop-in for ``smplx.create(model_path, 'mano', use_pca=..., num_pca_comps=..., flat_hand_mean=..., is_rhand=...,
batch_size=...)``.  The reference calls it with ``use_pca=False`` (``src/models/optimize_model.py:105-106``,
``baseline_model.py:141-142``, ``mlp_model.py:108-109``); loaders of other hand datasets call it with a PCA pose space, a flat hand
mean and a translation.

``MANO`` is an ``nn.Module`` exposing what the reference touches: ``.shapedirs`` (778,3,10) tensor that
callers mutate in place (``optimize_model.py:109-113``), ``.faces`` (np.ndarray (1538,3)), ``.J_regressor``
(16,778), ``.cuda()``, and ``__call__(global_orient=(N,3), hand_pose=(N,45), betas=(N,10))`` returning
an object with ``.vertices (N,778,3)`` and ``.joints (N,16,3)``, differentiable w.r.t. all three
inputs.  Forward and backward are the hand-written HIP kernels behind ``ihmr_mano_lbs_fwd`` /
``ihmr_mano_lbs_bwd``; there is no PyTorch/CPU implementation here.

Beyond that call (the published ``smplx`` MANO forward; parity unpinned): ``use_pca=True`` takes ``hand_pose``
``(N,K)`` coefficients of the first ``K = num_pca_comps`` rows of ``hands_components``; ``flat_hand_mean=True`` makes the hand mean
zero; an argument left as ``None`` is a zero tensor; ``transl (N,3)`` moves vertices and joints; ``return_tips=True`` appends the five
fingertip vertices to the joints (21 rows); ``return_full_pose=True`` also returns the (N,48) pose handed to Rodrigues.  These run the
kernels of ``include/ihmr_mano_ext.h`` before and after the unchanged skinning launches.  A call that uses none of them takes
today's path: the same launches, the same bits, the 5-field ``ManoOutput``.
"""
from __future__ import annotations

import os.path as osp
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import hip
from .assets import TIP_VERTEX_IDS, get_hand_components, get_mano_arrays

ManoOutput = namedtuple("ManoOutput", ["vertices", "joints", "betas", "global_orient", "hand_pose"])
# the result of a call with return_full_pose=True; ManoOutput keeps its five fields
ManoOutputFullPose = namedtuple("ManoOutputFullPose", ManoOutput._fields + ("full_pose",))


class _LbsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, orient, pose, betas, module):
        hip.require_gpu()
        orient, pose, betas = (t.contiguous().float() for t in (orient, pose, betas))
        N = orient.shape[0]
        dev = orient.device
        verts = torch.empty(N, 778, 3, device=dev)
        joints = torch.empty(N, 16, 3, device=dev)
        ws = torch.empty(hip.lib().ihmr_mano_workspace_bytes(N), dtype=torch.uint8, device=dev)
        hip.check(hip.lib().ihmr_mano_lbs_fwd(module._handle().handle, hip.ptr(orient), hip.ptr(pose), hip.ptr(betas), N,
                                              hip.ptr(verts), hip.ptr(joints), hip.ptr(ws), hip.stream_ptr()),
                  "ihmr_mano_lbs_fwd")
        ctx.save_for_backward(orient, pose, betas, ws)
        ctx.module = module
        return verts, joints

    @staticmethod
    def backward(ctx, d_verts, d_joints):
        orient, pose, betas, ws = ctx.saved_tensors
        N = orient.shape[0]
        dev = orient.device
        d_verts = torch.zeros(N, 778, 3, device=dev) if d_verts is None else d_verts.contiguous().float()
        d_joints = torch.zeros(N, 16, 3, device=dev) if d_joints is None else d_joints.contiguous().float()
        d_orient, d_pose, d_betas = torch.zeros_like(orient), torch.zeros_like(pose), torch.zeros_like(betas)
        mask = (1 if ctx.needs_input_grad[0] else 0) | (2 if ctx.needs_input_grad[1] else 0) | (4 if ctx.needs_input_grad[2] else 0)
        hip.check(hip.lib().ihmr_mano_lbs_bwd(ctx.module._handle().handle, N, hip.ptr(ws), hip.ptr(d_verts), hip.ptr(d_joints),
                                              hip.ptr(d_orient), hip.ptr(d_pose), hip.ptr(d_betas), mask, hip.stream_ptr()),
                  "ihmr_mano_lbs_bwd")
        return (d_orient if mask & 1 else None, d_pose if mask & 2 else None, d_betas if mask & 4 else None, None)


class _PcaFunction(torch.autograd.Function):
    """coefficients (N,K) -> pose45 (N,45) on the rows of ``comps`` (K,45): ``ihmr_mano_pca_fwd`` / ``ihmr_mano_pca_bwd``."""

    @staticmethod
    def forward(ctx, coeffs, comps):
        hip.require_gpu()
        c = coeffs.detach().contiguous().float()
        N, K = c.shape
        pose45 = torch.empty(N, hip.MANO_POSE_DIM, device=c.device)
        hip.check(hip.lib().ihmr_mano_pca_fwd(hip.ptr(c), hip.ptr(comps), N, K, hip.ptr(pose45), hip.stream_ptr()), "ihmr_mano_pca_fwd")
        ctx.save_for_backward(comps)
        ctx.K = K
        return pose45

    @staticmethod
    def backward(ctx, d_pose45):
        (comps,) = ctx.saved_tensors
        g = d_pose45.contiguous().float()
        d_coeffs = torch.empty(g.shape[0], ctx.K, device=g.device)
        hip.check(hip.lib().ihmr_mano_pca_bwd(hip.ptr(g), hip.ptr(comps), g.shape[0], ctx.K, hip.ptr(d_coeffs), hip.stream_ptr()),
                  "ihmr_mano_pca_bwd")
        return d_coeffs, None


class _PostFunction(torch.autograd.Function):
    """The output stage behind the skinning launch: translation and fingertips (``ihmr_mano_post_fwd`` / ``ihmr_mano_post_bwd``).
    ``transl`` (N,3) or None; ``tip_ids`` (5) int32 or None (16 joints)."""

    @staticmethod
    def forward(ctx, verts, joints, transl, tip_ids):
        v, j = verts.detach().contiguous().float(), joints.detach().contiguous().float()
        t = None if transl is None else transl.detach().contiguous().float()
        N = v.shape[0]
        verts_out = torch.empty_like(v)
        joints_out = torch.empty(N, 16 if tip_ids is None else 21, 3, device=v.device)
        hip.check(hip.lib().ihmr_mano_post_fwd(hip.ptr(v), hip.ptr(j), hip.ptr(t), hip.ptr(tip_ids), N, hip.ptr(verts_out),
                                               hip.ptr(joints_out), hip.stream_ptr()), "ihmr_mano_post_fwd")
        ctx.tip_ids = tip_ids
        return verts_out, joints_out

    @staticmethod
    def backward(ctx, d_verts_out, d_joints_out):
        gv, gj = d_verts_out.contiguous().float(), d_joints_out.contiguous().float()
        N = gv.shape[0]
        d_verts, d_joints = torch.empty_like(gv), torch.empty(N, 16, 3, device=gv.device)
        d_transl = torch.empty(N, 3, device=gv.device) if ctx.needs_input_grad[2] else None
        hip.check(hip.lib().ihmr_mano_post_bwd(hip.ptr(gv), hip.ptr(gj), hip.ptr(ctx.tip_ids), N, hip.ptr(d_verts), hip.ptr(d_joints),
                                               hip.ptr(d_transl), hip.stream_ptr()), "ihmr_mano_post_bwd")
        return d_verts, d_joints, d_transl, None


class MANO(nn.Module):
    def __init__(self, arrays: dict, is_rhand: bool = True, batch_size: int = 1, use_pca: bool = False, num_pca_comps: int = 6,
                 flat_hand_mean: bool = False, hand_components=None):
        super().__init__()
        self.is_rhand = is_rhand
        self.batch_size = batch_size
        self.use_pca, self.num_pca_comps, self.flat_hand_mean = bool(use_pca), int(num_pca_comps), bool(flat_hand_mean)
        self._arrays = {k: np.array(v, copy=True) for k, v in arrays.items()}
        if self.flat_hand_mean:                 # the device tables take pose_mean from here (build_mano_tables)
            self._arrays["hands_mean"] = np.zeros_like(self._arrays["hands_mean"])
        self.faces = self._arrays["faces"].astype(np.int64)
        self.register_buffer("shapedirs", torch.tensor(self._arrays["shapedirs"], dtype=torch.float32))
        self.register_buffer("J_regressor", torch.tensor(self._arrays["J_regressor"], dtype=torch.float32))
        self.register_buffer("v_template", torch.tensor(self._arrays["v_template"], dtype=torch.float32))
        self.register_buffer("hand_mean", torch.tensor(self._arrays["hands_mean"], dtype=torch.float32))
        comps = None                            # (K,45) with use_pca, else absent
        if self.use_pca:
            if not 1 <= self.num_pca_comps <= hip.MANO_POSE_DIM:
                raise ValueError(f"num_pca_comps must lie in 1..{hip.MANO_POSE_DIM}, got {num_pca_comps}")
            if hand_components is None:
                raise ValueError("use_pca=True needs hand_components (45,45)")
            comps = np.ascontiguousarray(np.asarray(hand_components, np.float32)[:self.num_pca_comps])
            if comps.shape != (self.num_pca_comps, hip.MANO_POSE_DIM):
                raise ValueError(f"hand_components must be (45,45), got {np.shape(hand_components)}")
            comps = torch.tensor(comps)
        # neither is in the state dict: a module saves and loads the keys it always has
        self.register_buffer("hand_components", comps, persistent=False)
        self.register_buffer("tip_ids", torch.tensor(TIP_VERTEX_IDS, dtype=torch.int32), persistent=False)
        self._dev_handle = None
        self._shapedirs_version = None

    def _handle(self) -> hip.ManoHandle:
        """Device constants; re-uploaded when a caller has mutated ``.shapedirs`` in place."""
        if self._dev_handle is None:
            arrays = dict(self._arrays)
            arrays["shapedirs"] = self.shapedirs.detach().cpu().numpy()
            self._dev_handle = hip.ManoHandle(arrays)
            self._shapedirs_version = self.shapedirs._version
        elif self.shapedirs._version != self._shapedirs_version:
            self._dev_handle.update_shapedirs(self.shapedirs.detach().cpu().numpy())
            self._shapedirs_version = self.shapedirs._version
        return self._dev_handle

    def forward(self, betas=None, global_orient=None, hand_pose=None, transl=None, return_verts=True, return_full_pose=False,
                return_tips=False, **kwargs):
        given = [t for t in (betas, global_orient, hand_pose, transl) if t is not None]
        plain = not self.use_pca and transl is None and not return_tips and not return_full_pose and return_verts
        if plain and len(given) == 3:           # the reference's call: today's path, no other launch
            verts, joints = _LbsFunction.apply(global_orient, hand_pose, betas, self)
            return ManoOutput(vertices=verts, joints=joints, betas=betas, global_orient=global_orient, hand_pose=hand_pose)
        N = given[0].shape[0] if given else self.batch_size
        dev = given[0].device if given else self.shapedirs.device
        zeros = lambda width: torch.zeros(N, width, device=dev)
        pose_width = self.num_pca_comps if self.use_pca else hip.MANO_POSE_DIM
        betas = zeros(10) if betas is None else betas
        global_orient = zeros(3) if global_orient is None else global_orient
        hand_pose = zeros(pose_width) if hand_pose is None else hand_pose
        if hand_pose.dim() != 2 or hand_pose.shape[1] != pose_width:
            raise ValueError(f"hand_pose must be (N,{pose_width}) with use_pca={self.use_pca}, got {tuple(hand_pose.shape)}")
        pose45 = _PcaFunction.apply(hand_pose, self.hand_components.to(dev)) if self.use_pca else hand_pose
        verts, joints = _LbsFunction.apply(global_orient, pose45, betas, self)
        if transl is not None or return_tips:
            verts, joints = _PostFunction.apply(verts, joints, transl, self.tip_ids.to(dev) if return_tips else None)
        out = dict(vertices=verts if return_verts else None, joints=joints, betas=betas, global_orient=global_orient, hand_pose=hand_pose)
        if not return_full_pose:
            return ManoOutput(**out)
        # one float32 addition per element, as the skinning launch forms it
        full_pose = torch.cat([global_orient.float(), pose45.float()], dim=1) + torch.cat([self.hand_mean.new_zeros(3), self.hand_mean]).to(dev)
        return ManoOutputFullPose(full_pose=full_pose, **out)


def create(model_path, model_type="mano", use_pca=False, num_pca_comps=6, flat_hand_mean=False, is_rhand=True, batch_size=1, **kwargs):
    """Same call shape as ``smplx.create``; reads a real MANO pkl when ``model_path`` exists, otherwise
    the deterministic synthetic asset (``ihmr_amd.assets``)."""
    if model_type != "mano":
        raise ValueError("only model_type='mano' is built")
    if use_pca and not (isinstance(num_pca_comps, (int, np.integer)) and 1 <= num_pca_comps <= hip.MANO_POSE_DIM):
        raise ValueError(f"num_pca_comps must be an integer in 1..{hip.MANO_POSE_DIM}, got {num_pca_comps!r}")
    comps = get_hand_components(model_path, is_rhand) if use_pca else None
    return MANO(get_mano_arrays(model_path, is_rhand), is_rhand=is_rhand, batch_size=batch_size, use_pca=use_pca,
                num_pca_comps=num_pca_comps, flat_hand_mean=flat_hand_mean, hand_components=comps)


def create_pair(model_root, batch_size, device):
    """``{"left", "right"}`` models from ``MANO_{LEFT,RIGHT}.pkl`` under ``model_root``, as every model of the reference loads them
    (optimize_model.py:97-117, baseline_model.py:133-153): a left hand whose first shape direction carries the right hand's x-sign
    (the published files) is flipped."""
    models = {hand_type: create(osp.join(model_root or "", f"MANO_{hand_type.upper()}.pkl"), "mano", use_pca=False,
                                is_rhand=(hand_type == "right"), batch_size=batch_size) for hand_type in ("left", "right")}
    if torch.mean(torch.abs(models["left"].shapedirs[:, 0, :] - models["right"].shapedirs[:, 0, :])) < 1e-7:
        models["left"].shapedirs[:, 0, :] *= -1
    return {k: m.to(device) for k, m in models.items()}

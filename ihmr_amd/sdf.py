"""Seam B -- drop-in for ``from sdf import SDFLoss`` (reference ``src/models/loss_utils.py:13``):
``SDFLoss(faces_right, faces_left, robustifier=None)`` -> ``nn.Module`` with ``.cuda()`` and
``__call__(hand_verts (B,2,778,3), return_per_vert_loss=True, return_origin_scale_loss=True)`` ->
``(losses (B,), per_vert (B,1556), losses_origin_scale (B,1556))`` (the reference reshapes the first to
(B,1), ``loss_utils.py:181-183``), differentiable w.r.t. ``hand_verts``.

All arithmetic is in the HIP kernels behind ``ihmr_sdf_collision`` (sparse voxel SDF + trilinear
sampling, semantics in DESIGN.md "SDF arithmetic spec"); the bounding boxes are detached, so the
gradient reaches only the sampled (other-hand) vertices, as in the upstream module.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import hip


def refuse_training_robustifier(opt):
    """The reference builds its train-mode collision module with ``robustifier = opt.sdf_robustifier`` (``loss_utils.py:36``); the fused
    training launches here (``ihmr_mlp_train_grad``) evaluate the collision term with the robustifier off.  Its default is ``None``; a
    training run that sets it would silently optimise another objective, so it is refused."""
    if getattr(opt, "isTrain", False) and getattr(opt, "sdf_robustifier", None) is not None:
        raise ValueError("sdf_robustifier = %r: the training steps evaluate the collision term without a robustifier (isTrain = True); "
                         "leave it at None" % (opt.sdf_robustifier,))


class _SdfFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hand_verts, module):
        hip.require_gpu()
        hv = hand_verts.contiguous().float()
        B = hv.shape[0]
        dev = hv.device
        loss = torch.empty(B, device=dev)
        per_vert = torch.empty(B, 1556, device=dev)
        origin = torch.empty(B, 1556, device=dev)
        dval = torch.empty(B, 1556, 3, device=dev)
        ws = module._workspace(B, dev)
        import ctypes as C
        options = hip.SdfOptions(int(bool(module.align_corners)), float(module.loss_divisor), int(bool(module.swap_xz)))
        hip.check(hip.lib().ihmr_sdf_collision_ex(hip.ptr(module.faces_right), hip.ptr(module.faces_left), hip.ptr(hv), B,
                                                  float(module.robustifier or 0.0), C.byref(options), hip.ptr(loss), hip.ptr(per_vert),
                                                  hip.ptr(origin), hip.ptr(dval), hip.ptr(ws), hip.stream_ptr()),
                  "ihmr_sdf_collision_ex")
        ctx.loss_divisor = float(module.loss_divisor)
        # box scale per entry (origin = per_vert * scale): recover it for the backward of `origin`
        ctx.save_for_backward(dval, per_vert, origin)
        return loss, per_vert, origin

    @staticmethod
    def backward(ctx, g_loss, g_per_vert, g_origin):
        dval, per_vert, origin = ctx.saved_tensors
        B = dval.shape[0]
        coef = torch.zeros(B, 1556, device=dval.device)
        if g_loss is not None:
            coef = coef + g_loss.reshape(B, 1) / ctx.loss_divisor
        if g_per_vert is not None:
            coef = coef + g_per_vert
        if g_origin is not None:
            scale = torch.where(per_vert != 0, origin / torch.where(per_vert != 0, per_vert, torch.ones_like(per_vert)),
                                torch.zeros_like(per_vert))
            coef = coef + g_origin * scale
        g = (coef[..., None] * dval).view(B, 2, 778, 3)
        # entry (h, v) is sampled at vertex v of hand 1-h
        return torch.flip(g, dims=[1]).contiguous(), None


class SDFLoss(nn.Module):
    def __init__(self, faces_right, faces_left, robustifier=None, grid_size=32, align_corners=False, loss_divisor=4.0, swap_xz=False):
        """``align_corners`` / ``loss_divisor`` / ``swap_xz`` (axis order of the grid as ``grid_sample`` sees it): the three conventions of the (absent, unpinned) upstream module that a maintainer
        holding the real package can switch to pin this seam (``include/ihmr_hip.h: ihmr_sdf_options``)."""
        super().__init__()
        assert grid_size == 32, "the kernels are built for the 32^3 grid of the upstream module"
        # one value for the options struct AND the autograd backward (the C side reads <= 0 as "default"; the backward divides by it)
        loss_divisor = float(loss_divisor)
        if not loss_divisor > 0.0:
            raise ValueError(f"SDFLoss(loss_divisor={loss_divisor}): must be > 0 (4 = num_hands^2 of the parent project, 1 = plain sum)")
        self.align_corners, self.loss_divisor, self.swap_xz = bool(align_corners), loss_divisor, bool(swap_xz)
        self.register_buffer("faces_right", torch.tensor(np.asarray(faces_right).astype(np.int32)))
        self.register_buffer("faces_left", torch.tensor(np.asarray(faces_left).astype(np.int32)))
        self.robustifier = robustifier
        self._ws = None

    def _workspace(self, B, dev):
        need = hip.lib().ihmr_sdf_workspace_bytes(B)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    def forward(self, hand_verts, scale_factor=0.2, return_per_vert_loss=False, return_origin_scale_loss=False):
        assert abs(scale_factor - 0.2) < 1e-12, "box margin is fixed at the upstream default 0.2"
        if self.faces_right.device != hand_verts.device:
            self.to(hand_verts.device)
        loss, per_vert, origin = _SdfFunction.apply(hand_verts, self)
        if return_per_vert_loss and return_origin_scale_loss:
            return loss, per_vert, origin
        if return_per_vert_loss:
            return loss, per_vert
        if return_origin_scale_loss:
            return loss, origin
        return loss


# ------------------------------------------------------------------------------------------ two-hand intersection volume
VOLUME_SUBDIVS = (1, 2, 4)


def close_boundary(faces, n_verts):
    """``faces`` (F,3) with every boundary loop closed by a triangle fan from the loop's lowest-numbered vertex.  No vertex is added; a
    closed mesh comes back unchanged (a copy).  MANO is open at the wrist, one loop of 16 edges: 1538 -> 1552 faces.  A boundary edge is
    a directed edge (a, b) of a face whose opposite (b, a) belongs to no face; a loop v0 -> v1 -> ... -> v_{m-1} -> v0 (v0 the lowest)
    gets the faces (v0, v_{i+1}, v_i), i = 1 .. m-2, which run against it.  Pure integer host logic: the +x ray parity of
    :func:`penetration_volume` is only right for closed meshes."""
    f = np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0 or f.min() < 0 or f.max() >= n_verts:
        raise ValueError(f"faces: a (F,3) table of vertex ids in [0, {n_verts}) is needed")
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64).tolist()
    have = {(a, b) for a, b in e}
    nxt = {}
    for a, b in e:
        if (b, a) not in have:
            if a in nxt:
                raise ValueError(f"vertex {a} starts two boundary edges: the boundary is no set of simple loops")
            nxt[a] = b
    added, left = [], set(nxt)
    while left:
        v0 = min(left)
        loop, v = [v0], nxt[v0]
        while v != v0:
            if v not in nxt or len(loop) > len(nxt):
                raise ValueError("an open boundary chain: the boundary is no set of simple loops")
            loop.append(v)
            v = nxt[v]
        left -= set(loop)
        added += [(v0, loop[i + 1], loop[i]) for i in range(1, len(loop) - 1)]
    if not added:
        return f.copy()
    return np.concatenate([f, np.asarray(added, f.dtype)])


_VOLUME_FACES = {}      # (device, bytes of the table, n_verts, closed) -> int32 device tensor


def _volume_faces(faces, n_verts, close, dev):
    """The (closed) face table on ``dev``, uploaded once per table and device."""
    if torch.is_tensor(faces):
        faces = faces.detach().cpu().numpy()
    f = np.ascontiguousarray(np.asarray(faces).astype(np.int32))
    key = (str(dev), f.tobytes(), int(n_verts), bool(close))
    if key not in _VOLUME_FACES:
        table = close_boundary(f, n_verts) if close else f
        if table.ndim != 2 or table.shape[1] != 3 or not 1 <= len(table) <= hip.VOLUME_MAX_FACES:
            raise ValueError(f"a face table of 1..{hip.VOLUME_MAX_FACES} triangles is needed, got shape {table.shape}")
        _VOLUME_FACES[key] = torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev)
    return _VOLUME_FACES[key]


def penetration_volume(verts_right, verts_left, faces_right, faces_left, subdiv=2, keep=None, close=True, return_bits=False):
    """How much of one hand lies inside the other: the voxels of one common (32 * subdiv)^3 grid that are inside both meshes
    (``ihmr_sdf_volume``; the definition is DESIGN.md section 8 and ``csrc/volume_pure.h``).  ``verts_*`` (B,n_verts,3) float32 device
    tensors in metres, ``faces_*`` (F,3) integer tables (closed with :func:`close_boundary` unless ``close=False``; cached per device),
    ``subdiv`` 1, 2 or 4, ``keep`` (B) bool: a sample left out costs no ray work and returns zeros.

    Returns ``(volume, counts, box, status)``, with ``return_bits`` also ``bits``: ``volume`` (B,) float64 in m^3 =
    ``count * (2 * (s / subdiv) / 32)^3`` formed in float64 from the float32 ``s``; ``counts`` (B,subdiv^3) int64 voxels per tile;
    ``box`` (B,4) float32 centre and half side of the common cube; ``status`` (B,) int32, 0 counted | 1 empty (the vertex boxes do not
    overlap) | 2 invalid (a non-finite vertex, or a cube of half side < 1e-5); ``bits`` (B,subdiv^3,1024) int32 words of the voxels
    inside both.  Everything stays on the device; nothing synchronises."""
    hip.require_gpu()
    if subdiv not in VOLUME_SUBDIVS:
        raise ValueError(f"subdiv = {subdiv!r}: 1, 2 or 4")
    dev = verts_right.device
    va, vb = verts_right.detach().to(dev, torch.float32).contiguous(), verts_left.detach().to(dev, torch.float32).contiguous()
    if va.dim() != 3 or vb.dim() != 3 or va.shape[2] != 3 or vb.shape[2] != 3 or va.shape[0] != vb.shape[0] or va.shape[0] < 1:
        raise ValueError(f"two (B,n_verts,3) vertex tensors of one batch size are needed, got {tuple(va.shape)} and {tuple(vb.shape)}")
    B, na, nb = va.shape[0], va.shape[1], vb.shape[1]
    if not (1 <= na <= hip.VOLUME_MAX_VERTS and 1 <= nb <= hip.VOLUME_MAX_VERTS):
        raise ValueError(f"1..{hip.VOLUME_MAX_VERTS} vertices per mesh, got {na} and {nb}")
    fa, fb = _volume_faces(faces_right, na, close, dev), _volume_faces(faces_left, nb, close, dev)
    k = None if keep is None else keep.to(dev, torch.uint8).contiguous()
    T = subdiv ** 3
    box = torch.empty(B, 4, device=dev, dtype=torch.float32)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    counts = torch.empty(B, T, device=dev, dtype=torch.int32)           # (the words are unsigned; a tile holds at most 32768 voxels)
    bits = torch.empty(B, T, 1024, device=dev, dtype=torch.int32) if return_bits else None
    hip.check(hip.lib().ihmr_sdf_volume(va.data_ptr(), fa.data_ptr(), na, len(fa), vb.data_ptr(), fb.data_ptr(), nb, len(fb), B, subdiv,
                                        None if k is None else k.data_ptr(), box.data_ptr(), status.data_ptr(), counts.data_ptr(),
                                        None if bits is None else bits.data_ptr(), hip.stream_ptr()), "ihmr_sdf_volume")
    counts = counts.to(torch.int64)
    cell = 2.0 * (box[:, 3].to(torch.float64) / float(subdiv)) / 32.0        # s / subdiv is exact in either precision: a power of two
    volume = counts.sum(dim=1).to(torch.float64) * (cell * cell * cell)
    return (volume, counts, box, status, bits) if return_bits else (volume, counts, box, status)


# ------------------------------------------------------------------------------------------ exact point-to-surface signed distance
_SURFACE_FACES = {}     # (device, bytes of the table, n_verts, closed) -> (int32 device tensor, F_dist)


def _surface_faces(faces, n_verts, close, dev):
    """``(table, F_dist)``: the face table on ``dev`` -- with ``close`` the fan triangles of :func:`close_boundary` appended, ``F_dist``
    the original face count -- uploaded once per table and device."""
    if torch.is_tensor(faces):
        faces = faces.detach().cpu().numpy()
    f = np.ascontiguousarray(np.asarray(faces).astype(np.int32))
    key = (str(dev), f.tobytes(), int(n_verts), bool(close))
    if key not in _SURFACE_FACES:
        table = close_boundary(f, n_verts) if close else f
        if table.ndim != 2 or table.shape[1] != 3 or not 1 <= len(f) <= len(table) <= hip.SURFACE_MAX_FACES:
            raise ValueError(f"a face table of 1..{hip.SURFACE_MAX_FACES} triangles is needed, got shape {table.shape}")
        _SURFACE_FACES[key] = (torch.from_numpy(np.ascontiguousarray(table, np.int32)).to(dev), len(f))
    return _SURFACE_FACES[key]


class _SurfaceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, verts, table, F_dist, signed, use):
        q, v = points.detach().to(torch.float32).contiguous(), verts.detach().to(points.device, torch.float32).contiguous()
        B, P, V, dev = q.shape[0], q.shape[1], v.shape[1], q.device
        dist = torch.empty(B, P, device=dev, dtype=torch.float64)
        face = torch.empty(B, P, device=dev, dtype=torch.int32)
        bary = torch.empty(B, P, 3, device=dev, dtype=torch.float64)
        hip.check(hip.lib().ihmr_surface_distance(q.data_ptr(), P, v.data_ptr(), V, table.data_ptr(), F_dist, len(table),
                                                  None if use is None else use.data_ptr(), B, int(bool(signed)), dist.data_ptr(),
                                                  face.data_ptr(), bary.data_ptr(), hip.stream_ptr()), "ihmr_surface_distance")
        ctx.save_for_backward(q, v, table, dist, face, bary, *(() if use is None else (use,)))
        ctx.F_dist, ctx.dtypes = F_dist, (points.dtype, verts.dtype)
        ctx.mark_non_differentiable(face, bary)
        return dist, face, bary

    @staticmethod
    def backward(ctx, g_dist, _g_face, _g_bary):
        q, v, table, dist, face, bary, *rest = ctx.saved_tensors
        use = rest[0] if rest else None
        B, P, V = q.shape[0], q.shape[1], v.shape[1]
        g = g_dist.to(torch.float64).contiguous()
        d_points = torch.empty_like(q) if ctx.needs_input_grad[0] else None
        d_verts = torch.empty_like(v) if ctx.needs_input_grad[1] else None
        hip.check(hip.lib().ihmr_surface_distance_bwd(q.data_ptr(), P, v.data_ptr(), V, table.data_ptr(), ctx.F_dist, len(table),
                                                      None if use is None else use.data_ptr(), B, dist.data_ptr(), face.data_ptr(),
                                                      bary.data_ptr(), g.data_ptr(), None if d_points is None else d_points.data_ptr(),
                                                      None if d_verts is None else d_verts.data_ptr(), hip.stream_ptr()),
                  "ihmr_surface_distance_bwd")
        return (None if d_points is None else d_points.to(ctx.dtypes[0]), None if d_verts is None else d_verts.to(ctx.dtypes[1]),
                None, None, None, None)


def surface_distance(points, verts, faces, signed=True, close=True, use=None):
    """The exact distance from every query point to a triangle mesh (``ihmr_surface_distance``; the definition is DESIGN.md section 8,
    row (f)8 and ``csrc/surface_pure.h``): ``points`` (B,P,3) and ``verts`` (B,V,3) float32 device tensors, ``faces`` (F,3) an integer
    table shared by the batch.  ``close=True`` appends the fan triangles of :func:`close_boundary` (MANO's wrist: 1538 + 14): the
    distance is taken to the original faces only -- the cap is not skin -- and the sign over all of them; tables are cached per device.
    ``signed=False`` skips the ray work.  ``use`` (B) bool: a sample left out costs nothing and returns zeros (``face`` -1).

    Returns ``(dist, face, bary)``: ``dist`` (B,P) float64 in the inputs' units, negative inside; ``face`` (B,P) int32 the closest face,
    ``bary`` (B,P,3) float64 the weights of the closest point on its vertices.  A query with a non-finite coordinate has ``dist`` NaN,
    ``face`` -1.  ``dist`` is differentiable with respect to ``points`` and ``verts`` (``ihmr_surface_distance_bwd``: the same bits on
    every run), so an attraction or contact term reaches vertices the grid loss of :class:`SDFLoss` cannot: its gradient stops at the
    other hand's box.  Everything stays on the device; nothing synchronises.

    The exact penetration depth as a heat map (``Evaluator.visualize_result`` paints the grid proxy)::

        d_right, _, _ = surface_distance(right, left, left_faces)               # the right hand's vertices against the left hand
        d_left, _, _ = surface_distance(left, right, right_faces)
        depth = torch.clamp(-torch.cat([d_right, d_left], dim=1), min=0)        # (B,1556) metres under the other hand's skin
        colours = render.penetration_colors(depth, layout="vertex")             # entry k belongs to vertex k of the merged mesh
    """
    hip.require_gpu()
    if points.dim() != 3 or verts.dim() != 3 or points.shape[2] != 3 or verts.shape[2] != 3 or points.shape[0] != verts.shape[0] or points.shape[0] < 1:
        raise ValueError(f"(B,P,3) points and (B,V,3) vertices of one batch size are needed, got {tuple(points.shape)} and {tuple(verts.shape)}")
    if points.shape[1] < 1 or not 1 <= verts.shape[1] <= hip.SURFACE_MAX_VERTS:
        raise ValueError(f"at least one query and 1..{hip.SURFACE_MAX_VERTS} vertices are needed, got {points.shape[1]} and {verts.shape[1]}")
    dev = points.device
    table, F_dist = _surface_faces(faces, verts.shape[1], close, dev)
    u = None if use is None else use.to(dev, torch.uint8).contiguous()
    return _SurfaceFunction.apply(points, verts, table, F_dist, signed, u)


class SDFLoss_Single(nn.Module):  # imported but never used by the reference (loss_utils.py:13)
    def __init__(self, *a, **k):
        super().__init__()
        raise NotImplementedError("SDFLoss_Single is not on the IHMR hot path")

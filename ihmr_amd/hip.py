"""ctypes binding of ``libihmr_hip.so`` (C ABI declared in ``include/ihmr_hip.h``).

The library is the product: every compute entry point of this package goes through it and there is
NO CPU fallback -- if the shared object is missing (and cannot be built with hipcc) or no GPU is
visible, the calls raise.  PyTorch is used only for device memory and streams: tensors are passed as
raw device pointers, the launch stream is ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes as C
import os
import os.path as osp
import subprocess

import numpy as np
import torch

_HERE = osp.dirname(osp.abspath(__file__))
LIB_PATH = osp.join(_HERE, "libihmr_hip.so")
SRC_DIR = osp.join(_HERE, "csrc")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC"]

NUM_VERTS, NUM_FACES, NUM_JOINTS, OPT_NPARAM = 778, 1538, 16, 122
EVAL_MAX_THRESHOLDS, EVAL_MAX_F_THRESHOLDS = 256, 8      # include/ihmr_hip.h: IHMR_EVAL_MAX_THRESHOLDS, IHMR_EVAL_MAX_F_THRESHOLDS
EVAL_MAX_CONTACT_THRESHOLDS = 8                          # include/ihmr_hip.h: IHMR_EVAL_MAX_CONTACT_THRESHOLDS
VOLUME_MAX_VERTS, VOLUME_MAX_FACES = 1024, 2048          # include/ihmr_hip.h: IHMR_VOLUME_MAX_VERTS, IHMR_VOLUME_MAX_FACES
SURFACE_MAX_VERTS, SURFACE_MAX_FACES = 1024, 2048        # include/ihmr_hip.h: IHMR_SURFACE_MAX_VERTS, IHMR_SURFACE_MAX_FACES
# include/ihmr_hip.h: parameter blocks (slot order of the 122-vector), filter / select losses, optimizers
PARAM_BLOCKS = dict(pred_cam_params=(1, 0, 3), pred_hand_trans=(2, 3, 3), pred_right_orient=(4, 6, 3), pred_left_orient=(8, 9, 3),
                    pred_right_pose_params=(16, 12, 45), pred_left_pose_params=(32, 57, 45),
                    pred_right_shape_params=(64, 102, 10), pred_left_shape_params=(128, 112, 10))   # name -> (bit, first slot, size)
LOSS_IDS = dict(joints_2d_loss_p=0, joints_3d_loss_p=1, collision_loss=2)
OPTIMIZERS = dict(adam=0, sgd=1)

class ManoArrays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents",
                                          "hands_mean", "faces", "tip_ids")]


class OptIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "cam", "trans", "orient", "pose", "shape",
        "init_joints_2d", "init_joints_3d", "init_hand_trans_j", "gt_joints_2d", "gt_joints_3d", "gt_hand_trans",
        "hand_type_array",
        "verts", "joints_3d", "joints_2d", "loss_batch", "coll_per_vert", "coll_origin_scale",
        "snap_params", "snap_loss", "selected", "adam_m", "adam_v", "workspace")] + [
        ("norm_batch", C.c_int), ("sdf_align_corners", C.c_int), ("sdf_loss_divisor", C.c_float), ("sdf_swap_xz", C.c_int),
        ("sdf_no_candidate_lists", C.c_int), ("sdf_no_static_reuse", C.c_int),
        ("no_fused_tail", C.c_int)]


class CopySeg(C.Structure):
    """``ihmr_copy_seg``: one 2-D strided copy of 32-bit words (rows, width, leading dimensions in dwords)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int), ("width", C.c_int), ("src_ld", C.c_int), ("dst_ld", C.c_int)]


COPY_MAX_SEGS = 32


def copy_segments(pairs):
    """``pairs``: (src, dst) device tensors of equal shape and 4- or 8-byte element type -- dst may be a strided 2-D view (a column
    slice of a packed matrix), src too; everything else contiguous.  One launch (``ihmr_copy_segments``) per 32 pairs."""
    segs = []
    for src, dst in pairs:
        assert src.shape == dst.shape and src.dtype == dst.dtype and src.is_cuda and dst.is_cuda, (src.shape, dst.shape, src.dtype, dst.dtype)
        k = src.element_size() // 4
        assert k in (1, 2)

        def geom(t):
            if t.is_contiguous():
                return 1, t.numel() * k, t.numel() * k
            assert t.dim() == 2 and t.stride(1) == 1, "a strided operand must be a column slice of a row-major matrix"
            return t.shape[0], t.shape[1] * k, t.stride(0) * k
        (rs, ws, ls), (rd, wd, ld) = geom(src), geom(dst)
        if (rs, ws) != (rd, wd):                 # one side flat, the other a 2-D slice: describe both as the slice's rows
            rows, width = (rd, wd) if rd > 1 else (rs, ws)
            ls = ls if rs > 1 else width
            ld = ld if rd > 1 else width
        else:
            rows, width = rs, ws
        segs.append(CopySeg(src.data_ptr(), dst.data_ptr(), rows, width, ls, ld))
    L, st = lib(), stream_ptr()
    for i in range(0, len(segs), COPY_MAX_SEGS):
        chunk = segs[i:i + COPY_MAX_SEGS]
        arr = (CopySeg * len(chunk))(*chunk)
        check(L.ihmr_copy_segments(arr, len(chunk), st), "ihmr_copy_segments")


class SdfOptions(C.Structure):
    _fields_ = [("align_corners", C.c_int), ("loss_divisor", C.c_float), ("swap_xz", C.c_int)]


class OptStage(C.Structure):
    _fields_ = [("param_mask", C.c_int), ("optimizer", C.c_int), ("lr", C.c_float), ("n_iters", C.c_int), ("save_freq", C.c_int),
                ("use_filter", C.c_int * 3), ("filter_factor", C.c_float * 3), ("select_loss", C.c_int), ("keep_lists", C.c_int)]


class OptWeights(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("joints_2d", "joints_3d", "trans", "shape_reg", "collision", "finger_reg")]


class MlpNet(C.Structure):
    """``ihmr_mlp_net``: one IHMR-MLP sub-network -- packed weights / biases of its four Linear layers, output -> column map."""
    _fields_ = [("w", C.c_void_p * 4), ("b", C.c_void_p * 4), ("ldw", C.c_int * 4), ("k_out", C.c_int), ("col", C.c_int * 122)]


class MlpTables(C.Structure):
    """``ihmr_mlp_tables``: the "prev" tables of MLPModel (mlp_model.py:297-356) + the batch's working rows."""
    _fields_ = [(n, C.c_void_p) for n in ("idx", "data_idxs_all", "img_feat_all", "prev_final", "prev_loss", "img_feat", "new_params",
                                          "final_params", "kept")]


class MlpStage(C.Structure):
    """``ihmr_mlp_stage``: filter / select criteria of one stage (select_better_params, mlp_model.py:592-637)."""
    _fields_ = [("n_filter", C.c_int), ("filter_loss", C.c_int * 4), ("filter_factor", C.c_float * 4), ("select_loss", C.c_int)]


class TrainWeights(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("joints_2d", "mano_pose", "mano_shape", "hand_trans", "shape_reg", "shape_residual")]


class RenderLights(C.Structure):
    """``ihmr_render_lights``: the three rotated light positions and their colours (float32)."""
    _fields_ = [("pos", C.c_float * 3 * 3), ("color", C.c_float * 3 * 3)]


TIMED_SDF_PREP, TIMED_SDF_DIST, TIMED_OPT_TAIL, TIMED_KERNELS = 0, 1, 2, 4


class KernelTimer(C.Structure):
    """``ihmr_kernel_timer`` (include/ihmr_hip.h): summed HIP-event time and launch count per timed kernel + the empty event pairs."""
    _fields_ = [("ms", C.c_double * TIMED_KERNELS), ("n", C.c_long * TIMED_KERNELS), ("ms_event_pair", C.c_double), ("n_event_pair", C.c_long)]

    def launch_ms(self, k):
        """Mean duration of kernel slot k's launches (event time minus the cost of an empty event pair)."""
        if self.n[k] <= 0:
            return None
        return self.ms[k] / self.n[k] - (self.ms_event_pair / self.n_event_pair if self.n_event_pair > 0 else 0.0)


_vp, _i, _f, _z, _P = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.POINTER
_conv = [_vp] * 5 + [_i] * 16 + [_vp, _z, _vp]
_raster = [_vp] * 4 + [_i] * 3 + [_vp] * 3 + [_P(RenderLights), _vp, _i, _vp, _vp, _vp, _i, _vp]
# THE binding: name -> (restype, argtypes) of every function include/ihmr_hip.h declares, in the header's own terms (a handle, a
# stream and a device pointer are c_void_p; a struct travels as a pointer to its ctypes mirror above).  lib() applies it;
# tests/test_abi_cpu.py compares it with the header's prototypes argument by argument and the mirrors with the compiler's layout.
SIGNATURES = {
    "ihmr_mano_create": (_i, [_P(ManoArrays), _P(_vp)]),
    "ihmr_mano_destroy": (_i, [_vp]),
    "ihmr_mano_update_shapedirs": (_i, [_vp, _vp]),
    "ihmr_mano_workspace_bytes": (_z, [_i]),
    "ihmr_mano_lbs_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "ihmr_mano_lbs_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "ihmr_sdf_workspace_bytes": (_z, [_i]),
    "ihmr_sdf_collision": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ihmr_sdf_collision_ex": (_i, [_vp, _vp, _vp, _i, _f, _P(SdfOptions), _vp, _vp, _vp, _vp, _vp, _vp]),
    "ihmr_sdf_dense_grid": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ihmr_opt_workspace_bytes": (_z, [_i]),
    "ihmr_opt_run_stage": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _P(OptStage), _vp]),
    "ihmr_opt_forward_losses": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _vp]),
    "ihmr_opt_sdf_stats": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _vp, _vp]),
    "ihmr_opt_sdf_counters": (_i, [_P(OptIO), _i, _vp, _i]),
    "ihmr_opt_sdf_inside_bits": (_i, [_P(OptIO), _i, _vp, _vp]),
    "ihmr_opt_stage_graph_create": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _P(OptStage), _P(_vp)]),
    "ihmr_opt_forward_graph_create": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _P(_vp)]),
    "ihmr_graph_launch": (_i, [_vp, _vp]),
    "ihmr_graph_destroy": (_i, [_vp]),
    "ihmr_opt_set_params": (_i, [_P(OptIO), _vp, _i, _vp]),
    "ihmr_eval_metrics": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ihmr_eval_mpvpe": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ihmr_eval_pa_joints": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ihmr_eval_pa_verts": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ihmr_eval_curve_joints": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "ihmr_eval_curve_verts": (_i, [_vp] * 7 + [_i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "ihmr_eval_mrrpe": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "ihmr_eval_contact": (_i, [_vp] * 7 + [_i, _vp, _i, _vp, _vp, _vp, _vp]),
    "ihmr_sdf_volume": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ihmr_surface_distance": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "ihmr_surface_distance_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ihmr_conv_igemm": (_i, _conv),
    "ihmr_maxpool3x3s2": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "ihmr_avgpool_relu": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_preprocess_images": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "ihmr_mlp_train_grad": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _P(TrainWeights)] + [_vp] * 8 + [_i, _vp, _i, _vp]),
    "ihmr_transpose": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_relu_backward": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_colsum": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ihmr_adam_step": (_i, [_vp, _vp, _vp, _vp, _z, _f, _f, _f, _f, _f, _i, _vp]),
    "ihmr_bn_workspace_bytes": (_z, [_i]),
    "ihmr_bn_train_forward": (_i, [_vp, C.c_long, _i, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp]),
    "ihmr_bn_train_backward": (_i, [_vp, _vp, C.c_long, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ihmr_conv_wgrad": (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp, _z, _vp]),
    "ihmr_dilate2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_interleave2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_pack_dgrad_weight": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "ihmr_maxpool3x3s2_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "ihmr_avgpool_relu_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_set_kernel_timer": (_i, [_P(KernelTimer)]),
    "ihmr_flush_kernel_timer": (_i, []),
    "ihmr_mlp_workspace_bytes": (_z, [_i]),
    "ihmr_mlp_stage_head": (_i, [_P(MlpNet), _P(MlpTables), _P(OptIO), _i, _vp, _vp]),
    "ihmr_mlp_forward_select": (_i, [_vp, _vp, _P(OptIO), _i, _P(OptWeights), _P(MlpTables), _P(MlpStage), _i, _vp, _vp]),
    "ihmr_mlp_camera_select": (_i, [_P(OptIO), _i, _P(OptWeights), _P(MlpTables), _P(MlpStage), _vp, _vp]),
    "ihmr_opt_forward_verts": (_i, [_vp, _P(OptIO), _i, _vp]),
    "ihmr_debug_force_lbs_bwd2_streaming": (_i, [_i]),
    "ihmr_debug_force_full_skin": (_i, [_i]),
    "ihmr_debug_force_generic_tail": (_i, [_i]),
    "ihmr_debug_prep_global_faces": (_i, [_i]),
    "ihmr_version": (C.c_char_p, []),
    "ihmr_copy_segments": (_i, [_P(CopySeg), _i, _vp]),
    "ihmr_root_align_joints": (_i, [_vp, _vp, _i, _vp]),
    "ihmr_augment_images": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _P(_i), _vp]),
    "ihmr_augment_labels": (_i, [_vp, _vp, _i, _i] + [_vp] * 15),
    "ihmr_render_workspace_bytes": (_z, [_i, _i]),
    "ihmr_render_meshes": (_i, _raster),
    "ihmr_draw_keypoints": (_i, [_vp, _vp, _vp, C.c_char_p, _i, _i, _i, _vp]),
    "ihmr_view_vertices": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp]),
    "ihmr_heat_colours": (_i, [_vp, _vp, _P(_f * 3), _f, _f, _i, _i, _i, _vp, _i, _vp]),
    "ihmr_paint_meshes": (_i, _raster),
    "ihmr_conv_igemm_bf16": (_i, _conv),
    "ihmr_pack_image_bf16": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ihmr_maxpool3x3s2_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "ihmr_avgpool_relu_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ihmr_cast_f32_bf16": (_i, [_vp, _vp, _z, _vp]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)      # every symbol include/ihmr_hip.h declares
# The same for include/ihmr_mano_ext.h, the second public header (the MANO layer's pose space and output stage);
# tests/test_mano_space_cpu.py compares it with that header's prototypes.  No name is in both tables.
SIGNATURES_EXT = {
    "ihmr_mano_pca_fwd": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ihmr_mano_pca_bwd": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ihmr_mano_post_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "ihmr_mano_post_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
}
MANO_POSE_DIM = 45                       # include/ihmr_mano_ext.h: IHMR_MANO_POSE_DIM


def bind(L, table=SIGNATURES):
    """Give every function of `table` (SIGNATURES or SIGNATURES_EXT) that the loaded library `L` exports its restype and argtypes.
    One rule for a library that lacks a symbol (an older build named with IHMR_HIP_LIBRARY for an A/B run against the parent
    commit): it is skipped, and a call of it raises AttributeError.  The product library is checked for every symbol where it is
    built."""
    for name, (restype, argtypes) in table.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def sources():
    include = osp.join(osp.dirname(_HERE), "include")
    return sorted(osp.join(SRC_DIR, f) for f in os.listdir(SRC_DIR) if f.endswith((".hip", ".h"))) + [
        osp.join(include, "ihmr_hip.h"), osp.join(include, "ihmr_mano_ext.h")]


HASH_PATH = osp.join(_HERE, "libihmr_hip.srchash")


def loaded_source_hash() -> str | None:
    """Source hash of the library this process would load, from its build record (None for an IHMR_HIP_LIBRARY override or a
    missing record).  bench.py quotes a committed profile only when the profile's recorded hash equals this."""
    if os.environ.get("IHMR_HIP_LIBRARY") or not osp.isfile(HASH_PATH):
        return None
    with open(HASH_PATH) as fh:
        rec = fh.read().split()
    return rec[0] if len(rec) == 2 else None


def _source_hash() -> str:
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    for f in sources():
        h.update(osp.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _file_hash(path: str) -> str:
    import hashlib
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def is_stale() -> bool:
    """The library is current iff the record written at build time matches BOTH the hash of the sources (+ flags) and the hash
    of the shared object itself -- content, not mtimes: the tree is copied to the GPU box, several ranks may import at once,
    and a library written by anything but :func:`build` (an experiment's hipcc line) must not pass for the product."""
    if not osp.isfile(LIB_PATH) or not osp.isfile(HASH_PATH):
        return True
    with open(HASH_PATH) as fh:
        rec = fh.read().split()
    return len(rec) != 2 or rec[0] != _source_hash() or rec[1] != _file_hash(LIB_PATH)


def build(force: bool = False, verbose: bool = False) -> str:
    """hipcc cross-compiles for gfx950 without a GPU (seconds).  Safe against concurrent callers (one rank per GPU): built
    under a lock file into a temporary name, then renamed into place."""
    if not force and not is_stale():
        return LIB_PATH
    import fcntl
    with open(LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or is_stale():             # another process may have built it while this one waited
                tmp = f"{LIB_PATH}.tmp{os.getpid()}"
                cmd = ["hipcc"] + HIPCC_FLAGS + [osp.join(SRC_DIR, "ihmr_hip.hip"), "-o", tmp]
                if verbose:
                    print(" ".join(cmd))
                subprocess.check_call(cmd)
                os.replace(tmp, LIB_PATH)
                with open(HASH_PATH + ".tmp", "w") as fh:
                    fh.write(_source_hash() + " " + _file_hash(LIB_PATH))
                os.replace(HASH_PATH + ".tmp", HASH_PATH)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


_LIB = None


def _resolve_library() -> str:
    """The product library.  `IHMR_HIP_LIBRARY` selects another build (profiling / A-B scripts use it instead of
    overwriting the product .so); otherwise the in-tree library, rebuilt when it is missing or older than its sources
    (hipcc present) -- a stale .so is never loaded silently."""
    override = os.environ.get("IHMR_HIP_LIBRARY")
    if override:
        if not osp.isfile(override):
            raise FileNotFoundError(f"IHMR_HIP_LIBRARY={override} does not exist")
        return override
    import shutil
    if shutil.which("hipcc"):
        return build()
    if not osp.isfile(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} is missing and hipcc is not available to build it")
    if is_stale():
        raise RuntimeError(f"{LIB_PATH} does not match its sources (or its build record {HASH_PATH} is missing) and hipcc is not "
                           "available to rebuild it: the ctypes structs of this package would not match the binary.  Rebuild where "
                           "hipcc exists, or name a library explicitly with IHMR_HIP_LIBRARY")
    return LIB_PATH


def lib():
    """Load (building on demand when hipcc is present) and bind (see bind() for a library that lacks a symbol).  Raises if
    unavailable -- never falls back."""
    global _LIB
    if _LIB is None:
        _LIB = bind(bind(C.CDLL(_resolve_library())), SIGNATURES_EXT)
    return _LIB


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"libihmr_hip: {what} failed with code {rc}")


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("ihmr_amd needs an MI355X (gfx950) GPU: the hot path has no CPU fallback")


def ptr(t: torch.Tensor | None):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ManoHandle:
    """Device-resident MANO constants (``ihmr_mano_create``)."""

    def __init__(self, arrays: dict, tip_ids=(744, 320, 443, 554, 671)):
        require_gpu()
        self._keep = dict(
            v_template=np.ascontiguousarray(arrays["v_template"], np.float32),
            shapedirs=np.ascontiguousarray(arrays["shapedirs"], np.float32),
            posedirs=np.ascontiguousarray(arrays["posedirs"], np.float32),
            J_regressor=np.ascontiguousarray(arrays["J_regressor"], np.float32),
            lbs_weights=np.ascontiguousarray(arrays["lbs_weights"], np.float32),
            parents=np.ascontiguousarray(arrays["parents"], np.int32),
            hands_mean=np.ascontiguousarray(arrays["hands_mean"], np.float32),
            faces=np.ascontiguousarray(arrays["faces"], np.int32),
            tip_ids=np.ascontiguousarray(tip_ids, np.int32),
        )
        a = ManoArrays(**{k: v.ctypes.data for k, v in self._keep.items()})
        h = C.c_void_p()
        check(lib().ihmr_mano_create(C.byref(a), C.byref(h)), "ihmr_mano_create")
        self.handle = h

    def update_shapedirs(self, shapedirs: np.ndarray):
        sd = np.ascontiguousarray(shapedirs, np.float32)
        check(lib().ihmr_mano_update_shapedirs(self.handle, sd.ctypes.data), "ihmr_mano_update_shapedirs")

    def __del__(self):
        try:
            import sys
            if sys is None or sys.is_finalizing():
                return  # the HIP runtime may already be gone at interpreter shutdown
            if getattr(self, "handle", None):
                lib().ihmr_mano_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

"""Each stage's tail does only what the stage can move -- against the generic tail forms and against the separate launches, bit for bit.

* A stage that moves only the translation (and possibly the camera) runs `opt_tail_kernel_trans`: the right hand is not skinned again,
  the left hand's next vertices are the kept pre-shift values plus the new shift (`OptWork::kept_left`, filled by the stage's first
  STEP launch).
* A hand none of whose axis-angles the stage refines keeps the rotations and the pose feature of its skeleton record in the STEP tails.

`ihmr_debug_force_generic_tail(1)` launches the generic forms only, `opt.no_fused_tail` runs the separate launches the tail
replaces.  Every comparison is
`np.array_equal` on `uint32` views: every array of `get_pred_result()`, the parameter blocks, the optimizer state, the snapshot
losses and parameters, the selection and the vertex buffer.

The translated-hand reuse of the collision grid (`sdf_no_static_reuse` = 0) is an acceleration of its own; the three runs of a case
share its setting.  The translation cases run a second pair -- the new tail against the separate launches -- with the reuse switched
off (`opt.sdf_no_translated_reuse`, `sdf_no_static_reuse` = 2), so the tail is checked with the left hand's grid kept and rebuilt."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STATE_KEYS = ("cam", "trans", "orient", "pose", "shape", "adam_m", "adam_v", "snap_loss", "snap_params", "selected", "verts", "joints_3d",
              "joints_2d", "loss_batch")


def _make_opt(B, epoch, freq, **extra):
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root="", strategy="opt_default", save_mid_freq=freq,
                                 optimizer="adam", opt_epoch=epoch, **extra)


def _batch(mano_arrays, kind, B):
    """The batches of tests/stage_cases.py (default / deep / far), built once, handed out unchanged."""
    from stage_cases import batch
    return batch(mano_arrays, kind, B)


def _stages(epoch, which):
    from ihmr_amd.strategies import make_opt_strategy
    trans, orient, pose, shape = make_opt_strategy(epoch)
    if which == "trans":
        return [trans]
    if which == "orient":
        return [orient]
    if which == "trans-cam":
        return [dict(trans, update_params=["pred_hand_trans", "pred_cam_params"])]
    if which == "shape":
        return [shape]
    if which == "left-shape":
        return [dict(shape, update_params=["pred_left_shape_params"])]
    assert which == "all"
    return [trans, orient, pose, shape]


def _run(batch, B, epoch, freq, which, generic=False, full=True, prepare=None, **extra):
    """One fresh instance (its stage graphs are captured under the switch), two passes (capture, replay).  full: optimize() as the
    driver runs it (the closing forward included); otherwise the stages alone.  prepare: called with the instance before its first input."""
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel
    prev = hip.lib().ihmr_debug_force_generic_tail(1 if generic else 0)
    try:
        m = OptimizeModel(_make_opt(B, epoch, freq, **extra))
        m.strategy = _stages(epoch, which)
        if prepare is not None:
            prepare(m)
        for rep in range(2):
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
    finally:
        hip.lib().ihmr_debug_force_generic_tail(prev)
    out = {f"export/{k}": np.ascontiguousarray(v) for k, v in m.get_pred_result().items() if isinstance(v, np.ndarray)}
    out.update({f"state/{k}": m.buf[k].cpu().numpy() for k in STATE_KEYS})
    out["selected_history"] = torch.stack(m.selected_history).cpu().numpy()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _check(batch, B, epoch, freq, which, translated_pair=False, **extra):
    new = _run(batch, B, epoch, freq, which, **extra)
    _assert_same(new, _run(batch, B, epoch, freq, which, generic=True, **extra), "stage tails vs generic tail forms")
    _assert_same(new, _run(batch, B, epoch, freq, which, no_fused_tail=True, **extra), "stage tails vs separate launches")
    if translated_pair:
        a = _run(batch, B, epoch, freq, which, sdf_no_translated_reuse=True, **extra)
        b = _run(batch, B, epoch, freq, which, sdf_no_translated_reuse=True, no_fused_tail=True, **extra)
        _assert_same(a, b, "stage tails vs separate launches, left hand's grid rebuilt")
    return new


@pytest.mark.parametrize("kind", ["default", "deep"])
@pytest.mark.parametrize("freq", [1, 2])
@pytest.mark.parametrize("n_iters", [1, 2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_translation_stage_alone(mano_arrays, B, n_iters, freq, kind):
    """n_iters = 1 launches no STEP tail, n_iters = 2 makes the filling launch and the stage's last launch neighbours, n_iters = 5 runs
    three launches on the kept vertices; B = 1: workgroup 0 also zeroes the collision counters."""
    batch = _batch(mano_arrays, kind, B)
    out = _check(batch, B, n_iters - 1, freq, "trans", translated_pair=True)
    if n_iters > 1:
        assert np.abs(out["state/adam_m"][:, 3:6]).max() > 0, "the stage computed no translation gradient"
        assert np.abs(out["state/adam_m"][:, 6:]).max() == 0


def test_translation_and_camera_in_one_stage(mano_arrays):
    batch = _batch(mano_arrays, "default", 3)
    out = _check(batch, 3, 2, 1, "trans-cam", translated_pair=True)
    assert np.abs(out["state/adam_m"][:, 0:3]).max() > 0 and np.abs(out["state/adam_m"][:, 3:6]).max() > 0


@pytest.mark.parametrize("B,fuse", [(3, 1), (64, 1), (3, 2)])
def test_opt_default_epoch_2(mano_arrays, B, fuse):
    """4 x 3 iterations through optimize(): the hand-over from the translation stage (right-hand vertices never rewritten, the
    candidate lists kept) to the orientation stage, and the shape stage behind the finger-pose stage; once with two fused batches."""
    batch = _batch(mano_arrays, "default", B)
    if fuse > 1:
        batch = {k: torch.cat([v] * fuse, dim=0) for k, v in batch.items()}
    out = _check(batch, B, 2, 1, "all", fuse_batches=fuse)
    assert np.abs(out["state/adam_m"][:, 102:]).max() > 0


@pytest.mark.parametrize("kind", ["far", "default", "deep"])
def test_shape_stage_alone(mano_arrays, kind):
    """far: only the fingertip vertices carry a gradient; deep: most vertices do.  The optimizer state after ONE iteration is
    (1 - beta1) x the shape gradient (+ the regulariser, computed the same way in every run): g_shape of the first iteration
    compared on its own."""
    batch = _batch(mano_arrays, kind, 3)
    first = _check(batch, 3, 0, 1, "shape")
    assert np.abs(first["state/adam_m"][:, 102:]).max() > 0, "no shape gradient"
    out = _check(batch, 3, 2, 1, "shape")
    if kind == "far":
        assert np.abs(out["state/loss_batch"][2]).max() == 0, "the far batch collides"
    else:
        assert np.abs(out["state/loss_batch"][2]).max() > 0, "no collision on this batch"


def test_left_shape_only_stage(mano_arrays):
    """Only `pred_left_shape_params` is refined: the right hand keeps its rotations AND its shape, the left hand's wrist and with it
    its shift move."""
    batch = _batch(mano_arrays, "default", 3)
    out = _check(batch, 3, 2, 1, "left-shape")
    assert np.abs(out["state/adam_m"][:, 112:]).max() > 0 and np.abs(out["state/adam_m"][:, 102:112]).max() == 0


TAIL_STATIC_LDS = 55840     # opt_tail_kernel's static LDS (tests/test_tail_build_cpu.py reads it from the build)
LDS_PER_WORKGROUP = 163840  # a workgroup's limit on gfx950: the fused tail is taken only when static + dynamic LDS fit it


def _dense_weights(arrays):
    """The lbs_weights of mano_cases.dense_weight_asset, checked on the host: some vertex has more than four non-zero weights (the
    kernels take their 16-joint loops) and the fused tail still fits -- 2 x 48 B of dynamic LDS per single-joint segment of <= 13 entries
    (csrc/mano_tables.h: LBS_SEG); otherwise the fused runs and the separate launches would be the same launches."""
    from mano_cases import dense_weight_asset
    w = dense_weight_asset(arrays)["lbs_weights"]
    assert int((w != 0).sum(axis=1).max()) > 4
    nseg = int(sum(-(-int(n) // 13) for n in (w != 0).sum(axis=0)))
    assert TAIL_STATIC_LDS + 2 * 48 * nseg <= LDS_PER_WORKGROUP, nseg
    return w


@pytest.mark.parametrize("which", ["trans", "orient"])
def test_dense_weights_reach_the_tails(mano_arrays, which):
    """The 16-joint blend of the tails' skinning phases, which MANO's own four weights per vertex never reach: three iterations of a
    translation stage (`opt_tail_kernel_trans`: the filling launch, then kept + shift) and of an orientation stage (`opt_tail_kernel<true,
    true>` phase 4) on an asset with up to seven weights per vertex, against the generic tail forms and against the separate launches
    (`lbs_skin_kernel` REUSE), bit for bit."""
    dense = {True: _dense_weights(mano_arrays[0]), False: _dense_weights(mano_arrays[1])}       # (asserted before anything is launched)

    def use_dense_weights(m):
        """Both MANO modules of a fresh instance: their device constants are made on first use, from these arrays."""
        for module in m.mano_models.values():
            module._arrays["lbs_weights"] = dense[module.is_rhand]
            module._dev_handle = None

    batch = _batch(mano_arrays, "default", 3)
    out = _check(batch, 3, 2, 1, which, prepare=use_dense_weights)
    lo = 3 if which == "trans" else 6
    assert np.abs(out["state/adam_m"][:, lo:lo + 3]).max() > 0, "the stage computed no gradient"

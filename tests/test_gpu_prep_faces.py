"""The ray-parity pairs of the collision prep kernel read the packed face table from LDS -- against the gather from global memory, byte for byte.

A hand that is not static stages its side's packed face table (`fpk`, 1600 words) in LDS at the top of `sdf_prep_kernel`, and every
(triangle, needed column) pair of the ray-parity phase reads its face word there; a static hand, whose `cur` array is busy, gathers
the word from global memory as before.  `ihmr_debug_prep_global_faces(1)` makes every hand gather: no hand fills or reads the LDS
table.  The pair test gets the same 32-bit word from another place, so nothing may differ -- not the results, and not the work done.

Every case runs twice on fresh instances (a captured graph keeps the switch it was captured with), switch off and on:

* launch sizes B = 64 (128 hands: the 1024-thread form) and B = 65 (130 hands: the smallest launch on the 512-thread form);
* the default asset on the deep-overlap batch (where the heavy hands are: at B = 64 some hands queue more than one window of pairs)
  and the five-finger asset with interlocked hands;
* `opt_default` at 3 iterations per stage plus the closing forward: the translation stage runs the static path, and over the
  schedule a list-reusing hand and a rebuilding hand both occur (asserted on the work counters);
* compared as raw bytes: every export of `get_pred_result`, `selected_history`, the inside bitmaps and boxes
  (`ihmr_opt_sdf_inside_bits`) after each stage, and the work counters -- `ray_tests`, `needed_voxels`, `inside_voxels` and the rest:
  the two paths must do the same work, not only reach the same result;
* one dense-grid call (`sdf_prep_kernel<true, 512>`) on the deep batch, the grid compared bit for bit."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEEP_SEED = 6475        # (tests/helpers.py: the deep batch of the collision tests)


def _make_opt(B, asset):
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root="synthetic:fingers" if asset == "fingers" else "", strategy="opt_default",
                                 save_mid_freq=1, optimizer="adam", opt_epoch=2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


class _Switch:
    """`ihmr_debug_prep_global_faces(force)` for the duration of a block; the previous value is put back."""

    def __init__(self, force):
        self.force = force

    def __enter__(self):
        from ihmr_amd import hip
        self.prev = hip.lib().ihmr_debug_prep_global_faces(1 if self.force else 0)

    def __exit__(self, *exc):
        from ihmr_amd import hip
        hip.lib().ihmr_debug_prep_global_faces(self.prev)


def _refine(B, asset, global_faces, batch=None):
    """One fresh instance under the switch: the four stages with the inside bitmaps read after each, the closing forward, everything
    with the work counters on.  Returns (what is compared, the counters, the batch)."""
    from ihmr_amd import two_hand
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    with _Switch(global_faces):
        m = OptimizeModel(_make_opt(B, asset))
        if batch is None:
            fwd = lambda p, s, t: two_hand.forward_from_packed(m.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
            batch = synthetic_opt_batch(B, fwd, seed=DEEP_SEED, interlock=asset == "fingers", overlap="deep" if asset == "deep" else None)
        out = {}
        m.set_input(batch); m.init_optimize()
        m.sdf_counters_start()
        m.selected_history = []
        for i, stage in enumerate(m.strategy):
            m.run_stage(stage)
            m.selected_history.append(m.buf["selected"].clone())
            out[f"inside_bits/{i}"], out[f"box/{i}"] = m.sdf_inside_bits()
        m.forward_losses(m.default_loss_weights)
        torch.cuda.synchronize()
        counters = m.sdf_counters_stop()
    out.update({f"export/{k}": np.ascontiguousarray(v) for k, v in m.get_pred_result().items() if isinstance(v, np.ndarray)})
    out["selected_history"] = torch.stack(m.selected_history).cpu().numpy()
    return out, counters, batch


@pytest.mark.parametrize("asset", ["deep", "fingers"])
@pytest.mark.parametrize("B", [64, 65])
def test_refinement_is_the_same_bytes_and_the_same_work(B, asset):
    lds, c_lds, batch = _refine(B, asset, False)
    glb, c_glb, _ = _refine(B, asset, True, batch)
    print(f"[prep faces] {asset} B = {B}: counters {c_lds}")
    # the schedule exercises what it is meant to: pairs were tested, inside voxels found, and voxels answered from kept candidate lists
    # (a list-reusing hand) as well as voxels whose lists were (re)built (a hand that starts over) both occur
    assert c_lds["ray_tests"] > 0 and c_lds["inside_voxels"] > 0 and c_lds["needed_voxels"] > 0
    assert c_lds["voxels_from_lists"] > 0 and c_lds["voxels_rebuilt"] > 0, c_lds
    assert any(lds[f"inside_bits/{i}"].any() for i in range(4))
    _assert_same(lds, glb, f"LDS face table vs global gather ({asset}, B = {B})")
    assert c_lds == c_glb, (c_lds, c_glb)


def test_dense_grid_is_the_same_bits(mano_arrays):
    """`sdf_prep_kernel<true, 512>`: every voxel is needed, every triangle queues all the columns of its box (several windows of pairs
    per hand)."""
    from helpers import oracle_two_hand_verts
    from ihmr_amd import hip
    right, left = mano_arrays
    B = 3
    hv, _ = oracle_two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
    dev = torch.device("cuda:0")
    fr, fl, hv = torch.tensor(right["faces"].astype(np.int32)).to(dev), torch.tensor(left["faces"].astype(np.int32)).to(dev), hv.to(dev)
    grids = []
    for global_faces in (False, True):
        with _Switch(global_faces):
            phi = torch.full((B, 2, 32, 32, 32), float("nan"), device=dev)
            ws = torch.empty(hip.lib().ihmr_sdf_workspace_bytes(B), dtype=torch.uint8, device=dev)
            hip.check(hip.lib().ihmr_sdf_dense_grid(hip.ptr(fr), hip.ptr(fl), hip.ptr(hv), B, hip.ptr(phi), hip.ptr(ws), hip.stream_ptr()), "ihmr_sdf_dense_grid")
            torch.cuda.synchronize()
        grids.append(phi.cpu().numpy())
    assert np.isfinite(grids[0]).all() and (grids[0] > 0).sum() > 1000, "the dense grid has no interior"
    assert np.array_equal(_bits(grids[0]), _bits(grids[1])), "the dense grid differs between the LDS face table and the global gather"

"""The refinement loop, the stand-alone collision entry points and the IHMR-MLP evaluation inside guarded buffers.

Every buffer these entry points are handed -- inputs, state, outputs and above all the workspaces, which are exactly
`ihmr_opt_workspace_bytes(B)` / `ihmr_sdf_workspace_bytes(B)` / `ihmr_mlp_workspace_bytes(B)` bytes long -- lies between 0xA5 guards
(tests/guarded.py), and the workspace starts out filled with 0x00, 0xFF (counters of -1, NaN floats) or 0xA5 (large indices):

  a. no guard is damaged, the pure inputs keep their bits, a stage with mask m leaves the parameter blocks outside m alone, and their
     optimizer slots hold what the stage's fresh optimizer holds for them (+0.0: every stage starts from a zeroed state, so for a
     model's first stage that is bit-identical to before);
  b. the results are the bits of the same run on ordinary allocations (which the oracle tests pin);
  c. the results do not depend on what the workspace held before the first call;
  d. a workspace sized for B = 8 serves a B = 8 and a B = 3 model in turn, and a forward_losses() between two stages changes nothing;
  e. the same for `ihmr_sdf_collision_ex` and `ihmr_sdf_dense_grid` through ctypes, and for the loop's diagnostics;
  f. the same for `MLPModel.test()` (`ihmr_mlp_forward_select` modes 0 - 3, `ihmr_mlp_camera_select`, `ihmr_mlp_stage_head`).

A damaged guard is reported with the buffer and the payload offset; tests/test_workspace_carve_cpu.py prints the carve table (region,
offset, bytes) to look the offset up in.  Nothing here undersizes a buffer on purpose: that the guard check is live is shown on the host
side (`test_guard_check_reports_a_flipped_byte`)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PURE_INPUTS = ("init_joints_2d", "init_joints_3d", "init_hand_trans_j", "gt_joints_2d", "gt_joints_3d", "gt_hand_trans", "hand_type_array")
RESULT_STATE = ("selected", "snap_loss", "snap_params", "adam_m", "adam_v")
BLOCK_VIEW = dict(pred_cam_params=lambda b: b["cam"], pred_hand_trans=lambda b: b["trans"], pred_right_orient=lambda b: b["orient"][0],
                  pred_left_orient=lambda b: b["orient"][1], pred_right_pose_params=lambda b: b["pose"][0],
                  pred_left_pose_params=lambda b: b["pose"][1], pred_right_shape_params=lambda b: b["shape"][0],
                  pred_left_shape_params=lambda b: b["shape"][1])
N_ITERS = 3
BATCHES = (("default", 3), ("deep", 3), ("deep", 1), ("deep", 8))


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _make_opt(B, **extra):
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root="", strategy="opt_default", save_mid_freq=1,
                                 optimizer="adam", opt_epoch=N_ITERS - 1, **extra)


def _batch(mano_arrays, kind, B):
    from stage_cases import batch
    return batch(mano_arrays, kind, B)


def _mask_of(stage):
    from ihmr_amd import hip
    m = 0
    for n in stage["update_params"]:
        m |= hip.PARAM_BLOCKS[n][0]
    return m


def _loop_cases():
    """(id, mask, switches): one mask per tail form a stage's stepping iterations can take, then every block, the camera alone, and every
    block through the separate launches."""
    import stage_cases as sc
    out = []
    for form in (sc.TAIL_TRANS, sc.TAIL_STEP_SKIN, sc.TAIL_STEP, sc.TAIL_PLAIN):
        mask = next(m for m in sc.REPRESENTATIVES if sc.plan(m).step_tail == form)
        out.append((f"{form}-mask{mask}", mask, {}))
    out += [("all-mask255", 255, {}), ("camera-mask1", 1, {}), ("separate-mask255", 255, dict(no_fused_tail=True))]
    assert sc.plan(255, no_fused_tail=1).step_tail == sc.TAIL_SEPARATE and sc.plan(1).step_tail == sc.TAIL_SEPARATE
    return out


LOOP_CASES = _loop_cases()


def _collect(m):
    out = {f"export/{k}": np.ascontiguousarray(v) for k, v in m.get_pred_result().items() if isinstance(v, np.ndarray)}
    out.update({f"state/{k}": m.buf[k].cpu().numpy() for k in RESULT_STATE})
    return out


def _run(batch, B, stages, graphs, fill, between=False, workspace=None, model=None, **extra):
    """forward_losses, the stages, forward_losses on a fresh instance -- on guarded buffers when `fill` is a byte (the workspace
    pre-filled with it once, before the first call), on the instance's own allocations when it is None -- with the checks of (a)
    after every call.  between: a forward_losses() between the stages.  Returns (results, instance, guards)."""
    from guarded import assert_guards, guard_model
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel
    m = model or OptimizeModel(_make_opt(B, use_graphs=graphs, **extra))
    guards = getattr(m, "_test_guards", None)
    if guards is None:
        guards = m._test_guards = guard_model(m, fill, workspace) if fill is not None else {}
    what = f"B = {B}, graphs = {graphs}, fill = {fill}"
    m.set_input(batch); m.init_optimize()
    torch.cuda.synchronize()
    inputs = {k: _bits(m.buf[k]) for k in PURE_INPUTS}
    m.forward_losses()
    torch.cuda.synchronize()
    assert_guards(guards, f"{what}: forward_losses")
    for i, stage in enumerate(stages):
        mask = _mask_of(stage)
        before = {n: _bits(view(m.buf)) for n, view in BLOCK_VIEW.items()}
        if i == 0 and model is None:
            assert not _bits(m.buf["adam_m"]).any() and not _bits(m.buf["adam_v"]).any()
        m.run_stage(stage)
        torch.cuda.synchronize()
        assert_guards(guards, f"{what}: stage {i} (mask {mask})")
        am, av = _bits(m.buf["adam_m"]), _bits(m.buf["adam_v"])
        for n, (bit, lo, size) in hip.PARAM_BLOCKS.items():
            if not mask & bit:
                assert np.array_equal(before[n], _bits(BLOCK_VIEW[n](m.buf))), f"{what}: stage {i} (mask {mask}) changed {n}"
                assert not am[:, lo:lo + size].any() and not av[:, lo:lo + size].any(), f"{what}: stage {i} (mask {mask}) left optimizer state for {n}"
        if between and i + 1 < len(stages):
            m.forward_losses()
    m.forward_losses()
    torch.cuda.synchronize()
    assert_guards(guards, f"{what}: closing forward_losses")
    for k in PURE_INPUTS:
        assert np.array_equal(inputs[k], _bits(m.buf[k])), f"{what}: input {k} was written"
    return _collect(m), m, guards


# ------------------------------------------------------------------------------------------------ the guard check itself
def test_guard_check_reports_a_flipped_byte():
    """Device memory: one guard byte flipped by a torch op from the host side is reported at its payload-relative offset, on either
    side; writing the whole payload damages nothing."""
    from guarded import GUARD_BYTE, SMALL_GUARD, Guarded
    g = Guarded(1000, fill=0xFF)
    assert g.data_ptr % 256 == 0 and g.view(torch.int32, (250,)).eq(-1).all()
    g.view(torch.float32, (10, 25)).zero_()
    assert g.guards_intact() is None
    for off in (1000, 1000 + SMALL_GUARD - 1, -1, -SMALL_GUARD):
        g.raw[g.lo + off] ^= 0x10
        assert g.guards_intact() == off, off
        g.raw[g.lo + off] = GUARD_BYTE
        assert g.guards_intact() is None


def test_guard_model_moves_every_buffer(mano_arrays):
    from guarded import SMALL_GUARD, WORKSPACE_GUARD, guard_model
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel
    m = OptimizeModel(_make_opt(3))
    old = {k: v.data_ptr() for k, v in m.buf.items()}
    guards = guard_model(m, 0xFF)
    assert guards.keys() == m.buf.keys()
    for k, g in guards.items():
        assert getattr(m.io, k) == g.data_ptr == m.buf[k].data_ptr() != old[k] and g.data_ptr % 256 == 0
        assert g.guard == (WORKSPACE_GUARD if k == "workspace" else SMALL_GUARD) and g.guards_intact() is None
    assert guards["workspace"].nbytes == hip.lib().ihmr_opt_workspace_bytes(3) and bool((m.buf["workspace"] == 0xFF).all())
    m.set_input(_batch(mano_arrays, "default", 3)); m.init_optimize(); m.forward_losses()
    torch.cuda.synchronize()
    # the launches really ran on the guarded memory: the workspace's fill is gone, the outputs are there
    assert not bool((guards["workspace"].payload_bytes() == 0xFF).all()) and float(guards["verts"].view(torch.float32, (2, 3, 778, 3)).abs().max()) > 0
    with pytest.raises(AssertionError):
        guard_model(m)                       # a graph has been captured on the old addresses


# ------------------------------------------------------------------------------------------------ a - c: the loop
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("case", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
@pytest.mark.parametrize("kind,B", BATCHES, ids=[f"{k}{b}" for k, b in BATCHES])
def test_one_stage_inside_guards(mano_arrays, kind, B, case, graphs):
    from guarded import FILLS
    from stage_cases import stage_for
    _, mask, extra = case
    batch, stages = _batch(mano_arrays, kind, B), [stage_for(mask, N_ITERS)]
    plain, _, _ = _run(batch, B, stages, graphs, None, **extra)
    assert plain["state/snap_loss"].shape[0] == N_ITERS and np.abs(plain["state/adam_m"]).max() > 0
    for fill in FILLS:
        got, _, _ = _run(batch, B, stages, graphs, fill, **extra)
        _same(got, plain, f"guarded, workspace pre-filled with {fill:#04x}, vs ordinary buffers")


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("kind,B", BATCHES, ids=[f"{k}{b}" for k, b in BATCHES])
def test_default_stages_in_sequence_inside_guards(mano_arrays, kind, B, graphs):
    """The four stages of opt_default on one instance: `keep_lists` carries the candidate lists across the stage boundaries, the
    translation stage fills and reads `kept_left`."""
    from guarded import FILLS
    from ihmr_amd.strategies import make_opt_strategy
    batch, stages = _batch(mano_arrays, kind, B), make_opt_strategy(N_ITERS - 1)
    plain, _, _ = _run(batch, B, stages, graphs, None)
    for fill in FILLS:
        got, _, _ = _run(batch, B, stages, graphs, fill)
        _same(got, plain, f"guarded, workspace pre-filled with {fill:#04x}, vs ordinary buffers")


# ------------------------------------------------------------------------------------------------ d: reuse
@pytest.mark.parametrize("order", ["8 then 3", "3 then 8"])
def test_one_workspace_serves_two_batch_sizes(mano_arrays, order):
    """A workspace of ihmr_opt_workspace_bytes(8): the B = 8 deep batch and the B = 3 default batch run on it in turn (two instances,
    one memory); each gives the bits of a fresh run of its own, whatever the other left behind."""
    from guarded import WORKSPACE_GUARD, Guarded, assert_guards
    from ihmr_amd import hip
    from ihmr_amd.strategies import make_opt_strategy
    stages = make_opt_strategy(N_ITERS - 1)
    b8, b3 = _batch(mano_arrays, "deep", 8), _batch(mano_arrays, "default", 3)
    fresh = {8: _run(b8, 8, stages, True, None)[0], 3: _run(b3, 3, stages, True, None)[0]}
    ws = Guarded(hip.lib().ihmr_opt_workspace_bytes(8), guard=WORKSPACE_GUARD, fill=0xFF)
    guards = []
    for B in ((8, 3) if order == "8 then 3" else (3, 8)):
        got, _, g = _run(b8 if B == 8 else b3, B, stages, True, 0xFF, workspace=ws)
        assert g["workspace"] is ws
        guards.append(g)
        _same(got, fresh[B], f"{order}: B = {B} on the shared workspace vs a fresh run")
    for g in guards:
        assert_guards(g, f"{order}: at the end")


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("kind,B", [("default", 3), ("deep", 3)])
def test_forward_losses_between_stages_changes_nothing(mano_arrays, kind, B, graphs):
    """forward_losses() is a single-shot collision launch on the loop's workspace: the instance forgets its lists (`_lists_live`) and the
    next stage rebuilds them -- an exact acceleration less, the same bits.  (`sdf_no_translated_reuse`: the one acceleration that is
    not exact is off in both runs.)"""
    from ihmr_amd.strategies import make_opt_strategy
    batch, stages = _batch(mano_arrays, kind, B), make_opt_strategy(N_ITERS - 1)
    straight, _, _ = _run(batch, B, stages, graphs, 0xA5, sdf_no_translated_reuse=True)
    got, m, _ = _run(batch, B, stages, graphs, 0xA5, between=True, sdf_no_translated_reuse=True)
    _same(got, straight, "with a forward_losses() between the stages vs without")
    # ... and a second batch through the same instance (graphs replayed, lists of the previous batch in the workspace)
    again, _, _ = _run(batch, B, stages, graphs, 0xA5, model=m, sdf_no_translated_reuse=True)
    _same(again, straight, "second pass of the same instance")


# ------------------------------------------------------------------------------------------------ e: the collision entry points
def _hand_pairs(mano_arrays, geometry, B):
    from helpers import DEEP_SEED, POINT_CLOUD_SEED, oracle_two_hand_verts, point_cloud_pairs
    if geometry == "ball":
        hv, _ = oracle_two_hand_verts(mano_arrays, B, 77)
        c = hv.mean(dim=2, keepdim=True)
        d = hv - c
        return (c + 0.08 * d / d.norm(dim=3, keepdim=True).clamp_min(1e-9)).contiguous()
    hv, _ = oracle_two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
    return point_cloud_pairs(hv, POINT_CLOUD_SEED) if geometry == "point cloud" else hv


def _faces(mano_arrays):
    right, left = mano_arrays
    return (torch.tensor(right["faces"].astype(np.int32)).cuda(), torch.tensor(left["faces"].astype(np.int32)).cuda())


def _guarded_collision(mano_arrays, hv, fill):
    from guarded import WORKSPACE_GUARD, Guarded, assert_guards
    from ihmr_amd import hip
    L, B = hip.lib(), hv.shape[0]
    fr, fl = _faces(mano_arrays)
    g = dict(hand_verts=Guarded(B * 2 * 778 * 3 * 4), loss=Guarded(B * 4), per_vert=Guarded(B * 1556 * 4), origin_scale=Guarded(B * 1556 * 4),
             dval=Guarded(B * 1556 * 3 * 4), workspace=Guarded(L.ihmr_sdf_workspace_bytes(B), guard=WORKSPACE_GUARD, fill=fill))
    g["hand_verts"].copy_in(hv.cuda())
    p = lambda k: C.c_void_p(g[k].data_ptr)
    hip.check(L.ihmr_sdf_collision_ex(hip.ptr(fr), hip.ptr(fl), p("hand_verts"), B, 0.0, None, p("loss"), p("per_vert"), p("origin_scale"),
                                      p("dval"), p("workspace"), hip.stream_ptr()), "ihmr_sdf_collision_ex")
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_sdf_collision_ex, B = {B}, fill = {fill:#04x}")
    assert torch.equal(g["hand_verts"].view(torch.float32, tuple(hv.shape)).cpu(), hv), "the input vertices were written"
    return dict(loss=g["loss"].view(torch.float32, (B,)).cpu(), per_vert=g["per_vert"].view(torch.float32, (B, 1556)).cpu(),
                origin_scale=g["origin_scale"].view(torch.float32, (B, 1556)).cpu(), dval=g["dval"].view(torch.float32, (B, 1556, 3)).cpu())


def _plain_collision(mano_arrays, hv):
    """`SDFLoss` on ordinary allocations; dval = d per_vert / d(query vertex) read off the gradient of sum(per_vert) (coefficient 1.0:
    the backward hands dval through unchanged, entry (h, v) at vertex v of hand 1 - h)."""
    from ihmr_amd.sdf import SDFLoss
    right, left = mano_arrays
    B = hv.shape[0]
    x = hv.clone().cuda().requires_grad_(True)
    loss, pv, osc = SDFLoss(right["faces"], left["faces"]).cuda()(x, return_per_vert_loss=True, return_origin_scale_loss=True)
    pv.sum().backward()
    return dict(loss=loss.detach().cpu(), per_vert=pv.detach().cpu(), origin_scale=osc.detach().cpu(),
                dval=torch.flip(x.grad.view(B, 2, 778, 3), dims=[1]).reshape(B, 1556, 3).cpu())


def _check_collision(mano_arrays, geometry, B):
    from guarded import FILLS
    hv = _hand_pairs(mano_arrays, geometry, B)
    plain = _plain_collision(mano_arrays, hv)
    assert int((plain["per_vert"] > 0).sum()) > 100 * B, "the pairs must penetrate"
    for fill in FILLS:
        _same(_guarded_collision(mano_arrays, hv, fill), plain, f"{geometry} B = {B}: guarded, workspace pre-filled with {fill:#04x}, vs SDFLoss")
    return hv, plain


def test_collision_entry_point_inside_guards_deep(mano_arrays):
    """Deep overlap, B = 3: guards, the bits of `SDFLoss`, independence of the fill -- and the guarded outputs against the oracle with
    the tolerances of test_gpu_parity.py::test_sdf_collision_matches_oracle."""
    from oracle.sdf_ref import SDFLossRef
    from test_gpu_parity import _report
    right, left = mano_arrays
    hv, _ = _check_collision(mano_arrays, "deep", 3)
    got = _guarded_collision(mano_arrays, hv, 0xFF)
    x = hv.clone().requires_grad_(True)
    l_ref, pv_ref, os_ref = SDFLossRef(right["faces"], left["faces"])(x, return_per_vert_loss=True, return_origin_scale_loss=True)
    w = torch.linspace(0.5, 1.5, 3)
    (l_ref * w).sum().backward()
    assert int((pv_ref > 0).sum()) > 50, "test batch must actually penetrate"
    _report("guarded sdf per_vert", got["per_vert"], pv_ref.detach(), atol=1e-6)
    _report("guarded sdf origin_scale [m]", got["origin_scale"], os_ref.detach(), atol=1e-7)
    _report("guarded sdf loss", got["loss"], l_ref.detach(), atol=1e-5, rtol=1e-6)
    grad = torch.flip(((w / 4.0).view(3, 1, 1) * got["dval"]).view(3, 2, 778, 3), dims=[1])      # SDFLoss's backward, loss_divisor 4
    _report("guarded sdf d/dverts", grad, x.grad, atol=1e-4 * float(x.grad.abs().max()))


@pytest.mark.parametrize("geometry,B", [("point cloud", 2), ("deep", 65)], ids=["point-cloud-2", "deep-65"])
def test_collision_entry_point_inside_guards(mano_arrays, geometry, B):
    """The point cloud needs almost every column of the right hand's grid (the fullest inside lists); B = 65 is 130 hands, more than
    SDF_PREP_SMALL_MAX_HANDS = 128: the 512-thread prep form."""
    _check_collision(mano_arrays, geometry, B)


@pytest.mark.parametrize("geometry,B", [("deep", 3), ("point cloud", 2), ("ball", 2)], ids=["deep-3", "point-cloud-2", "ball-2"])
def test_dense_grid_inside_guards(mano_arrays, geometry, B):
    """`ihmr_sdf_dense_grid`: phi and its workspace guarded; "ball" takes the distance kernel's survivor-list overflow path."""
    from guarded import FILLS, WORKSPACE_GUARD, Guarded, assert_guards
    from ihmr_amd import hip
    L = hip.lib()
    hv = _hand_pairs(mano_arrays, geometry, B).cuda()
    fr, fl = _faces(mano_arrays)
    plain = torch.empty(B, 2, 32, 32, 32, device="cuda")
    ws = torch.empty(L.ihmr_sdf_workspace_bytes(B), dtype=torch.uint8, device="cuda")
    hip.check(L.ihmr_sdf_dense_grid(hip.ptr(fr), hip.ptr(fl), hip.ptr(hv), B, hip.ptr(plain), hip.ptr(ws), hip.stream_ptr()), "ihmr_sdf_dense_grid")
    torch.cuda.synchronize()
    assert int((plain > 0).sum()) > 0
    for fill in FILLS:
        g = dict(phi=Guarded(B * 2 * 32768 * 4), workspace=Guarded(L.ihmr_sdf_workspace_bytes(B), guard=WORKSPACE_GUARD, fill=fill))
        hip.check(L.ihmr_sdf_dense_grid(hip.ptr(fr), hip.ptr(fl), hip.ptr(hv), B, C.c_void_p(g["phi"].data_ptr), C.c_void_p(g["workspace"].data_ptr),
                                        hip.stream_ptr()), "ihmr_sdf_dense_grid")
        torch.cuda.synchronize()
        assert_guards(g, f"ihmr_sdf_dense_grid, {geometry} B = {B}, fill = {fill:#04x}")
        assert np.array_equal(_bits(g["phi"].view(torch.float32, (B, 2, 32, 32, 32))), _bits(plain)), f"{geometry}: phi differs, fill {fill:#04x}"


def test_public_collision_workspace_size_is_the_restated_formula():
    from ihmr_amd import hip
    from test_workspace_carve_cpu import BATCHES as SIZES, sdf_public_workspace_bytes
    for B in SIZES:
        assert hip.lib().ihmr_sdf_workspace_bytes(B) == sdf_public_workspace_bytes(B), B


class _HostGuarded:
    """A host array between 0xA5 guards (the diagnostics copy to host memory)."""

    def __init__(self, dtype, shape, guard=256):
        self.n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.raw = np.full(guard + self.n + guard, 0xA5, np.uint8)
        self.guard = guard
        self.array = self.raw[guard:guard + self.n].view(dtype).reshape(shape)

    @property
    def ptr(self):
        return C.c_void_p(self.raw.ctypes.data + self.guard)

    def intact(self):
        return bool((self.raw[:self.guard] == 0xA5).all() and (self.raw[self.guard + self.n:] == 0xA5).all())


def test_loop_diagnostics_inside_guards(mano_arrays):
    """`ihmr_opt_sdf_counters`, `ihmr_opt_sdf_inside_bits` and `ihmr_opt_sdf_stats` after a guarded stage on the deep batch: their host
    outputs are guarded, the guards of the loop's buffers stay intact."""
    from guarded import assert_guards, guard_model
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel, _weights
    from ihmr_amd.strategies import make_opt_strategy
    B, L = 3, hip.lib()
    m = OptimizeModel(_make_opt(B, use_graphs=False))
    guards = guard_model(m, 0xFF)
    m.set_input(_batch(mano_arrays, "deep", B)); m.init_optimize()
    io = C.byref(m.io)
    counters = _HostGuarded(np.uint64, (16,))
    hip.check(L.ihmr_opt_sdf_counters(io, B, None, 1), "ihmr_opt_sdf_counters")
    try:
        m.run_stage(make_opt_strategy(N_ITERS - 1)[1])
    finally:
        hip.check(L.ihmr_opt_sdf_counters(io, B, counters.ptr, 0), "ihmr_opt_sdf_counters")      # (switches the counters off again)
    assert_guards(guards, "after a counted stage")
    stats = _HostGuarded(np.uint64, (4,))
    mr, ml = m._mano_handles()
    w = _weights(m.default_loss_weights)
    hip.check(L.ihmr_opt_sdf_stats(mr, ml, io, B, C.byref(w), stats.ptr, hip.stream_ptr()), "ihmr_opt_sdf_stats")
    bits, box = _HostGuarded(np.uint32, (2, B, 1024)), _HostGuarded(np.float32, (2, B, 4))
    hip.check(L.ihmr_opt_sdf_inside_bits(io, B, bits.ptr, box.ptr), "ihmr_opt_sdf_inside_bits")
    torch.cuda.synchronize()
    assert_guards(guards, "after the diagnostics")
    assert counters.intact() and bits.intact() and box.intact() and stats.intact()
    named = dict(zip(OptimizeModel.SDF_COUNTERS, counters.array.tolist()))
    print("[guarded] counters of the stage:", named, "stats of one launch pair:", stats.array.tolist())
    assert named["inside_voxels"] > 0 and named["needed_voxels"] >= named["inside_voxels"]
    assert stats.array[2] > 0 and stats.array[3] >= stats.array[2]
    assert bits.array.any() and np.isfinite(box.array).all() and (box.array[..., 3] > 0).all()


# ------------------------------------------------------------------------------------------------ f: IHMR-MLP evaluation
def _mlp_opt(B, **kw):
    d = dict(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, input_nc=3, num_joints=42,
             total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20, trans_params_dim=3,
             model_root="", mean_param_file="mean_mano_params.pkl", checkpoints_dir="./checkpoints", strategy="mlp_default")
    d.update(kw)
    return types.SimpleNamespace(**d)


_MLP_BATCHES = {}


def _mlp_batch(mano_arrays, B):
    """The synthetic IHMR-MLP batch with a non-contiguous, unordered dataset index into tables of 2B + 3 rows."""
    from helpers import synthetic_mlp_batch
    if B not in _MLP_BATCHES:
        b = synthetic_mlp_batch(mano_arrays, B, seed=4100 + B)
        b["index"] = torch.tensor([(5 * i + 2) % (2 * B + 3) for i in range(B)], dtype=torch.long)
        assert len(set(b["index"].tolist())) == B
        _MLP_BATCHES[B] = b
    return _MLP_BATCHES[B]


TABLES = ("data_idxs_all", "img_feat_all", "prev_final", "prev_loss")


def _mlp_run(mano_arrays, B, fill, graph):
    """MLPModel.test() twice (the second call finds the first one's rows in the tables; with `graph` it is a replay).  fill: the core's
    buffers, the four tables and the hidden-activation workspace are guarded, both workspaces pre-filled with it."""
    from guarded import WORKSPACE_GUARD, Guarded, assert_guards, guard_model
    from helpers import seeded_state_dict
    from ihmr_amd import hip
    from ihmr_amd.mlp_model import MLPModel
    from ihmr_amd.strategies import make_mlp_strategy
    batch, num_data, strategy = _mlp_batch(mano_arrays, B), 2 * B + 3, make_mlp_strategy()
    m = MLPModel(_mlp_opt(B, use_test_graph=graph))
    guards = guard_model(m._core, fill) if fill is not None else {}
    m.set_update_info(strategy, num_data)
    for sid in range(len(strategy)):
        m.add_new_network(sid)
        m.sub_network_list[sid].load_state_dict(seeded_state_dict(m.sub_network_list[sid], 700 + sid, last_scale=0.05))
    m.eval()
    # rows no batch touches carry a pattern, so that "untouched" means something
    gen = torch.Generator().manual_seed(17)
    pattern = {k: torch.rand(getattr(m, k).shape, generator=gen).to(m.device) for k in TABLES[1:]}
    for k in TABLES:
        t = getattr(m, k)
        if k in pattern:
            t.copy_(pattern[k])
        if fill is not None:
            guards[k] = Guarded(t.numel() * t.element_size())
            setattr(m, k, guards[k].copy_in(t))
    m.set_input(batch)
    if fill is not None:
        g = m._glue()
        guards["mlp_workspace"] = Guarded(hip.lib().ihmr_mlp_workspace_bytes(B), guard=WORKSPACE_GUARD, fill=fill)
        assert g["ws"].numel() == guards["mlp_workspace"].nbytes
        g["ws"] = guards["mlp_workspace"].payload_bytes()
    out = []
    absent = torch.ones(num_data, dtype=torch.bool)
    absent[batch["index"]] = False
    for rep in range(2):
        m.set_input(batch); m.test()
        torch.cuda.synchronize()
        assert_guards(guards, f"MLPModel.test() call {rep}, B = {B}, fill = {fill}")
        res = {f"export/{k}": v for k, v in m.get_pred_result().items()}
        res["kept"] = torch.stack(m.kept_history).cpu().numpy()
        for k in TABLES:
            res[f"table/{k}"] = getattr(m, k).cpu().numpy().astype(np.uint8 if k == "data_idxs_all" else np.float32)
        for k in TABLES[1:]:
            assert np.array_equal(_bits(res[f"table/{k}"][absent.numpy()]), _bits(pattern[k].cpu()[absent])), f"{k}: a row outside the batch was written"
        assert not res["table/data_idxs_all"][absent.numpy()].any() and res["table/data_idxs_all"][~absent.numpy()].all()
        out.append(res)
    print(f"[guarded] MLP B = {B}: kept per stage {out[0]['kept'].sum(axis=1).tolist()}, second call {out[1]['kept'].sum(axis=1).tolist()}")
    assert out[0]["kept"].shape == (len(strategy), B)
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("B", [3, 17])
def test_mlp_evaluation_inside_guards(mano_arrays, B, graph):
    from guarded import FILLS
    plain = _mlp_run(mano_arrays, B, None, graph)
    for fill in FILLS:
        got = _mlp_run(mano_arrays, B, fill, graph)
        for rep in range(2):
            _same(got[rep], plain[rep], f"MLPModel.test() call {rep}: guarded, workspaces pre-filled with {fill:#04x}, vs ordinary buffers")

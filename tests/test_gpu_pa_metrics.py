"""The Procrustes-aligned metrics on the device (``ihmr_eval_pa_joints`` / ``ihmr_eval_pa_verts``, csrc/evaluate.h + csrc/eval_pure.h)
against the float64 numpy statement of tests/pa_cases.py, and the paths above them: ``Evaluator.update_device_pa`` /
``update_device_pa_verts`` against the host records, ``run_optimize --pa_metrics`` with and without ``--host_eval``.

The bar on a per-point error is 1e-9 m, the project's absolute floor for metric comparisons: the inputs are the same float32 numbers
on both sides, both sides work in float64, and every case with three or more valid points has the gap g >= 1e-2 of pa_cases.py, so
the two routes (Horn + Jacobi here, SVD there) agree to ~1e-14.  Both kernels work per sample: B = 1 and the case-table batch."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pa_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
GUARD = 64          # NaN-filled doubles on either side of every output


@pytest.fixture(scope="module")
def joints():
    names, pred, gt, scale = PC.joint_batch()
    ref = [PC.joints_statement(pred[b], gt[b], scale[b]) for b in range(len(names))]
    return types.SimpleNamespace(names=names, pred=pred, gt=gt, scale=scale, out=np.stack([r[0] for r in ref]), pe=np.stack([r[1] for r in ref]))


@pytest.fixture(scope="module")
def verts():
    names, pred, gt, weight, scale = PC.vert_batch()
    ref = [[PC.verts_statement(pred[b, h], gt[b, h], weight[b, h], scale[b]) for h in range(2)] for b in range(len(names))]
    return types.SimpleNamespace(names=names, pred=pred, gt=gt, weight=weight, scale=scale,
                                 out=np.array([[r[0] for r in row] for row in ref]), pe=np.array([[r[1] for r in row] for row in ref]))


def _guarded(n):
    import torch
    return torch.full((n + 2 * GUARD,), float("nan"), device="cuda", dtype=torch.float64)


def _take(buf, shape):
    """The payload of a guarded buffer; asserts both guard regions still hold NaN."""
    import torch
    n = int(np.prod(shape))
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), "a guard region was written"
    return buf[GUARD:GUARD + n].cpu().numpy().reshape(shape)


def run_joints(pred, gt, scale=None, point_err=True):
    import torch

    from ihmr_amd import hip
    B = pred.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    p, g, s = up(pred), up(gt), None if scale is None else up(scale)
    out, pe = _guarded(B * 6), _guarded(B * 3 * 42) if point_err else None
    off = GUARD * 8
    rc = hip.lib().ihmr_eval_pa_joints(p.data_ptr(), g.data_ptr(), None if s is None else s.data_ptr(), B, out.data_ptr() + off,
                                       None if pe is None else pe.data_ptr() + off, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return _take(out, (B, 3, 2)), None if pe is None else _take(pe, (B, 3, 42))


def run_verts(pred, gt, weight, scale=None, point_err=True):
    import torch

    from ihmr_amd import hip
    B = pred.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    pr, pl, gr, gl, w, s = up(pred[:, 0]), up(pred[:, 1]), up(gt[:, 0]), up(gt[:, 1]), up(weight), None if scale is None else up(scale)
    out, pe = _guarded(B * 4), _guarded(B * 2 * 778) if point_err else None
    off = GUARD * 8
    rc = hip.lib().ihmr_eval_pa_verts(pr.data_ptr(), pl.data_ptr(), gr.data_ptr(), gl.data_ptr(), w.data_ptr(), None if s is None else s.data_ptr(),
                                      B, out.data_ptr() + off, None if pe is None else pe.data_ptr() + off, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return _take(out, (B, 2, 2)), None if pe is None else _take(pe, (B, 2, 778))


def _check(names, out, pe, ref_out, ref_pe):
    for b, name in enumerate(names):
        for s in range(out.shape[1]):
            d = float(np.abs(pe[b, s] - ref_pe[b, s]).max())
            print(f"[pa] {name} set {s}: count {out[b, s, 1]:.0f} sum {out[b, s, 0]:.6e} max |point_err - statement| {d:.2e}")
            assert d <= TOL, (name, s, d)
            assert out[b, s, 1] == ref_out[b, s, 1], (name, s, out[b, s, 1], ref_out[b, s, 1])
            if ref_out[b, s, 1] == 0:
                assert out[b, s, 0] == 0.0 and not pe[b, s].any(), (name, s)
            assert abs(out[b, s, 0] - pe[b, s].sum()) <= 1e-12 * abs(pe[b, s].sum()), (name, s)
    assert np.isfinite(out).all() and np.isfinite(pe).all()


def test_joint_errors_match_the_float64_statement(joints):
    out, pe = run_joints(joints.pred, joints.gt, joints.scale)
    _check(joints.names, out, pe, joints.out, joints.pe)
    left_out = {n: [int(c) for c in joints.out[joints.names.index(n), :, 1]] for n in
                ("one_valid", "none_valid", "weight_sum_1p5", "coincident_prediction", "two_valid", "three_valid")}
    assert left_out == dict(one_valid=[0, 0, 0], none_valid=[0, 0, 0], weight_sum_1p5=[0, 0, 0], coincident_prediction=[0, 0, 0],
                            two_valid=[2, 0, 0], three_valid=[3, 2, 0]), left_out        # what the table is meant to hold
    i = joints.names.index("two_valid")
    assert pe[i].max() <= TOL                                  # two points are mapped onto their targets
    out_null, _ = run_joints(joints.pred, joints.gt, joints.scale, point_err=False)
    assert out_null.tobytes() == out.tobytes()
    out_1, pe_1 = run_joints(joints.pred[:1], joints.gt[:1])   # B = 1, no scale array
    assert out_1.tobytes() == out[:1].tobytes() and pe_1.tobytes() == pe[:1].tobytes()


def test_joint_errors_do_not_depend_on_the_place_in_the_batch(joints):
    out, pe = run_joints(joints.pred, joints.gt, joints.scale)
    again = run_joints(joints.pred, joints.gt, joints.scale)
    assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == pe.tobytes()
    perm = np.random.RandomState(1).permutation(len(joints.names))
    out_p, pe_p = run_joints(joints.pred[perm], joints.gt[perm], joints.scale[perm])
    assert out_p.tobytes() == out[perm].tobytes() and pe_p.tobytes() == pe[perm].tobytes()


def test_vertex_errors_match_the_float64_statement(verts):
    out, pe = run_verts(verts.pred, verts.gt, verts.weight, verts.scale)
    _check(verts.names, out, pe, verts.out, verts.pe)
    assert [int(c) for c in out[verts.names.index("left_without_annotation"), :, 1]] == [778, 0]
    assert [int(c) for c in out[verts.names.index("right_without_annotation"), :, 1]] == [0, 778]
    out_null, _ = run_verts(verts.pred, verts.gt, verts.weight, verts.scale, point_err=False)
    assert out_null.tobytes() == out.tobytes()
    perm = np.array([3, 0, 4, 2, 1])
    out_p, pe_p = run_verts(verts.pred[perm], verts.gt[perm], verts.weight[perm], verts.scale[perm])
    assert out_p.tobytes() == out[perm].tobytes() and pe_p.tobytes() == pe[perm].tobytes()
    again = run_verts(verts.pred, verts.gt, verts.weight, verts.scale)
    assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == pe.tobytes()
    i = verts.names.index("both_hands")                        # B = 1, no scale array (the case's scale is 1)
    out_1, pe_1 = run_verts(verts.pred[i:i + 1], verts.gt[i:i + 1], verts.weight[i:i + 1])
    assert out_1.tobytes() == out[i:i + 1].tobytes() and pe_1.tobytes() == pe[i:i + 1].tobytes()


def test_refusals_launch_nothing():
    import torch

    from ihmr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    x = torch.zeros(2 * 778 * 3, device="cuda")
    out = torch.full((16,), float("nan"), device="cuda", dtype=torch.float64)
    p, o = x.data_ptr(), out.data_ptr()
    assert L.ihmr_eval_pa_joints(None, p, None, 1, o, None, st) == -1
    assert L.ihmr_eval_pa_joints(p, None, None, 1, o, None, st) == -1
    assert L.ihmr_eval_pa_joints(p, p, None, 1, None, None, st) == -1
    assert L.ihmr_eval_pa_joints(p, p, None, 0, o, None, st) == -1
    assert L.ihmr_eval_pa_joints(p, p, None, -3, o, None, st) == -1
    for k in range(5):
        args = [p, p, p, p, p]
        args[k] = None
        assert L.ihmr_eval_pa_verts(*args, None, 1, o, None, st) == -1
    assert L.ihmr_eval_pa_verts(p, p, p, p, p, None, 1, None, None, st) == -1
    assert L.ihmr_eval_pa_verts(p, p, p, p, p, None, 0, o, None, st) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_device_path_agrees_with_the_host_records(joints, verts):
    """`Evaluator(pa_metrics=True)` records against `update_device_pa` / `update_device_pa_verts` on 9 samples with a keep mask."""
    import torch

    from ihmr_amd.evaluator import Evaluator
    B = 9
    rows = [joints.names.index(n) for n in ("all_42", "right_hand_only_21", "missing_wrist_41", "three_valid", "two_valid", "weight_sum_1p5",
                                            "mirrored", "fractional_weights", "coincident_prediction")]
    vrow = np.arange(B) % len(verts.names)
    keep = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], bool)
    scale = np.float32([1, 1.5, 1, 1, 2, 1, 1, 0.5, 1])
    one_hot = np.zeros(778, np.float32); one_hot[0] = 1.0
    mano = types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=np.stack([one_hot] * 16))
    data_list = {i: dict(scale=float(scale[i])) for i in range(B)}
    res = dict(pred_cam_params=np.zeros((B, 3)), pred_shape_params=np.zeros((B, 20)), pred_pose_params=np.zeros((B, 96)), pred_hand_trans=np.zeros((B, 3)),
               pred_joints_3d=joints.pred[rows], gt_joints_3d=joints.gt[rows], collision_loss_origin_scale=np.zeros((B, 1556), np.float32),
               pred_right_hand_verts=verts.pred[vrow, 0], pred_left_hand_verts=verts.pred[vrow, 1], gt_right_hand_verts=verts.gt[vrow, 0],
               gt_left_hand_verts=verts.gt[vrow, 1], mano_params_weight=verts.weight[vrow])
    host = Evaluator(dict(right=mano, left=mano), data_list=data_list, pa_metrics=True)
    host.update(np.arange(B), res)
    host.pred_results = [r for r, k in zip(host.pred_results, keep) if k]
    dev = Evaluator(dict(right=mano, left=mano))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    k, sc = torch.from_numpy(keep), up(scale)
    dev.update_device_pa(up(res["pred_joints_3d"]), up(res["gt_joints_3d"]), keep=k, scale=sc)
    dev.update_device_pa_verts(up(res["pred_right_hand_verts"]), up(res["pred_left_hand_verts"]), up(res["gt_right_hand_verts"]),
                               up(res["gt_left_hand_verts"]), up(res["mano_params_weight"]), keep=k, scale=sc)
    hs, ds = host.pa_metric_sums(), dev.pa_metric_sums()
    print("[pa] host sums", hs.tolist(), "device sums", ds.tolist())
    assert hs[1] > 0 and hs[3] > 0 and hs[5] > 0
    for i in (1, 3, 5):
        assert hs[i] == ds[i], (i, hs[i], ds[i])
    for i in (0, 2, 4):
        assert abs(hs[i] - ds[i]) <= 1e-9 * abs(hs[i]), (i, hs[i], ds[i])
    for name in ("pa_inter_mpjpe_3d", "pa_mpjpe_3d", "pa_mpvpe_3d"):
        assert abs(getattr(host, name) - getattr(dev, name)) <= 1e-9 * getattr(host, name), name
    assert len(dev.metric_sums()) == 9 and not dev.metric_sums().any()      # the PA parts stay out of the nine sums


def test_a_masked_out_row_without_finite_targets_leaves_every_pa_and_curve_sum_untouched(joints, verts):
    """Padding duplicates are masked out by `keep`; what such a row holds must not reach a sum.  The row here passes the PA set rules
    (a finite, spread-out prediction, weights 1) with GT coordinates of Inf: its aligned errors are NaN, and 0 * NaN is NaN -- `keep`
    is a selection on every part of `update_device_pa`, `update_device_pa_verts`, `update_device_curves`, `update_device_curve_verts`."""
    import torch

    from ihmr_amd.evaluator import Evaluator
    rows = np.flatnonzero(np.isfinite(joints.out).all(axis=(1, 2)) & np.isfinite(joints.pe).all(axis=(1, 2)))[:12]
    assert len(rows) == 12
    vrow = np.arange(12) % 3                                       # three mesh samples
    one_hot = np.zeros(778, np.float32); one_hot[0] = 1.0
    mano = types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=np.stack([one_hot] * 16))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(jp, jg, vp, vg, vw, scale, keep):
        ev = Evaluator(dict(right=mano, left=mano))
        k, sc = None if keep is None else torch.from_numpy(keep), up(scale)
        ev.update_device_pa(up(jp), up(jg), keep=k, scale=sc)
        ev.update_device_pa_verts(up(vp[:, 0]), up(vp[:, 1]), up(vg[:, 0]), up(vg[:, 1]), up(vw), keep=k, scale=sc)
        ev.update_device_curves(up(jp), up(jg), keep=k, scale=sc)
        ev.update_device_curve_verts(up(vp[:, 0]), up(vp[:, 1]), up(vg[:, 0]), up(vg[:, 1]), up(vw), keep=k, scale=sc)
        return ev

    keep = np.ones(12, bool)
    keep[4] = False
    good = (joints.pred[rows], joints.gt[rows], verts.pred[vrow], verts.gt[vrow], verts.weight[vrow], joints.scale[rows])
    bad_gt = np.full((1, 42, 4), np.inf, np.float32)
    bad_gt[..., 3] = 1.0
    bad = (joints.pred[rows[:1]], bad_gt, verts.pred[:1], np.full_like(verts.gt[:1], np.inf), np.ones((1, 2), np.float32), np.ones(1, np.float32))
    # not vacuous: the appended row alone, unmasked, poisons the PA sums
    alone = run(*bad, None).pa_metric_sums()
    print("[pa] the appended row alone:", alone.tolist())
    assert not np.isfinite(alone[0]) and not np.isfinite(alone[2]) and not np.isfinite(alone[4]) and alone[1] == 42 and alone[5] == 2 * 778
    base = run(*good, keep)
    masked = run(*[np.concatenate([a, b]) for a, b in zip(good, bad)], np.concatenate([keep, [False]]))

    def same_plus_a_zero_row(a, b, what):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert len(a) == 12 and len(b) == 13 and b[:-1].tobytes() == a.tobytes() and not b[-1].any() and np.isfinite(b).all(), what
        assert not a[4].any() and a[0].any(), what                # the masked row of the base batch, and a kept one

    for name in ("_device_pa_parts", "_device_pa_vert_parts", "_device_curve_parts"):
        assert len(getattr(base, name)) == len(getattr(masked, name)) == 1
        same_plus_a_zero_row(getattr(base, name)[0], getattr(masked, name)[0], name)
    (csum_a, fc_a, counted_a), (csum_b, fc_b, counted_b) = base._device_curve_vert_parts[0], masked._device_curve_vert_parts[0]
    same_plus_a_zero_row(csum_a, csum_b, "curve vertex counts")
    same_plus_a_zero_row(counted_a, counted_b, "hands counted and kept")
    # the F counts are read only for the hands that `counted` names: the kept rows are the base batch's, the last row is never read
    assert fc_b[:-1].cpu().numpy().tobytes() == fc_a.cpu().numpy().tobytes()
    assert masked.pa_metric_sums().tobytes() == base.pa_metric_sums().tobytes() and np.isfinite(base.pa_metric_sums()).all()
    assert masked.curve_sums().tobytes() == base.curve_sums().tobytes() and np.isfinite(base.curve_sums()).all()
    assert base.pa_metric_sums()[[1, 3, 5]].min() > 0 and base.curve_sums()[100] > 0


def test_run_optimize_pa_metrics_device_and_host_agree():
    """20 samples at batch 8 (padded to 24): the PA values of the device path and of the records agree; without the flag the
    returned dict has exactly the four keys it had before the PA metrics existed, with the values the flagged run reports too."""
    from ihmr_amd import run_optimize
    base = ["--num_samples", "20", "--batchSize", "8", "--opt_epoch", "2", "--save_mid_freq", "1"]
    plain = run_optimize.main(base)
    dev = run_optimize.main(base + ["--pa_metrics"])
    host = run_optimize.main(base + ["--pa_metrics", "--host_eval"])
    assert sorted(plain) == ["collision_ave", "collision_max", "inter_mpjpe_3d", "mpjpe_3d"]
    assert sorted(dev) == sorted(host) == sorted(list(plain) + ["pa_inter_mpjpe_3d", "pa_mpjpe_3d"])
    for k in plain:
        assert dev[k] == plain[k], (k, dev[k], plain[k])
    for k in ("pa_inter_mpjpe_3d", "pa_mpjpe_3d"):
        print(f"[pa] run_optimize {k}: device {dev[k]!r} host {host[k]!r}")
        assert dev[k] > 0 and abs(dev[k] - host[k]) <= 1e-9 * abs(host[k]), (k, dev[k], host[k])

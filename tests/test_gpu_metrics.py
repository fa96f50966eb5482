"""The two oldest evaluator kernels -- ``ihmr_eval_metrics`` (MPJPE, the aligned "inter" MPJPE, collision_ave, collision_max) and
``ihmr_eval_mpvpe`` (csrc/evaluate.h) -- against the float64 statement of tests/metric_cases.py on every case class, and
``Evaluator.update_device`` / ``update_device_verts`` above them.

Counts, NaN positions and the depth maximum are exact, the depth mean is a float64 sum of the same float32 values on both sides
(1e-12 relative).  An error sum is held to the bar of metric_cases.py: per counted point 3 x the largest distance of the reference's own
float32 route (the host functions on the float32 arrays) from the statement over the sample's class, plus one float32 ulp of the
sample's largest |coordinate| / scale.  Every output sits in a guarded buffer pre-filled with 0xFF."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metric_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu


def _aligned_host(pred, gt, w, scale):
    from ihmr_amd import evaluator as EV
    with np.errstate(invalid="ignore", divide="ignore"):
        return EV.get_single_pa_inter_joints_error(pred, gt, w, scale)


def _unit_scale(classes):
    return {c: [dict(s, scale=np.float32(1.0)) for s in ss] for c, ss in classes.items()}


@pytest.fixture(scope="module")
def J():
    from ihmr_amd import evaluator as EV
    classes = MC.joint_classes()
    cls, samples = MC.flatten(classes)
    pred, gt, coll, inter, scale = MC.joint_arrays(samples)
    maxima = {True: MC.joint_class_maxima(classes, EV.get_single_joints_error, _aligned_host),
              False: MC.joint_class_maxima(_unit_scale(classes), EV.get_single_joints_error, _aligned_host)}
    ref = {(ws, wi): np.stack([MC.joints_statement(s["pred"], s["gt"], s["coll"], s["interacting"] if wi else True,
                                                   float(s["scale"]) if ws else 1.0) for s in samples])
           for ws in (True, False) for wi in (True, False)}
    return types.SimpleNamespace(cls=cls, samples=samples, pred=pred, gt=gt, coll=coll, inter=inter, scale=scale, maxima=maxima, ref=ref)


@pytest.fixture(scope="module")
def M(mano_arrays):
    from ihmr_amd import evaluator as EV
    root_w = np.stack([np.asarray(m["J_regressor"])[0] for m in mano_arrays]).astype(np.float32)
    classes = MC.mesh_classes()
    cls, samples = MC.flatten(classes)
    pred, gt, weight, scale = MC.mesh_arrays(samples)
    maxima = {True: MC.mesh_class_maxima(classes, root_w, EV.get_single_verts_error),
              False: MC.mesh_class_maxima(_unit_scale(classes), root_w, EV.get_single_verts_error)}
    ref = {ws: np.array([[MC.verts_statement(s["pred"][h], s["gt"][h], root_w[h], s["weight"][h], float(s["scale"]) if ws else 1.0)
                          for h in range(2)] for s in samples]) for ws in (True, False)}
    return types.SimpleNamespace(cls=cls, samples=samples, pred=pred, gt=gt, weight=weight, scale=scale, root_w=root_w, maxima=maxima, ref=ref)


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _take(out, shape):
    """The float64 payload of a guarded, 0xFF-filled output: the guards intact, every word written."""
    import torch
    assert out.guards_intact() is None, f"guard damaged at payload offset {out.guards_intact()}"
    unwritten = (out.view(torch.int64, shape) == -1).nonzero()
    assert unwritten.numel() == 0, f"output words never written: {unwritten.tolist()[:8]}"
    return out.view(torch.float64, shape).cpu().numpy().copy()


def run_metrics(pred, gt, coll, inter=None, scale=None):
    import torch

    from guarded import Guarded
    from ihmr_amd import hip
    B = len(pred)
    p, g, c = _up(pred), _up(gt), _up(coll)
    s, it = None if scale is None else _up(scale), None if inter is None else _up(inter, np.uint8)
    out = Guarded(B * 6 * 8, fill=0xFF)
    rc = hip.lib().ihmr_eval_metrics(p.data_ptr(), g.data_ptr(), c.data_ptr(), None if s is None else s.data_ptr(),
                                     None if it is None else it.data_ptr(), B, out.data_ptr, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return _take(out, (B, 6))


def run_mpvpe(pred, gt, weight, root_w, scale=None):
    import torch

    from guarded import Guarded
    from ihmr_amd import hip
    B = len(pred)
    pr, pl, gr, gl, w, rw = _up(pred[:, 0]), _up(pred[:, 1]), _up(gt[:, 0]), _up(gt[:, 1]), _up(weight), _up(root_w)
    s = None if scale is None else _up(scale)
    out = Guarded(B * 4 * 8, fill=0xFF)
    rc = hip.lib().ihmr_eval_mpvpe(pr.data_ptr(), pl.data_ptr(), gr.data_ptr(), gl.data_ptr(), rw.data_ptr(), w.data_ptr(),
                                   None if s is None else s.data_ptr(), B, out.data_ptr, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return _take(out, (B, 2, 2))


def joint_bars(s, want, class_max, with_scale):
    al = MC.point_allowance([s["pred"], s["gt"][:, :3]], s["scale"] if with_scale else 1.0)
    return MC.sum_bar(want[1], class_max[0], al), MC.sum_bar(want[3], class_max[1], al)


def check_joints(J, out, with_scale, with_inter, tag):
    ref, maxima = J.ref[(with_scale, with_inter)], J.maxima[with_scale]
    seen, bad = {}, []          # every mismatch of the exact words is collected, so one run names them all
    for b, (cls, s) in enumerate(zip(J.cls, J.samples)):
        got, want = out[b], ref[b]
        if not (got[1] == want[1] and got[3] == want[3]):
            bad.append((s["name"], "counts", got[[1, 3]].tolist(), want[[1, 3]].tolist()))
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            bad.append((s["name"], "NaN positions", got.tolist(), want.tolist()))
            continue
        bars = joint_bars(s, want, maxima[cls], with_scale)
        for k, bar in zip((0, 2), bars):
            if not np.isnan(want[k]) and got[k + 1] == want[k + 1]:
                d = abs(got[k] - want[k])
                r = seen.setdefault((cls, k), [0.0, 0.0])
                r[0], r[1] = max(r[0], d / max(want[k + 1], 1.0)), max(r[1], d / bar if bar > 0 else float(d > 0))
        if not np.isnan(want[4]):
            if not abs(got[4] - want[4]) <= 1e-12 * abs(want[4]):
                bad.append((s["name"], "depth mean", got[4], want[4]))
            if got[5] != want[5]:
                bad.append((s["name"], "depth max", got[5], want[5]))
    for cls in dict.fromkeys(J.cls):
        (dj, rj), (da, ra) = seen.get((cls, 0), (0.0, 0.0)), seen.get((cls, 2), (0.0, 0.0))
        print(f"[parity] eval_metrics {tag} {cls}: float32 route max per point: joint {maxima[cls][0]:.2e} aligned {maxima[cls][1]:.2e}; "
              f"device |sum - statement| per point: joint {dj:.2e} ({rj:.2f} of the bar) aligned {da:.2e} ({ra:.2f} of the bar)")
    assert not bad, (tag, bad)
    assert max(v[1] for v in seen.values()) <= 1.0, (tag, {k: v for k, v in seen.items() if v[1] > 1.0})


@pytest.mark.parametrize("with_scale,with_inter", [(True, True), (True, False), (False, True), (False, False)])
def test_eval_metrics_matches_the_statement_on_every_class(J, with_scale, with_inter):
    out = run_metrics(J.pred, J.gt, J.coll, J.inter if with_inter else None, J.scale if with_scale else None)
    check_joints(J, out, with_scale, with_inter, f"scale={'ptr' if with_scale else 'NULL'} interacting={'ptr' if with_inter else 'NULL'}")


@pytest.mark.parametrize("with_scale", [True, False])
def test_eval_mpvpe_matches_the_statement_on_every_class(M, with_scale):
    out = run_mpvpe(M.pred, M.gt, M.weight, M.root_w, M.scale if with_scale else None)
    ref, maxima, seen = M.ref[with_scale], M.maxima[with_scale], {}
    for b, (cls, s) in enumerate(zip(M.cls, M.samples)):
        for h in range(2):
            got, want = out[b, h], ref[b, h]
            assert got[1] == want[1], (s["name"], h, "count", got.tolist(), want.tolist())
            assert not np.isnan(got).any()
            if want[1] == 0:
                assert got[0] == 0.0, (s["name"], h)
                continue
            bar = MC.sum_bar(want[1], maxima[cls], MC.point_allowance([s["pred"][h], s["gt"][h]], s["scale"] if with_scale else 1.0))
            d = abs(got[0] - want[0])
            r = seen.setdefault(cls, [0.0, 0.0])
            r[0], r[1] = max(r[0], d / want[1]), max(r[1], d / bar)
    for cls, (d, r) in seen.items():
        print(f"[parity] eval_mpvpe scale={'ptr' if with_scale else 'NULL'} {cls}: float32 route max per vertex {maxima[cls]:.2e}; "
              f"device |sum - statement| per vertex {d:.2e} ({r:.2f} of the bar)")
    assert max(r for _, r in seen.values()) <= 1.0, seen
    i = [s["name"] for s in M.samples].index("equal/offset")
    assert out[i, :, 0].tolist() == [0.0, 0.0] and out[i, :, 1].tolist() == [778.0, 778.0]


def test_a_sample_does_not_depend_on_its_place_in_the_batch(J, M):
    n = len(J.samples)
    rows = MC.big_batch_rows(n)
    big = run_metrics(J.pred[rows], J.gt[rows], J.coll[rows], J.inter[rows], J.scale[rows])
    single = [run_metrics(J.pred[i:i + 1], J.gt[i:i + 1], J.coll[i:i + 1], J.inter[i:i + 1], J.scale[i:i + 1]) for i in range(n)]
    for r, i in enumerate(rows):
        assert big[r].tobytes() == single[i][0].tobytes(), (r, J.samples[i]["name"], big[r].tolist(), single[i][0].tolist())
    n = len(M.samples)
    rows = MC.big_batch_rows(n)
    big = run_mpvpe(M.pred[rows], M.gt[rows], M.weight[rows], M.root_w, M.scale[rows])
    single = [run_mpvpe(M.pred[i:i + 1], M.gt[i:i + 1], M.weight[i:i + 1], M.root_w, M.scale[i:i + 1]) for i in range(n)]
    for r, i in enumerate(rows):
        assert big[r].tobytes() == single[i][0].tobytes(), (r, M.samples[i]["name"])


def test_refusals_launch_nothing():
    import torch

    from ihmr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    x = torch.zeros(2 * 778 * 3, device="cuda")
    out = torch.full((16,), float("nan"), device="cuda", dtype=torch.float64)
    p, o = x.data_ptr(), out.data_ptr()
    for k in range(3):
        args = [p, p, p]
        args[k] = None
        assert L.ihmr_eval_metrics(*args, None, None, 1, o, st) != 0
    assert L.ihmr_eval_metrics(p, p, p, None, None, 1, None, st) != 0
    for B in (0, -3):
        assert L.ihmr_eval_metrics(p, p, p, None, None, B, o, st) != 0
        assert L.ihmr_eval_mpvpe(p, p, p, p, p, p, None, B, o, st) != 0
    for k in range(6):
        args = [p, p, p, p, p, p]
        args[k] = None
        assert L.ihmr_eval_mpvpe(*args, None, 1, o, st) != 0
    assert L.ihmr_eval_mpvpe(p, p, p, p, p, p, None, 1, None, st) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------------------------ the Evaluator above the kernels
def _mano(root_w):
    jr = lambda h: np.concatenate([root_w[h][None], np.zeros((15, MC.NV), np.float32)])
    return dict(right=types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=jr(0)),
                left=types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=jr(1)))


def _device_sums(J, rows, keep):
    import torch

    from ihmr_amd.evaluator import Evaluator
    dev = Evaluator()
    dev.update_device(_up(J.pred[rows]), _up(J.gt[rows]), _up(J.coll[rows]), keep=torch.from_numpy(keep), interacting=torch.from_numpy(J.inter[rows].astype(bool)),
                      scale=_up(J.scale[rows]))
    return dev


def test_update_device_sums_the_statement_rows_under_a_keep_mask(J):
    from ihmr_amd.evaluator import Evaluator
    ref = J.ref[(True, True)]
    n = len(J.samples)
    finite = ~np.isnan(ref).any(axis=1)
    assert 0 < (~finite).sum() < n
    for tag, keep in (("finite rows", finite & (np.arange(n) % 7 != 3)), ("every row", np.ones(n, bool))):
        got = _device_sums(J, np.arange(n), keep).metric_sums()
        want = np.concatenate([ref[keep].sum(axis=0), [float(np.sum(J.inter[keep] != 0))], [0.0, 0.0]])
        print(f"[parity] update_device, {tag}: device sums {got.tolist()} statement {want.tolist()}")
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, got, want)
        assert got[1] == want[1] and got[3] == want[3] and got[6] == want[6] and got[7:].tolist() == [0.0, 0.0], (tag, got, want)
        if tag == "every row":
            assert np.isnan(want[[2, 4, 5]]).all() and not np.isnan(want[0])
            continue
        bars = np.array([joint_bars(s, ref[b], J.maxima[True][c], True) for b, (c, s) in enumerate(zip(J.cls, J.samples))])
        assert abs(got[0] - want[0]) <= bars[keep, 0].sum() and abs(got[2] - want[2]) <= bars[keep, 1].sum(), (got, want, bars[keep].sum(axis=0))
        assert abs(got[4] - want[4]) <= 1e-12 * want[4] and abs(got[5] - want[5]) <= 1e-12 * want[5], (got, want)
        # the four printed numbers: the device path against the host Evaluator on the same kept samples (float32 arrays, its own route)
        host = Evaluator(data_list={i: dict(scale=float(s["scale"]), hand_type="interacting" if s["interacting"] else "right") for i, s in enumerate(J.samples)})
        idx = np.flatnonzero(keep)
        z = lambda *shape: np.zeros((len(idx),) + shape)
        host.update(idx, dict(pred_cam_params=z(3), pred_shape_params=z(20), pred_pose_params=z(96), pred_hand_trans=z(3),
                              pred_joints_3d=J.pred[idx], gt_joints_3d=J.gt[idx], collision_loss_origin_scale=J.coll[idx]))
        m_host, m_dev = Evaluator.metrics_from_sums(host.metric_sums()), Evaluator.metrics_from_sums(got)
        route = np.array([[ref[b, 1] * J.maxima[True][c][0], ref[b, 3] * J.maxima[True][c][1]] for b, c in enumerate(J.cls)])
        assert abs(m_dev["mpjpe_3d"] - m_host["mpjpe_3d"]) <= (bars[keep, 0].sum() + route[keep, 0].sum()) / want[1]
        assert abs(m_dev["inter_mpjpe_3d"] - m_host["inter_mpjpe_3d"]) <= (bars[keep, 1].sum() + route[keep, 1].sum()) / want[3]
        for k in ("collision_ave", "collision_max"):
            assert abs(m_dev[k] - m_host[k]) <= 1e-12 * abs(m_host[k]), (k, m_dev[k], m_host[k])
            assert m_dev[k] == getattr(_device_sums(J, np.arange(n), keep), k)


def test_a_masked_out_row_of_nan_leaves_every_sum_untouched(J, M):
    """Padding duplicates are masked out by `keep`; what such a row holds -- NaN, Inf -- must not reach a sum."""
    import torch

    from ihmr_amd.evaluator import Evaluator
    ref = J.ref[(True, True)]
    rows = np.flatnonzero(~np.isnan(ref).any(axis=1))[:12]
    keep = np.ones(len(rows), bool)
    keep[4] = False
    base = _device_sums(J, rows, keep)
    bad = types.SimpleNamespace(pred=np.concatenate([J.pred[rows], np.full((1, 42, 3), np.nan, np.float32)]),
                                gt=np.concatenate([J.gt[rows], np.full((1, 42, 4), np.inf, np.float32)]),
                                coll=np.concatenate([J.coll[rows], np.full((1, MC.ND), np.nan, np.float32)]),
                                inter=np.concatenate([J.inter[rows], [1]]).astype(np.uint8), scale=np.concatenate([J.scale[rows], [np.float32(1.0)]]))
    bad.gt[-1, :, 3] = 1.0
    masked = _device_sums(bad, np.arange(len(rows) + 1), np.concatenate([keep, [False]]))
    a, b = base._device_parts[0].cpu().numpy(), masked._device_parts[0].cpu().numpy()
    assert b[:-1].tobytes() == a.tobytes() and not b[-1].any() and not np.isnan(b).any(), b[-1]
    assert masked.metric_sums().tobytes() == base.metric_sums().tobytes(), (masked.metric_sums(), base.metric_sums())
    # the same for the meshes
    idx = [i for i, s in enumerate(M.samples) if s["name"].split("/")[0] in ("plain", "scaled", "hand_weight")]
    keep = np.ones(len(idx), bool)
    keep[1] = False

    def verts(pred, gt, weight, scale, keep):
        dev = Evaluator(_mano(M.root_w))
        dev.update_device_verts(_up(pred[:, 0]), _up(pred[:, 1]), _up(gt[:, 0]), _up(gt[:, 1]), _up(weight), keep=torch.from_numpy(keep), scale=_up(scale))
        return dev

    base = verts(M.pred[idx], M.gt[idx], M.weight[idx], M.scale[idx], keep)
    nan_mesh = np.full((1, 2, MC.NV, 3), np.nan, np.float32)
    masked = verts(np.concatenate([M.pred[idx], nan_mesh]), np.concatenate([M.gt[idx], np.full_like(nan_mesh, np.inf)]),
                   np.concatenate([M.weight[idx], np.ones((1, 2), np.float32)]), np.concatenate([M.scale[idx], [np.float32(1.0)]]), np.concatenate([keep, [False]]))
    a, b = base._device_vert_parts[0].cpu().numpy(), masked._device_vert_parts[0].cpu().numpy()
    assert b[:-1].tobytes() == a.tobytes() and not b[-1].any(), b[-1]
    assert masked.metric_sums().tobytes() == base.metric_sums().tobytes() and base.metric_sums()[8] > 0


def test_update_device_verts_sums_the_statement_rows_under_a_keep_mask(M):
    import torch

    from ihmr_amd.evaluator import Evaluator
    n = len(M.samples)
    keep = np.arange(n) % 5 != 2
    dev = Evaluator(_mano(M.root_w))
    dev.update_device_verts(_up(M.pred[:, 0]), _up(M.pred[:, 1]), _up(M.gt[:, 0]), _up(M.gt[:, 1]), _up(M.weight), keep=torch.from_numpy(keep), scale=_up(M.scale))
    got, ref = dev.metric_sums(), M.ref[True]
    want = ref[keep].sum(axis=(0, 1))
    bars = np.array([[MC.sum_bar(ref[b, h, 1], M.maxima[True][c], MC.point_allowance([s["pred"][h], s["gt"][h]], s["scale"])) for h in range(2)]
                     for b, (c, s) in enumerate(zip(M.cls, M.samples))])
    print(f"[parity] update_device_verts: device sums {got[7:].tolist()} statement {want.tolist()} bar {bars[keep].sum():.3e}")
    assert got[8] == want[1] > 0 and not got[:7].any()
    assert abs(got[7] - want[0]) <= bars[keep].sum(), (got[7], want[0], bars[keep].sum())
    host = Evaluator(_mano(M.root_w), data_list={i: dict(scale=float(s["scale"])) for i, s in enumerate(M.samples)})
    idx = np.flatnonzero(keep)
    z = lambda *shape: np.zeros((len(idx),) + shape)
    host.update(idx, dict(pred_cam_params=z(3), pred_shape_params=z(20), pred_pose_params=z(96), pred_hand_trans=z(3), pred_joints_3d=z(42, 3),
                          gt_joints_3d=z(42, 4), collision_loss_origin_scale=z(MC.ND), pred_right_hand_verts=M.pred[idx, 0], pred_left_hand_verts=M.pred[idx, 1],
                          gt_right_hand_verts=M.gt[idx, 0], gt_left_hand_verts=M.gt[idx, 1], mano_params_weight=M.weight[idx]))
    assert abs(dev.mpvpe_3d - host.mpvpe_3d) <= (bars[keep].sum() + 1e-9 * want[0]) / want[1], (dev.mpvpe_3d, host.mpvpe_3d)
    assert dev.mpvpe_3d == Evaluator.metrics_from_sums(got)["mpvpe_3d"]

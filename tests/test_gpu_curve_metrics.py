"""The curve metrics on the device (``ihmr_eval_curve_joints`` / ``ihmr_eval_curve_verts``, csrc/evaluate.h + csrc/eval_pure.h) against
the float64 numpy statement of tests/curve_cases.py, and the paths above them: ``Evaluator.update_device_curves`` /
``update_device_curve_verts`` against the host records, ``run_optimize --curve_metrics`` with and without ``--host_eval``.

COUNTS are compared exactly.  That is a fair demand because every statement value lies >= 1e-8 from every threshold it meets
(tests/test_curve_metrics_cpu.py asserts it on every case and table), and a device value lies within 1e-9 of the statement's: the
inputs are the same float32 numbers, both sides work in float64, the alignments agree to ~1e-14 (tests/pa_cases.py).  The per-point
errors have no output of their own; they are bracketed: with the table {e - 1e-9, e + 1e-9 : e a statement error} the device counts
equal the statement's only if every device error lies inside its bracket.  Both kernels work per sample / per hand: B = 1, 3, 5."""
import itertools
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import curve_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = CC.TOL
GUARD = 64          # NaN-filled doubles on either side of every output
NV = CC.NV
GENERIC_T, GENERIC_F = (1, 2, 64, 65, 256), (0, 1, 2, 8)


def _chunks(n):
    """A batch of n in launches of 5, 3 and 1 samples."""
    out, at = [], 0
    while at < n:
        size = 5 if n - at >= 5 else 3 if n - at >= 3 else 1
        out.append(slice(at, at + size))
        at += size
    return out


@pytest.fixture(scope="module")
def joints():
    names, pred, gt, scale = CC.joint_batch()
    return types.SimpleNamespace(names=names, pred=pred, gt=gt, scale=scale, ref=CC.joint_reference())


@pytest.fixture(scope="module")
def verts():
    names, pred, gt, weight, scale = CC.vert_batch()
    return types.SimpleNamespace(names=names, pred=pred, gt=gt, weight=weight, scale=scale, ref=CC.vert_reference())


def _guarded(n, fill=float("nan")):
    import torch
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda", dtype=torch.float64)
    buf[GUARD:GUARD + n] = fill
    return buf


def _take(buf, shape):
    """The payload of a guarded buffer; asserts both guard regions still hold NaN."""
    import torch
    n = int(np.prod(shape))
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), "a guard region was written"
    return buf[GUARD:GUARD + n].cpu().numpy().reshape(shape)


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def run_joints(pred, gt, scale, thr):
    import torch

    from ihmr_amd import hip
    B, T = pred.shape[0], len(thr)
    p, g, s, t = _up(pred), _up(gt), None if scale is None else _up(scale), _up(thr, np.float64)
    out = _guarded(B * 3 * (T + 1))
    rc = hip.lib().ihmr_eval_curve_joints(p.data_ptr(), g.data_ptr(), None if s is None else s.data_ptr(), B, t.data_ptr(), T,
                                          out.data_ptr() + GUARD * 8, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = _take(out, (B, 3, T + 1))
    assert not np.isnan(got).any()
    return got


def run_verts(pred, gt, weight, scale, thr, fthr, nn=True):
    """counts (B,2,2,T+1), f_counts (B,2,2,2,F), nn_dist (B,2,2,2,778) or None; every output NaN-prefilled between guards."""
    import torch

    from ihmr_amd import hip
    B, T, F = pred.shape[0], len(thr), len(fthr)
    pr, pl, gr, gl, w = _up(pred[:, 0]), _up(pred[:, 1]), _up(gt[:, 0]), _up(gt[:, 1]), _up(weight)
    s, t, ft, rw = None if scale is None else _up(scale), _up(thr, np.float64), _up(np.asarray(fthr), np.float64) if F else None, _up(CC.root_weights())
    counts, fc, nd = _guarded(B * 4 * (T + 1)), _guarded(B * 8 * F), _guarded(B * 8 * NV) if nn else None
    off = GUARD * 8
    rc = hip.lib().ihmr_eval_curve_verts(pr.data_ptr(), pl.data_ptr(), gr.data_ptr(), gl.data_ptr(), rw.data_ptr(), w.data_ptr(),
                                         None if s is None else s.data_ptr(), B, t.data_ptr(), T, None if ft is None else ft.data_ptr(), F,
                                         counts.data_ptr() + off, fc.data_ptr() + off if F else None, None if nd is None else nd.data_ptr() + off,
                                         hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = _take(counts, (B, 2, 2, T + 1)), _take(fc, (B, 2, 2, 2, F)), None if nd is None else _take(nd, (B, 2, 2, 2, NV))
    assert all(x is None or not np.isnan(x).any() for x in got), "an output was not fully written"
    return got


def _joint_counts(joints, rows, thr):
    return np.stack([np.stack([np.concatenate([CC.counts_of(e, thr), [len(e)]]) for e in joints.ref[b]]) for b in rows])


def _vert_counts(verts, rows, thr, fthr):
    both = [[CC.hand_counts(verts.ref[b][h], thr, fthr) for h in range(2)] for b in rows]
    return np.array([[c for c, _ in row] for row in both]), np.array([[f for _, f in row] for row in both]).reshape(len(both), 2, 2, 2, len(fthr))


# ------------------------------------------------------------------------------------------------------------------ joints
def test_joint_counts_equal_the_statement(joints):
    n = len(joints.names)
    for T in GENERIC_T:
        thr = CC.pck_table(T)
        for sl in _chunks(n):
            got = run_joints(joints.pred[sl], joints.gt[sl], joints.scale[sl], thr)
            want = _joint_counts(joints, range(n)[sl], thr)
            assert np.array_equal(got, want), (T, [joints.names[b] for b in range(n)[sl]], np.argwhere(got != want)[:5])
    rows = [joints.names.index(c) for c in CC.DEFAULT_JOINT_CASES]
    for b in rows:                                                                 # the default table, B = 1
        got = run_joints(joints.pred[b:b + 1], joints.gt[b:b + 1], joints.scale[b:b + 1], CC.DEFAULT_TABLE)
        assert np.array_equal(got, _joint_counts(joints, [b], CC.DEFAULT_TABLE)), joints.names[b]
    # known answer: an error EQUAL to a threshold counts, and the device's error IS the dyadic number (one ulp less would not count it)
    b = joints.names.index("dyadic")
    got = run_joints(joints.pred[b:b + 1], joints.gt[b:b + 1], None, CC.KNOWN_TABLE)
    assert np.array_equal(got, _joint_counts(joints, [b], CC.KNOWN_TABLE)) and np.array_equal(got[0, 0], [2, 2, 42, 42, 42, 42])
    got = run_joints(joints.pred[b:b + 1], joints.gt[b:b + 1], None, np.array([np.nextafter(CC.KNOWN, 0.0), CC.KNOWN]))
    assert np.array_equal(got[0, 0], [2, 42, 42])


def test_joint_errors_lie_within_1e_9_of_the_statement(joints):
    finer = True
    for b, name in enumerate(joints.names):
        e = np.unique(np.concatenate(joints.ref[b]))
        if not len(e):
            continue
        for band in (TOL, 1e-12):
            thr = np.unique(np.concatenate([e - band, e + band]))
            assert len(thr) <= 256 and (np.diff(thr) > 0).all()
            got = run_joints(joints.pred[b:b + 1], joints.gt[b:b + 1], joints.scale[b:b + 1], thr)
            same = np.array_equal(got, _joint_counts(joints, [b], thr))
            if band == TOL:
                assert same, name
            else:
                finer = finer and same
    print(f"[curves] joint populations: every device error within 1e-9 of the statement; within 1e-12 on every case: {finer}")


def test_joint_counts_do_not_depend_on_the_place_in_the_batch(joints):
    thr = CC.pck_table(65)
    rows = np.array([joints.names.index(c) for c in ("all_42", "missing_wrist_41", "dyadic", "all_42", "three_valid")])   # one case twice
    got = run_joints(joints.pred[rows], joints.gt[rows], joints.scale[rows], thr)
    assert got[0].tobytes() == got[3].tobytes() and np.array_equal(got, _joint_counts(joints, rows, thr))
    perm = np.array([4, 2, 0, 3, 1])
    got_p = run_joints(joints.pred[rows[perm]], joints.gt[rows[perm]], joints.scale[rows[perm]], thr)
    assert got_p.tobytes() == got[perm].tobytes()
    assert run_joints(joints.pred[rows], joints.gt[rows], joints.scale[rows], thr).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------------------------ vertices
def test_vertex_counts_equal_the_statement(verts):
    n = len(verts.names)
    for T, F in itertools.product(GENERIC_T, GENERIC_F):
        thr, fthr = CC.pck_table(T), CC.F_TABLES[F]
        for sl in _chunks(n):
            counts, fc, _ = run_verts(verts.pred[sl], verts.gt[sl], verts.weight[sl], verts.scale[sl], thr, fthr, nn=(T == 64))
            want_c, want_f = _vert_counts(verts, range(n)[sl], thr, fthr)
            where = (T, F, [verts.names[b] for b in range(n)[sl]])
            assert np.array_equal(counts, want_c), where + (np.argwhere(counts != want_c)[:5],)
            assert np.array_equal(fc, want_f), where + (np.argwhere(fc != want_f)[:5],)
    for name in CC.DEFAULT_VERT_CASES:                                             # the default tables, B = 1
        b = verts.names.index(name)
        counts, fc, _ = run_verts(verts.pred[b:b + 1], verts.gt[b:b + 1], verts.weight[b:b + 1], verts.scale[b:b + 1], CC.DEFAULT_TABLE, CC.F_TABLES[2])
        want_c, want_f = _vert_counts(verts, [b], CC.DEFAULT_TABLE, CC.F_TABLES[2])
        assert np.array_equal(counts, want_c) and np.array_equal(fc, want_f), name
    # what the table is meant to hold, as the device sees it
    counts, fc, _ = run_verts(verts.pred[4:], verts.gt[4:], verts.weight[4:], verts.scale[4:], CC.pck_table(2), CC.F_TABLES[8])     # B = 5
    at = {name: k for k, name in enumerate(verts.names[4:])}
    assert counts[at["coincident_prediction"], :, 0, 2].tolist() == [NV, NV] and not counts[at["coincident_prediction"], :, 1].any()
    assert not fc[at["coincident_prediction"], :, 1].any() and fc[at["coincident_prediction"], :, 0].any()
    assert (fc[at["identical"]] == NV).all()                                       # every distance below every threshold: F = 1
    assert not fc[at["far_apart"]].any() and counts[at["far_apart"], 1, :, 2].tolist() == [NV, NV]      # P + R = 0: F = 0
    assert not counts[at["far_apart"], 0].any() and not counts[at["dyadic"], 1].any()                   # a hand with weight 0


def test_known_answer_distances_are_exact_and_a_distance_on_a_threshold_does_not_count(verts):
    b = verts.names.index("dyadic")
    counts, fc, nd = run_verts(verts.pred[b:b + 1], verts.gt[b:b + 1], verts.weight[b:b + 1], None, CC.KNOWN_TABLE, CC.KNOWN_F_TABLE)
    want = np.full(NV, CC.KNOWN)
    want[0] = 0.0
    assert np.array_equal(nd[0, 0, 0, 0], want) and np.array_equal(nd[0, 0, 0, 1], want)
    assert np.array_equal(counts[0, 0, 0], [1, 1, NV, NV, NV, NV])                 # PCK: an error EQUAL to a threshold counts
    assert np.array_equal(fc[0, 0, 0], [[1, 1, NV], [1, 1, NV]])                   # F: a distance EQUAL to a threshold does not
    want_c, want_f = _vert_counts(verts, [b], CC.KNOWN_TABLE, CC.KNOWN_F_TABLE)
    assert np.array_equal(counts, want_c) and np.array_equal(fc, want_f)
    assert not nd[0, 1].any() and not fc[0, 1].any() and not counts[0, 1].any()    # the left hand has no annotation
    i = verts.names.index("identical")
    _, _, nd = run_verts(verts.pred[i:i + 1], verts.gt[i:i + 1], verts.weight[i:i + 1], verts.scale[i:i + 1], CC.pck_table(1), ())
    assert not nd[0, :, 0].any() and nd[0, :, 1].max() <= TOL                      # identical meshes: every raw distance is 0


def test_distances_and_vertex_errors_lie_within_1e_9_of_the_statement(verts):
    n = len(verts.names)
    worst = 0.0
    for sl in _chunks(n):
        _, _, nd = run_verts(verts.pred[sl], verts.gt[sl], verts.weight[sl], verts.scale[sl], CC.pck_table(1), ())      # F = 0: the distances alone
        for k, b in enumerate(range(n)[sl]):
            for h in range(2):
                d = float(np.abs(nd[k, h] - verts.ref[b][h]["nn"]).max())
                print(f"[curves] {verts.names[b]} hand {h}: max |nn_dist - statement| {d:.2e} (largest distance {verts.ref[b][h]['nn'].max():.3e})")
                assert d <= TOL, (verts.names[b], h, d)
                worst = max(worst, d)
    print(f"[curves] nn_dist: max |device - statement| over all cases {worst:.2e}")
    finer = True
    for b, name in enumerate(verts.names):                                         # the two error populations, bracketed 128 errors a launch
        for h in range(2):
            st = verts.ref[b][h]
            for k, on in enumerate((st["counted"], st["pa_kept"])):
                e = np.unique(st["err"][k]) if on else []
                for at in range(0, len(e), 128):
                    for band in (TOL, 1e-12):
                        thr = np.unique(np.concatenate([e[at:at + 128] - band, e[at:at + 128] + band]))
                        counts, _, _ = run_verts(verts.pred[b:b + 1], verts.gt[b:b + 1], verts.weight[b:b + 1], verts.scale[b:b + 1], thr, (), nn=False)
                        same = np.array_equal(counts[0, h, k], np.concatenate([CC.counts_of(st["err"][k], thr), [NV]]))
                        if band == TOL:
                            assert same, (name, h, k, at)
                        else:
                            finer = finer and same
    print(f"[curves] vertex populations: every device error within 1e-9 of the statement; within 1e-12 on every case: {finer}")


def test_vertex_results_do_not_depend_on_place_or_on_the_optional_output(verts):
    thr, fthr = CC.pck_table(65), CC.F_TABLES[8]
    rows = np.array([verts.names.index(c) for c in ("both_hands", "coincident_prediction", "left_without_annotation", "both_hands", "far_apart")])
    args = lambda r: (verts.pred[r], verts.gt[r], verts.weight[r], verts.scale[r], thr, fthr)
    counts, fc, nd = run_verts(*args(rows))
    assert counts[0].tobytes() == counts[3].tobytes() and fc[0].tobytes() == fc[3].tobytes() and nd[0].tobytes() == nd[3].tobytes()
    perm = np.array([2, 4, 1, 0, 3])
    counts_p, fc_p, nd_p = run_verts(*args(rows[perm]))
    assert counts_p.tobytes() == counts[perm].tobytes() and fc_p.tobytes() == fc[perm].tobytes() and nd_p.tobytes() == nd[perm].tobytes()
    counts_0, fc_0, none = run_verts(*args(rows), nn=False)                        # nn_dist = NULL: the same counts
    assert none is None and counts_0.tobytes() == counts.tobytes() and fc_0.tobytes() == fc.tobytes()
    again = run_verts(*args(rows))
    assert again[0].tobytes() == counts.tobytes() and again[1].tobytes() == fc.tobytes() and again[2].tobytes() == nd.tobytes()


def test_sample_scale_against_prescaled_thresholds(joints, verts):
    """A dyadic scale: err / s <= tau and err <= tau * s are the same comparison, bit for bit."""
    for s in (0.5, 4.0):
        thr, fthr = CC.pck_table(64), np.array(CC.F_TABLES[8])
        rows = slice(0, 5)
        sc = np.full(5, s, np.float32)
        assert run_joints(joints.pred[rows], joints.gt[rows], sc, thr).tobytes() == run_joints(joints.pred[rows], joints.gt[rows], None, thr * s).tobytes()
        a = run_verts(verts.pred[rows], verts.gt[rows], verts.weight[rows], sc, thr, fthr)
        b = run_verts(verts.pred[rows], verts.gt[rows], verts.weight[rows], None, thr * s, fthr * s)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (a[2] * s).tobytes() == b[2].tobytes()
        assert a[1].any() and a[0][..., :-1].any()


def test_refusals_launch_nothing():
    import torch

    from ihmr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    x = torch.zeros(2 * NV * 3, device="cuda")
    thr = torch.tensor([0.01, 0.02], device="cuda", dtype=torch.float64)
    outs = [torch.full((8 * NV + 64,), float("nan"), device="cuda", dtype=torch.float64) for _ in range(3)]
    p, t, (o, fo, nd) = x.data_ptr(), thr.data_ptr(), [b.data_ptr() for b in outs]
    J = L.ihmr_eval_curve_joints
    assert J(None, p, None, 1, t, 2, o, st) == -1 and J(p, None, None, 1, t, 2, o, st) == -1
    assert J(p, p, None, 1, None, 2, o, st) == -1 and J(p, p, None, 1, t, 2, None, st) == -1
    for B, T in ((0, 2), (-3, 2), (1, 0), (1, -1), (1, 257)):
        assert J(p, p, None, B, t, T, o, st) == -1, (B, T)
    V = L.ihmr_eval_curve_verts
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert V(*args, None, 1, t, 2, t, 2, o, fo, nd, st) == -1, k
    assert V(*[p] * 6, None, 1, None, 2, t, 2, o, fo, nd, st) == -1 and V(*[p] * 6, None, 1, t, 2, t, 2, None, fo, nd, st) == -1
    for B, T, F in ((0, 2, 2), (-1, 2, 2), (1, 0, 2), (1, 257, 2), (1, 2, -1), (1, 2, 9)):
        assert V(*[p] * 6, None, B, t, T, t, F, o, fo, nd, st) == -1, (B, T, F)
    assert V(*[p] * 6, None, 1, t, 2, None, 2, o, fo, nd, st) == -1               # F > 0 needs its table ...
    assert V(*[p] * 6, None, 1, t, 2, t, 2, o, None, nd, st) == -1                # ... and its output
    torch.cuda.synchronize()
    assert all(torch.isnan(b).all() for b in outs)
    from ihmr_amd.evaluator import Evaluator
    with pytest.raises(ValueError):                                               # device contents cannot be checked by the library: Python does
        Evaluator(thresholds=[0.02, 0.01])


# ------------------------------------------------------------------------------------------------------------------ Evaluator, runner
def test_device_path_equals_the_host_records_element_for_element():
    """A masked batch with GT meshes: `curve_sums()` of the device path and of the records are the same vector, so every metric of
    `curve_metrics_from_sums` is bit-equal -- the collision AUCs, taken from `update_device`'s columns, included."""
    import torch

    from ihmr_amd.evaluator import Evaluator
    res, data_list, keep = CC.evaluator_batch()
    thr, fthr = CC.pck_table(CC.EVAL_T), CC.F_TABLES[CC.EVAL_F]
    B = len(keep)
    host = Evaluator(CC.mano_models(), data_list=data_list, curve_metrics=True, thresholds=thr, f_thresholds=fthr)
    host.update(np.arange(B), {k: v.copy() for k, v in res.items()})
    host.pred_results = [r for r, k in zip(host.pred_results, keep) if k]
    dev = Evaluator(CC.mano_models(), curve_metrics=True, thresholds=thr, f_thresholds=fthr)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    k, sc = torch.from_numpy(keep), up(np.float32([data_list[b]["scale"] for b in range(B)]))
    inter = torch.tensor([data_list[b]["hand_type"] == "interacting" for b in range(B)])
    dev.update_device(up(res["pred_joints_3d"]), up(res["gt_joints_3d"]), up(res["collision_loss_origin_scale"]), keep=k, interacting=inter, scale=sc)
    dev.update_device_curves(up(res["pred_joints_3d"]), up(res["gt_joints_3d"]), keep=k, scale=sc)
    dev.update_device_curve_verts(up(res["pred_right_hand_verts"]), up(res["pred_left_hand_verts"]), up(res["gt_right_hand_verts"]),
                                  up(res["gt_left_hand_verts"]), up(res["mano_params_weight"]), keep=k, scale=sc)
    hs, ds = host.curve_sums(), dev.curve_sums()
    assert np.array_equal(hs, CC.expected_curve_sums(thr, fthr))
    assert hs.tobytes() == ds.tobytes(), np.nonzero(hs != ds)
    hm, dm = Evaluator.curve_metrics_from_sums(hs, thr, fthr), Evaluator.curve_metrics_from_sums(ds, thr, fthr)
    assert sorted(hm) == sorted(dm) and len(hm) == 14
    for name in hm:
        assert np.asarray(hm[name]).tobytes() == np.asarray(dm[name]).tobytes(), name
        assert not np.isnan(hm[name]).any(), name
        print(f"[curves] {name}: {np.asarray(hm[name]).ravel()[:4]}")
    assert len(dev.metric_sums()) == 9 and len(dev.pa_metric_sums()) == 6 and not dev.pa_metric_sums().any()     # the curve parts stay out of both
    dev.clear()
    assert not dev.curve_sums().any()


def test_run_optimize_curve_metrics_device_and_host_agree():
    """20 samples at batch 8 (padded to 24): the curve metrics of the device path and of the records agree; without the flag the
    returned dict has exactly the four keys it had before."""
    from ihmr_amd import run_optimize
    base = ["--num_samples", "20", "--batchSize", "8", "--opt_epoch", "2", "--save_mid_freq", "1"]
    plain = run_optimize.main(base)
    dev = run_optimize.main(base + ["--curve_metrics"])
    host = run_optimize.main(base + ["--curve_metrics", "--host_eval"])
    assert sorted(plain) == ["collision_ave", "collision_max", "inter_mpjpe_3d", "mpjpe_3d"]
    aucs = ["auc_j3d", "auc_pa_inter_j3d", "auc_pa_j3d", "collision_auc_ave", "collision_auc_max"]
    curves = ["pck_j3d", "pck_pa_inter_j3d", "pck_pa_j3d"]
    assert sorted(dev) == sorted(host) == sorted(list(plain) + aucs + curves)      # IHMR-OPT exports no GT meshes: no vertex metric
    for k in plain:
        assert dev[k] == plain[k], (k, dev[k], plain[k])
    for k in aucs:
        print(f"[curves] run_optimize {k}: device {dev[k]!r} host {host[k]!r}")
        assert 0 <= dev[k] <= 1 and abs(dev[k] - host[k]) <= 1e-9, (k, dev[k], host[k])
    for k in curves:
        assert len(dev[k]) == 100 and np.abs(np.asarray(dev[k]) - np.asarray(host[k])).max() <= 1e-9 and dev[k][-1] > 0, k

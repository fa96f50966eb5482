"""The curve metrics without a GPU: ``calc_collision_auc`` against the reference's recorded results (tests/golden/metrics_curves.npz),
the host functions of ihmr_amd/evaluator.py against the float64 statement of tests/curve_cases.py, the known answers, the margin
condition of every case, the Evaluator's records and sums, the curve helpers of csrc/eval_pure.h built for the host with ASan / UBSan
(tests/eval_curve_driver.cpp), and the build: both kernels without scratch memory, every declared symbol exported."""
import math
import os
import pickle
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj  # noqa: E402
import curve_cases as CC  # noqa: E402
import hostbuild  # noqa: E402

from ihmr_amd import evaluator as E  # noqa: E402

GENERIC_T, GENERIC_F = (1, 2, 64, 65, 256), (0, 1, 2, 8)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "metrics_curves.npz")))


# ------------------------------------------------------------------------------------------------------------------ collision AUC
def test_collision_auc_equals_the_reference_to_the_last_bit(golden):
    names = list(golden["names"])
    assert names == list(CC.collision_cases()) and len(names) >= 10
    thr = E.COLLISION_AUC_THRESHOLDS
    assert np.array_equal(thr, np.linspace(0.5, 15)) and len(thr) == 50
    for name in names:
        for kind in ("32", "64"):
            x, want = golden[f"{name}_in{kind}"], golden[f"{name}_auc{kind}"]
            assert x.dtype == (np.float32 if kind == "32" else np.float64)
            got = E.calc_collision_auc(x)
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (name, kind, got, want)
            # the additive route: strict counts of two halves, summed, then the integral
            h = len(x) // 2
            counts = E.curve_counts(x[:h], thr, strict=True) + E.curve_counts(x[h:], thr, strict=True)
            assert abs(E.curve_auc(counts, len(x), thr) - want) <= 1e-12, (name, kind)
    # a value EQUAL to a threshold is not below it
    x = golden["on_thresholds_in64"]
    assert x[0] == thr[0] and x[1] == thr[7] and E.curve_counts(x, thr, strict=True)[0] == 0 and E.curve_counts(x, thr)[0] == 1
    assert golden["on_thresholds_auc64"] != golden["on_thresholds_auc32"]        # ... which the float32 rounding of the same values moves
    assert golden["all_below_auc64"] == 1.0 and golden["all_above_auc64"] == 0.0


def test_counts_and_auc_edge_rules():
    assert np.array_equal(E.curve_counts([0.5, 1.0, 1.5], [1.0, 2.0]), [2.0, 3.0])
    assert np.array_equal(E.curve_counts([0.5, 1.0, 1.5], [1.0, 2.0], strict=True), [1.0, 3.0])
    assert np.array_equal(E.curve_counts([], [1.0, 2.0]), [0.0, 0.0]) and E.curve_counts([], [1.0]).dtype == np.float64
    assert math.isnan(E.curve_auc([3.0], 3, [0.01]))                  # one threshold: no interval to integrate over
    assert math.isnan(E.curve_auc([0.0, 0.0], 0, [0.01, 0.02]))       # no points
    assert E.curve_auc([0.0, 4.0], 4, [0.01, 0.02]) == 0.5
    for bad in ([0.02, 0.01], [0.01, 0.01], [0.01, float("nan")], [0.01, float("inf")], [], [[0.01, 0.02]], np.linspace(0, 1, 257)):
        with pytest.raises(ValueError):
            E.Evaluator(thresholds=bad)
    for bad in ([0.015, 0.005], [0.005, 0.005], np.linspace(0.001, 0.1, 9)):
        with pytest.raises(ValueError):
            E.Evaluator(f_thresholds=bad)
    ev = E.Evaluator(f_thresholds=())
    assert len(ev.f_thresholds) == 0 and np.array_equal(ev.thresholds, np.linspace(0, 0.05, 100))
    assert np.array_equal(E.Evaluator().f_thresholds, [0.005, 0.015])
    assert np.array_equal(E.fscore_from_counts([0, 778, 389], [0, 778, 778], 778.0), [0.0, 1.0, CC.fscore_of(389.0, 778.0)])


# ------------------------------------------------------------------------------------------------------------------ the cases
def test_margin_holds_on_every_case_and_table():
    """A condition on the inputs: every statement value lies >= 1e-8 from every threshold it is compared with, except exact zeros and
    the dyadic known answers, which EQUAL a threshold on every side."""
    bad = CC.all_margin_violations([CC.pck_table(T) for T in GENERIC_T], [CC.F_TABLES[F] for F in GENERIC_F])
    assert not bad, bad[:10]
    jn, vn = CC.joint_batch()[0], CC.vert_batch()[0]
    for name in CC.DEFAULT_JOINT_CASES:
        assert not [x for e in CC.joint_reference()[jn.index(name)] for x in CC.margin_violations(e, CC.DEFAULT_TABLE)], name
    for name in CC.DEFAULT_VERT_CASES:
        for st in CC.vert_reference()[vn.index(name)]:
            assert not CC.margin_violations(st["err"][[st["counted"], st["pa_kept"]]], CC.DEFAULT_TABLE), name
    for e in CC.joint_reference()[jn.index("dyadic")]:
        assert not CC.margin_violations(e, CC.KNOWN_TABLE)
    st = CC.vert_reference()[vn.index("dyadic")][0]
    assert not CC.margin_violations(st["err"], CC.KNOWN_TABLE) and not CC.margin_violations(st["nn"], CC.KNOWN_F_TABLE)
    assert not CC.evaluator_margin_violations()
    # the check sees what it is meant to see
    assert CC.margin_violations([0.01 + 5e-9], [0.01]) and not CC.margin_violations([0.01 + 2e-8, 0.0, CC.KNOWN], [0.01, 0.0, CC.KNOWN])
    assert CC.margin_violations([0.01], [0.01])                        # equal, but not one of the exact values
    n_values = sum(len(e) for pops in CC.joint_reference() for e in pops) + sum(
        NV * (st["counted"] + st["pa_kept"]) * 3 for hands in CC.vert_reference() for st in hands for NV in (CC.NV,))
    assert n_values > 30000, n_values
    for T in GENERIC_T:
        t = CC.pck_table(T)
        assert len(t) == T and (np.diff(t) > 0).all()
    assert [len(CC.F_TABLES[F]) for F in GENERIC_F] == list(GENERIC_F)


def test_the_case_tables_hold_what_they_are_meant_to_hold():
    jn, pred, gt, scale = CC.joint_batch()
    n = {name: [len(e) for e in pops] for name, pops in zip(jn, CC.joint_reference())}
    assert n["all_42"] == [42, 42, 42] and n["right_hand_only_21"] == [21, 21, 21]
    assert n["missing_wrist_41"] == [21, 41, 41]                       # no valid right wrist: the right hand leaves j3d, not the PA sets
    assert n["weight_sum_1p5"] == [0, 0, 0] and n["coincident_prediction"] == [42, 0, 0] and n["none_valid"] == [0, 0, 0]
    vn, P, G, W, S = CC.vert_batch()
    ref = {name: hands for name, hands in zip(vn, CC.vert_reference())}
    assert [st["counted"] for st in ref["left_without_annotation"]] == [True, False]
    assert [(st["counted"], st["pa_kept"]) for st in ref["coincident_prediction"]] == [(True, False)] * 2
    for st in ref["identical"]:
        assert not st["nn"][0].any() and not st["err"][0].any() and st["nn"][1].max() <= 1e-12
        c, fc = CC.hand_counts(st, CC.pck_table(2), CC.F_TABLES[8])
        assert (fc == CC.NV).all() and all(CC.fscore_of(a, b) == 1.0 for a, b in zip(fc[:, 0].ravel(), fc[:, 1].ravel()))
    st = ref["far_apart"][1]
    assert st["counted"] and st["pa_kept"] and st["nn"].min() > 0.1 > max(CC.F_TABLES[8])
    assert not CC.hand_counts(st, CC.pck_table(2), CC.F_TABLES[8])[1].any() and CC.fscore_of(0.0, 0.0) == 0.0      # the P + R = 0 branch


def test_known_answers():
    jn, pred, gt, scale = CC.joint_batch()
    i = jn.index("dyadic")
    j3d = CC.joint_reference()[i][0]
    want = np.full(42, CC.KNOWN)
    want[[0, 21]] = 0.0
    assert np.array_equal(j3d, want)
    host = E.get_single_joints_error(pred[i].astype(np.float64), gt[i, :, :3].astype(np.float64), gt[i, :, 3:], 1.0)
    assert np.array_equal(np.array(host), want)
    # an error EQUAL to a threshold counts: [1/1024, 1/128, KNOWN, 1/64, 1/16]
    assert np.array_equal(E.curve_counts(host, CC.KNOWN_TABLE), [2, 2, 42, 42, 42])
    assert np.array_equal(CC.joint_counts(pred[i], gt[i], 1.0, CC.KNOWN_TABLE)[0], [2, 2, 42, 42, 42, 42])
    vn, P, G, W, S = CC.vert_batch()
    b = vn.index("dyadic")
    st = CC.vert_reference()[b][0]
    wantv = np.full(CC.NV, CC.KNOWN)
    wantv[0] = 0.0
    assert np.array_equal(st["err"][0], wantv) and np.array_equal(st["nn"][0, 0], wantv) and np.array_equal(st["nn"][0, 1], wantv)
    counts, d_pg, d_gp = E.get_single_fscore_counts(P[b, 0], G[b, 0], CC.root_weights()[0], 1.0, CC.KNOWN_F_TABLE, aligned=False)
    assert np.array_equal(d_pg, wantv) and np.array_equal(d_gp, wantv)
    # a distance EQUAL to a threshold does not count: [1/128, KNOWN, 1/64]
    assert np.array_equal(counts, [[1, 1, 778], [1, 1, 778]])
    assert np.array_equal(CC.hand_counts(st, CC.KNOWN_TABLE, CC.KNOWN_F_TABLE)[0][0], [1, 1, 778, 778, 778, 778])


def test_host_functions_match_the_statement():
    jn, pred, gt, scale = CC.joint_batch()
    tables = [CC.pck_table(T) for T in GENERIC_T]
    for i, name in enumerate(jn):
        p, g, s = pred[i], gt[i], float(scale[i])
        host = [E.get_single_joints_error(p.astype(np.float64), g[:, :3].astype(np.float64), g[:, 3:], s),
                E.get_single_pa_error(p, g[:, :3], g[:, 3], s),
                E.get_single_pa_error(p[:21], g[:21, :3], g[:21, 3], s) + E.get_single_pa_error(p[21:], g[21:, :3], g[21:, 3], s)]
        for h, e in zip(host, CC.joint_reference()[i]):
            assert len(h) == len(e) and (len(e) == 0 or np.abs(np.array(h) - e).max() <= 1e-12), name
            for t in tables:
                assert np.array_equal(E.curve_counts(h, t), CC.counts_of(e, t)), name
    vn, P, G, W, S = CC.vert_batch()
    rw = CC.root_weights()
    for b, name in enumerate(vn):
        for h in range(2):
            st = CC.vert_reference()[b][h]
            if not st["counted"]:
                continue
            v3d = np.array(E.get_single_verts_error(P[b, h], G[b, h], rw[h], float(S[b])))
            assert np.abs(v3d - st["err"][0]).max() <= 1e-12 * max(1.0, st["err"][0].max()), name
            for k, aligned in enumerate((False, True)):
                r = E.get_single_fscore_counts(P[b, h], G[b, h], rw[h], float(S[b]), CC.F_TABLES[8], aligned)
                assert (r is not None) == (st["pa_kept"] if aligned else True), name
                if r is not None:
                    assert np.abs(r[1] - st["nn"][k, 0]).max() <= 1e-12 * max(1.0, st["nn"][k].max()), name
                    assert np.abs(r[2] - st["nn"][k, 1]).max() <= 1e-12 * max(1.0, st["nn"][k].max()), name
                    assert np.array_equal(r[0], CC.hand_counts(st, CC.pck_table(2), CC.F_TABLES[8])[1][k]), name
    rng = np.random.RandomState(4)
    a, c = rng.randn(30, 3), rng.randn(50, 3)
    d_pg, d_gp = E.nn_distances(a, c)
    full = np.linalg.norm(a[:, None] - c[None], axis=2)
    assert d_pg.shape == (30,) and d_gp.shape == (50,) and np.allclose(d_pg, full.min(1), rtol=1e-14) and np.allclose(d_gp, full.min(0), rtol=1e-14)


# ------------------------------------------------------------------------------------------------------------------ Evaluator
def _evaluators(**kw):
    res, data_list, keep = CC.evaluator_batch()
    ev = E.Evaluator(CC.mano_models(), data_list=data_list, **kw)
    ev.update(np.arange(len(keep)), {k: v.copy() for k, v in res.items()})
    return ev, keep


def test_evaluator_sums_equal_the_statement_and_add_up():
    thr, fthr = CC.pck_table(CC.EVAL_T), CC.F_TABLES[CC.EVAL_F]
    ev, keep = _evaluators(curve_metrics=True, thresholds=thr, f_thresholds=fthr)
    full = list(ev.pred_results)
    ev.pred_results = [r for r, k in zip(full, keep) if k]
    got, want = ev.curve_sums(), CC.expected_curve_sums(thr, fthr)
    T, F = len(thr), len(fthr)
    assert got.dtype == np.float64 and len(got) == 5 * (T + 1) + 2 * (F + 1) + 2 * 51
    assert np.array_equal(got, want), np.nonzero(got != want)
    m = E.Evaluator.curve_metrics_from_sums(got, thr, fthr)
    pops, hands, cmax, cave = CC.evaluator_statement()
    for name, e in zip(E.CURVE_POPULATIONS, pops):
        assert len(e) > 0 and np.array_equal(m[f"pck_{name}"], CC.counts_of(e, thr) / len(e)), name
        assert abs(m[f"auc_{name}"] - CC.auc_of(CC.counts_of(e, thr), len(e), thr)) <= 1e-15 and 0 < m[f"auc_{name}"] <= 1, name
    assert m["fscore_raw"].shape == m["fscore_pa"].shape == (F,) and (m["fscore_raw"] > 0).all() and (m["fscore_pa"] <= 1).all()
    # the collision AUCs are the reference's function on the per-sample values
    assert abs(m["collision_auc_max"] - E.calc_collision_auc(cmax)) <= 1e-15 and abs(m["collision_auc_ave"] - E.calc_collision_auc(cave)) <= 1e-15
    assert 0 < m["collision_auc_max"] < m["collision_auc_ave"] < 1
    # two evaluators' sums add up to one's: every count exactly; a sum of F values to rounding (each part is a correctly rounded sum)
    a, b = E.Evaluator(CC.mano_models(), curve_metrics=True, thresholds=thr, f_thresholds=fthr), E.Evaluator(
        CC.mano_models(), curve_metrics=True, thresholds=thr, f_thresholds=fthr)
    a.pred_results, b.pred_results = ev.pred_results[:3], ev.pred_results[3:]
    both = a.curve_sums() + b.curve_sums()
    fcols = np.zeros(len(got), bool)
    fcols[5 * (T + 1):5 * (T + 1) + 2 * (F + 1)] = True
    fcols[[5 * (T + 1) + F, 5 * (T + 1) + 2 * F + 1]] = False           # the two hand counts
    assert np.array_equal(both[~fcols], got[~fcols]) and np.abs(both[fcols] - got[fcols]).max() <= 1e-13
    # nothing counted: NaN everywhere, no exception
    empty = E.Evaluator.curve_metrics_from_sums(E.Evaluator(curve_metrics=True).curve_sums())
    assert all(np.isnan(v).all() for v in empty.values()) and len(empty["pck_j3d"]) == 100 and len(empty["fscore_raw"]) == 2


def test_without_the_flag_records_sums_and_pickles_are_unchanged():
    off, _ = _evaluators()
    on, _ = _evaluators(curve_metrics=True)
    pa, _ = _evaluators(pa_metrics=True)
    both, _ = _evaluators(pa_metrics=True, curve_metrics=True)
    new = {"curve_j3d_error", "pa_inter_j3d_error", "pa_j3d_error", "pa_v3d_error"} | set(E.Evaluator.NN_KEYS)
    expected = {"data_idx", "pred_cam_params", "pred_shape_params", "pred_pose_params", "pred_hand_trans", "pred_joints_3d",
                "collision_loss_origin_scale", "gt_joints_3d", "img_path", "img_path_relative", "annot_type", "hand_type", "hand_type_valid",
                "scale", "j3d_error", "pa_no_rot_inter_j3d_error", "v3d_error"} | set(E.Evaluator.VERT_KEYS)
    for a, b, c, d in zip(off.pred_results, on.pred_results, pa.pred_results, both.pred_results):
        assert set(a) == expected and set(b) == expected | new and set(d) == set(b)
        for k in a:                      # byte for byte, dtype included: j3d_error keeps its dtype
            assert pickle.dumps(a[k]) == pickle.dumps(b[k]), k
        assert all(pickle.dumps(c[k]) == pickle.dumps(d[k]) for k in c)            # the PA lists are the ones pa_metrics computes
        assert all(pickle.dumps(b[k]) == pickle.dumps(d[k]) for k in b)
        assert all(isinstance(x, float) for x in b["curve_j3d_error"]) and len(b["curve_j3d_error"]) == len(a["j3d_error"])
    assert np.array_equal(off.metric_sums(), on.metric_sums()) and len(off.metric_sums()) == 9
    assert np.array_equal(off.pa_metric_sums(), np.zeros(6)) and np.array_equal(pa.pa_metric_sums(), both.pa_metric_sums())
    assert not off.curve_sums().any()                                  # records without the lists count nothing
    back = pickle.loads(pickle.dumps(off))
    assert all(set(r) == expected for r in back.pred_results)
    # an evaluator pickled before the curve metrics existed has none of the new attributes
    for k in ("curve_metrics", "thresholds", "f_thresholds", "_device_curve_parts", "_device_curve_vert_parts"):
        back.__dict__.pop(k)
    res, _, _ = CC.evaluator_batch()
    back.update(np.arange(2), {k: v[:2].copy() for k, v in res.items()})
    assert all(set(r) == expected for r in back.pred_results) and np.array_equal(back.pa_metric_sums(), np.zeros(6))
    # a model without GT meshes: no distance lists, the vertex populations stay empty
    plain = E.Evaluator(curve_metrics=True)
    plain.update(np.arange(2), {k: v[:2].copy() for k, v in res.items() if "verts" not in k and k != "mano_params_weight"})
    assert all(not (set(r) & set(E.Evaluator.NN_KEYS)) and "pa_v3d_error" not in r for r in plain.pred_results)
    m = E.Evaluator.curve_metrics_from_sums(plain.curve_sums())
    assert np.isnan(m["auc_v3d"]) and np.isnan(m["fscore_raw"]).all() and m["auc_j3d"] > 0


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_curve")
    exe = hostbuild.build("eval_curve_driver.cpp", d)
    count = [0]

    def run(op, payload):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        np.ascontiguousarray(payload, np.float64).tofile(fin)
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, np.float64)
    return run


def test_pure_threshold_index_is_exact(driver):
    values = np.concatenate([e for pops in CC.joint_reference() for e in pops] + [CC.vert_reference()[0][0]["err"].ravel(),
                            [0.0, -1.0, 1e30, float("inf"), -float("inf"), float("nan"), CC.KNOWN]])
    tables = [CC.pck_table(T) for T in GENERIC_T] + [CC.DEFAULT_TABLE, CC.KNOWN_TABLE, np.array(CC.F_TABLES[8]), np.array(CC.KNOWN_F_TABLE),
                                                     E.COLLISION_AUC_THRESHOLDS, np.arange(1.0, 4.0), np.arange(1.0, 8.0)]
    for t in tables:
        v = np.concatenate([values, t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)])       # the thresholds themselves and their neighbours
        got = driver("index", np.concatenate([[len(t)], t, v])).reshape(-1, 2)
        finite = ~np.isnan(v)
        assert np.array_equal(got[finite, 0], np.searchsorted(t, v[finite], side="left"))         # the thresholds < v: v <= t[k] from there on
        assert np.array_equal(got[finite, 1], np.searchsorted(t, v[finite], side="right"))        # the thresholds <= v: v < t[k] from there on
        assert (got[~finite] == len(t)).all()                                                     # a NaN satisfies no comparison
        # the histogram over the index, summed from the left, is the count per threshold
        for col, strict in ((0, False), (1, True)):
            hist = np.bincount(got[:, col].astype(int), minlength=len(t) + 1)
            assert np.array_equal(np.cumsum(hist)[:len(t)], CC.counts_of(v, t, strict))
    assert np.array_equal(driver("index", np.array([0.0, 1.0, 2.0])), np.zeros(4))                # an empty table


def test_pure_squared_distance_and_fscore_match_numpy_bit_for_bit(driver):
    vn, P, G, W, S = CC.vert_batch()
    rng = np.random.RandomState(12)
    recs = []
    for b in range(len(vn)):
        i, j = rng.randint(0, CC.NV, 400), rng.randint(0, CC.NV, 400)
        recs.append(np.concatenate([P[b, 0, i], G[b, 1, j]], axis=1).astype(np.float64))
    recs.append(rng.randn(2000, 6) * 10.0 ** rng.randint(-6, 3, (2000, 1)))
    r = np.concatenate(recs)
    d = r[:, :3] - r[:, 3:]
    want = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert driver("sqdist", r.ravel()).tobytes() == want.tobytes()
    counts = np.array([[a, b, 778.0] for a in (0, 1, 5, 389, 777, 778) for b in (0, 1, 7, 400, 778)], np.float64)
    got = driver("fscore", counts.ravel())
    assert got.tobytes() == np.array([CC.fscore_of(a, b, n) for a, b, n in counts]).tobytes()
    assert got[0] == 0.0 and got[-1] == 1.0
    assert got.tobytes() == E.fscore_from_counts(counts[:, 0], counts[:, 1], 778.0).tobytes()


# ------------------------------------------------------------------------------------------------------------------ the build
def test_curve_kernels_use_no_scratch_and_the_header_is_exported():
    import ctypes

    from ihmr_amd import hip
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("eval_curve_joints_kernel", "eval_curve_verts_kernel"):
            if k in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == ["eval_curve_joints_kernel", "eval_curve_verts_kernel"], sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert 0 < m["group_segment_fixed_size"] < 64 * 1024, (name, m)
    assert seen["eval_curve_verts_kernel"]["group_segment_fixed_size"] >= 3 * 778 * 8            # the target set of a pass lies in LDS
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:[A-Za-z_][\w ]*?[\s*]+)(ihmr_\w+)\s*\(", header, flags=re.M))
    assert {"ihmr_eval_curve_joints", "ihmr_eval_curve_verts"} <= declared
    assert declared == set(hip.EXPORTED_SYMBOLS), declared ^ set(hip.EXPORTED_SYMBOLS)
    assert int(re.search(r"#define IHMR_EVAL_MAX_THRESHOLDS (\d+)", header).group(1)) == hip.EVAL_MAX_THRESHOLDS == E.MAX_THRESHOLDS == 256
    assert int(re.search(r"#define IHMR_EVAL_MAX_F_THRESHOLDS (\d+)", header).group(1)) == hip.EVAL_MAX_F_THRESHOLDS == E.MAX_F_THRESHOLDS == 8
    L = ctypes.CDLL(hip.build())
    for sym in declared:
        getattr(L, sym)

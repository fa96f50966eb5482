"""The interacting-hand metrics (MRRPE, contact consistency) without a GPU: the known answers, the host functions of
ihmr_amd/evaluator.py against the float64 statement of tests/contact_cases.py on every case, the margin condition, the Evaluator's
records and sums (additive over split batches; byte-identical with the flag off), the refusals, six wrong rules that the cases tell
apart, csrc/contact_pure.h built for the host with ASan / UBSan (tests/contact_host_driver.cpp walks a sample in the kernel's order)
and the build: both kernels without scratch memory, the LDS the header names, every declared symbol exported."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj  # noqa: E402
import contact_cases as CT  # noqa: E402
import curve_cases as CC  # noqa: E402
import hostbuild  # noqa: E402

from ihmr_amd import evaluator as E  # noqa: E402

TOL = CT.TOL


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _close(a, b, tol):
    """|a - b| <= tol where both are finite; NaN and +-Inf positions and values exact."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    with np.errstate(all="ignore"):
        return a.shape == b.shape and _same(np.where(fin, 0.0, a), np.where(fin, 0.0, b)) and bool((np.abs(a - b)[fin] <= tol).all())


# ------------------------------------------------------------------------------------------------------------------ known answers
def test_known_answers_in_dyadic_coordinates():
    c = CT.mesh_cases()["dyadic"]
    for fn in (lambda table: CT.case_statement("dyadic", tuple(table)),
               lambda table: dict(zip(("pair_sum", "pairs", "total", "near"), E.get_single_contact(c.pr, c.pl, c.gr, c.gl, c.scale, table)))):
        s = fn(CT.TABLES[2])                                        # tau_c = 3 mm: the 778 pairs (i, i), each exactly 2^-8 apart in pred
        assert s["pairs"] == 778 and s["pair_sum"] == 778 * CT.KNOWN_PRED and s["pair_sum"] / s["pairs"] == 2.0 ** -8
        total = s["counts"].sum(axis=0) if "counts" in s else s["total"]
        assert total.tolist() == [[0, 0, 1556], [1556, 1556, 1556]]
        assert (s["near"][:, 0] == CT.KNOWN_PRED).all() and (s["near"][:, 1] == CT.KNOWN_GT).all()
        s = fn(CT.KNOWN_TABLE)                                      # tau_c = 2^-9 exactly: equality is not contact
        assert s["pairs"] == 0 and s["pair_sum"] == 0.0
        total = s["counts"].sum(axis=0) if "counts" in s else s["total"]
        assert total.tolist() == [[0, 0, 0], [0, 0, 1556], [0, 0, 1556], [1556, 1556, 1556]]
    per_hand = CT.case_statement("dyadic", CT.KNOWN_TABLE)["counts"]
    assert per_hand[0].tolist() == per_hand[1].tolist() == [[0, 0, 0], [0, 0, 778], [0, 0, 778], [778, 778, 778]]
    names, P, G, S, I = CT.joint_batch()
    ref = dict(zip(names, CT.joint_reference()))
    assert ref["dyadic"] == (CT.KNOWN_MRRPE, 1.0) and ref["pred_is_gt"] == (0.0, 1.0)
    assert ref["right_wrist_weight_0"] == ref["left_wrist_weight_0"] == ref["negative_weight"] == ref["not_interacting"] == (0.0, 0.0)
    assert ref["fractional_weights"][1] == ref["other_joints_weight_0"][1] == 1.0
    assert np.isnan(ref["nan_joint"][0]) and ref["nan_joint"][1] == 1.0 and np.isfinite(ref["nan_elsewhere"][0])


def test_the_case_table_holds_what_it_claims():
    pairs = lambda prefix: [CT.case_statement(n, CT.TABLES[2])["pairs"] for n in CT.mesh_cases() if n.startswith(prefix) and n.endswith("_same")]
    assert pairs("default") == [23, 31, 32] and pairs("deep") == [65, 69, 78] and pairs("fingers") == [26, 30]
    for name in CT.mesh_cases():
        s = CT.case_statement(name, CT.TABLES[2])
        if name.endswith("_same"):                                  # pred = gt: the mean GT contact distance, precision = recall = 1
            assert 0 < s["dev"] < 0.003 and (s["counts"][:, :, 0] == s["counts"][:, :, 1]).all() and (s["counts"][:, :, 0] == s["counts"][:, :, 2]).all()
            assert 15 <= s["counts"][:, 0, 2].min() and s["counts"][:, 0, 2].max() <= 76
    far, deep = CT.case_statement("far_apart", CT.TABLES[2]), CT.case_statement("deep_0_noise", CT.TABLES[2])
    assert far["counted"] and far["pairs"] == 0 and not far["counts"].any() and deep["pairs"] == 65 and 0.004 < deep["dev"] < 0.006
    assert not CT.case_statement("right_weight_0", CT.TABLES[2])["counted"] and not CT.case_statement("left_weight_neg", CT.TABLES[2])["counted"]
    assert CT.case_statement("left_weight_1e-8", CT.TABLES[2])["pairs"] == 65
    assert CT.case_statement("scale_0p25", CT.TABLES[2])["pairs"] < 65 < CT.case_statement("scale_1p7", CT.TABLES[2])["pairs"]
    gt_nan = CT.case_statement("nan_in_gt", CT.TABLES[2])
    assert 0 < gt_nan["pairs"] < 65 and np.isinf(gt_nan["near"][1, 1]).sum() == 1 and not np.isnan(gt_nan["near"]).any()
    all_nan = CT.case_statement("left_pred_all_nan", CT.TABLES[2])
    assert np.isnan(all_nan["pair_sum"]) and np.isposinf(all_nan["near"][:, 0]).all() and not all_nan["counts"][:, :, :2].any()


def test_every_value_keeps_the_margin_from_every_threshold():
    assert CT.all_margin_violations() == []
    # the exactly-equal dyadic values are the one exception, and they are really there
    d = CT.case_distances("dyadic")
    assert (d["near"][:, 1] == CT.KNOWN_TABLE[0]).all() and (d["near"][:, 0] == CT.KNOWN_TABLE[2]).all()
    assert CT.margin_violations([0.003 + 5e-9], CT.TABLES[2]) and not CT.margin_violations([0.003 + 2e-8], CT.TABLES[2])


# ------------------------------------------------------------------------------------------------------------------ host functions
@pytest.mark.parametrize("K", sorted(CT.TABLES))
def test_host_functions_equal_the_statement_on_every_case(K):
    table = CT.TABLES[K]
    for name, c in CT.mesh_cases().items():
        s = CT.contact_of(CT.case_distances(name), True, table)          # the host function knows no weights: the caller decides
        pair_sum, pairs, counts, near = E.get_single_contact(c.pr, c.pl, c.gr, c.gl, c.scale, table)
        assert pairs == s["pairs"] and _same(counts, s["counts"].sum(axis=0)) and counts.shape == (K, 3), name
        assert _close(near, s["near"], 0.0) and near.shape == (2, 2, 778), name
        assert _close(pair_sum, s["pair_sum"], max(1, pairs) * TOL), (name, pair_sum, s["pair_sum"])


def test_host_mrrpe_equals_the_statement_on_every_case():
    names, P, G, S, I = CT.joint_batch()
    for b, name in enumerate(names):
        e, counted = CT.mrrpe_of(P[b], G[b], S[b], True)                 # interacting is the caller's rule
        got = E.get_single_mrrpe(P[b], G[b, :, :3], G[b, :, 3:], S[b])
        assert len(got) == counted and (not got or _close(got[0], e, 0.0)), (name, got, e)
        assert _same(got, E.get_single_mrrpe(P[b], G[b, :, :3], G[b, :, 3], S[b]))         # the weights as a column or as a vector


# ------------------------------------------------------------------------------------------------------------------ the Evaluator
def _evaluator(**kw):
    res, data_list, keep, inter = CT.evaluator_batch()
    return E.Evaluator(CC.mano_models(), data_list=data_list, **kw)


def _update(ev, rows):
    res = CT.evaluator_batch()[0]
    rows = np.asarray(rows)
    ev.update(rows, {k: v[rows].copy() for k, v in res.items()})


@pytest.mark.parametrize("K", sorted(CT.TABLES))
def test_records_and_sums_are_the_statement_and_add_over_split_batches(K):
    table = CT.TABLES[K]
    res, data_list, keep, inter = CT.evaluator_batch()
    kept = np.nonzero(keep)[0]
    whole = _evaluator(interaction_metrics=True, contact_thresholds=table)
    _update(whole, kept)
    want = CT.expected_sums(*CT.evaluator_statement(table), table)
    got = whole.interaction_sums()
    assert got.shape == (5 + 3 * K,) and got.dtype == np.float64
    assert _same(got[[1, 3, 4]], want[[1, 3, 4]]) and _same(got[5:], want[5:]), (got, want)
    assert want[1] >= 4 and want[3] >= 3 and want[4] > want[3] and want[5:].all()
    assert np.isnan(want[2]) == np.isnan(got[2])                         # the batch carries a NaN prediction: its deviation is NaN
    parts = []
    for rows in (kept[:3], kept[3:4], kept[4:]):
        ev = _evaluator(interaction_metrics=True, contact_thresholds=table)
        _update(ev, rows)
        parts.append(ev.interaction_sums())
        w = CT.expected_sums(*CT.evaluator_statement(table, rows), table)
        assert _same(parts[-1][[1, 3, 4]], w[[1, 3, 4]]) and _same(parts[-1][5:], w[5:])
        assert _close(parts[-1][[0, 2]], w[[0, 2]], 1e-9 * np.abs(w[[0, 2]]).max() if np.isfinite(w[[0, 2]]).all() else 0.0) or np.isnan(w[2])
    total = sum(parts)
    assert _same(total[[1, 3, 4]], got[[1, 3, 4]]) and _same(total[5:], got[5:]) and abs(total[0] - got[0]) <= 1e-12 * got[0]
    # the records: mrrpe a list of 0 or 1 values; the contact keys only with four meshes and both hands annotated
    for r, b in zip(whole.pred_results, kept):
        e, counted = CT.mrrpe_of(res["pred_joints_3d"][b], res["gt_joints_3d"][b], data_list[b]["scale"])
        assert len(r["mrrpe"]) == counted and (not counted or _close(r["mrrpe"][0], e, 0.0))
        c = CT.mesh_cases()[CT.EVAL_CASES[b]]
        assert ("contact_pairs" in r) == c.counted and ("contact_counts" in r) == ("contact_pair_sum" in r) == c.counted
        if c.counted:
            s = CT.contact_of(CT.case_distances(c.name), True, table)
            assert r["contact_pairs"] == s["pairs"] and _same(r["contact_counts"], s["counts"].sum(axis=0))
    # without the NaN sample every metric is the statement's
    rows = [b for b in kept if CT.EVAL_CASES[b] != "nan_in_pred"]
    ev = _evaluator(interaction_metrics=True, contact_thresholds=table)
    _update(ev, rows)
    m = ev.metrics_from_packed(ev.packed_sums())
    want = CT.metrics_of(*CT.evaluator_statement(table, rows), table)
    for k in ("mrrpe", "contact_dev", "contact_rate", "contact_precision", "contact_recall", "contact_f1"):
        assert _close(m[k], want[k], 1e-9 * np.nanmax(np.abs(want[k]))), (k, m[k], want[k])
    assert 0 < m["contact_rate"] < 1 and (m["contact_f1"] > 0).all() and m["mrrpe"] > 0
    assert list(m)[:4] == ["mpjpe_3d", "inter_mpjpe_3d", "collision_ave", "collision_max"]
    # a model without GT meshes: MRRPE only
    plain = E.Evaluator(interaction_metrics=True)
    plain.update(kept[:3], {k: v[kept[:3]].copy() for k, v in res.items() if "verts" not in k and k != "mano_params_weight"})
    s = plain.interaction_sums()
    assert all("mrrpe" in r and "contact_pairs" not in r for r in plain.pred_results) and s[1] > 0 and not s[2:].any()
    m = E.Evaluator.interaction_metrics_from_sums(s)
    assert np.isnan(m["contact_dev"]) and np.isnan(m["contact_rate"]) and np.isnan(m["contact_f1"]).all() and m["mrrpe"] > 0


def test_metrics_from_sums_at_its_edges():
    f = E.Evaluator.interaction_metrics_from_sums
    m = f(np.array([0.5, 2, 0.9, 3, 4, 10, 20, 40, 0, 0, 5], np.float64))
    assert m["mrrpe"] == 0.25 and m["contact_dev"] == 0.9 / 3 and m["contact_rate"] == 0.75
    assert m["contact_precision"][0] == 0.5 and m["contact_recall"][0] == 0.25 and m["contact_f1"][0] == 2 * 0.5 * 0.25 / 0.75
    assert np.isnan(m["contact_precision"][1]) and m["contact_recall"][1] == 0.0 and np.isnan(m["contact_f1"][1])
    m = f(np.array([0, 0, 0, 0, 0, 0, 7, 9], np.float64), (0.003,))
    assert m["contact_precision"][0] == 0.0 and m["contact_recall"][0] == 0.0 and m["contact_f1"][0] == 0.0       # P + R = 0: F1 = 0
    assert all(np.isnan(m[k]) for k in ("mrrpe", "contact_dev", "contact_rate"))
    with pytest.raises(AssertionError):
        f(np.zeros(8))                                                   # the default table has two thresholds


PARENT_ATTRIBUTES = ["pa_metrics", "curve_metrics", "thresholds", "f_thresholds", "inputSize", "left_hand_faces", "right_hand_faces",
                     "root_weights", "data_list", "image_root", "save_verts", "pred_results", "_device_parts", "_device_vert_parts",
                     "_device_pa_parts", "_device_pa_vert_parts", "_device_curve_parts", "_device_curve_vert_parts"]


def test_flag_off_nothing_changes():
    res, data_list, keep, inter = CT.evaluator_batch()
    rows = [b for b in np.nonzero(keep)[0] if CT.EVAL_CASES[b] != "nan_in_pred"]      # the PA metrics' SVD takes no NaN mesh
    new = {"mrrpe", "contact_pair_sum", "contact_pairs", "contact_counts"}
    for kw in (dict(), dict(pa_metrics=True, curve_metrics=True)):
        off, on = _evaluator(**kw), _evaluator(interaction_metrics=True, **kw)
        assert list(off.__dict__) == PARENT_ATTRIBUTES                   # a default Evaluator pickles with the attributes it had
        assert list(on.__dict__) == PARENT_ATTRIBUTES + ["interaction_metrics", "contact_thresholds", "_device_mrrpe_parts", "_device_contact_parts"]
        _update(off, rows)
        _update(on, rows)
        for a, b in zip(off.pred_results, on.pred_results):
            assert not (set(a) & new) and list(b)[:len(a)] == list(a) and set(b) - set(a) <= new and "mrrpe" in b
            for k in a:                                                  # byte for byte, dtype included
                assert pickle.dumps(a[k]) == pickle.dumps(b[k]), k
        for name in ("metric_sums", "pa_metric_sums", "curve_sums", "volume_sums"):
            assert getattr(off, name)().tobytes() == getattr(on, name)().tobytes(), name
        p_off, p_on = off.packed_sums(), on.packed_sums()
        assert len(p_on) == len(p_off) + 11 and p_on[:len(p_off)].tobytes() == p_off.tobytes()      # the last family: no slice moves
        assert p_on[len(p_off):].tobytes() == on.interaction_sums().tobytes()
        assert not off.interaction_sums().any() and len(off.interaction_sums()) == 11
        assert "mrrpe" not in off.metrics_from_packed(p_off)
        back = pickle.loads(pickle.dumps(off))
        assert list(back.__dict__) == PARENT_ATTRIBUTES and not hasattr(back, "interaction_metrics")
        on.clear()
        off.clear()
        assert on._device_mrrpe_parts == [] and on._device_contact_parts == [] and not on.interaction_sums().any()
        assert list(off.__dict__) == PARENT_ATTRIBUTES
    empty = pickle.dumps(E.Evaluator())
    assert b"interaction" not in empty and b"contact" not in empty and b"mrrpe" not in empty


@pytest.mark.parametrize("table", [(), tuple(np.linspace(0.001, 0.009, 9)), (0.005, 0.003), (0.003, 0.003), (0.003, float("nan")),
                                   (0.003, float("inf")), ((0.003, 0.005),)])
def test_threshold_table_refusals(table):
    with pytest.raises(ValueError):
        E.Evaluator(interaction_metrics=True, contact_thresholds=table)
    with pytest.raises(ValueError):
        E.Evaluator.interaction_metrics_from_sums(np.zeros(5 + 3 * max(1, len(table))), table)


def test_the_flag_is_required():
    with pytest.raises(ValueError):
        E.Evaluator(contact_thresholds=(0.003,))
    ev = E.Evaluator()
    for call in (lambda: ev.update_device_mrrpe(None, None), lambda: ev.update_device_contact(None, None, None, None, None)):
        with pytest.raises(RuntimeError, match="interaction_metrics=True"):
            call()
    assert E.Evaluator(interaction_metrics=True).contact_thresholds.tolist() == [0.003, 0.005] == list(E.CONTACT_THRESHOLDS)
    assert len(E.Evaluator(interaction_metrics=True, contact_thresholds=CT.TABLES[8]).contact_thresholds) == 8 == E.MAX_CONTACT_THRESHOLDS


# ------------------------------------------------------------------------------------------------------------------ wrong rules
def _beyond(got, want, bar):
    """The largest distance of ``got`` from ``want`` in units of ``bar`` (a NaN / Inf mismatch counts as infinitely far)."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    fin = np.isfinite(got) & np.isfinite(want)
    if not _same(np.where(fin, 0.0, got), np.where(fin, 0.0, want)):
        return np.inf
    with np.errstate(all="ignore"):
        return float((np.abs(got - want)[fin] / bar).max()) if fin.any() else 0.0


def test_six_wrong_rules_each_land_ten_times_beyond_the_bar():
    """The bars: a count differs by less than 1 (counts are exact), a distance or a sum per pair by at most 1e-9 m, a reported ratio by
    1e-9.  Each wrong rule lands at least ten bars away on some case of the table."""
    t, table = CT.mesh_cases(), CT.TABLES[2]
    worst = {}
    # 1. non-strict comparison: equality becomes contact
    d = CT.case_distances("dyadic")
    right = CT.case_statement("dyadic", CT.KNOWN_TABLE)
    worst["non_strict"] = max(_beyond((d["d_gt"] <= CT.KNOWN_TABLE[0]).sum(), right["pairs"], 1.0),
                              _beyond((d["near"][:, 1] <= CT.KNOWN_TABLE[0]).sum(), right["counts"][:, 0, 2].sum(), 1.0))
    # 2. the contact pairs taken from the prediction instead of the ground truth
    worst["pairs_from_pred"] = max(_beyond((CT.case_distances(n)["d_pred"] < table[0]).sum(), CT.case_statement(n, table)["pairs"], 1.0)
                                   for n in t if n.endswith("_shift"))
    # 3. the left wrist's absolute error instead of the error of the wrist-to-wrist vector
    names, P, G, S, I = CT.joint_batch()
    b = names.index("offset")
    wrong = np.linalg.norm(P[b, 21].astype(np.float64) - G[b, 21, :3].astype(np.float64)) / S[b]
    worst["absolute_root"] = _beyond(wrong, CT.joint_reference()[b][0], TOL)
    # 4. the scale ignored
    c = t["scale_1p7"]
    wrong = CT.contact_of(CT.distances(c.pr, c.pl, c.gr, c.gl, 1.0), True, table)
    worst["scale_ignored"] = max(_beyond(wrong["pairs"], CT.case_statement("scale_1p7", table)["pairs"], 1.0),
                                 _beyond(CT.mrrpe_of(P[names.index("scaled")], G[names.index("scaled")], 1.0)[0],
                                         CT.joint_reference()[names.index("scaled")][0], TOL))
    # 5. left and right swapped: the right hand's counts in the left hand's row
    worst["hands_swapped"] = max(_beyond(CT.case_statement(n, table)["counts"][::-1], CT.case_statement(n, table)["counts"], 1.0) for n in t)
    # 6. macro instead of micro: the mean of the per-sample precisions instead of sum tp / sum pp
    samples = [CT.case_statement(n, table) for n in t if n.endswith("_noise")]
    micro = CT.metrics_of(samples, [], table)["contact_precision"]
    macro = np.mean([s["counts"].sum(axis=0)[:, 0] / s["counts"].sum(axis=0)[:, 1] for s in samples], axis=0)
    worst["macro_counts"] = _beyond(macro, micro, TOL)
    print(worst)
    assert len(worst) >= 6 and all(v >= 10 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("contact")
    exe = hostbuild.build("contact_host_driver.cpp", d)
    count = [0]

    def run(op, payload):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        np.ascontiguousarray(payload, np.float64).tofile(fin)
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, np.float64)
    return run


def _drive_sample(driver, c, table):
    K = len(table)
    out = driver("sample", np.concatenate([[c.scale, K], table] + [m.astype(np.float64).ravel() for m in (c.pr, c.pl, c.gr, c.gl)]))
    return out[0], out[1], out[2:2 + 6 * K].reshape(2, K, 3), out[2 + 6 * K:].reshape(2, 2, 778)


def test_the_kernels_walk_on_the_host_is_the_statement_on_the_whole_table(driver):
    worst_sum, worst_near = 0.0, 0.0
    for name, c in CT.mesh_cases().items():
        tables = [CT.TABLES[8]] + ([CT.TABLES[1], CT.TABLES[2]] if name in ("deep_0_noise", "dyadic", "scale_1p7") else []) + ([CT.KNOWN_TABLE] if c.known else [])
        for table in tables:
            s = CT.contact_of(CT.case_distances(name), True, tuple(table))
            pair_sum, pairs, counts, near = _drive_sample(driver, c, table)
            assert pairs == s["pairs"] and _same(counts, s["counts"]), (name, len(table))         # |C| and every count EXACT
            assert _close(pair_sum, s["pair_sum"], max(1, s["pairs"]) * TOL) and _close(near, s["near"], TOL), (name, len(table))
            if np.isfinite(s["pair_sum"]):
                worst_sum = max(worst_sum, abs(pair_sum - s["pair_sum"]))
            fin = np.isfinite(s["near"]) & np.isfinite(near)
            worst_near = max(worst_near, float(np.abs(np.where(fin, near, 0.0) - np.where(fin, s["near"], 0.0)).max()))
            if c.known:
                assert pair_sum == s["pair_sum"] and _same(near, s["near"])
    print(f"[driver] worst |pair sum - statement| = {worst_sum:.3e} m, worst |near - statement| = {worst_near:.3e} m")


def test_the_filter_never_changes_a_decision(driver):
    inf, nan = float("inf"), float("nan")
    special = [0.0, -0.0, -1.0, 5e-324, 1e-300, 1e300, inf, -inf, nan]
    for tau in sorted(set(sum(map(tuple, CT.TABLES.values()), ())) | set(CT.KNOWN_TABLE) | {1e-120, 1e160}):
        for sc in (1.0, 0.25, 1.7, 1e-3, 1e3, 1e-200, 1e200, 0.0, -1.0, inf, -inf, nan):
            with np.errstate(all="ignore"):
                t2 = (np.float64(tau) * sc) ** 2
            centre = [t2, t2 * (1 + 2.0 ** -20), t2 * (1 + 2.0 ** -21), t2 * (1 - 2.0 ** -20)]
            sq = list(special)
            for x in centre:
                if np.isfinite(x):
                    y_up = y_dn = np.float64(x)
                    for _ in range(4):                                   # the threshold's float64 neighbours, four either side
                        y_up, y_dn = np.nextafter(y_up, inf), np.nextafter(y_dn, -inf)
                        sq += [y_up, y_dn]
                    sq.append(x)
            sq = np.array(sq, np.float64)
            out = driver("decide", np.concatenate([[tau, sc], sq]))
            limit, dec = out[-1], out[:-1].reshape(-1, 2)
            with np.errstate(all="ignore"):
                want = np.sqrt(sq) / np.float64(sc) < tau
            assert np.array_equal(dec[:, 0], want.astype(np.float64)), (tau, sc)
            assert np.array_equal(dec[:, 1], dec[:, 0]), (tau, sc, limit)
            if not (0 < sc < inf) or not 1e-100 <= tau * sc < 1e150:
                assert limit == inf, (tau, sc, limit)                    # no filter where the proof does not hold
            else:
                assert t2 < limit < t2 * (1 + 2.0 ** -19)
    # on real data the filter leaves only a sliver to the literal expression
    d = CT.case_distances("deep_0_noise")
    sq = (d["d_gt"] ** 2).ravel()[::7]
    out = driver("decide", np.concatenate([[0.003, 1.0], sq]))
    assert np.array_equal(out[:-1].reshape(-1, 2)[:, 1], (np.sqrt(sq) < 0.003).astype(np.float64)) and (sq > out[-1]).mean() > 0.99


def test_contact_index_minimum_and_mrrpe_are_exact(driver):
    inf, nan = float("inf"), float("nan")
    for table in list(CT.TABLES.values()) + [CT.KNOWN_TABLE]:
        t = np.asarray(table, np.float64)
        v = np.concatenate([t, np.nextafter(t, inf), np.nextafter(t, -inf), [0.0, -1.0, inf, -inf, nan, 1e30], CT.case_distances("deep_0_noise")["near"].ravel()[::5]])
        got = driver("index", np.concatenate([[len(t)], t, v]))
        with np.errstate(all="ignore"):
            want = np.array([np.sum(~(x < t)) for x in v], np.float64)    # the thresholds x does not lie below; NaN: all of them
        assert np.array_equal(got, want)
        assert got[v == t[0]][0] == 1 and got[np.isnan(v)][0] == len(t) and got[v == -inf][0] == 0
    assert driver("min", [nan, 3.0, nan, 2.0, 5.0, nan])[0] == 2.0 and driver("min", [nan, nan])[0] == inf
    assert driver("min", [inf, nan])[0] == inf and driver("min", [4.0, -inf, nan])[0] == -inf and driver("min", [])[0:].tolist() == [inf]
    names, P, G, S, I = CT.joint_batch()
    rec = np.concatenate([np.concatenate([P[b, 0], P[b, 21], G[b, 0, :3], G[b, 21, :3], [G[b, 0, 3], G[b, 21, 3], S[b]]]).astype(np.float64)
                          for b in range(len(names))])
    got = driver("mrrpe", rec).reshape(-1, 2)
    want = np.array([CT.mrrpe_of(P[b], G[b], S[b], True) for b in range(len(names))])
    assert got.tobytes() == want.tobytes() or _same(got, want)           # bit for bit (a NaN's payload aside)
    assert _same(got, want) and (got[~np.isnan(got[:, 0])] == want[~np.isnan(want[:, 0])]).all()


# ------------------------------------------------------------------------------------------------------------------ the build
def test_the_two_kernels_use_no_scratch_and_the_lds_the_header_names():
    import ctypes

    from ihmr_amd import hip
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("eval_mrrpe_kernel", "eval_contact_kernel"):
            if k in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == ["eval_contact_kernel", "eval_mrrpe_kernel"], sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    pure = open(os.path.join(ROOT, "ihmr_amd", "csrc", "contact_pure.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (CTP_NV|CTP_MAX_K|CTP_THREADS|CTP_SLOTS) (\d+)", pure)}
    assert const == dict(CTP_NV=778, CTP_MAX_K=8, CTP_THREADS=256, CTP_SLOTS=4)
    expr = re.search(r"#define CTP_LDS_BYTES \((.*)\)\s+//", pure).group(1)
    lds = eval(expr, {"__builtins__": {}}, const)
    assert lds == 37840 == 6 * 778 * 8 + 64 + 320 + 108 + 4                           # six target arrays, table, partial sums, histograms, pairs
    assert seen["eval_contact_kernel"]["group_segment_fixed_size"] == lds < 64 * 1024 and seen["eval_mrrpe_kernel"]["group_segment_fixed_size"] == 0
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:[A-Za-z_][\w ]*?[\s*]+)(ihmr_\w+)\s*\(", header, flags=re.M))
    assert {"ihmr_eval_mrrpe", "ihmr_eval_contact"} <= declared
    assert declared == set(hip.EXPORTED_SYMBOLS), declared ^ set(hip.EXPORTED_SYMBOLS)
    assert int(re.search(r"#define IHMR_EVAL_MAX_CONTACT_THRESHOLDS (\d+)", header).group(1)) == hip.EVAL_MAX_CONTACT_THRESHOLDS == E.MAX_CONTACT_THRESHOLDS == 8
    L = ctypes.CDLL(hip.build())
    for sym in ("ihmr_eval_mrrpe", "ihmr_eval_contact"):
        getattr(L, sym)

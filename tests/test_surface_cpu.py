"""The exact point-to-surface signed distance without a GPU: the known answers of the float64 statement
of tests/surface_ref.py, its analytic gradient against central differences, the margin rule on the whole case table,
csrc/surface_pure.h built for the host with ASan / UBSan (tests/surface_host_driver.cpp walks every case in the kernels' order and is
run as a program), four wrong rules that the cases tell apart, the Evaluator with the flag off (byte-identical) and on (sums additive
over split batches), and the build: both kernels without scratch memory or spills, the LDS the header names, every declared symbol
exported."""
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
import surface_ref as SR  # noqa: E402

from ihmr_amd import evaluator as E  # noqa: E402

DIST_TOL, BARY_TOL = 1e-12, 1e-9            # the driver's distance [m] and weights against the statement


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("name", ["cube", "cube_bad_faces", "tetrahedron", "nothing_usable"])
def test_known_answers_are_exact(name):
    c, st = SR.cases()[name], SR.statement(name)
    assert len(c.known) >= 3
    for i, (q, dist, face, bary) in enumerate(c.known):
        assert _same(st["dist"][i], dist) and st["face"][i] == face and st["bary"][i].tolist() == list(bary), (name, i, st["dist"][i], st["face"][i], st["bary"][i])
        assert _same(c.points[i], np.float32(q))
    if name == "cube_bad_faces":        # the three faces in front and the two behind do not count: the cube's answers, ids shifted by 3
        use = SR.usable_faces(c.verts, c.faces)
        assert use.tolist() == [False] * 3 + [True] * 12 + [False] * 2
        cube = SR.statement("cube")
        assert _same(st["dist"][:8], cube["dist"]) and _same(st["face"][:8], cube["face"] + 3) and _same(st["bary"][:8], cube["bary"])
        assert np.isnan(st["dist"][8:]).all() and (st["face"][8:] == -1).all() and not st["bary"][8:].any()


def test_the_unsigned_distance_and_an_open_table():
    c = SR.cases()["cube"]
    plain = SR.surface_distance(c.points, c.verts, c.faces, 12, signed=False)
    assert _same(plain["dist"], np.abs(SR.statement("cube")["dist"])) and _same(plain["face"], SR.statement("cube")["face"])
    # without its cap the hand is open: the distances are the closed hand's, some parities are not
    full, cut = SR.statement("deep_0_r_on_l"), SR.statement("open_mesh")
    assert _same(np.abs(full["dist"]), np.abs(cut["dist"])) and _same(full["face"], cut["face"])


def test_a_sphere_is_met_within_its_polyhedrons_own_bound():
    sv, sf = SR.icosphere(2, 0.5)
    assert sv.shape == (162, 3) and sf.shape == (320, 3)
    r_in, r_out = SR.sphere_bounds(sv, sf)
    assert 0.48 < r_in < r_out <= 0.5 + 1e-7
    for P in SR.SIZES:
        c, st = SR.cases()[f"sphere_P{P}"], SR.statement(f"sphere_P{P}")
        r = np.linalg.norm(c.points.astype(np.float64), axis=1)
        assert c.shape[0] == P and ((st["dist"] < 0) == (r < r_in)).all()
        d = np.abs(st["dist"])
        lo = np.where(r > r_out, r - r_out, r_in - r)                   # the polyhedron lies between the two spheres
        hi = np.where(r > r_out, r - r_in, r_out - r)
        assert (d >= lo - 1e-12).all() and (d <= hi + 1e-12).all()
        assert np.abs(d - np.abs(r - 0.5)).max() <= (r_out - r_in) + 1e-7


def test_the_case_table_holds_what_it_claims():
    t = SR.cases()
    assert [c.shape[0] for n, c in t.items() if n.startswith("sphere_P")] == [1, 255, 256, 257, 778, 1025]
    inside = {n: int((SR.statement(n)["dist"] < 0).sum()) for n in t}
    assert all(inside[n] > 0 for n in t if n.endswith(("_r_on_l", "_l_on_r"))) and inside["deep_0_r_on_l"] > 100
    assert inside["apart_1m"] == 0 and SR.statement("apart_1m")["dist"].min() > 0.8
    assert inside["shifted_2m"] == inside["deep_0_r_on_l"] == inside["scale_1p7"]
    assert np.abs(SR.statement("shifted_2m")["dist"] - SR.statement("deep_0_r_on_l")["dist"]).max() < 1e-6      # float32 inputs moved by 2 m
    assert t["deep_0_r_on_l"].shape == (778, 778, 1552, 1538) and t["open_mesh"].shape == (778, 778, 1538, 1538)
    # every region is met on the hands: weights with two, one and no zero
    zeros = (SR.statement("deep_0_r_on_l")["bary"] == 0).sum(axis=1)
    assert {0, 1, 2} <= set(zeros.tolist())


def test_every_case_keeps_the_margins():
    assert SR.margin_violations() == []
    assert SR.evaluator_threshold_violations() == []
    # the check sees what it should: a ray through a vertex, a start on a plane
    on_edge = SR.surface_distance(np.float32([[0.5, 0.0, 0.5]]), SR.CUBE_VERTS, SR.CUBE_FACES, 12)
    on_plane = SR.surface_distance(np.float32([[1.0, 0.25, 0.5]]), SR.CUBE_VERTS, SR.CUBE_FACES, 12)
    assert on_edge["margin"] < SR.RAY_MARGIN and on_plane["margin"] < SR.RAY_MARGIN


# ------------------------------------------------------------------------------------------------------------------ gradient
@pytest.mark.parametrize("name", ["tetrahedron", "cube", "sphere_P255"])
def test_statement_gradient_against_central_differences(name):
    c = SR.cases()[name]
    q, v = c.points.astype(np.float64)[:48], c.verts.astype(np.float64)
    q = q[np.isfinite(q).all(axis=1)]
    f = lambda qq, vv: SR.surface_distance(qq, vv, c.faces, c.F_dist)["dist"]
    h = 1e-6
    base = f(q, v)
    # a query within h of a region boundary or of a tie has one-sided slopes that differ: it is left out by that test alone
    dq = np.zeros((len(q), 3))
    smooth = np.ones(len(q), bool)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        up, dn = f(q + e, v), f(q - e, v)
        dq[:, k] = (up - dn) / (2 * h)
        smooth &= np.abs((up - base) - (base - dn)) / h < 1e-4
    st = SR.surface_distance(q, v, c.faces, c.F_dist)
    g = np.linspace(0.5, 1.5, len(q))
    d_points, d_verts = SR.gradient(q, v, c.faces, st, g)
    assert smooth.sum() >= min(24, len(q) - 4), smooth.sum()
    assert np.abs(d_points[smooth] - g[smooth, None] * dq[smooth]).max() < 1e-6
    assert np.abs(np.linalg.norm(d_points[smooth], axis=1) - g[smooth]).max() < 1e-12          # |n| = 1
    if len(v) <= 8:
        gs = np.where(smooth, g, 0.0)
        want = np.zeros_like(v)
        for i in range(len(v)):
            for k in range(3):
                e = np.zeros_like(v)
                e[i, k] = h
                want[i, k] = (gs * (f(q, v + e) - f(q, v - e))).sum() / (2 * h)
        got = SR.gradient(q, v, c.faces, st, gs)[1]
        assert np.abs(got - want).max() < 1e-5 and np.abs(want).max() > 0.1, (got, want)
        assert np.abs(got.sum(axis=0) + SR.gradient(q, v, c.faces, st, gs)[0].sum(axis=0)).max() < 1e-12     # a common shift changes nothing


def test_gradient_is_zero_on_the_surface_and_for_a_nan():
    c = SR.cases()["cube_bad_faces"]
    q = np.concatenate([c.points, np.float32([[1.0, 1.0, 1.0]])])                        # the last one IS vertex 7
    st = SR.surface_distance(q, c.verts, c.faces, c.F_dist)
    d_points, d_verts = SR.gradient(q, c.verts, c.faces, st, np.ones(len(q)))
    assert st["dist"][-1] == 0 and not d_points[-1].any() and not d_points[8:10].any() and np.isfinite(d_verts[:8]).all()
    assert np.abs(d_points[0] - [0, 0, 1]).max() == 0 and np.abs(d_points[4] - [0, 0, 1]).max() == 0      # outside and inside: away from the inside


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("surface")
    exe = hostbuild.build("surface_host_driver.cpp", d)
    count = [0]

    def run(c, g=None, signed=1, F_dist=None):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        P, V, F_total, fd = c.shape
        g = np.ones(P) if g is None else g
        with open(fin, "wb") as fh:
            for a in (np.array([P, V, F_total, fd if F_dist is None else F_dist, signed], np.int32), c.points, c.verts, c.faces, np.asarray(g, np.float64)):
                fh.write(np.ascontiguousarray(a).tobytes())
        hostbuild.run(exe, fin, fout)
        out = np.fromfile(fout, np.float64)
        cut = np.cumsum([P, P, 3 * P, 3 * P, 3 * V])
        assert len(out) == cut[-1]
        dist, face, bary, d_points, d_verts = np.split(out, cut[:-1])
        return dict(dist=dist, face=face.astype(np.int64), bary=bary.reshape(P, 3), d_points=d_points.reshape(P, 3), d_verts=d_verts.reshape(V, 3))
    return run


def test_the_kernels_walk_on_the_host_is_the_statement_on_the_whole_table(driver):
    worst = [0.0, 0.0]
    for name, c in SR.cases().items():
        d, w = SR.check_against_statement(c, SR.statement(name), driver(c), DIST_TOL, BARY_TOL, name)
        worst = [max(worst[0], d), max(worst[1], w)]
    print(f"[driver] worst ||dist| - statement| = {worst[0]:.3e} m, worst |weight - statement| = {worst[1]:.3e}")
    c = SR.cases()["cube"]
    plain = driver(c, signed=0)
    assert _same(plain["dist"], np.abs(SR.statement("cube")["dist"])) and _same(plain["face"], SR.statement("cube")["face"])


@pytest.mark.parametrize("name", ["deep_0_r_on_l", "cube_bad_faces", "tetrahedron", "sphere_P257"])
def test_the_backward_walk_on_the_host_is_the_statements_gradient(driver, name):
    c, st = SR.cases()[name], SR.statement(name)
    g = np.random.RandomState(3).uniform(0.5, 1.5, c.shape[0])
    got = driver(c, g=g)
    d_points, d_verts = SR.gradient(c.points, c.verts, c.faces, st, g)
    # ties aside (the known answers decide them alike), the driver's face is the statement's: compare where it is
    same = got["face"] == st["face"]
    assert same.mean() > 0.9
    ulp = 2.0 ** -23
    assert np.abs(got["d_points"][same] - d_points[same]).max() <= 1.5 * ulp + 1e-9
    if same.all():
        terms = np.zeros_like(d_verts)
        ids = c.faces[np.where(st["face"] >= 0, st["face"], 0)]
        for k in range(3):
            np.add.at(terms, ids[st["face"] >= 0, k], np.abs(st["bary"][st["face"] >= 0, k] * g[st["face"] >= 0])[:, None] * np.ones(3))
        assert (np.abs(got["d_verts"] - d_verts) <= ulp * np.maximum(terms, 1.0) + 1e-9).all()
    nan = np.isnan(st["dist"])
    assert not got["d_points"][nan].any()


# ------------------------------------------------------------------------------------------------------------------ wrong rules
def test_four_wrong_rules_each_land_ten_times_beyond_the_bar():
    """The bars: a distance within 1e-9 m (the device bar; the driver's is tighter), a count exact (bar 1), a depth sum within 1e-9
    relative.  Each wrong rule lands at least ten bars away on some case of the table."""
    worst = {}
    c, st = SR.cases()["cap_probe"], SR.statement("cap_probe")
    cap = SR.surface_distance(c.points, c.verts, c.faces, len(c.faces))                      # 1. cap faces counted as surface
    worst["cap_is_surface"] = float(np.abs(np.abs(cap["dist"]) - np.abs(st["dist"])).max() / SR.TOL)
    assert (cap["face"] >= SR.NF).any() and (st["face"] < SR.NF).all()
    c, st = SR.cases()["deep_0_r_on_l"], SR.statement("deep_0_r_on_l")
    plain = SR.surface_distance(c.points, c.verts, c.faces, c.F_dist, signed=False)         # 2. the sign ignored
    worst["sign_ignored"] = float(np.abs(plain["dist"] - st["dist"]).max() / SR.TOL)
    near = SR.vertex_distance(c.points, c.verts)                                             # 3. vertex-to-vertex instead of surface
    worst["vertex_to_vertex"] = float(np.abs(near - np.abs(st["dist"])).max() / SR.TOL)
    assert (near >= np.abs(st["dist"]) - 1e-12).all()
    right = SR.expected_surface_sums(SR.THRESHOLDS)                                          # 4. the scale ignored
    wrong = SR.expected_surface_sums(SR.THRESHOLDS, scale=1.0)
    worst["scale_ignored"] = max(float(np.abs(wrong[5:] - right[5:]).max()), float(np.abs(wrong[0] - right[0]) / (1e-9 * right[0])))
    print(worst)
    assert len(worst) >= 4 and all(v >= 10 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------------ the Evaluator
PARENT_ATTRIBUTES = ["pa_metrics", "curve_metrics", "thresholds", "f_thresholds", "inputSize", "left_hand_faces", "right_hand_faces",
                     "root_weights", "data_list", "image_root", "save_verts", "pred_results", "_device_parts", "_device_vert_parts",
                     "_device_pa_parts", "_device_pa_vert_parts", "_device_curve_parts", "_device_curve_vert_parts"]


def _records(n=3):
    rng = np.random.RandomState(11)
    g = rng.normal(0, 0.05, (n, 42, 3)).astype(np.float32)
    res = dict(pred_cam_params=np.zeros((n, 3), np.float32), pred_shape_params=np.zeros((n, 20), np.float32),
               pred_pose_params=np.zeros((n, 96), np.float32), pred_hand_trans=np.zeros((n, 3), np.float32),
               pred_joints_3d=g + rng.normal(0, 0.01, g.shape).astype(np.float32),
               gt_joints_3d=np.concatenate([g, np.ones((n, 42, 1), np.float32)], axis=2),
               collision_loss_origin_scale=rng.uniform(0, 0.01, (n, 1556)).astype(np.float32))
    return res


def test_flag_off_nothing_changes():
    res = _records()
    for kw in (dict(), dict(pa_metrics=True, curve_metrics=True, interaction_metrics=True)):
        extra = ["interaction_metrics", "contact_thresholds", "_device_mrrpe_parts", "_device_contact_parts"] if kw else []
        off, on = E.Evaluator(CC.mano_models(), **kw), E.Evaluator(CC.mano_models(), surface_metrics=True, **kw)
        assert list(off.__dict__) == PARENT_ATTRIBUTES + extra
        assert list(on.__dict__) == PARENT_ATTRIBUTES + extra + ["surface_metrics", "surface_thresholds", "_device_surface_parts"]
        for ev in (off, on):
            ev.update(np.arange(3), {k: v.copy() for k, v in res.items()})
        assert pickle.dumps(off.pred_results) == pickle.dumps(on.pred_results)                # the records: byte for byte
        for name in ("metric_sums", "pa_metric_sums", "curve_sums", "volume_sums", "interaction_sums"):
            assert getattr(off, name)().tobytes() == getattr(on, name)().tobytes(), name
        p_off, p_on = off.packed_sums(), on.packed_sums()
        assert len(p_on) == len(p_off) + 11 and p_on[:len(p_off)].tobytes() == p_off.tobytes()      # the last family: no slice moves
        assert not p_on[len(p_off):].any() and not off.surface_sums().any() and len(off.surface_sums()) == 11
        m_off, m_on = off.metrics_from_packed(p_off), on.metrics_from_packed(p_on)
        assert "pen_depth_max" not in m_off and list(m_on)[:len(m_off)] == list(m_off) and np.isnan(m_on["pen_depth_max"])
        back = pickle.loads(pickle.dumps(off))
        assert list(back.__dict__) == PARENT_ATTRIBUTES + extra and not hasattr(back, "surface_metrics")
        on.clear()
        off.clear()
        assert on._device_surface_parts == [] and list(off.__dict__) == PARENT_ATTRIBUTES + extra
    empty = pickle.dumps(E.Evaluator())
    assert b"surface" not in empty and pickle.dumps(E.Evaluator()) == empty
    with pytest.raises(ValueError):
        E.Evaluator(surface_thresholds=(0.003,))
    with pytest.raises(RuntimeError, match="surface_metrics=True"):
        E.Evaluator().update_device_surface(None, None)
    assert E.Evaluator(surface_metrics=True).surface_thresholds.tolist() == [0.003, 0.005] == list(E.SURFACE_THRESHOLDS)
    for table in ((), tuple(np.linspace(0.001, 0.009, 9)), (0.005, 0.003), (0.003, float("nan"))):
        with pytest.raises(ValueError):
            E.Evaluator(surface_metrics=True, surface_thresholds=table)


def _parts_of(rows, table):
    """What ``update_device_surface`` leaves for the given rows of the statement's batch, as host tensors."""
    import torch
    per = [SR.expected_surface_sums(table, rows=[b]) for b in rows]
    return (torch.from_numpy(np.stack([p[:5] for p in per])), torch.from_numpy(np.stack([p[5:].reshape(len(table), 3) for p in per])))


@pytest.mark.parametrize("K", sorted(SR.TABLES))
def test_surface_sums_add_over_split_batches_and_give_the_metrics(K):
    table = SR.TABLES[K]
    B = len(SR.evaluator_batch()["keep"])
    whole = E.Evaluator(CC.mano_models(), surface_metrics=True, surface_thresholds=table)
    whole._device_surface_parts.append(_parts_of(range(B), table))
    want = SR.expected_surface_sums(table)
    got = whole.surface_sums()
    assert got.shape == (5 + 3 * K,) and _same(got[2:], want[2:]) and np.abs(got[:2] - want[:2]).max() <= 1e-12 * want[0]
    assert want[3] >= 3 and 0 < want[4] < want[3] and want[2] > 100 and want[5:].all()
    split = E.Evaluator(CC.mano_models(), surface_metrics=True, surface_thresholds=table)
    for rows in (range(0, 2), range(2, 3), range(3, B)):
        split._device_surface_parts.append(_parts_of(rows, table))
    assert _same(split.surface_sums()[2:], got[2:]) and np.abs(split.surface_sums()[:2] - got[:2]).max() <= 1e-12 * got[0]
    m = whole.metrics_from_packed(whole.packed_sums())
    assert m["pen_depth_max"] == got[0] / got[3] and m["pen_depth_ave"] == got[1] / got[3] and m["pen_vertex_rate"] == got[2] / (1556 * got[3])
    assert 1.0 < m["pen_depth_max"] < 60 and 0 < m["pen_depth_ave"] < m["pen_depth_max"] and 0 < m["pen_vertex_rate"] < 0.5
    c = got[5:].reshape(K, 3)
    assert _same(m["surface_contact_precision"], c[:, 0] / c[:, 1]) and _same(m["surface_contact_recall"], c[:, 0] / c[:, 2])
    assert ((0 < m["surface_contact_f1"]) & (m["surface_contact_f1"] < 1)).all()
    f = E.Evaluator.surface_metrics_from_sums
    m = f(np.array([6.0, 3.0, 1556.0, 2, 0, 0, 0, 5, 1, 2, 4], np.float64))
    assert m["pen_depth_max"] == 3.0 and m["pen_depth_ave"] == 1.5 and m["pen_vertex_rate"] == 0.5
    assert np.isnan(m["surface_contact_precision"][0]) and m["surface_contact_recall"][0] == 0 and np.isnan(m["surface_contact_f1"][0])
    assert m["surface_contact_precision"][1] == 0.5 and m["surface_contact_recall"][1] == 0.25
    assert all(np.isnan(v).all() for v in f(np.zeros(11)).values())
    with pytest.raises(AssertionError):
        f(np.zeros(8))


# ------------------------------------------------------------------------------------------------------------------ the build
def test_the_two_kernels_use_no_scratch_and_the_lds_the_header_names():
    import ctypes

    from ihmr_amd import hip
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("surface_dist_kernel", "surface_dist_bwd_kernel"):
            if k + "PK" in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == ["surface_dist_bwd_kernel", "surface_dist_kernel"], sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)                                          # four waves per SIMD at the least
    pure = open(os.path.join(ROOT, "ihmr_amd", "csrc", "surface_pure.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (SRF_MAX_VERTS|SRF_MAX_FACES|SRF_THREADS|SRF_BWD_SLOTS) (\d+)", pure)}
    assert const == dict(SRF_MAX_VERTS=1024, SRF_MAX_FACES=2048, SRF_THREADS=256, SRF_BWD_SLOTS=4)
    lds = {k: eval(v, {"__builtins__": {}}, const) for k, v in re.findall(r"#define (SRF_LDS_BYTES|SRF_BWD_LDS_BYTES) \((.*)\)\s+//", pure)}
    assert lds == dict(SRF_LDS_BYTES=1024 * 12 + 2048 * 4, SRF_BWD_LDS_BYTES=256 * 60)
    assert seen["surface_dist_kernel"]["group_segment_fixed_size"] == lds["SRF_LDS_BYTES"] == 20480
    assert seen["surface_dist_bwd_kernel"]["group_segment_fixed_size"] == lds["SRF_BWD_LDS_BYTES"] == 15360
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:[A-Za-z_][\w ]*?[\s*]+)(ihmr_\w+)\s*\(", header, flags=re.M))
    assert {"ihmr_surface_distance", "ihmr_surface_distance_bwd"} <= declared
    assert declared == set(hip.EXPORTED_SYMBOLS), declared ^ set(hip.EXPORTED_SYMBOLS)
    limits = {k: int(v) for k, v in re.findall(r"#define (IHMR_SURFACE_MAX_VERTS|IHMR_SURFACE_MAX_FACES) (\d+)", header)}
    assert limits == dict(IHMR_SURFACE_MAX_VERTS=hip.SURFACE_MAX_VERTS, IHMR_SURFACE_MAX_FACES=hip.SURFACE_MAX_FACES) and hip.SURFACE_MAX_VERTS == 1024
    L = ctypes.CDLL(hip.build())
    for sym in ("ihmr_surface_distance", "ihmr_surface_distance_bwd"):
        getattr(L, sym)

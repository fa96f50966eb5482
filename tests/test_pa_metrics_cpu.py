"""The Procrustes-aligned metrics without a GPU: the host functions of ihmr_amd/evaluator.py against the reference's recorded results
(tests/golden/metrics_pa.npz) and the float64 statement of tests/pa_cases.py; csrc/eval_pure.h built for the host with ASan / UBSan
(tests/eval_pure_driver.cpp) against the same statement; the Evaluator's records, sums and their reduction over two gloo ranks; and the
build: both kernels without scratch memory, every declared symbol exported."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj  # noqa: E402
import hostbuild  # noqa: E402
import pa_cases as PC  # noqa: E402

from ihmr_amd import evaluator as E  # noqa: E402

TOL = 1e-9          # [m] the float64 route; the float32 route of the reference is held to 1e-7 like tests/golden/metrics.npz


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "metrics_pa.npz")))


def _valid_sets():
    """(name, set index, pred (n,3), gt (n,3)) float64 of every set of every case that the set rules keep."""
    out = []
    for name, (pred, gt, scale) in PC.joint_cases().items():
        for s, (lo, hi) in enumerate(PC.JOINT_SETS):
            w = gt[lo:hi, 3]
            if PC.set_errors(pred[lo:hi], gt[lo:hi, :3], w) is not None:
                out.append((f"{name}/{s}", pred[lo:hi][w > 0].astype(np.float64), gt[lo:hi, :3][w > 0].astype(np.float64)))
    names, P, G, W, S = PC.vert_batch()
    for b, name in enumerate(names):
        for h in range(2):
            out.append((f"verts/{name}/{h}", P[b, h].astype(np.float64), G[b, h].astype(np.float64)))
    return out


def test_every_case_is_well_conditioned():
    """g = (s2 + d s3) / s1 >= 1e-2 for every kept set with three or more points: a condition on the inputs; no case is left out."""
    sets = _valid_sets()
    assert len(sets) >= 40
    for name, p, g in sets:
        if len(p) >= 3:
            assert PC.gap(p, g) >= PC.GAP_MIN, (name, PC.gap(p, g))
    counts = sorted({len(p) for _, p, _ in sets})
    assert counts[:3] == [2, 3, 4] and 42 in counts and 778 in counts


# ------------------------------------------------------------------------------------------------------------------ against the reference
def test_calc_transform_and_use_rot_match_the_reference(golden):
    for name in golden["names"]:
        pred, gt, scale = golden[f"{name}_pred"], golden[f"{name}_gt"], float(golden[f"{name}_scale"])
        valid = gt[:, 3] > 0
        assert pred.dtype == np.float32 and gt.dtype == np.float32
        a32 = E.calc_transform(pred[valid].copy(), gt[valid, :3].copy())
        a64 = E.calc_transform(pred[valid].astype(np.float64), gt[valid, :3].astype(np.float64))
        assert a32.shape == a64.shape == (int(valid.sum()), 3)
        assert np.abs(a32 - golden[f"{name}_aligned32"]).max() <= 1e-7, name
        assert np.abs(a64 - golden[f"{name}_aligned64"]).max() <= TOL, name
        e32 = E.get_single_pa_inter_joints_error(pred, gt[:, :3], gt[:, 3:], scale, use_rot=True)
        e64 = E.get_single_pa_inter_joints_error(pred.astype(np.float64), gt[:, :3].astype(np.float64), gt[:, 3:].astype(np.float64), scale, use_rot=True)
        assert len(e32) == len(e64) == int(valid.sum())
        assert np.abs(np.array(e32) - golden[f"{name}_ref32"]).max() <= 1e-7, name
        assert np.abs(np.array(e64) - golden[f"{name}_ref64"]).max() <= TOL, name
        # the keyword's default is the behaviour from before the keyword existed
        assert (E.get_single_pa_inter_joints_error(pred, gt[:, :3], gt[:, 3:], scale)
                == E.get_single_pa_inter_joints_error(pred, gt[:, :3], gt[:, 3:], scale, use_rot=False)
                == (np.linalg.norm(E.calc_transform_no_rot(pred[valid].copy(), gt[valid, :3].copy()) - gt[valid, :3], axis=1) / scale).tolist())


def test_procrustes_align_is_the_reference_in_float64_except_for_two_and_three_points(golden):
    far = 0.0
    for name in golden["names"]:
        pred, gt, scale = golden[f"{name}_pred"], golden[f"{name}_gt"], float(golden[f"{name}_scale"])
        valid = gt[:, 3] > 0
        err = np.array(E.get_single_pa_error(pred, gt[:, :3], gt[:, 3], scale))
        aligned = E.procrustes_align(pred[valid], gt[valid, :3])
        assert aligned.dtype == np.float64 and np.abs(aligned - PC.procrustes_rows(pred[valid], gt[valid, :3])).max() <= 1e-12
        d = float(np.abs(err - golden[f"{name}_ref64"]).max())
        if valid.sum() not in (2, 3):
            assert d <= TOL, (name, d)
            far = max(far, float(np.abs(golden[f"{name}_ref32"] - golden[f"{name}_ref64"]).max()))
        elif valid.sum() == 3:
            assert d > 1e-3, (name, d)                  # the reference read the (3,3) input as coordinates x points
        else:
            assert err.max() <= TOL, (name, err)        # points in rows: two points land on their targets
            assert golden[f"{name}_ref64"].max() > 1e-3  # ... which the reference's reading of (2,3) does not do
    # the reference's own float32 route lies farther from float64 than the bar the device path is held to
    assert far > TOL, far


def test_set_rules():
    rng = np.random.RandomState(3)
    g = rng.randn(21, 3) * 0.05
    p = g + rng.randn(21, 3) * 0.01
    w = np.zeros(21)
    w[[2, 4, 6, 9, 11]] = 0.3                                        # five valid joints, weight sum 1.5
    assert E.get_single_pa_error(p, g, w, 1.0) == []
    w[[2, 4, 6, 9, 11]] = 0.4                                        # the same five at sum 2.0 are kept
    assert len(E.get_single_pa_error(p, g, w, 1.0)) == 5
    assert E.get_single_pa_error(p, g, np.zeros(21), 1.0) == []
    # var1 == 0: the reference divides by zero.  The inputs are float32 numbers, as everything a model exports: in float64 the sum of
    # up to 2^29 equal float32 values is exact, so their mean is the value itself and var1 is exactly 0 on the host and on the device
    same = np.tile(p[:1].astype(np.float32), (21, 1))
    assert E.procrustes_align(same, g) is None and E.get_single_pa_error(same, g, np.ones(21), 1.0) == []
    one = np.zeros(21)
    one[5] = 2.5                                                     # weight sum >= 2 on ONE point: var1 == 0 again
    assert E.get_single_pa_error(p, g, one, 1.0) == []
    e1, e2 = E.get_single_pa_error(p, g, np.ones(21), 1.0), E.get_single_pa_error(p, g, np.ones(21), 2.0)
    assert np.allclose(np.array(e1) / 2.0, e2, rtol=1e-15, atol=0)   # scale_factor divides
    # an exact similarity leaves nothing; a mirrored set cannot be rotated onto its target
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    assert np.abs(E.procrustes_align(1.7 * g @ R.T + [1.0, 2.0, 3.0], g) - g).max() <= 1e-14
    mirrored = E.procrustes_align(g * [-1.0, 1.0, 1.0], g)
    assert np.abs(mirrored - g).max() > 1e-3
    for name, p, g in _valid_sets():
        assert np.abs(E.procrustes_align(p, g) - PC.procrustes_rows(p, g)).max() <= 1e-12, name


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_pure")
    exe = hostbuild.build("eval_pure_driver.cpp", d)
    count = [0]

    def run(op, payload):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        np.ascontiguousarray(payload, np.float64).tofile(fin)
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, np.float64)
    return run


def _moments(p, g):
    m1, m2 = p.mean(axis=0), g.mean(axis=0)
    x1, x2 = p - m1, g - m2
    return np.concatenate([[len(p)], m1, m2, (x1.T @ x2).ravel(), [np.sum(x1 ** 2)]])


def _check_transforms(sets, T):
    worst = 0.0
    for (name, p, g), r in zip(sets, T):
        R, scale, t = r[:9].reshape(3, 3), r[9], r[10:]
        assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12, name
        d = float(np.abs(scale * (p @ R.T) + t - PC.procrustes_rows(p, g)).max())
        worst = max(worst, d)
        assert d <= TOL, (name, d)
    return worst


def test_pure_header_on_the_case_table(driver):
    sets = _valid_sets()
    T = driver("moments", np.concatenate([_moments(p, g) for _, p, g in sets])).reshape(-1, 13)
    assert len(T) == len(sets)
    print("[eval_pure] case table: max |aligned - statement| =", _check_transforms(sets, T))
    # the error function, on one set
    name, p, g = sets[0]
    e = driver("errors", np.concatenate([_moments(p, g), np.concatenate([p, g], axis=1).ravel()]))
    assert np.abs(e - np.linalg.norm(PC.procrustes_rows(p, g) - g, axis=1)).max() <= TOL


def test_pure_header_on_ten_thousand_seeded_moment_sets(driver):
    rng = np.random.RandomState(10000)
    sets = []
    for i in range(10000):
        n = int(rng.choice([3, 4, 5, 8, 21, 42, 100]))
        g = PC._cloud(rng, n)
        mode = i % 4
        s, t = rng.uniform(0.3, 3.0), rng.randn(3) * (3.0 if mode == 1 else 0.1)
        p = s * (g @ PC._rotation(rng, rng.uniform(0.0, np.pi)).T) + t + rng.randn(n, 3) * 0.004
        if mode == 2:
            p = p * np.array([1.0, 1.0, -1.0])                      # the reflection branch of the SVD form
        if n >= 3 and PC.gap(p, g) < PC.GAP_MIN:                    # keep the table inside the stated conditioning
            continue
        sets.append((f"seeded {i}", p, g))
    assert len(sets) >= 9000, len(sets)
    T = driver("moments", np.concatenate([_moments(p, g) for _, p, g in sets])).reshape(-1, 13)
    print(f"[eval_pure] {len(sets)} seeded sets: max |aligned - statement| =", _check_transforms(sets, T))


def test_pure_header_returns_finite_values_for_degenerate_moments(driver):
    z3 = np.zeros(3)
    u, v = np.array([1.0, 2.0, -0.5]), np.array([0.3, -1.0, 2.0])
    u2, v2 = np.array([0.5, -1.0, 0.25]), np.array([-2.0, 0.1, 0.7])
    recs = [np.concatenate([[5], z3, z3, np.zeros(9), [0.0]]),                                   # all-zero M, var1 == 0
            np.concatenate([[5], z3 + 1, z3 - 1, np.zeros(9), [2.0]]),                           # all-zero M, var1 > 0
            np.concatenate([[2], z3, z3, np.outer(u, v).ravel(), [u @ u]]),                      # rank 1
            np.concatenate([[3], z3, z3, (np.outer(u, v) + np.outer(u2, v2)).ravel(), [u @ u + u2 @ u2]]),   # rank 2
            np.concatenate([[2], z3, z3, np.outer(u, -u).ravel(), [u @ u]])]                     # rank 1, a half turn: a double top eigenvalue
    T = driver("moments", np.concatenate(recs)).reshape(-1, 13)
    assert np.isfinite(T).all()
    for r in T:
        R = r[:9].reshape(3, 3)
        assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    assert T[0, 9] == 0.0 and T[1, 9] == 0.0 and np.array_equal(T[0, :9].reshape(3, 3), np.eye(3))
    # rank 1 from two points: x1 = +-u, x2 = +-v; the aligned points are +-v * (|u||v| / |u|^2) * ... = the targets' direction
    R, scale = T[2, :9].reshape(3, 3), T[2, 9]
    assert np.abs(scale * (R @ u) - v * (np.linalg.norm(u) / np.linalg.norm(v)) * (np.linalg.norm(v) / np.linalg.norm(u))).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ Evaluator
def _pred(num, seed=0, with_verts=True):
    rng = np.random.RandomState(seed)
    gt = rng.normal(0, 0.05, (num, 42, 3)).astype(np.float32)
    pred = gt + rng.normal(0, 0.005, (num, 42, 3)).astype(np.float32)
    w = np.ones((num, 42, 1), np.float32)
    w[1, 21:] = 0                       # sample 1: right hand only
    w[2, :] = 0                         # sample 2: nothing valid
    d = dict(pred_cam_params=np.zeros((num, 3), np.float32), pred_shape_params=np.zeros((num, 20), np.float32),
             pred_pose_params=np.zeros((num, 96), np.float32), pred_hand_trans=np.zeros((num, 1, 3), np.float32),
             pred_joints_3d=pred, gt_joints_3d=np.concatenate([gt, w], 2),
             collision_loss_origin_scale=np.abs(rng.normal(0, 1e-3, (num, 1556))).astype(np.float32))
    if with_verts:
        gv = rng.normal(0, 0.04, (2, num, 778, 3)).astype(np.float32)
        pv = gv + rng.normal(0, 0.003, (2, num, 778, 3)).astype(np.float32)
        mw = np.ones((num, 2), np.float32)
        mw[0, 1] = 0
        d.update(gt_right_hand_verts=gv[0], gt_left_hand_verts=gv[1], pred_right_hand_verts=pv[0], pred_left_hand_verts=pv[1], mano_params_weight=mw)
    return d


def _mano():
    import types
    one_hot = np.zeros(778, np.float32)
    one_hot[0] = 1.0
    m = types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=np.stack([one_hot] * 16))
    return dict(right=m, left=m)


def test_evaluator_records_sums_and_properties():
    num = 5
    res = _pred(num)
    off, on = E.Evaluator(_mano()), E.Evaluator(_mano(), pa_metrics=True)
    off.update(np.arange(num), {k: v.copy() for k, v in res.items()})
    on.update(np.arange(num), {k: v.copy() for k, v in res.items()})
    new_keys = {"pa_inter_j3d_error", "pa_j3d_error", "pa_v3d_error"}
    for a, b in zip(off.pred_results, on.pred_results):
        assert set(b) - set(a) == new_keys and not (set(a) & new_keys)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    assert len(off.metric_sums()) == 9 and np.array_equal(off.metric_sums(), on.metric_sums())
    assert np.array_equal(off.pa_metric_sums(), np.zeros(6))
    # a model without GT meshes: no pa_v3d_error key, as v3d_error stays empty
    plain = E.Evaluator(pa_metrics=True)
    plain.update(np.arange(num), _pred(num, with_verts=False))
    assert all("pa_v3d_error" not in r and r["v3d_error"] == [] for r in plain.pred_results)
    assert np.isnan(plain.pa_mpvpe_3d) and "pa_mpvpe_3d" not in E.Evaluator.pa_metrics_from_sums(plain.pa_metric_sums())
    # the sums against the statement
    gt = res["gt_joints_3d"]
    st = [PC.joints_statement(res["pred_joints_3d"][i], gt[i], 1.0)[0] for i in range(num)]
    sv = [PC.verts_statement(res[f"pred_{side}_hand_verts"][i], res[f"gt_{side}_hand_verts"][i], res["mano_params_weight"][i][h], 1.0)[0]
          for i in range(num) for h, side in enumerate(("right", "left"))]
    want = np.array([sum(s[0, 0] for s in st), sum(s[0, 1] for s in st), sum(s[1, 0] + s[2, 0] for s in st), sum(s[1, 1] + s[2, 1] for s in st),
                     sum(s[0] for s in sv), sum(s[1] for s in sv)])
    got = on.pa_metric_sums()
    assert got[1] == want[1] == 42 * 3 + 21 and got[3] == want[3] == 42 * 3 + 21 and got[5] == want[5] == 778 * (2 * num - 1)
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert [len(r["pa_inter_j3d_error"]) for r in on.pred_results] == [42, 21, 0, 42, 42]
    assert abs(on.pa_inter_mpjpe_3d - want[0] / want[1]) <= 1e-15 and abs(on.pa_mpjpe_3d - want[2] / want[3]) <= 1e-15
    assert abs(on.pa_mpvpe_3d - want[4] / want[5]) <= 1e-15
    assert 0 < on.pa_mpjpe_3d and 0 < on.pa_inter_mpjpe_3d and 0 < on.pa_mpvpe_3d
    on.clear()
    assert np.array_equal(on.pa_metric_sums(), np.zeros(6))


def test_default_evaluator_pickles_as_before():
    """pa_metrics off: the records, the nine sums and a pickled evaluator's records carry nothing new."""
    import pickle
    ev = E.Evaluator(_mano())
    ev.update(np.arange(3), _pred(3))
    back = pickle.loads(pickle.dumps(ev))
    expected = {"data_idx", "pred_cam_params", "pred_shape_params", "pred_pose_params", "pred_hand_trans", "pred_joints_3d",
                "collision_loss_origin_scale", "gt_joints_3d", "img_path", "img_path_relative", "annot_type", "hand_type", "hand_type_valid",
                "scale", "j3d_error", "pa_no_rot_inter_j3d_error", "v3d_error"} | set(E.Evaluator.VERT_KEYS)
    assert all(set(r) == expected for r in back.pred_results)
    assert np.array_equal(back.metric_sums(), ev.metric_sums()) and len(back.metric_sums()) == 9
    # an evaluator pickled before the PA metrics existed has none of the new attributes
    for k in ("pa_metrics", "_device_pa_parts", "_device_pa_vert_parts"):
        back.__dict__.pop(k)
    back.update(np.arange(3, 5), {k: v[3:5] for k, v in _pred(5).items()})
    assert all(set(r) == expected for r in back.pred_results) and np.array_equal(back.pa_metric_sums(), np.zeros(6))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, num, bs, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from ihmr_amd import dist as D
    r, w = D.init_dist("gloo")
    idx, pad = D.shard_indices(num, bs, r, w)
    full = _pred(num)
    ev = E.Evaluator(_mano(), pa_metrics=True)
    for s in range(0, len(idx), bs):
        sel, keep = idx[s:s + bs], ~pad[s:s + bs]
        ev.update(sel, {k: v[sel] for k, v in full.items()})
        new = ev.pred_results[-len(sel):]
        ev.pred_results = ev.pred_results[:-len(sel)] + [p for p, k in zip(new, keep) if k]   # mask padding duplicates
    total = D.reduce_metrics(np.concatenate([ev.metric_sums(), ev.pa_metric_sums()]))           # one all-reduce, as run_optimize does
    if rank == 0:
        np.save(out, total)
    torch.distributed.destroy_process_group()


def test_two_rank_reduction_of_the_pa_sums(tmp_path):
    num, bs, world = 13, 4, 2          # 13 samples pad to 16 = 2 ranks x 2 batches of 4
    out = str(tmp_path / "sums.npy")
    mp.spawn(_worker, args=(world, _free_port(), num, bs, out), nprocs=world, join=True)
    got = np.load(out)
    ev = E.Evaluator(_mano(), pa_metrics=True)
    ev.update(np.arange(num), _pred(num))
    ref = np.concatenate([ev.metric_sums(), ev.pa_metric_sums()])
    assert len(got) == 15 and np.array_equal(got[[9 + 1, 9 + 3, 9 + 5]], ref[[10, 12, 14]])
    assert np.allclose(got, ref, rtol=1e-10, atol=1e-12), (got, ref)   # float64 sums, different association
    m = E.Evaluator.pa_metrics_from_sums(got[9:])
    assert 0 < m["pa_mpjpe_3d"] and 0 < m["pa_inter_mpjpe_3d"] and 0 < m["pa_mpvpe_3d"]


# ------------------------------------------------------------------------------------------------------------------ the build
def test_pa_kernels_use_no_scratch_and_the_header_is_exported(tmp_path):
    """Both 4 x 4 arrays of the Jacobi solver live in registers: no private segment, no spills.  Every `ihmr_*` function that
    include/ihmr_hip.h declares is in EXPORTED_SYMBOLS and in the built library."""
    import ctypes

    from ihmr_amd import hip
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("eval_pa_joints_kernel", "eval_pa_verts_kernel"):
            if k in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == ["eval_pa_joints_kernel", "eval_pa_verts_kernel"], sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert seen["eval_pa_joints_kernel"]["group_segment_fixed_size"] == 0 and seen["eval_pa_verts_kernel"]["group_segment_fixed_size"] == 4 * 10 * 8
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:[A-Za-z_][\w ]*?[\s*]+)(ihmr_\w+)\s*\(", header, flags=re.M))
    assert {"ihmr_eval_pa_joints", "ihmr_eval_pa_verts", "ihmr_eval_metrics"} <= declared
    assert declared == set(hip.EXPORTED_SYMBOLS), declared ^ set(hip.EXPORTED_SYMBOLS)
    L = ctypes.CDLL(hip.build())
    for sym in declared:
        getattr(L, sym)

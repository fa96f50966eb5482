"""``ihmr_eval_mrrpe`` / ``ihmr_eval_contact`` on the GPU against the float64 statement of tests/contact_cases.py, through the C ABI in
guarded buffers pre-filled with 0xFF and again with 0x00: ``|C|`` and every count EXACT, the pair sum within ``|C|`` x 1e-9 m, ``near``
within 1e-9 m (exact on the known answers, on +inf and on NaN positions); ``near = NULL``, batch independence bit for bit, the ``use``
mask, the refusals; then ``Evaluator.update_device_mrrpe`` / ``update_device_contact`` against the host records and ``run_optimize
--mrrpe``.

Measured on the MI355X (the prints below): the worst |pair sum - statement| and |near - statement| over the whole table are recorded in
DESIGN.md section 8, row (f)7."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_cases as CT  # noqa: E402
import curve_cases as CC  # noqa: E402
from guarded import Guarded, assert_guards  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = CT.TOL
NV = CT.NV


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _close(a, b, tol):
    """|a - b| <= tol where both are finite; NaN and +-Inf positions and values exact."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    with np.errstate(all="ignore"):
        return a.shape == b.shape and _same(np.where(fin, 0.0, a), np.where(fin, 0.0, b)) and bool((np.abs(a - b)[fin] <= tol).all())


# ------------------------------------------------------------------------------------------------------------------ the C ABI, guarded
def _launch_contact(cases, table, use=None, with_near=True, with_scale=True, fill=0xFF, override=None):
    """One call of ``ihmr_eval_contact`` on a batch of cases, every buffer guarded, the outputs pre-filled with ``fill``.  Returns
    (rc, dict of numpy outputs); the guards are checked."""
    from ihmr_amd import hip
    override = override or {}
    B, K = len(cases), len(table)
    arrays = dict(pr=np.stack([c.pr for c in cases]), pl=np.stack([c.pl for c in cases]), gr=np.stack([c.gr for c in cases]),
                  gl=np.stack([c.gl for c in cases]), weight=np.stack([c.weight for c in cases]),
                  scale=np.array([c.scale for c in cases], np.float32), thr=np.asarray(table, np.float64))
    if use is not None:
        arrays["use"] = np.asarray(use, np.uint8)
    g = {k: Guarded(a.nbytes) for k, a in arrays.items()}
    for k, a in arrays.items():
        g[k].copy_in(torch.from_numpy(a).cuda())
    g.update(pair=Guarded(B * 2 * 2 * 8, fill=fill), counts=Guarded(B * 2 * K * 3 * 8, fill=fill))
    if with_near:
        g["near"] = Guarded(B * 2 * 2 * NV * 8, fill=fill)
    ptr = lambda k: None if override.get("null") == k else g[k].data_ptr
    rc = hip.lib().ihmr_eval_contact(ptr("pr"), ptr("pl"), ptr("gr"), ptr("gl"), ptr("weight"), ptr("scale") if with_scale else None,
                                     g["use"].data_ptr if use is not None else None, override.get("B", B), ptr("thr"), override.get("K", K),
                                     ptr("pair"), ptr("counts"), g["near"].data_ptr if with_near else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_eval_contact B={B} K={K}")
    out = dict(pair=g["pair"].view(torch.float64, (B, 2, 2)).cpu().numpy(), counts=g["counts"].view(torch.float64, (B, 2, K, 3)).cpu().numpy())
    if with_near:
        out["near"] = g["near"].view(torch.float64, (B, 2, 2, NV)).cpu().numpy()
    return rc, out


def _bytes_equal(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a if k in b) and a.keys() & b.keys() >= {"pair", "counts"}


def _run_contact(cases, table, use=None):
    """The call with 0xFF-filled outputs; the same call with zero-filled outputs must give the same bytes (so every word was written),
    and so must the call without the near buffer."""
    rc, out = _launch_contact(cases, table, use)
    rc0, out0 = _launch_contact(cases, table, use, fill=0x00)
    rcn, outn = _launch_contact(cases, table, use, with_near=False)
    assert rc == 0 and rc0 == 0 and rcn == 0
    assert _bytes_equal(out, out0) and "near" in out0 and _bytes_equal(out, outn) and "near" not in outn
    return out


WORST = dict(pair_sum=0.0, near=0.0)


def _check_contact(cases, table, out, use=None):
    for b, c in enumerate(cases):
        what = f"{c.name} K={len(table)} row {b}"
        used = use is None or bool(use[b])
        s = CT.contact_of(CT.case_distances(c.name), c.counted and used, tuple(table))
        assert out["pair"][b, 1].tobytes() == np.zeros(2).tobytes(), what                   # the left hand's row carries no pairs
        assert out["pair"][b, 0, 1] == s["pairs"], (what, out["pair"][b, 0, 1], s["pairs"])
        assert _same(out["counts"][b], s["counts"]), (what, out["counts"][b], s["counts"])
        print(f"[contact] {what}: |C| {s['pairs']}, pair sum device {out['pair'][b, 0, 0]!r} statement {s['pair_sum']!r}")
        assert _close(out["pair"][b, 0, 0], s["pair_sum"], max(1, s["pairs"]) * TOL), what
        assert _close(out["near"][b], s["near"], TOL), what
        if not s["counted"]:
            assert not out["pair"][b].view(np.uint64).any() and not out["counts"][b].view(np.uint64).any() and not out["near"][b].view(np.uint64).any(), what
            continue
        if c.known:
            assert out["pair"][b, 0, 0] == s["pair_sum"] and _same(out["near"][b], s["near"]), what
        if np.isfinite(s["pair_sum"]):
            WORST["pair_sum"] = max(WORST["pair_sum"], abs(out["pair"][b, 0, 0] - s["pair_sum"]))
        fin = np.isfinite(s["near"])
        WORST["near"] = max(WORST["near"], float(np.abs(np.where(fin, out["near"][b], 0.0) - np.where(fin, s["near"], 0.0)).max()))


def _chunks(cases):
    """Batches of 5, 3 and 1 samples, in turn."""
    out, i, turn = [], 0, 0
    while i < len(cases):
        k = (5, 3, 1)[turn % 3]
        turn += 1
        if k <= len(cases) - i:
            out.append(cases[i:i + k])
            i += k
    return out


@pytest.mark.parametrize("K", sorted(CT.TABLES))
def test_every_case_is_the_statement(K):
    cases = list(CT.mesh_cases().values())
    sizes = set()
    for batch in _chunks(cases):
        sizes.add(len(batch))
        _check_contact(batch, CT.TABLES[K], _run_contact(batch, CT.TABLES[K]))
    assert sizes == {1, 3, 5}
    print(f"[contact] K={K}: worst |pair sum - statement| = {WORST['pair_sum']:.3e} m, worst |near - statement| = {WORST['near']:.3e} m")


def test_known_answers_are_exact():
    t = CT.mesh_cases()
    batch = [t["dyadic"], t["deep_0_same"], t["dyadic"]]
    out = _run_contact(batch, CT.KNOWN_TABLE)                       # tau_c = 2^-9 exactly: equality is not contact
    assert out["pair"][0].tolist() == out["pair"][2].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    for b in (0, 2):
        assert out["counts"][b].tolist() == [[[0, 0, 0], [0, 0, 778], [0, 0, 778], [778, 778, 778]]] * 2
        assert (out["near"][b, :, 0] == CT.KNOWN_PRED).all() and (out["near"][b, :, 1] == CT.KNOWN_GT).all()
    out = _run_contact(batch, CT.TABLES[2])
    assert out["pair"][0, 0].tolist() == [778 * CT.KNOWN_PRED, 778.0] and out["pair"][0, 0, 0] / out["pair"][0, 0, 1] == 2.0 ** -8
    assert out["counts"][0].tolist() == [[[0, 0, 778], [778, 778, 778]]] * 2
    _check_contact(batch, CT.TABLES[2], out)
    # without a scale pointer the scale is 1
    rc, plain = _launch_contact(batch, CT.TABLES[2], with_scale=False)
    assert rc == 0 and _bytes_equal(plain, out)


def test_batch_independence_and_the_use_mask():
    t = CT.mesh_cases()
    cases = [t[k] for k in ("deep_0_noise", "scale_1p7", "right_weight_0", "nan_in_gt", "fingers_1_shift")]
    table = CT.TABLES[2]
    base = _run_contact(cases, table)
    perm = [3, 0, 4, 2, 1]
    got = _run_contact([cases[p] for p in perm], table)
    for k in base:
        assert got[k].tobytes() == base[k][perm].tobytes(), k
    rep = _run_contact([cases[1]] * 5, table)
    for k in base:
        assert all(rep[k][b].tobytes() == base[k][1].tobytes() for b in range(5)), k
    single = _run_contact([cases[1]], table)
    for k in base:
        assert single[k][0].tobytes() == base[k][1].tobytes(), k
    use = np.array([1, 0, 1, 0, 1], np.uint8)
    masked = _run_contact(cases, table, use=use)
    _check_contact(cases, table, masked, use=use)
    for k in base:
        assert masked[k][use > 0].tobytes() == base[k][use > 0].tobytes(), k
        assert not masked[k][use == 0].view(np.uint64).any(), k
    every = _run_contact(cases, table, use=np.array([1, 2, 255, 1, 7], np.uint8))            # any non-zero byte is "use"
    assert _bytes_equal(every, base)


@pytest.mark.parametrize("override", [dict(B=0), dict(B=-1), dict(K=0), dict(K=9), dict(null="pr"), dict(null="pl"), dict(null="gr"),
                                      dict(null="gl"), dict(null="weight"), dict(null="thr"), dict(null="pair"), dict(null="counts")])
def test_contact_refusals_write_nothing(override):
    cases = [CT.mesh_cases()["dyadic"]]
    rc, out = _launch_contact(cases, CT.TABLES[2], override=override)
    assert rc != 0
    for k, v in out.items():
        assert (v.view(np.uint8) == 0xFF).all(), k


# ------------------------------------------------------------------------------------------------------------------ MRRPE
def _launch_mrrpe(rows, interacting=True, with_scale=True, fill=0xFF, override=None):
    from ihmr_amd import hip
    override = override or {}
    names, P, G, S, I = CT.joint_batch()
    rows = np.asarray(rows)
    B = len(rows)
    arrays = dict(pred=P[rows], gt=G[rows], scale=S[rows], inter=I[rows].astype(np.uint8))
    g = {k: Guarded(a.nbytes) for k, a in arrays.items()}
    for k, a in arrays.items():
        g[k].copy_in(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    g["out"] = Guarded(B * 2 * 8, fill=fill)
    ptr = lambda k: None if override.get("null") == k else g[k].data_ptr
    rc = hip.lib().ihmr_eval_mrrpe(ptr("pred"), ptr("gt"), ptr("scale") if with_scale else None, ptr("inter") if interacting else None,
                                   override.get("B", B), ptr("out"), hip.stream_ptr())
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_eval_mrrpe B={B}")
    return rc, g["out"].view(torch.float64, (B, 2)).cpu().numpy()


@pytest.mark.parametrize("B", [1, 3, 5])
def test_mrrpe_is_the_statement_per_sample(B):
    names, P, G, S, I = CT.joint_batch()
    ref = np.array(CT.joint_reference())
    n, worst = len(names), 0.0
    for start in range(0, n, B):
        rows = np.arange(start, min(n, start + B))
        rc, out = _launch_mrrpe(rows)
        rc0, out0 = _launch_mrrpe(rows, fill=0x00)
        assert rc == 0 and rc0 == 0 and out.tobytes() == out0.tobytes()
        assert _same(out[:, 1], ref[rows, 1]) and _close(out[:, 0], ref[rows, 0], TOL), (rows, out, ref[rows])      # counts and NaN positions exact
        for r, o in zip(rows, out):
            if names[r] in ("dyadic", "pred_is_gt") or not ref[r, 1]:
                assert o[0] == ref[r, 0], names[r]
            if np.isfinite(ref[r, 0]):
                worst = max(worst, abs(o[0] - ref[r, 0]))
    print(f"[mrrpe] B={B}: worst |e - statement| = {worst:.3e} m")
    # without the mask every sample is interacting; without the scale it is 1
    rows = np.arange(min(n, 5))[:B] + names.index("scaled")
    rc, out = _launch_mrrpe(rows, interacting=False, with_scale=False)
    want = np.array([CT.mrrpe_of(P[r], G[r], 1.0, True) for r in rows])
    assert rc == 0 and _same(out[:, 1], want[:, 1]) and _close(out[:, 0], want[:, 0], TOL)


def test_mrrpe_over_more_samples_than_a_block_and_in_any_order():
    names, P, G, S, I = CT.joint_batch()
    rows = np.random.RandomState(5).randint(0, len(names), 131)                               # three blocks of 64 threads, the last partial
    rc, out = _launch_mrrpe(rows)
    ref = np.array(CT.joint_reference())[rows]
    assert rc == 0 and _same(out[:, 1], ref[:, 1]) and _close(out[:, 0], ref[:, 0], TOL)
    base = {r: _launch_mrrpe([r])[1][0].tobytes() for r in set(rows.tolist())}
    assert all(out[i].tobytes() == base[r] for i, r in enumerate(rows.tolist()))              # bit for bit wherever a sample stands


@pytest.mark.parametrize("override", [dict(B=0), dict(B=-3), dict(null="pred"), dict(null="gt"), dict(null="out")])
def test_mrrpe_refusals_write_nothing(override):
    rc, out = _launch_mrrpe([0, 1, 2], override=override)
    assert rc != 0 and (out.view(np.uint8) == 0xFF).all()


# ------------------------------------------------------------------------------------------------------------------ the Evaluator
@pytest.mark.parametrize("K", [2, 8])
def test_evaluator_device_path_over_two_masked_batches_equals_the_host_records(K):
    from ihmr_amd.evaluator import Evaluator
    table = CT.TABLES[K]
    res, data_list, keep, inter = CT.evaluator_batch()
    B = len(keep)
    host = Evaluator(CC.mano_models(), data_list=data_list, interaction_metrics=True, contact_thresholds=table)
    kept = np.nonzero(keep)[0]
    host.update(kept, {k: v[kept].copy() for k, v in res.items()})
    dev = Evaluator(CC.mano_models(), interaction_metrics=True, contact_thresholds=table)
    scale = np.array([data_list[b]["scale"] for b in range(B)], np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for lo, hi in ((0, 4), (4, B)):
        sl = slice(lo, hi)
        masks = dict(keep=torch.from_numpy(keep[sl]), interacting=torch.from_numpy(inter[sl]), scale=up(scale[sl]))
        dev.update_device_mrrpe(up(res["pred_joints_3d"][sl]), up(res["gt_joints_3d"][sl]), **masks)
        dev.update_device_contact(up(res["pred_right_hand_verts"][sl]), up(res["pred_left_hand_verts"][sl]), up(res["gt_right_hand_verts"][sl]),
                                  up(res["gt_left_hand_verts"][sl]), up(res["mano_params_weight"][sl]), **masks)
    got, want = dev.interaction_sums(), host.interaction_sums()
    stated = CT.expected_sums(*CT.evaluator_statement(table), table)
    print(f"[evaluator] K={K} device {got[:5]!r} host {want[:5]!r}")
    integer = [1, 3, 4] + list(range(5, 5 + 3 * K))
    assert _same(got[integer], want[integer]) and _same(got[integer], stated[integer])        # element for element
    assert want[1] >= 4 and want[3] >= 3 and want[4] > want[3]
    for k in (0, 2):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])
    m = dev.metrics_from_packed(dev.packed_sums())
    assert 0 < m["contact_rate"] < 1 and m["mrrpe"] > 0 and len(m["contact_f1"]) == K
    assert not dev.metric_sums().any() and dev.pred_results == []                             # the family leaves the other sums alone
    dev.clear()
    assert not dev.interaction_sums().any()
    plain = Evaluator(CC.mano_models())
    with pytest.raises(RuntimeError):
        plain.update_device_mrrpe(up(res["pred_joints_3d"]), up(res["gt_joints_3d"]))


def test_run_optimize_mrrpe_device_host_and_two_ranks_agree():
    from ihmr_amd import run_optimize
    args = ["--num_samples", "14", "--batchSize", "4", "--opt_epoch", "2", "--mrrpe"]
    one = run_optimize.main(args)
    host = run_optimize.main(args + ["--host_eval"])
    plain = run_optimize.main(args[:-1])
    assert sorted(one) == sorted(host) == sorted(list(plain) + ["mrrpe"]) and "mrrpe" not in plain      # no contact part: no GT meshes
    for k in plain:
        assert one[k] == plain[k], k
    print(f"[mrrpe] run_optimize device {one['mrrpe']!r} host {host['mrrpe']!r}")
    assert one["mrrpe"] > 0 and abs(one["mrrpe"] - host["mrrpe"]) <= 1e-9
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, IHMR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "ihmr_amd.run_optimize"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "mrrpe : " in r.stdout
    two = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert two["world"] == 2 and not any(k.startswith("contact_") for k in two)
    for k in ("mrrpe", "mpjpe_3d", "collision_ave"):
        assert abs(two[k] - one[k]) <= 1e-12 * max(1.0, abs(one[k])), (k, two[k], one[k])

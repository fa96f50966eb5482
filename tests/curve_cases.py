"""The curve metrics (PCK counts, F-score counts, collision AUC) stated in float64 numpy, and the case tables of the CPU and GPU tests.

Every error is float64 arithmetic on float32 arrays, divided by the sample's scale before it is compared with a threshold.

* five error populations: ``j3d`` (valid joints of a hand whose wrist is valid; the root subtraction cumulative, right hand then left),
  ``pa_inter_j3d`` (all valid joints, one alignment), ``pa_j3d`` (one alignment per hand), ``v3d`` (778 vertices of a hand with
  ``mano_params_weight > 0``, both meshes relative to their own root = root_weights . mesh), ``pa_v3d`` (the aligned vertex error);
* ``counts[k] = #(err <= tau_k)``, non-strict; ``auc`` = trapezoid of ``counts / n`` over ``(tau_k - tau_0) / (tau_{T-1} - tau_0)``;
* F-score of one hand: ``d_pg[i] = min_j |p_i - g_j| / scale``, ``d_gp[j] = min_i |p_i - g_j| / scale``, each squared distance
  ``(dx*dx + dy*dy) + dz*dz``, the minimum on the squares, one root; ``P = #(d_pg < tau) / 778``, ``R = #(d_gp < tau) / 778``, strict;
  ``F = 2 P R / (P + R)`` or 0 when ``P + R = 0``.  raw: p = pred - root(pred), g = gt - root(gt); pa: p = the aligned prediction,
  g = gt, and a hand the PA rules leave out is not counted.

MARGIN.  A count is exact only if no value lies within rounding of a threshold.  Every statement error and every nearest-neighbour
distance of every case lies at least ``MARGIN`` = 1e-8 from every threshold of every table it is compared with -- ten times the 1e-9
bar on a per-point device value, so a device value inside that bar cannot change a count -- EXCEPT values that are exact on every
side and EQUAL to a threshold: 0 (x - x at a root) and the dyadic known answers (tests/test_curve_metrics_cpu.py asserts this on every
case and table).
The tables' end points below were searched on the CPU until the condition held.
"""
import functools

import numpy as np

import pa_cases as PC

NV = 778
MARGIN = 1e-8
TOL = 1e-9
COLLISION_THRESHOLDS = np.linspace(0.5, 15)

# ------------------------------------------------------------------------------------------------------------------ threshold tables
# T = 64 / 65 straddle the wave width, 256 and 8 are the limits of the entry points.  (lo, hi) per T; `python tests/curve_cases.py`
# prints what violates the margin (nothing, for the values below).
PCK_ENDS = {1: (0.0, 0.0213), 2: (0.0031, 0.0417), 64: (0.0007, 0.0613), 65: (0.0007, 0.0613), 256: (0.0007, 0.0613)}
F_TABLES = {0: (), 1: (0.0101,), 2: (0.005, 0.015), 8: tuple(np.linspace(0.002, 0.03, 8))}
DEFAULT_TABLE = np.linspace(0, 0.05, 100)            # kept to the smallest cases: DEFAULT_JOINT_CASES / DEFAULT_VERT_CASES
KNOWN = 5.0 / 512                                    # the known-answer error: |(3, 4, 0)| * 2^-9, exact
KNOWN_TABLE = np.array([1.0 / 1024, 1.0 / 128, KNOWN, 1.0 / 64, 1.0 / 16])
KNOWN_F_TABLE = (1.0 / 128, KNOWN, 1.0 / 64)


def pck_table(T):
    lo, hi = PCK_ENDS[T]
    return np.array([hi]) if T == 1 else np.linspace(lo, hi, T)


# ------------------------------------------------------------------------------------------------------------------ statement
def counts_of(errors, thresholds, strict=False):
    e, t = np.asarray(errors, np.float64).reshape(-1), np.asarray(thresholds, np.float64).reshape(-1)
    return np.array([np.sum(e < x) if strict else np.sum(e <= x) for x in t], np.float64)


def auc_of(counts, n, thresholds):
    t = np.asarray(thresholds, np.float64)
    if n == 0 or len(t) < 2:
        return float("nan")
    y, x = np.asarray(counts, np.float64) / n, (t - t[0]) / (t[-1] - t[0])
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0))


def fscore_of(n_pg, n_gp, n=NV):
    P, R = n_pg / n, n_gp / n
    return 2.0 * P * R / (P + R) if P + R > 0 else 0.0


def _norm3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def joint_errors(pred, gt, scale=1.0):
    """One sample: pred (42,3), gt (42,4) float32 -> three float64 arrays, the populations j3d, pa_inter_j3d, pa_j3d."""
    a, b, w = pred.astype(np.float64), gt[:, :3].astype(np.float64), gt[:, 3].astype(np.float64)
    j3d = []
    for root in (0, 21):
        if w[root] > 0:
            a, b = a - a[root], b - b[root]
            rows = [j for j in range(root, root + 21) if w[j] > 0]
            j3d += list(_norm3(a[rows] - b[rows]) / float(scale))
    pops = [np.array(j3d)]
    for sets in ((PC.JOINT_SETS[0],), PC.JOINT_SETS[1:]):
        e = []
        for lo, hi in sets:
            r = PC.set_errors(pred[lo:hi], gt[lo:hi, :3], gt[lo:hi, 3], scale)
            if r is not None:
                e += list(r[gt[lo:hi, 3] > 0])
        pops.append(np.array(e))
    return pops


def joint_counts(pred, gt, scale, thresholds):
    """(3, T+1): per population [#err <= tau_k ..., number of points]."""
    return np.stack([np.concatenate([counts_of(e, thresholds), [len(e)]]) for e in joint_errors(pred, gt, scale)])


def nn_sq(p, g):
    d = p[:, None, :] - g[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return d2.min(axis=1), d2.min(axis=0)


def hand_statement(pred, gt, root_w, weight, scale=1.0):
    """One hand: pred, gt (778,3) float32 -> dict(counted, pa_kept, err (2,778) [v3d, pa_v3d], nn (2,2,778) [raw / pa][p->g / g->p]);
    zeros where the hand (or its pa half) does not count."""
    out = dict(counted=bool(weight > 0), pa_kept=False, err=np.zeros((2, NV)), nn=np.zeros((2, 2, NV)))
    if not out["counted"]:
        return out
    P, G, rw, s = pred.astype(np.float64), gt.astype(np.float64), root_w.astype(np.float64), float(scale)
    p, g = P - rw @ P, G - rw @ G
    out["err"][0] = _norm3(p - g) / s
    a, b = nn_sq(p, g)
    out["nn"][0] = np.sqrt(a) / s, np.sqrt(b) / s
    if np.sum((P - P.mean(axis=0)) ** 2) > 0.0:
        out["pa_kept"] = True
        al = PC.procrustes_rows(P, G)
        out["err"][1] = _norm3(al - G) / s
        a, b = nn_sq(al, G)
        out["nn"][1] = np.sqrt(a) / s, np.sqrt(b) / s
    return out


def hand_counts(st, thresholds, f_thresholds):
    """counts (2,T+1) and f_counts (2,2,F) of a :func:`hand_statement`."""
    T, F = len(thresholds), len(f_thresholds)
    counts, fc = np.zeros((2, T + 1)), np.zeros((2, 2, F))
    for k, on in enumerate((st["counted"], st["pa_kept"])):
        if on:
            counts[k] = np.concatenate([counts_of(st["err"][k], thresholds), [NV]])
            for d in range(2):
                fc[k, d] = counts_of(st["nn"][k, d], f_thresholds, strict=True)
    return counts, fc


# ------------------------------------------------------------------------------------------------------------------ cases
def root_weights():
    """(2,778) float32: the right hand's root is vertex 0 (one-hot: the root-relative values of a dyadic mesh are exact), the left
    hand's a seeded convex combination of all vertices, like a row of the MANO joint regressor."""
    w = np.zeros((2, NV))
    w[0, 0] = 1.0
    r = np.random.RandomState(16).rand(NV)
    w[1] = r / r.sum()
    return w.astype(np.float32)


def _dyadic_joints():
    g = np.stack([np.arange(42) % 4, (np.arange(42) // 4) % 4, np.arange(42) // 16], axis=1) / 16.0
    off = np.tile(np.array([[3.0, 4.0, 0.0]]) / 512, (42, 1))
    off[[0, 21]] = 0.0                                           # both roots coincide with their targets
    return (g + off).astype(np.float32), np.concatenate([g, np.ones((42, 1))], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def joint_batch():
    """names, pred (B,42,3), gt (B,42,4), scale (B) float32: the PA case table (it holds a sample without a valid right wrist, sets
    left out by the weight-sum rule and by coincident predictions) plus the known-answer sample ``dyadic``: every non-root joint's
    error is exactly KNOWN, both roots' exactly 0."""
    names, pred, gt, scale = PC.joint_batch()
    p, g = _dyadic_joints()
    return list(names) + ["dyadic"], np.concatenate([pred, p[None]]), np.concatenate([gt, g[None]]), np.concatenate([scale, np.float32([1.0])])


@functools.lru_cache(maxsize=None)
def vert_batch():
    """names, pred (B,2,778,3), gt (B,2,778,3) [right, left], mano_params_weight (B,2), scale (B) float32."""
    names, P, G, W, S = PC.vert_batch()            # both hands, a hand with weight 0 on either side, a mirrored mesh, an exact similarity
    names, P, G, W, S = list(names), list(P), list(G), list(W), list(S)
    rng = np.random.RandomState(2778)

    def add(name, p, g, weight=(1.0, 1.0), scale=1.0):
        names.append(name); P.append(np.float32(p)); G.append(np.float32(g)); W.append(np.float32(weight)); S.append(np.float32(scale))

    g = np.stack([PC._cloud(rng, NV), PC._cloud(rng, NV)])
    add("coincident_prediction", np.tile(np.array([0.1, 0.2, 0.3]), (2, NV, 1)), g)          # var1 == 0: the pa halves are left out
    g = np.float32(np.stack([PC._cloud(rng, NV), PC._cloud(rng, NV)]))
    add("identical", g.copy(), g, scale=0.5)                                                  # every raw distance 0, F = 1
    # further apart than every threshold, raw and aligned: the prediction on a sphere of 100 m around its root, the target a cloud of
    # metres that it has nothing in common with.  Left hand only: with a one-hot root, vertex 0 of both root-relative meshes is 0
    u = rng.randn(2, NV, 3)
    add("far_apart", 100.0 * u / np.linalg.norm(u, axis=2, keepdims=True), rng.randn(2, NV, 3) * np.array([6.0, 3.5, 1.5]), weight=(0.0, 1.0))
    # known answer, right hand: a dyadic grid (pitch 1/16) and the same grid shifted by (3, 4, 0) / 512 except at the root vertex:
    # v3d error and both nearest-neighbour distances are exactly KNOWN (0 at vertex 0)
    i = np.arange(NV)
    grid = np.stack([i % 8, (i // 8) % 8, i // 64], axis=1) / 16.0
    off = np.tile(np.array([[3.0, 4.0, 0.0]]) / 512, (NV, 1))
    off[0] = 0.0
    add("dyadic", np.stack([grid + off, grid + off]), np.stack([grid, grid]), weight=(1.0, 0.0))
    return names, np.stack(P), np.stack(G), np.stack(W), np.array(S, np.float32)


DEFAULT_JOINT_CASES = ("all_42", "right_hand_only_21", "missing_wrist_41", "dyadic")
DEFAULT_VERT_CASES = ("both_hands", "left_without_annotation")


@functools.lru_cache(maxsize=None)
def joint_reference():
    """Per case the three error populations (computed once, shared by every test)."""
    names, pred, gt, scale = joint_batch()
    return [joint_errors(pred[b], gt[b], scale[b]) for b in range(len(names))]


@functools.lru_cache(maxsize=None)
def vert_reference():
    """Per case and hand the :func:`hand_statement` (computed once, shared by every test)."""
    names, P, G, W, S = vert_batch()
    rw = root_weights()
    return [[hand_statement(P[b, h], G[b, h], rw[h], W[b, h], S[b]) for h in range(2)] for b in range(len(names))]


def collision_cases():
    """name -> per-sample penetration depths [mm] (float64) for the collision AUC: the golden's inputs are built from these."""
    rng = np.random.RandomState(515)
    thr = COLLISION_THRESHOLDS
    return {
        "all_below": rng.uniform(0.0, 0.49, 40),
        "all_above": rng.uniform(15.5, 40.0, 40),
        "single_low": np.array([0.25]),
        "single_mid": np.array([7.3]),
        "on_thresholds": np.array([thr[0], thr[7], thr[7], thr[24], thr[49], 3.0]),     # a value EQUAL to a threshold is not below it
        "realistic": np.abs(rng.normal(0, 4.0, 500)),
        "realistic_small": np.abs(rng.normal(0, 1.5, 37)),
        "wide": rng.uniform(0.0, 30.0, 200),
        "two_values": np.array([0.6, 14.9]),
        "zeros": np.zeros(5),
    }


EXACT_VALUES = (0.0, KNOWN)


def margin_violations(values, thresholds):
    """The (value, threshold) pairs closer than MARGIN.  A pair of EQUAL numbers is none where the value is exact on every side:
    0 (x - x at a root, identical meshes) and the dyadic known answer."""
    v, t = np.asarray(values, np.float64).reshape(-1, 1), np.asarray(thresholds, np.float64).reshape(1, -1)
    bad = (np.abs(v - t) < MARGIN) & ~((v == t) & np.isin(v, EXACT_VALUES))
    return [(float(v[i, 0]), float(t[0, k])) for i, k in zip(*np.nonzero(bad))]


def all_margin_violations(pck_tables, f_tables):
    """Every case against the given tables: the generic tables on every case (the known-answer cases included: none of their values
    may come close to a generic threshold either)."""
    bad = []
    jn, vn = joint_batch()[0], vert_batch()[0]
    for t in pck_tables:
        for name, pops in zip(jn, joint_reference()):
            bad += [("joints", name) + x for e in pops for x in margin_violations(e, t)]
        for name, hands in zip(vn, vert_reference()):
            bad += [("verts", name) + x for st in hands for x in margin_violations(st["err"][[st["counted"], st["pa_kept"]]], t)]
    for t in f_tables:
        if len(t):
            for name, hands in zip(vn, vert_reference()):
                bad += [("nn", name) + x for st in hands for x in margin_violations(st["nn"][[st["counted"], st["pa_kept"]]], t)]
    return bad


# ------------------------------------------------------------------------------------------------------------------ an Evaluator batch
EVAL_T, EVAL_F = 64, 2           # the tables of the Evaluator tests: pck_table(EVAL_T), F_TABLES[EVAL_F]


def mano_models():
    """Stand-ins for the two MANO models: what the Evaluator reads of them (faces, row 0 of the joint regressor)."""
    import types
    rw = root_weights()
    mk = lambda h: types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=np.stack([rw[h]] * 16))
    return dict(right=mk(0), left=mk(1))


@functools.lru_cache(maxsize=None)
def evaluator_batch():
    """One exported batch with GT meshes: sample b carries vertex case b and a joint case, the vertex case's scale, a hand type (two
    samples are not interacting), penetration depths whose per-sample max / mean [mm] spread over the collision thresholds, and a
    keep mask (two padding duplicates).  Returns (pred_results dict, data_list, keep (B,) bool)."""
    jn, jp, jg, _ = joint_batch()
    vn, P, G, W, S = vert_batch()
    B = len(vn)
    rows = [jn.index(n) for n in ("all_42", "right_hand_only_21", "missing_wrist_41", "three_valid", "two_valid", "weight_sum_1p5", "mirrored",
                                  "coincident_prediction", "dyadic")]
    assert len(rows) == B
    rng = np.random.RandomState(99)
    sigma = np.array([0.1, 0.3, 0.6, 1.0, 1.5, 2.5, 3.5, 5.0, 6.0]) * 1e-3
    coll = np.abs(rng.normal(0, 1.0, (B, 2 * NV)) * sigma[:, None]).astype(np.float32)
    hand_type = ["interacting"] * B
    hand_type[1], hand_type[6] = "right", "left"
    keep = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], bool)
    res = dict(pred_cam_params=np.zeros((B, 3), np.float32), pred_shape_params=np.zeros((B, 20), np.float32),
               pred_pose_params=np.zeros((B, 96), np.float32), pred_hand_trans=np.zeros((B, 3), np.float32),
               pred_joints_3d=jp[rows], gt_joints_3d=jg[rows], collision_loss_origin_scale=coll,
               pred_right_hand_verts=P[:, 0], pred_left_hand_verts=P[:, 1], gt_right_hand_verts=G[:, 0], gt_left_hand_verts=G[:, 1],
               mano_params_weight=W)
    data_list = {b: dict(scale=float(S[b]), hand_type=hand_type[b]) for b in range(B)}
    return res, data_list, keep


@functools.lru_cache(maxsize=None)
def evaluator_statement():
    """Of the kept samples of :func:`evaluator_batch`: the five error populations, per variant the per-hand (d_pg, d_gp) pairs, and
    the per-sample (max, mean) penetration depth [mm] of the interacting ones."""
    res, data_list, keep = evaluator_batch()
    rw = root_weights()
    pops, hands, cmax, cave = [[] for _ in range(5)], ([], []), [], []
    for b in np.nonzero(keep)[0]:
        s = data_list[b]["scale"]
        for k, e in enumerate(joint_errors(res["pred_joints_3d"][b], res["gt_joints_3d"][b], s)):
            pops[k] += list(e)
        for h, side in enumerate(("right", "left")):
            st = hand_statement(res[f"pred_{side}_hand_verts"][b], res[f"gt_{side}_hand_verts"][b], rw[h], res["mano_params_weight"][b, h], s)
            for k, on in enumerate((st["counted"], st["pa_kept"])):
                if on:
                    pops[3 + k] += list(st["err"][k])
                    hands[k].append((st["nn"][k, 0], st["nn"][k, 1]))
        if data_list[b]["hand_type"] == "interacting":
            c = res["collision_loss_origin_scale"][b].astype(np.float64)
            cmax.append(np.max(c) * 1000)
            cave.append(np.mean(c) * 1000)
    return [np.array(p) for p in pops], hands, np.array(cmax), np.array(cave)


def expected_curve_sums(thresholds, f_thresholds):
    """The vector ``Evaluator.curve_sums()`` is to return for the kept samples of :func:`evaluator_batch`, from the statement."""
    import math
    pops, hands, cmax, cave = evaluator_statement()
    out = [np.concatenate([counts_of(e, thresholds), [len(e)]]) for e in pops]
    for hs in hands:
        F = [[fscore_of(a, b) for a, b in zip(counts_of(pg, f_thresholds, True), counts_of(gp, f_thresholds, True))] for pg, gp in hs]
        out.append(np.array([math.fsum(row[k] for row in F) for k in range(len(f_thresholds))] + [float(len(hs))]))
    for c in (cmax, cave):
        out.append(np.concatenate([counts_of(c, COLLISION_THRESHOLDS, True), [len(c)]]))
    return np.concatenate(out)


def evaluator_margin_violations():
    pops, hands, cmax, cave = evaluator_statement()
    bad = [x for e in pops for x in margin_violations(e, pck_table(EVAL_T))]
    bad += [x for hs in hands for pair in hs for d in pair for x in margin_violations(d, F_TABLES[EVAL_F])]
    # the device's per-sample mean is a float64 sum in another order and its max the same float32 number: 1e-8 mm is ample
    return bad + margin_violations(np.concatenate([cmax, cave]), COLLISION_THRESHOLDS)


if __name__ == "__main__":       # prints what violates the margin (nothing, as committed)
    print("evaluator batch", evaluator_margin_violations())
    for T in PCK_ENDS:
        print("T", T, all_margin_violations([pck_table(T)], []))
    for F, t in F_TABLES.items():
        print("F", F, all_margin_violations([], [t]))
    print("default", [x for x in all_margin_violations([DEFAULT_TABLE], []) if x[1] in DEFAULT_JOINT_CASES + DEFAULT_VERT_CASES])

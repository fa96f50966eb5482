"""The interacting-hand metrics (MRRPE, contact consistency) stated in float64 numpy, and the seeded case
tables of the CPU and GPU tests.  Nothing here imports ``ihmr_amd.evaluator``.

All arithmetic is float64 on float32 arrays.  Every squared distance is ``(dx*dx + dy*dy) + dz*dz``, every distance one root, and
every distance is divided by the sample's scale before it is compared with a threshold or summed.

* MRRPE of one sample, counted when ``w[0] > 0`` and ``w[21] > 0`` (and the sample is interacting):
  ``e = |(P[21] - P[0]) - (G[21] - G[0])| / scale``.  A non-finite input gives a non-finite e, which is counted.
* a sample's contact part is counted when both ``mano_params_weight`` are > 0 (and the sample is kept and interacting).
  ``d_X(i, j) = sqrt(sq_dist(R_X[i], L_X[j])) / scale`` for X in {pred, gt}; comparisons are literal (a NaN is never in contact).
  ``C = {(i, j) : d_gt(i, j) < tau_c}`` (strict), tau_c the first threshold; the sample leaves ``[sum over C of d_pred, |C|]``.
* ``near_X(right, i) = min_j d_X(i, j)``, ``near_X(left, j) = min_i d_X(i, j)``: the minimum on the squares (a NaN never replaces the
  running minimum, a vertex without a comparable partner keeps +inf), then one root.  Per threshold tau_k a vertex is in contact in X
  when ``near_X < tau_k`` (strict); ``tp`` = in contact in both, ``pp`` = in pred, ``gp`` = in gt.
* a sample that is not counted has zeros everywhere.

MARGIN.  A count is exact only if no value lies within rounding of a threshold: every GT pair distance of every case lies at least
``MARGIN`` = 1e-8 from tau_c, and every ``near`` value from every threshold of every table -- ten times the 1e-9 bar on a device value
-- EXCEPT the dyadic known answers, which are exact on every side and EQUAL to a threshold on purpose.  ``python tests/contact_cases.py``
prints what violates the condition (nothing, as committed); the table ends and the seeds were searched on the CPU until it held.
"""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

NV = 778
MARGIN = 1e-8
TOL = 1e-9                                           # the project's bar on a float64 device value [m]
F32 = np.float32

# ------------------------------------------------------------------------------------------------------------------ threshold tables
# K = 1, 2 (the default) and 8 (the entry point's limit); every table starts at 3 mm, so the contact PAIRS are the same under each.
TABLES = {1: (0.003,), 2: (0.003, 0.005), 8: tuple(np.linspace(0.003, 0.0171, 8))}
KNOWN_GT, KNOWN_PRED = 2.0 ** -9, 2.0 ** -8          # the shifts of the known-answer sample: near_gt and near_pred of every vertex
KNOWN_TABLE = (KNOWN_GT, 0.003, KNOWN_PRED, 0.005)   # tau_c = 2^-9 exactly: equality is not contact, |C| = 0
EXACT_VALUES = (KNOWN_GT, KNOWN_PRED)


# ------------------------------------------------------------------------------------------------------------------ statement
def mrrpe_of(pred, gt, scale=1.0, interacting=True):
    """(e, counted) of one sample: pred (42,3), gt (42,4) [xyz, weight]."""
    p, g = np.asarray(pred).astype(np.float64), np.asarray(gt).astype(np.float64)
    if not (g[0, 3] > 0 and g[21, 3] > 0 and interacting):
        return 0.0, 0.0
    d = (p[21] - p[0]) - (g[21, :3] - g[0, :3])
    with np.errstate(all="ignore"):
        return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / np.float64(scale)), 1.0


def sq_matrix(right, left):
    d = np.asarray(right).astype(np.float64)[:, None, :] - np.asarray(left).astype(np.float64)[None, :, :]
    with np.errstate(all="ignore"):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _near(sq, sc):
    """(2,778): row 0 = min over j per right vertex, row 1 = min over i per left vertex; a NaN never enters the minimum."""
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(sq), np.inf, sq)
        return np.stack([np.sqrt(m.min(axis=1)) / sc, np.sqrt(m.min(axis=0)) / sc])


def distances(pr, pl, gr, gl, scale):
    """dict(d_pred, d_gt (778,778), near (2,2,778) [hand, pred / gt, v]) of one sample, whether or not it is counted."""
    sc = np.float64(scale)
    sp, sg = sq_matrix(pr, pl), sq_matrix(gr, gl)
    with np.errstate(all="ignore"):
        out = dict(d_pred=np.sqrt(sp) / sc, d_gt=np.sqrt(sg) / sc)
    out["near"] = np.stack([_near(sp, sc), _near(sg, sc)], axis=1)
    return out


def contact_of(dist, counted, thresholds):
    """The words of one sample from its :func:`distances`: dict(counted, pair_sum, pairs, dev, counts (2,K,3) per hand, near (2,2,778)).
    ``pair_sum`` is the correctly ordered numpy sum; ``dev`` the sample's deviation (NaN without pairs)."""
    thr = np.asarray(thresholds, np.float64)
    K = len(thr)
    if not counted:
        return dict(counted=False, pair_sum=0.0, pairs=0, dev=float("nan"), counts=np.zeros((2, K, 3)), near=np.zeros((2, 2, NV)))
    with np.errstate(all="ignore"):
        in_c = dist["d_gt"] < thr[0]
        hit = dist["near"][:, :, None, :] < thr[None, None, :, None]              # (hand, pred / gt, K, v)
    pairs = int(in_c.sum())
    pair_sum = float(np.sum(dist["d_pred"][in_c]))
    counts = np.stack([(hit[:, 0] & hit[:, 1]).sum(axis=2), hit[:, 0].sum(axis=2), hit[:, 1].sum(axis=2)], axis=2).astype(np.float64)
    return dict(counted=True, pair_sum=pair_sum, pairs=pairs, dev=pair_sum / pairs if pairs else float("nan"), counts=counts,
                near=dist["near"])


def metrics_of(samples, mrrpes, thresholds):
    """The reported metrics from per-sample statements: ``samples`` the :func:`contact_of` dicts, ``mrrpes`` the (e, counted) pairs."""
    nan = float("nan")
    ratio = lambda a, b: a / b if b > 0 else nan
    es = [e for e, c in mrrpes if c]
    counted = [s for s in samples if s["counted"]]
    devs = [s["dev"] for s in counted if s["pairs"] > 0]
    c = sum((s["counts"].sum(axis=0) for s in counted), np.zeros((len(thresholds), 3)))
    P = np.array([ratio(tp, pp) for tp, pp, _ in c])
    R = np.array([ratio(tp, gp) for tp, _, gp in c])
    with np.errstate(all="ignore"):
        f1 = np.array([nan if np.isnan(p + r) else (2 * p * r / (p + r) if p + r > 0 else 0.0) for p, r in zip(P, R)])
    return dict(mrrpe=ratio(float(np.sum(es)), len(es)), contact_dev=ratio(float(np.sum(devs)), len(devs)),
                contact_rate=ratio(len(devs), len(counted)), contact_precision=P, contact_recall=R, contact_f1=f1)


def expected_sums(samples, mrrpes, thresholds):
    """The vector ``Evaluator.interaction_sums()`` is to return: [sum e, n, sum dev, with contact, counted, (tp, pp, gp) x K]."""
    es = [e for e, c in mrrpes if c]
    counted = [s for s in samples if s["counted"]]
    devs = [s["dev"] for s in counted if s["pairs"] > 0]
    c = sum((s["counts"].sum(axis=0) for s in counted), np.zeros((len(thresholds), 3)))
    return np.concatenate([[float(np.sum(es)), len(es), float(np.sum(devs)), len(devs), len(counted)], c.reshape(-1)]).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ mesh cases
class Case:
    def __init__(self, name, pr, pl, gr, gl, weight=(1.0, 1.0), scale=1.0, known=False):
        f = lambda a: np.ascontiguousarray(a, F32)
        self.name, self.pr, self.pl, self.gr, self.gl = name, f(pr), f(pl), f(gr), f(gl)
        self.weight, self.scale, self.known = np.asarray(weight, F32), F32(scale), known

    @property
    def counted(self):
        return bool(self.weight[0] > 0 and self.weight[1] > 0)


def lattice():
    """778 points of spacing 1/64 m: every coordinate and every shift by 2^-9 / 2^-8 is exact in float32."""
    i = np.arange(NV)
    return np.stack([i % 8, (i // 8) % 8, i // 64], axis=1) / 64.0


@functools.lru_cache(maxsize=None)
def gt_pairs():
    """name -> (right, left) float32 (778,3): the hand pairs of tests/volume_ref.py's generator (``helpers.oracle_two_hand_verts``)."""
    import helpers as H
    from ihmr_amd.assets import synthetic_mano
    mitten = synthetic_mano(True), synthetic_mano(False)
    fingers = synthetic_mano(True, kind="fingers"), synthetic_mano(False, kind="fingers")
    out = OrderedDict()
    for prefix, hv in (("default", H.oracle_two_hand_verts(mitten, 3, 11)[0]),
                       ("deep", H.oracle_two_hand_verts(mitten, 3, H.DEEP_SEED, overlap="deep")[0]),
                       ("fingers", H.oracle_two_hand_verts(fingers, 2, 12, interlock=True)[0])):
        hv = hv.numpy().astype(F32)
        for b in range(len(hv)):
            out[f"{prefix}_{b}"] = (hv[b, 0], hv[b, 1])
    return out


NOISE_SIGMA, SHIFT = 0.002, np.array([0.01, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def mesh_cases():
    """name -> Case.  Per GT pair three predictions (noise, the left hand shifted by 1 cm, pred = gt), then the edge cases on
    ``deep_0`` and the dyadic known answer."""
    t = OrderedDict()

    def add(name, *a, **kw):
        t[name] = Case(name, *a, **kw)

    for k, (name, (gr, gl)) in enumerate(gt_pairs().items()):
        rng = np.random.RandomState(7100 + k)
        add(f"{name}_noise", gr + rng.normal(0, NOISE_SIGMA, gr.shape), gl + rng.normal(0, NOISE_SIGMA, gl.shape), gr, gl)
        add(f"{name}_shift", gr, gl + SHIFT, gr, gl)
        add(f"{name}_same", gr, gl, gr, gl)
    gr, gl = gt_pairs()["deep_0"]
    pr, pl = t["deep_0_noise"].pr, t["deep_0_noise"].pl
    far = np.array([1.0, 0.0, 0.0])
    add("far_apart", pr, pl + far, gr, gl + far)                                        # counted, |C| = 0: no contact
    add("right_weight_0", pr, pl, gr, gl, weight=(0.0, 1.0))
    add("left_weight_1e-8", pr, pl, gr, gl, weight=(1.0, 1e-8))                         # > 0: counted
    add("left_weight_neg", pr, pl, gr, gl, weight=(1.0, -1.0))
    add("scale_0p25", pr, pl, gr, gl, scale=0.25)
    add("scale_1p7", pr, pl, gr, gl, scale=1.7)
    add("shifted_2m", pr + F32(2.0), pl + F32(2.0), gr + F32(2.0), gl + F32(2.0))
    nan_p = pr.copy()
    nan_p[345, 1] = np.nan
    add("nan_in_pred", nan_p, pl, gr, gl)
    nan_g = gl.copy()
    nan_g[np.unravel_index(np.argmin(sq_matrix(gr, gl)), (NV, NV))[1], 2] = np.nan          # the left vertex of the closest GT pair
    add("nan_in_gt", pr, pl, gr, nan_g)                                                 # its pairs leave C, its near_gt is +inf
    all_nan = np.full_like(pl, np.nan)
    add("left_pred_all_nan", pr, all_nan, gr, gl)                                       # near_pred = +inf everywhere
    g = lattice()
    add("dyadic", g, g + [0.0, 0.0, KNOWN_PRED], g, g + [0.0, 0.0, KNOWN_GT], known=True)
    return t


_DIST = {}


def case_distances(name):
    """The :func:`distances` of one case, computed once and shared by every test."""
    if name not in _DIST:
        c = mesh_cases()[name]
        _DIST[name] = distances(c.pr, c.pl, c.gr, c.gl, c.scale)
    return _DIST[name]


@functools.lru_cache(maxsize=None)
def case_statement(name, table):
    """:func:`contact_of` of one case under the threshold table ``table`` (a tuple)."""
    return contact_of(case_distances(name), mesh_cases()[name].counted, table)


# ------------------------------------------------------------------------------------------------------------------ joint cases
@functools.lru_cache(maxsize=None)
def joint_batch():
    """names, pred (B,42,3), gt (B,42,4), scale (B) float32, interacting (B) bool."""
    rng = np.random.RandomState(4221)
    names, P, G, S, I = [], [], [], [], []

    def add(name, p, g, w=None, scale=1.0, inter=True):
        w = np.ones(42) if w is None else np.asarray(w, np.float64)
        names.append(name); P.append(F32(p)); G.append(F32(np.concatenate([g, w[:, None]], axis=1))); S.append(F32(scale)); I.append(inter)

    def hands():
        g = rng.normal(0, 0.05, (42, 3))
        g[21:] += [0.12, 0.01, -0.03]
        return g + rng.normal(0, 0.01, (42, 3)), g

    def weights(**kw):
        w = np.ones(42)
        for k, v in kw.items():
            w[int(k[1:])] = v
        return w

    add("plain", *hands())
    p, g = hands()
    add("offset", p + [0.5, -1.0, 2.0], g + [-3.0, 0.25, 0.7])                          # a common offset of either side drops out
    add("scaled", *hands(), scale=1.7)
    add("scaled_small", *hands(), scale=0.25)
    add("right_wrist_weight_0", *hands(), w=weights(j0=0.0))
    add("left_wrist_weight_0", *hands(), w=weights(j21=0.0))
    add("fractional_weights", *hands(), w=weights(j0=1e-8, j21=0.5))                    # > 0: counted
    add("negative_weight", *hands(), w=weights(j21=-1.0))
    add("other_joints_weight_0", *hands(), w=np.where(np.isin(np.arange(42), (0, 21)), 1.0, 0.0))
    add("not_interacting", *hands(), inter=False)
    p, g = hands()
    add("pred_is_gt", F32(g), F32(g))                                                   # exactly 0
    g = np.stack([np.arange(42) % 4, (np.arange(42) // 4) % 4, np.arange(42) // 16], axis=1) / 16.0
    p = g.copy()
    p[21] += np.array([3.0, 4.0, 0.0]) / 512                                            # e = 5 / 512 exactly
    add("dyadic", p, g)
    p, g = hands()
    p[21, 1] = np.nan
    add("nan_joint", p, g)                                                              # NaN, counted
    p, g = hands()
    p[5, 0] = np.nan
    add("nan_elsewhere", p, g)                                                          # not a wrist: finite
    return names, np.stack(P), np.stack(G), np.array(S, F32), np.array(I, bool)


KNOWN_MRRPE = 5.0 / 512


@functools.lru_cache(maxsize=None)
def joint_reference():
    names, P, G, S, I = joint_batch()
    return [mrrpe_of(P[b], G[b], S[b], I[b]) for b in range(len(names))]


# ------------------------------------------------------------------------------------------------------------------ margins
def margin_violations(values, thresholds):
    v, t = np.asarray(values, np.float64).reshape(-1, 1), np.asarray(thresholds, np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        bad = (np.abs(v - t) < MARGIN) & ~((v == t) & np.isin(v, EXACT_VALUES))
    return [(float(v[i, 0]), float(t[0, k])) for i, k in zip(*np.nonzero(bad))]


def all_margin_violations(tables=None):
    """Every case against the given tables (default: all of TABLES); the known-answer case against KNOWN_TABLE as well."""
    bad = []
    for name, c in mesh_cases().items():
        d = case_distances(name)
        for table in ([KNOWN_TABLE] if c.known else []) + list(TABLES.values() if tables is None else tables):
            bad += [("pair", name) + x for x in margin_violations(d["d_gt"], table[:1])]
            bad += [("near", name) + x for x in margin_violations(d["near"], table)]
    return bad


# ------------------------------------------------------------------------------------------------------------------ an Evaluator batch
EVAL_CASES = ("deep_0_noise", "default_1_shift", "right_weight_0", "fingers_0_noise", "far_apart", "scale_1p7", "deep_2_same", "nan_in_pred",
              "default_0_noise", "dyadic")
EVAL_JOINTS = ("plain", "offset", "scaled", "right_wrist_weight_0", "fractional_weights", "not_interacting", "pred_is_gt", "dyadic",
               "negative_weight", "scaled_small")


@functools.lru_cache(maxsize=None)
def evaluator_batch():
    """One exported batch with GT meshes: sample b carries mesh case EVAL_CASES[b] and joint case EVAL_JOINTS[b], the mesh case's
    scale, a hand type (samples 3 and 8 are not interacting) and a keep mask (samples 1 and 6 are padding duplicates).  Returns
    (pred_results dict, data_list, keep (B,) bool, interacting (B,) bool)."""
    t = mesh_cases()
    names, P, G, _, _ = joint_batch()
    rows = [names.index(n) for n in EVAL_JOINTS]
    cases = [t[n] for n in EVAL_CASES]
    B = len(cases)
    inter = np.ones(B, bool)
    inter[[3, 8]] = False
    keep = np.ones(B, bool)
    keep[[1, 6]] = False
    res = dict(pred_cam_params=np.zeros((B, 3), F32), pred_shape_params=np.zeros((B, 20), F32), pred_pose_params=np.zeros((B, 96), F32),
               pred_hand_trans=np.zeros((B, 3), F32), pred_joints_3d=P[rows].copy(), gt_joints_3d=G[rows].copy(),
               collision_loss_origin_scale=np.zeros((B, 2 * NV), F32),
               pred_right_hand_verts=np.stack([c.pr for c in cases]), pred_left_hand_verts=np.stack([c.pl for c in cases]),
               gt_right_hand_verts=np.stack([c.gr for c in cases]), gt_left_hand_verts=np.stack([c.gl for c in cases]),
               mano_params_weight=np.stack([c.weight for c in cases]))
    data_list = {b: dict(scale=float(cases[b].scale), hand_type="interacting" if inter[b] else "right") for b in range(B)}
    return res, data_list, keep, inter


def evaluator_statement(table, rows=None):
    """(samples, mrrpes) of the kept rows of :func:`evaluator_batch` (``rows``: a subset of them): the contact statement of a kept,
    interacting sample with both hands annotated (else not counted) and its MRRPE pair."""
    res, data_list, keep, inter = evaluator_batch()
    samples, mrrpes = [], []
    for b in (range(len(keep)) if rows is None else rows):
        if not keep[b]:
            continue
        c = mesh_cases()[EVAL_CASES[b]]
        samples.append(contact_of(case_distances(c.name), c.counted and bool(inter[b]), tuple(table)))
        mrrpes.append(mrrpe_of(res["pred_joints_3d"][b], res["gt_joints_3d"][b], data_list[b]["scale"], bool(inter[b])))
    return samples, mrrpes


if __name__ == "__main__":       # prints what violates the margin (nothing, as committed) and the cases' contact figures
    for K, table in TABLES.items():
        print("K", K, all_margin_violations([table]))
    for name, c in mesh_cases().items():
        s = case_statement(name, TABLES[2])
        d = case_distances(name)
        with np.errstate(all="ignore"):
            closest = np.nanmin(np.abs(d["d_gt"] - TABLES[2][0]))
        print(f"{name:20s} counted {s['counted']!s:5s} |C| {s['pairs']:4d} dev {s['dev']:.6f} counts@3mm {s['counts'][:, 0].tolist()} "
              f"closest pair to tau_c {closest:.2e}")

"""Host-side evaluation, mirroring the metric half of the reference's ``src/utils/evaluator.py`` and
``src/utils/metric_utils.py`` (CPU / numpy in the reference too), and its visualisation half (``evaluator.py:184-291``):
``Evaluator.visualize_result`` renders the stored meshes over their images on the GPU (:mod:`ihmr_amd.render`) and
``python -m ihmr_amd.evaluator METHOD DATASET`` is the reference's ``main()``.

``Evaluator.update(data_idxs, pred_results)`` consumes the dict of ``get_pred_result()`` exactly like
``evaluator.py:38-97``; the four reported metrics are ``mpjpe_3d``, ``inter_mpjpe_3d``, ``collision_ave``,
``collision_max`` (``evaluator.py:149-181``, printed by ``optimize.py:98-102``), plus ``mpvpe_3d`` for the models that
export GT meshes (IHMR-Baseline / IHMR-MLP; see :func:`get_single_verts_error`).  For multi-GPU runs
``metric_sums()`` returns the additive form that :func:`ihmr_amd.dist.reduce_metrics` all-reduces.

``Evaluator.update_device(...)`` is the same arithmetic on the GPU (``ihmr_eval_metrics``): it takes
the DEVICE tensors of a model (no export to numpy), leaves (B,6) float64 partial results on the device and only
adds them up when the metrics are asked for -- the per-sample Python loop and the 1 MB/batch device-to-host copies
of ``get_pred_result()`` drop out of a throughput run.

``Evaluator(curve_metrics=True)`` adds the other half of a hand-mesh result table: the PCK curve (share of points whose error is at most
tau) and its AUC for five error populations, the mesh F-score at 5 mm / 15 mm and the reference's collision AUC
(:func:`calc_collision_auc`).  None of them follows from the sums above; all of them follow from COUNTS per threshold, which add over
batches and ranks (:meth:`Evaluator.curve_sums`, :meth:`Evaluator.curve_metrics_from_sums`).  ``update_device_curves`` /
``update_device_curve_verts`` count on the GPU (``ihmr_eval_curve_joints`` / ``ihmr_eval_curve_verts``).

``Evaluator(volume_metric=True)`` adds the two-hand intersection volume in cm^3 (``pen_volume``, ``pen_rate``): the voxels of one grid
common to both hands that lie inside both (``ihmr_sdf_volume``), where ``collision_ave`` / ``collision_max`` are
depths read at vertices.  It is device-only (:meth:`Evaluator.update_device_volume`, :meth:`Evaluator.volume_sums`): no record, no
pickled file and none of the other sums changes with it.

``Evaluator(interaction_metrics=True)`` adds what compares how the two hands sit RELATIVE TO EACH OTHER with the ground truth
(DESIGN.md section 8, row (f)7): ``mrrpe``, the error of the vector from the right wrist to the left wrist, and the contact
consistency -- ``contact_dev`` (how far apart the predicted vertices of a vertex pair are that touches in the ground truth),
``contact_rate`` and, per threshold of ``contact_thresholds``, the micro-averaged ``contact_precision`` / ``contact_recall`` /
``contact_f1`` of the per-vertex contact maps.  Host records (:func:`get_single_mrrpe`, :func:`get_single_contact`) and device
(:meth:`Evaluator.update_device_mrrpe` / :meth:`Evaluator.update_device_contact`: ``ihmr_eval_mrrpe`` / ``ihmr_eval_contact``) add up
in :meth:`Evaluator.interaction_sums`.

``Evaluator(surface_metrics=True)`` measures against the SURFACE of the other hand (``ihmr_surface_distance``, DESIGN.md section 8, row
(f)8): ``pen_depth_max`` / ``pen_depth_ave`` / ``pen_vertex_rate`` -- the depth of a vertex under the other hand's skin in true
millimetres, the exact counterparts of ``collision_max`` / ``collision_ave`` -- and, with GT meshes, ``surface_contact_precision`` /
``surface_contact_recall`` / ``surface_contact_f1`` per threshold of ``surface_thresholds``, where a vertex is in contact when its
distance to the other hand's surface (not to its nearest vertex) lies below the threshold.  Device-only, like the volume
(:meth:`Evaluator.update_device_surface`, :meth:`Evaluator.surface_sums`).
"""
from __future__ import annotations

import os
import os.path as osp
import sys

import numpy as np


def _ratio(a, b):
    """a / b as a float, NaN where nothing was counted (b = 0)."""
    return float(a / b) if b > 0 else float("nan")


def get_single_joints_error(pred, gt, joint_weights, scale_factor):
    """metric_utils.py:23-38 -- per-hand MPJPE; the root subtraction is cumulative on the same copies."""
    a, b = pred.copy(), gt.copy()
    errors = []
    for i in (0, 21):
        if joint_weights[i, 0] > 0:
            a -= a[i:i + 1, :]
            b -= b[i:i + 1, :]
            for j in range(21):
                if joint_weights[i + j, 0] > 0:
                    errors.append(np.linalg.norm(a[i + j] - b[i + j]) / scale_factor)
    return errors


def calc_transform_no_rot(S1, S2):
    """metric_utils.py:107-117 -- per-axis mean / std alignment."""
    m1, m2 = np.mean(S1, axis=0).reshape(1, 3), np.mean(S2, axis=0).reshape(1, 3)
    s1, s2 = np.std(S1, axis=0).reshape(1, 3), np.std(S2, axis=0).reshape(1, 3)
    return (S1 - m1) / s1 * s2 + m2


def calc_transform(S1, S2):
    """metric_utils.py:59-104 -- similarity Procrustes alignment of S1 onto S2, restated with the reference's dtype behaviour: the
    covariance and the SVD run in the dtype of the inputs (float32 arrays stay float32; only the sign matrix is float64, which lifts
    the rotation and everything after it to float64), and, like the reference, the inputs are transposed to coordinates x points
    ONLY when ``S1.shape[0]`` is neither 3 nor 2.  A set of exactly 3 or exactly 2 points, shaped (3,3) or (2,3), is therefore read
    as coordinates x points and a different problem is solved (for (2,3): in two dimensions).  :func:`procrustes_align` is the
    points-in-rows form that the Evaluator's PA metrics are defined by."""
    transposed = S1.shape[0] != 3 and S1.shape[0] != 2
    if transposed:
        S1, S2 = S1.T, S2.T
    assert S2.shape[1] == S1.shape[1]
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = np.sum(X1 ** 2)
    K = X1.dot(X2.T)
    U, _, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(U.shape[0])
    Z[-1, -1] *= np.sign(np.linalg.det(U.dot(V.T)))
    R = V.dot(Z.dot(U.T))
    scale = np.trace(R.dot(K)) / var1
    t = mu2 - scale * (R.dot(mu1))
    S1_hat = scale * R.dot(S1) + t
    return S1_hat.T if transposed else S1_hat


def get_single_pa_inter_joints_error(pred, gt, joints_valid, scale_factor, use_rot=False):
    """metric_utils.py:120-143; ``use_rot=True`` aligns with :func:`calc_transform` (the reference's reading of 3 and 2 valid
    joints included), the default with :func:`calc_transform_no_rot`."""
    v = joints_valid[:, 0] if joints_valid.ndim == 2 else joints_valid
    if np.sum(v) < 2.0:
        return []
    p, g = pred[v > 0, :3], gt[v > 0, :3]
    transform = calc_transform if use_rot else calc_transform_no_rot
    return (np.linalg.norm(transform(p.copy(), g.copy()) - g, axis=1) / scale_factor).tolist()


PA_MIN_WEIGHT_SUM = 2.0        # metric_utils.py:131: the SUM of the weights, not the number of valid points


def procrustes_align(S1, S2):
    """S1 (n,3) aligned onto S2 (n,3) by the similarity transform (proper rotation, scale, translation) of least squared error:
    always points in rows, always float64.  For n not in {2, 3} this is :func:`calc_transform` on float64 inputs; 2 points are
    mapped onto their targets exactly.  Returns None when all points of S1 coincide (``var1 == 0``): the reference divides by zero
    there, this build leaves the set out (a deviation, so that one sample cannot turn a float64 sum into NaN).  The test is exact
    for float32 inputs, which is what the models export: a float64 sum of equal float32 values is exact, so is their mean."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    assert S1.ndim == 2 and S1.shape[1] == 3 and S1.shape == S2.shape and len(S1) > 0
    m1, m2 = S1.mean(axis=0), S2.mean(axis=0)
    X1, X2 = S1 - m1, S2 - m2
    var1 = np.sum(X1 ** 2)
    if var1 == 0.0:
        return None
    K = X1.T @ X2                                   # K[a][b] = sum x1_a x2_b
    U, _, Vh = np.linalg.svd(K)                     # full 3 x 3 factors: the basis of a rank-deficient K is completed
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T
    scale = np.trace(R @ K) / var1
    return scale * (S1 @ R.T) + (m2 - scale * (R @ m1))


def get_single_pa_error(pred, gt, weights, scale_factor):
    """Aligned per-point errors of ONE set (the valid points of ``pred`` / ``gt`` (n,3)), by the set rules shared with the device
    (``ihmr_eval_pa_joints`` / ``ihmr_eval_pa_verts``): a point is valid when its weight is > 0; the set is left out ([]) when the
    sum of its weights is < 2.0 or when :func:`procrustes_align` refuses it."""
    w = np.asarray(weights, np.float64).reshape(-1)
    if np.sum(w) < PA_MIN_WEIGHT_SUM or not (w > 0).any():
        return []
    g = np.asarray(gt, np.float64)[w > 0, :3]
    aligned = procrustes_align(np.asarray(pred)[w > 0, :3], g)
    if aligned is None:
        return []
    return (np.linalg.norm(aligned - g, axis=1) / scale_factor).tolist()


def get_single_verts_error(pred_verts, gt_verts, root_weights, scale_factor):
    """MPVPE of ONE hand (BASELINE.json names the metric; the reference exports what it needs -- predicted and GT
    meshes, ``baseline_model.py:365-368``, ``mlp_model.py:708-711`` -- but never computes it).
    Defined like the reference's MPJPE (``metric_utils.py:23-38``: root-relative per hand, L2 per point, / scale):
    both meshes are made relative to their own wrist, the wrist being regressed from the mesh itself with row 0 of
    the MANO joint regressor (``root_weights`` (778,)), then the 778 per-vertex distances."""
    pr = pred_verts.astype(np.float64) - root_weights.astype(np.float64) @ pred_verts.astype(np.float64)
    gr = gt_verts.astype(np.float64) - root_weights.astype(np.float64) @ gt_verts.astype(np.float64)
    return (np.linalg.norm(pr - gr, axis=1) / scale_factor).tolist()


# ------------------------------------------------------------------------------------------ curve metrics: PCK / AUC, F-score, collision AUC
CURVE_THRESHOLDS = np.linspace(0, 0.05, 100)        # PCK thresholds in the error's units (metres / scale)
F_THRESHOLDS = (0.005, 0.015)                       # F-score thresholds: 5 mm and 15 mm
COLLISION_AUC_THRESHOLDS = np.linspace(0.5, 15)     # metric_utils.py:149-153 [mm]
CURVE_POPULATIONS = ("j3d", "pa_inter_j3d", "pa_j3d", "v3d", "pa_v3d")
MAX_THRESHOLDS, MAX_F_THRESHOLDS = 256, 8           # include/ihmr_hip.h


def calc_collision_auc(collision_all):
    """metric_utils.py:146-160, operation for operation: the share of samples whose penetration depth [mm] is below a threshold, over
    ``np.linspace(0.5, 15)``, integrated by the trapezoid rule over the normalised threshold."""
    col_all = collision_all
    start = 0.5
    end = 15
    xs = list()
    ratios = list()
    for thresh in np.linspace(start, end):
        ratio = np.mean(col_all < thresh)
        x = (thresh - start) / (end - start)
        xs.append(x)
        ratios.append(ratio)
    return _trapz(ratios, xs)


def _trapz(y, x):
    """``np.trapz`` (``np.trapezoid`` from numpy 2.0 on), the same operations in the same order."""
    y, x = np.asanyarray(y), np.asanyarray(x)
    return (np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum()


def check_thresholds(thresholds, limit, what="thresholds", allow_empty=False):
    """A threshold table as float64: 1-D, at most ``limit`` entries, finite and strictly ascending -- else ValueError."""
    t = np.array(thresholds, dtype=np.float64)
    if t.ndim != 1 or len(t) > limit or (len(t) == 0 and not allow_empty):
        raise ValueError(f"{what}: a 1-D table of {0 if allow_empty else 1}..{limit} values is needed, got shape {t.shape}")
    if not np.isfinite(t).all() or not (np.diff(t) > 0).all():
        raise ValueError(f"{what} must be finite and strictly ascending")
    return t


def curve_counts(errors, thresholds, strict=False):
    """(T,) float64: the number of ``errors`` that are <= each threshold (``strict``: < each threshold)."""
    e, t = np.asarray(errors, np.float64).reshape(-1), np.asarray(thresholds, np.float64)
    hit = (e[None, :] < t[:, None]) if strict else (e[None, :] <= t[:, None])
    return hit.sum(axis=1).astype(np.float64)


def curve_auc(counts, n, thresholds):
    """Trapezoid of ``counts / n`` over x_k = (tau_k - tau_0) / (tau_{T-1} - tau_0), the formula of :func:`calc_collision_auc`.
    NaN without points (n = 0) and for a single threshold."""
    t = np.asarray(thresholds, np.float64)
    if not n > 0 or len(t) < 2:
        return float("nan")
    return float(_trapz(np.asarray(counts, np.float64) / n, (t - t[0]) / (t[-1] - t[0])))


def nn_distances(pred, gt):
    """Brute-force nearest-neighbour distances between two point sets, float64: ``d_pg[i] = min_j |p_i - g_j|`` and
    ``d_gp[j] = min_i |p_i - g_j|``.  Every squared distance is ``(dx*dx + dy*dy) + dz*dz``; the minimum is taken on the squares and
    the root once (min is exact and sqrt monotone: the order of the search cannot change a bit)."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    d = p[:, None, :] - g[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(d2.min(axis=1)), np.sqrt(d2.min(axis=0))


def fscore_from_counts(n_pg, n_gp, n):
    """F = 2 P R / (P + R) with P = n_pg / n, R = n_gp / n; 0 where P + R = 0.  Elementwise over the thresholds."""
    P, R = np.asarray(n_pg, np.float64) / n, np.asarray(n_gp, np.float64) / n
    den = P + R
    return np.where(den > 0, 2.0 * P * R / np.where(den > 0, den, 1.0), 0.0)


def get_single_fscore_counts(pred_verts, gt_verts, root_weights, scale, f_thresholds, aligned):
    """ONE hand: ``(counts (2,F), d_pg, d_gp)`` with ``counts[0][k] = #(d_pg < tau_k)`` and ``counts[1][k] = #(d_gp < tau_k)`` (strict),
    the distances divided by ``scale``.  ``aligned=False``: both meshes relative to their own root as in
    :func:`get_single_verts_error`, the difference taken as (P_i - root P) - (G_j - root G).  ``aligned=True``: the prediction mapped
    onto the target by :func:`procrustes_align`; None when the PA rules leave the hand out."""
    P, G = np.asarray(pred_verts).astype(np.float64), np.asarray(gt_verts).astype(np.float64)
    if aligned:
        p, g = procrustes_align(P, G), G
        if p is None:
            return None
    else:
        rw = np.asarray(root_weights).astype(np.float64)
        p, g = P - rw @ P, G - rw @ G
    d_pg, d_gp = nn_distances(p, g)
    d_pg, d_gp = d_pg / scale, d_gp / scale
    return np.stack([curve_counts(d_pg, f_thresholds, strict=True), curve_counts(d_gp, f_thresholds, strict=True)]), d_pg, d_gp


# ------------------------------------------------------------------------------------------ interacting-hand metrics: MRRPE, contact
CONTACT_THRESHOLDS = (0.003, 0.005)                 # contact thresholds in metres / scale; the first one defines the contact PAIRS
MAX_CONTACT_THRESHOLDS = 8                          # include/ihmr_hip.h: IHMR_EVAL_MAX_CONTACT_THRESHOLDS
SURFACE_THRESHOLDS = (0.003, 0.005)                 # surface-contact thresholds in metres / scale (at most MAX_CONTACT_THRESHOLDS)


def get_single_mrrpe(pred, gt, joint_weights, scale_factor):
    """[e] with ``e = |(P[21] - P[0]) - (G[21] - G[0])| / scale`` in float64 -- the error of the vector from the right wrist to the
    left wrist -- or [] unless the weights of both wrists are > 0.  A non-finite input gives a non-finite e, which is counted."""
    w = np.asarray(joint_weights).reshape(-1)
    if not (w[0] > 0 and w[21] > 0):
        return []
    p, g = np.asarray(pred)[:, :3].astype(np.float64), np.asarray(gt)[:, :3].astype(np.float64)
    d = (p[21] - p[0]) - (g[21] - g[0])
    with np.errstate(all="ignore"):
        return [float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / np.float64(scale_factor))]


def pair_sq_distances(right, left):
    """(778,778) float64: ``sq[i][j] = (dx*dx + dy*dy) + dz*dz`` of right[i] - left[j]."""
    d = np.asarray(right).astype(np.float64)[:, None, :] - np.asarray(left).astype(np.float64)[None, :, :]
    with np.errstate(all="ignore"):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def get_single_contact(pred_r, pred_l, gt_r, gt_l, scale, thresholds):
    """Contact consistency of ONE sample with both hands annotated: ``(pair_sum, pair_count, counts (K,3), near (2,2,778))``.
    ``d_X(i, j) = sqrt(sq_dist(R_X[i], L_X[j])) / scale``; the contact pairs are ``C = {(i, j): d_gt(i, j) < thresholds[0]}`` (strict,
    a NaN distance is never in contact), ``pair_sum`` the sum of ``d_pred`` over C, ``pair_count = |C|``.  ``near[h][x][v]``: the
    distance from vertex v of hand h (0 = right) to the nearest vertex of the other hand in the predicted (x = 0) / target (x = 1)
    pair -- the minimum on the squares, which a NaN never enters, then one root; +inf / scale without a comparable partner.
    ``counts[k] = [tp, pp, gp]``: of the 1556 vertices those with ``near < thresholds[k]`` in both, in pred, in gt."""
    thr, sc = np.asarray(thresholds, np.float64), np.float64(scale)
    near = np.zeros((2, 2, len(pred_r)), np.float64)
    with np.errstate(all="ignore"):
        sq = [pair_sq_distances(pred_r, pred_l), pair_sq_distances(gt_r, gt_l)]
        in_c = np.sqrt(sq[1]) / sc < thr[0]
        d_pred = (np.sqrt(sq[0]) / sc)[in_c]
        for x in range(2):
            comparable = np.where(np.isnan(sq[x]), np.inf, sq[x])
            near[0, x], near[1, x] = np.sqrt(comparable.min(axis=1)) / sc, np.sqrt(comparable.min(axis=0)) / sc
        hit = near[None] < thr[:, None, None, None]                       # (K, hand, pred / gt, v)
    counts = np.stack([(hit[:, :, 0] & hit[:, :, 1]).sum(axis=(1, 2)), hit[:, :, 0].sum(axis=(1, 2)), hit[:, :, 1].sum(axis=(1, 2))], axis=1)
    return float(np.sum(d_pred)), int(in_c.sum()), counts.astype(np.float64), near


def load_image_bgr(path):
    """The default image loader of :meth:`Evaluator.visualize_result`: (H,W,3) uint8 in BGR order, as ``cv2.imread`` returns it."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def write_image_bgr(path, img):
    """Writes a (H,W,3) uint8 BGR array by the path's extension (stands for ``cv2.imwrite``, evaluator.py:255)."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(np.asarray(img)[:, :, ::-1])).save(path)


class Evaluator:
    def __init__(self, mano_models=None, data_list=None, image_root="", inputSize=224, pa_metrics=False, curve_metrics=False,
                 thresholds=None, f_thresholds=None, volume_metric=False, volume_subdiv=2, interaction_metrics=False, contact_thresholds=None,
                 surface_metrics=False, surface_thresholds=None):
        self.pa_metrics = pa_metrics    # records carry the Procrustes-aligned errors too (off: records and files as before)
        # records carry what the PCK curves, the F-scores and the collision AUC are counted from (off: records and files as before)
        self.curve_metrics = curve_metrics
        self.thresholds = check_thresholds(CURVE_THRESHOLDS if thresholds is None else thresholds, MAX_THRESHOLDS)
        self.f_thresholds = check_thresholds(F_THRESHOLDS if f_thresholds is None else f_thresholds, MAX_F_THRESHOLDS, "f_thresholds", True)
        self.inputSize = inputSize      # evaluator.py:27 (model.inputSize): the visualisation renders at twice this size by default
        self.left_hand_faces = None if mano_models is None else mano_models["left"].faces
        self.right_hand_faces = None if mano_models is None else mano_models["right"].faces
        # wrist row of the joint regressor per hand (MPVPE root), (2,778): 0 = right, 1 = left
        self.root_weights = None
        if mano_models is not None and hasattr(mano_models["right"], "J_regressor"):
            jr = lambda m: np.asarray(m.J_regressor.detach().cpu().numpy() if hasattr(m.J_regressor, "detach") else m.J_regressor)[0]
            self.root_weights = np.stack([jr(mano_models["right"]), jr(mano_models["left"])]).astype(np.float32)
        self.data_list = data_list or {}        # list (the reference's dataset.data_list) or dict: data_idx -> metadata
        self.image_root = image_root
        self.save_verts = True
        self.pred_results = []
        for name in self.DEVICE_ACCUMULATORS[:-1]:
            setattr(self, name, [])
        if volume_metric:               # off: no attribute is added, a default Evaluator pickles byte for byte as before
            if volume_subdiv not in (1, 2, 4):
                raise ValueError(f"volume_subdiv = {volume_subdiv!r}: 1, 2 or 4")
            self.volume_metric, self.volume_subdiv = True, int(volume_subdiv)
            self._device_volume_parts = []
        if interaction_metrics:         # off: no attribute is added either
            self.interaction_metrics = True
            self.contact_thresholds = check_thresholds(CONTACT_THRESHOLDS if contact_thresholds is None else contact_thresholds,
                                                       MAX_CONTACT_THRESHOLDS, "contact_thresholds")
            for name in self.INTERACTION_ACCUMULATORS:
                setattr(self, name, [])
        elif contact_thresholds is not None:
            raise ValueError("contact_thresholds needs interaction_metrics=True")
        if surface_metrics:             # off: no attribute is added either
            self.surface_metrics = True
            self.surface_thresholds = check_thresholds(SURFACE_THRESHOLDS if surface_thresholds is None else surface_thresholds,
                                                       MAX_CONTACT_THRESHOLDS, "surface_thresholds")
            for name in self.SURFACE_ACCUMULATORS:
                setattr(self, name, [])
        elif surface_thresholds is not None:
            raise ValueError("surface_thresholds needs surface_metrics=True")

    # What the update_device_* methods leave on the device, one entry per batch, summed lazily.  The names and their order in __dict__
    # are part of the pickled file; the last one exists only with volume_metric.
    DEVICE_ACCUMULATORS = (
        "_device_parts",              # (B,7) float64: the six words of ihmr_eval_metrics + [interacting]
        "_device_vert_parts",         # (B,2) float64 [sum of per-vertex errors, count]
        "_device_pa_parts",           # (B,4) float64 [sum of set 0, count, sum of the per-hand sets, count]
        "_device_pa_vert_parts",      # (B,2) float64 [sum of aligned per-vertex errors, count]
        "_device_curve_parts",        # (B,3,T+1) float64 counts of the joint populations
        "_device_curve_vert_parts",   # ((B,2,T+1) counts, (B,2,2,2,F) per-hand F counts, (B,2,2) hand counted and kept)
        "_device_volume_parts")       # (B,4) float64 [cm^3, interacting and kept, of those with count > 0, invalid]

    # The same for the interacting-hand metrics; both exist only with interaction_metrics (as the volume's only with volume_metric).
    INTERACTION_ACCUMULATORS = (
        "_device_mrrpe_parts",        # (B,2) float64 [e, counted]
        "_device_contact_parts")      # ((B,3) [the sample's deviation, has contact pairs, counted], (B,K,3) [tp, pp, gp] of both hands)

    # The same for the surface metrics; it exists only with surface_metrics.
    SURFACE_ACCUMULATORS = (
        "_device_surface_parts",)     # ((B,5) [max depth mm, mean depth mm, inside vertices, counted, counted with GT], (B,K,3) [tp, pp, gp])

    def clear(self):
        self.pred_results = []
        for name in self.DEVICE_ACCUMULATORS:
            if name in self.__dict__ or name != "_device_volume_parts":
                setattr(self, name, [])
        for name in self.INTERACTION_ACCUMULATORS + self.SURFACE_ACCUMULATORS:
            if name in self.__dict__:
                setattr(self, name, [])

    def _device_rows(self, name, item=None):
        """The parts of accumulator ``name`` (of a tuple-valued one: their entry ``item``) as one device tensor, in the order they were
        added; None when the attribute is absent (an older pickle) or empty."""
        parts = getattr(self, name, None)
        if not parts:
            return None
        import torch
        return torch.cat(parts if item is None else [p[item] for p in parts], dim=0)

    def _add_device_sums(self, sums, name, item=None):
        """Adds the column sums of accumulator ``name`` to ``sums`` (a view of a host vector) in place."""
        d = self._device_column_sums(name, item)
        if d is not None:
            sums += d

    def _device_column_sums(self, name, item=None):
        """The column sums of :meth:`_device_rows` on the host, or None.  One reduction over all samples in the order they were added:
        the float64 sum does not depend on how the samples were grouped into batches / launch sequences."""
        rows = self._device_rows(name, item)
        return None if rows is None else rows.sum(dim=0).cpu().numpy()

    def _on_device(self, attr, dev, make):
        """``make(dev)``, kept in ``self.<attr>`` and made again only for another device."""
        cached = self.__dict__.get(attr)
        if not isinstance(cached, tuple) or cached[0] != dev:
            cached = (dev, make(dev))
            setattr(self, attr, cached)
        return cached[1]

    def _root_w(self, dev, what):
        import torch
        assert self.root_weights is not None, f"Evaluator needs the MANO models (J_regressor) for {what}"
        return self._on_device("_root_w_dev", dev, lambda d: torch.from_numpy(self.root_weights).to(d).contiguous())

    def _curve_tables(self, dev):
        """The two threshold tables on ``dev`` (float64; the second None when empty), uploaded once per device."""
        import torch
        up = lambda t: torch.from_numpy(t).to(dev) if len(t) else None
        return self._on_device("_curve_tables_dev", dev, lambda d: (up(self.thresholds), up(self.f_thresholds)))

    @staticmethod
    def _launch(entry, inputs, scale, out_shapes, args):
        """One launch of the evaluation entry point ``entry``: ``inputs`` (and ``scale`` unless None) as float32 contiguous tensors on
        the device of the first, one new (B, *shape) float64 tensor per ``out_shapes``; ``args(inputs, scale, B, outs)`` lays them out
        in the entry point's order (a tensor stands for its pointer, None for NULL; the stream follows).  Returns the outputs."""
        import torch

        from . import hip
        hip.require_gpu()
        B, dev = inputs[0].shape[0], inputs[0].device
        # only the pointer is read: a tensor that already is float32, contiguous and on the device is taken as it is
        f = lambda t: t if t.dtype == torch.float32 and t.device == dev and t.is_contiguous() else t.detach().to(dev, torch.float32).contiguous()
        ins, sc = [f(t) for t in inputs], None if scale is None else f(scale)
        outs = [torch.empty(B, *shape, device=dev, dtype=torch.float64) for shape in out_shapes]
        ptr = lambda a: a if a is None or isinstance(a, int) else a.data_ptr()
        hip.check(getattr(hip.lib(), entry)(*map(ptr, args(ins, sc, B, outs)), hip.stream_ptr()), entry)
        return outs

    def _kept(self, keep, *parts):
        """``parts`` (B,...) with the rows outside ``keep`` (B) bool set to zero -- a selection, not a product: a masked-out row may hold
        NaN / Inf, and 0 * NaN is NaN.  The sums and counts are >= 0, so a kept row keeps its bits and a dropped one is +0."""
        if keep is None:
            return parts
        import torch
        dev = parts[0].device
        zero = self._on_device("_zero_dev", dev, lambda d: torch.zeros((), dtype=torch.float64, device=d))
        k = keep.to(dev, torch.bool)
        return tuple(torch.where(k.reshape((-1,) + (1,) * (p.dim() - 1)), p, zero) for p in parts)

    def update_device_curves(self, pred_joints_3d, gt_joints_3d, keep=None, scale=None):
        """Counts per threshold of the three joint populations of one batch from device tensors (``ihmr_eval_curve_joints``);
        arguments as :meth:`update_device_pa`.  Accumulates lazily, see :meth:`curve_sums`."""
        thr, T = self._curve_tables(pred_joints_3d.device)[0], len(self.thresholds)
        out, = self._launch("ihmr_eval_curve_joints", (pred_joints_3d, gt_joints_3d), scale, [(3, T + 1)],
                            lambda i, sc, B, o: (*i, sc, B, thr, T, *o))
        self._device_curve_parts.append(self._kept(keep, out)[0])

    def update_device_curve_verts(self, pred_right, pred_left, gt_right, gt_left, mano_params_weight, keep=None, scale=None):
        """Counts per threshold of the two vertex populations and the per-hand F-scores (raw and aligned) of one batch from device
        tensors (``ihmr_eval_curve_verts``); arguments as :meth:`update_device_verts`."""
        root_w = self._root_w(pred_right.device, "the root-relative vertex errors")
        thr, fthr = self._curve_tables(pred_right.device)
        T, F = len(self.thresholds), len(self.f_thresholds)
        counts, fc = self._launch("ihmr_eval_curve_verts", (pred_right, pred_left, gt_right, gt_left, mano_params_weight), scale,
                                  [(2, 2, T + 1), (2, 2, 2, F)],
                                  lambda i, sc, B, o: (*i[:4], root_w, i[4], sc, B, thr, T, fthr, F, o[0], o[1] if F else None, None))
        # the counts stay what they are: F is formed per hand on the host (:func:`fscore_from_counts`, the one formula of both paths),
        # of the hands that `counted` names -- which is why `fc` needs no selection of its own
        counted = (counts[..., T] > 0).to(counts.dtype)                     # (B,2,2): hand, raw / pa
        csum, counted = self._kept(keep, counts[:, 0] + counts[:, 1], counted)
        self._device_curve_vert_parts.append((csum, fc, counted))

    def update_device_pa(self, pred_joints_3d, gt_joints_3d, keep=None, scale=None):
        """Procrustes-aligned joint errors of one batch from device tensors (``ihmr_eval_pa_joints``): pred_joints_3d (B,42,3),
        gt_joints_3d (B,42,4); ``keep`` and ``scale`` as in :meth:`update_device`.  Accumulates lazily, see :meth:`pa_metric_sums`."""
        import torch
        out, = self._launch("ihmr_eval_pa_joints", (pred_joints_3d, gt_joints_3d), scale, [(3, 2)], lambda i, sc, B, o: (*i, sc, B, *o, None))
        self._device_pa_parts.append(self._kept(keep, torch.cat([out[:, 0], out[:, 1] + out[:, 2]], dim=1))[0])

    def update_device_pa_verts(self, pred_right, pred_left, gt_right, gt_left, mano_params_weight, keep=None, scale=None):
        """PA-MPVPE partial sums of one batch from device tensors (``ihmr_eval_pa_verts``); arguments as :meth:`update_device_verts`."""
        out, = self._launch("ihmr_eval_pa_verts", (pred_right, pred_left, gt_right, gt_left, mano_params_weight), scale, [(2, 2)],
                            lambda i, sc, B, o: (*i, sc, B, *o, None))
        self._device_pa_vert_parts.append(self._kept(keep, out[:, 0] + out[:, 1])[0])

    def update_device(self, pred_joints_3d, gt_joints_3d, collision_loss_origin_scale, keep=None, interacting=None, scale=None):
        """Metrics of one batch straight from device tensors: pred_joints_3d (B,42,3), gt_joints_3d (B,42,4),
        collision_loss_origin_scale (B,1556); ``keep`` (B) bool masks out padding duplicates (evaluator.py:137-146),
        ``interacting`` (B) bool = hand_type == 'interacting' (default all), ``scale`` (B) (default 1)."""
        import torch
        dev = pred_joints_3d.device
        it = None if interacting is None else interacting.to(dev, torch.uint8).contiguous()
        out, = self._launch("ihmr_eval_metrics", (pred_joints_3d, gt_joints_3d, collision_loss_origin_scale), scale, [(6,)],
                            lambda i, sc, B, o: (*i, sc, it, B, *o))
        n_inter = torch.ones(len(out), device=dev, dtype=torch.float64) if it is None else it.to(torch.float64)
        self._device_parts.append(self._kept(keep, torch.cat([out, n_inter[:, None]], dim=1))[0])      # [.., n_interacting]

    def update_device_verts(self, pred_right, pred_left, gt_right, gt_left, mano_params_weight, keep=None, scale=None):
        """MPVPE partial sums of one batch from device tensors: the four meshes (B,778,3) and ``mano_params_weight`` (B,2)
        (a hand counts when its MANO annotation exists, i.e. weight > 0).  ``ihmr_eval_mpvpe``."""
        root_w = self._root_w(pred_right.device, "MPVPE")
        out, = self._launch("ihmr_eval_mpvpe", (pred_right, pred_left, gt_right, gt_left, mano_params_weight), scale, [(4,)],
                            lambda i, sc, B, o: (*i[:4], root_w, i[4], sc, B, *o))
        self._device_vert_parts.append(self._kept(keep, out[:, 0:2] + out[:, 2:4])[0])

    def update_device_volume(self, pred_right, pred_left, keep=None, interacting=None):
        """Two-hand intersection volume of one batch from device tensors (``ihmr_sdf_volume`` through
        :func:`ihmr_amd.sdf.penetration_volume`, ``Evaluator(volume_metric=True, volume_subdiv=2)``): the two predicted meshes
        (B,778,3), the MANO faces with the wrist closed.  ``keep`` (B) bool masks out padding duplicates, ``interacting`` (B) bool =
        hand_type == 'interacting' (default all); a sample outside either mask is not ray-traced and counts nowhere.  Accumulates
        lazily, see :meth:`volume_sums`.  The metric is device-only: there is no host-records path, the records, ``metric_sums()``,
        ``pa_metric_sums()``, ``curve_sums()`` and pickled files carry nothing of it."""
        import torch

        from . import hip, sdf
        if not getattr(self, "volume_metric", False):
            raise RuntimeError("update_device_volume needs Evaluator(volume_metric=True)")
        hip.require_gpu()
        assert self.right_hand_faces is not None and self.left_hand_faces is not None, "Evaluator needs the MANO models' faces"
        B, dev = pred_right.shape[0], pred_right.device
        use = torch.ones(B, dtype=torch.bool, device=dev)
        for mask in (keep, interacting):
            if mask is not None:
                use = use & mask.to(dev, torch.bool)
        volume, _, _, status = sdf.penetration_volume(pred_right, pred_left, self.right_hand_faces, self.left_hand_faces,
                                                      subdiv=self.volume_subdiv, keep=use)
        n = use.to(torch.float64)
        zero = torch.zeros_like(n)
        self._device_volume_parts.append(torch.stack([volume * 1e6, n, torch.where(volume > 0, n, zero),
                                                      torch.where(status == 2, n, zero)], dim=1))

    def volume_sums(self):
        """[sum of the intersection volumes in cm^3, interacting samples kept, those of them with a voxel inside both hands, those of
        them the kernel called invalid] (float64, additive over batches and ranks): what :meth:`update_device_volume` left on the
        device.  Zeros for an Evaluator without ``volume_metric``."""
        sums = np.zeros(4, dtype=np.float64)
        self._add_device_sums(sums, "_device_volume_parts")
        return sums

    @staticmethod
    def volume_metrics_from_sums(s):
        """``pen_volume``: mean intersection volume [cm^3] over the interacting samples; ``pen_rate``: the share of them whose hands
        intersect at all.  NaN where no sample was counted."""
        return dict(pen_volume=_ratio(s[0], s[1]), pen_rate=_ratio(s[2], s[1]))

    def _interaction_on(self, what):
        if not getattr(self, "interaction_metrics", False):
            raise RuntimeError(f"{what} needs Evaluator(interaction_metrics=True)")

    def _use_mask(self, dev, *masks):
        """The conjunction of the given (B) bool masks as uint8 on ``dev``, None when none is given."""
        import torch
        use = None
        for mask in masks:
            if mask is not None:
                m = mask.to(dev, torch.bool)
                use = m if use is None else use & m
        return None if use is None else use.to(torch.uint8).contiguous()

    def update_device_mrrpe(self, pred_joints_3d, gt_joints_3d, keep=None, interacting=None, scale=None):
        """MRRPE of one batch from device tensors (``ihmr_eval_mrrpe``): pred_joints_3d (B,42,3), gt_joints_3d (B,42,4); ``keep``,
        ``interacting`` and ``scale`` as in :meth:`update_device`.  A sample counts when both wrist weights are > 0 and it is kept and
        interacting.  Accumulates lazily, see :meth:`interaction_sums`."""
        self._interaction_on("update_device_mrrpe")
        it = self._use_mask(pred_joints_3d.device, interacting)
        out, = self._launch("ihmr_eval_mrrpe", (pred_joints_3d, gt_joints_3d), scale, [(2,)], lambda i, sc, B, o: (*i, sc, it, B, *o))
        self._device_mrrpe_parts.append(self._kept(keep, out)[0])

    def update_device_contact(self, pred_right, pred_left, gt_right, gt_left, mano_params_weight, keep=None, interacting=None, scale=None):
        """Contact consistency of one batch from device tensors (``ihmr_eval_contact``): the four meshes (B,778,3) and
        ``mano_params_weight`` (B,2).  A sample counts when both hands are annotated (weight > 0) and it is kept and interacting
        (``keep``, ``interacting`` (B) bool, default all): the conjunction of the two masks is the kernel's ``use``, a row outside
        it does no pair work and leaves zeros.  Accumulates lazily, see :meth:`interaction_sums`."""
        import torch
        self._interaction_on("update_device_contact")
        dev, K = pred_right.device, len(self.contact_thresholds)
        thr = self._on_device("_contact_table_dev", dev, lambda d: torch.from_numpy(self.contact_thresholds).to(d))
        use = self._use_mask(dev, keep, interacting)
        pair, counts = self._launch("ihmr_eval_contact", (pred_right, pred_left, gt_right, gt_left, mano_params_weight), scale,
                                    [(2, 2), (2, K, 3)], lambda i, sc, B, o: (*i, sc, use, B, thr, K, o[0], o[1], None))
        w = mano_params_weight.to(dev)
        counted = (w[:, 0] > 0) & (w[:, 1] > 0)
        if use is not None:
            counted = counted & (use != 0)
        pair = pair[:, 0] + pair[:, 1]                                         # the two hands' rows: [sum of d_pred over C, |C|]
        has = counted & (pair[:, 1] > 0)
        zero, one = torch.zeros_like(pair[:, 0]), torch.ones_like(pair[:, 0])
        # the sample's deviation by a selection: 0 / 0 of a sample without contact pairs never enters a sum
        dev_b = torch.where(has, pair[:, 0] / torch.where(has, pair[:, 1], one), zero)
        rows = torch.stack([dev_b, torch.where(has, one, zero), torch.where(counted, one, zero)], dim=1)
        self._device_contact_parts.append((rows, counts[:, 0] + counts[:, 1]))

    def interaction_sums(self):
        """``[sum of e, n, sum of the per-sample contact deviations, samples with contact pairs, samples counted, (tp, pp, gp) per
        contact threshold]`` (float64, 5 + 3 K values, additive over batches and ranks): the records of an
        ``Evaluator(interaction_metrics=True)`` whose ``hand_type`` is 'interacting' plus what :meth:`update_device_mrrpe` /
        :meth:`update_device_contact` left on the device.  Zeros (K of the default table) for an Evaluator without the flag."""
        K = len(getattr(self, "contact_thresholds", CONTACT_THRESHOLDS))
        sums = np.zeros(5 + 3 * K, dtype=np.float64)
        inter = [p for p in self.pred_results if p["hand_type"] == "interacting"]
        e = [x for p in inter for x in p.get("mrrpe", [])]
        sums[0], sums[1] = float(np.sum(np.asarray(e, dtype=np.float64))), len(e)
        recs = [p for p in inter if "contact_pairs" in p]
        devs = [p["contact_pair_sum"] / p["contact_pairs"] for p in recs if p["contact_pairs"] > 0]
        sums[2], sums[3], sums[4] = float(np.sum(np.asarray(devs, dtype=np.float64))), len(devs), len(recs)
        for p in recs:
            sums[5:] += np.asarray(p["contact_counts"], np.float64).reshape(-1)
        self._add_device_sums(sums[:2], "_device_mrrpe_parts")
        self._add_device_sums(sums[2:5], "_device_contact_parts", 0)
        d = self._device_column_sums("_device_contact_parts", 1)
        if d is not None:
            sums[5:] += d.reshape(-1)
        return sums

    @staticmethod
    def interaction_metrics_from_sums(s, contact_thresholds=None):
        """``mrrpe``; ``contact_dev`` (mean of the per-sample deviations over the counted samples with contact pairs), ``contact_rate``
        (their share of the counted samples); ``contact_precision`` / ``contact_recall`` / ``contact_f1`` (K,), micro-averaged over the
        vertices of all counted samples: P = tp / pp, R = tp / gp, F1 = 2 P R / (P + R), 0 when P + R = 0.  NaN where a denominator
        count is 0.  The table is the one the sums were counted with (default: the Evaluator's default)."""
        thr = check_thresholds(CONTACT_THRESHOLDS if contact_thresholds is None else contact_thresholds, MAX_CONTACT_THRESHOLDS, "contact_thresholds")
        s = np.asarray(s, np.float64)
        assert len(s) == 5 + 3 * len(thr), (len(s), len(thr))
        c = s[5:].reshape(len(thr), 3)
        nan = float("nan")
        P = np.array([_ratio(tp, pp) for tp, pp, _ in c])
        R = np.array([_ratio(tp, gp) for tp, _, gp in c])
        den = P + R
        with np.errstate(all="ignore"):
            f1 = np.where(np.isnan(den), nan, np.where(den > 0, 2.0 * P * R / np.where(den > 0, den, 1.0), 0.0))
        return dict(mrrpe=_ratio(s[0], s[1]), contact_dev=_ratio(s[2], s[3]), contact_rate=_ratio(s[3], s[4]),
                    contact_precision=P, contact_recall=R, contact_f1=f1)

    def update_device_surface(self, pred_right, pred_left, gt_right=None, gt_left=None, mano_params_weight=None, scale=None, keep=None,
                              interacting=None):
        """Penetration depth and surface contact of one batch from device tensors (``ihmr_surface_distance`` through
        :func:`ihmr_amd.sdf.surface_distance`, ``Evaluator(surface_metrics=True)``): per mesh pair two calls, each hand's 778 vertices
        against the other hand's mesh with the wrist closed.  ``keep`` and ``interacting`` (B) bool, default all: their conjunction is
        the kernel's ``use``, a sample outside it does no work and counts nowhere.  ``scale`` (B), default 1: every distance is divided
        by it.  ``depth = max(0, -dist) / scale``; a sample leaves the maximum and the mean of its 1556 depths in millimetres and the
        number of its vertices with ``dist < 0``.  With the GT meshes and ``mano_params_weight`` (B,2), a sample whose two weights are > 0
        also leaves, per threshold, the vertices in contact (``dist / scale < tau``, strict; inside is contact) in both mesh pairs, in
        the prediction and in the ground truth.  Accumulates lazily, see :meth:`surface_sums`.  Device-only: the records,
        every other ``*_sums()`` and pickled files carry nothing of it."""
        import torch

        from . import hip, sdf
        if not getattr(self, "surface_metrics", False):
            raise RuntimeError("update_device_surface needs Evaluator(surface_metrics=True)")
        hip.require_gpu()
        assert self.right_hand_faces is not None and self.left_hand_faces is not None, "Evaluator needs the MANO models' faces"
        if (gt_right is None) != (gt_left is None) or (gt_right is not None and mano_params_weight is None):
            raise ValueError("the contact part needs gt_right, gt_left and mano_params_weight together")
        B, dev, K = pred_right.shape[0], pred_right.device, len(self.surface_thresholds)
        use = torch.ones(B, dtype=torch.bool, device=dev)
        for mask in (keep, interacting):
            if mask is not None:
                use = use & mask.to(dev, torch.bool)
        sc = torch.ones(B, dtype=torch.float64, device=dev) if scale is None else scale.detach().to(dev, torch.float32).to(torch.float64)

        def both_hands(right, left, rows):
            d_r = sdf.surface_distance(right.detach(), left.detach(), self.left_hand_faces, use=rows)[0]
            d_l = sdf.surface_distance(left.detach(), right.detach(), self.right_hand_faces, use=rows)[0]
            return torch.cat([d_r, d_l], dim=1)                                  # (B,1556): a row outside `rows` is zero

        zero = self._on_device("_zero_dev", dev, lambda d: torch.zeros((), dtype=torch.float64, device=d))
        dp = both_hands(pred_right, pred_left, use)
        depth = torch.where(dp < 0, -dp, zero) / sc[:, None]                    # a NaN distance (a NaN vertex) has depth 0
        n = use.to(torch.float64)
        inside = ((dp < 0) & use[:, None]).sum(dim=1).to(torch.float64)
        rows = [torch.where(use, depth.max(dim=1).values * 1000.0, zero), torch.where(use, depth.mean(dim=1) * 1000.0, zero), inside, n]
        counts = torch.zeros(B, K, 3, dtype=torch.float64, device=dev)
        with_gt = torch.zeros_like(n)
        if gt_right is not None:
            w = mano_params_weight.to(dev)
            counted = use & (w[:, 0] > 0) & (w[:, 1] > 0)
            dg = both_hands(gt_right, gt_left, counted)
            thr = self._on_device("_surface_table_dev", dev, lambda d: torch.from_numpy(self.surface_thresholds).to(d))
            live = counted[:, None, None]
            in_p = ((dp / sc[:, None])[:, None, :] < thr[None, :, None]) & live           # (B,K,1556)
            in_g = ((dg / sc[:, None])[:, None, :] < thr[None, :, None]) & live
            counts = torch.stack([(in_p & in_g).sum(dim=2), in_p.sum(dim=2), in_g.sum(dim=2)], dim=2).to(torch.float64)
            with_gt = counted.to(torch.float64)
        self._device_surface_parts.append((torch.stack(rows + [with_gt], dim=1), counts))

    def surface_sums(self):
        """``[sum of the per-sample maximum depths, sum of the per-sample mean depths (mm), vertices inside the other hand, samples
        counted, samples counted with GT meshes, (tp, pp, gp) per surface threshold]`` (float64, 5 + 3 K values, additive over batches
        and ranks): what :meth:`update_device_surface` left on the device.  Zeros (K of the default table) for an Evaluator without
        ``surface_metrics``."""
        K = len(getattr(self, "surface_thresholds", SURFACE_THRESHOLDS))
        sums = np.zeros(5 + 3 * K, dtype=np.float64)
        self._add_device_sums(sums[:5], "_device_surface_parts", 0)
        d = self._device_column_sums("_device_surface_parts", 1)
        if d is not None:
            sums[5:] += d.reshape(-1)
        return sums

    @staticmethod
    def surface_metrics_from_sums(s, surface_thresholds=None):
        """``pen_depth_max`` / ``pen_depth_ave``: the mean over the counted samples of the maximum / mean depth of the 1556 vertices
        under the other hand's surface [mm]; ``pen_vertex_rate``: the share of their vertices that lie inside the other hand;
        ``surface_contact_precision`` / ``surface_contact_recall`` / ``surface_contact_f1`` (K,), micro-averaged over the vertices of the
        samples counted with GT meshes exactly as ``contact_*``.  NaN where a denominator is 0."""
        thr = check_thresholds(SURFACE_THRESHOLDS if surface_thresholds is None else surface_thresholds, MAX_CONTACT_THRESHOLDS, "surface_thresholds")
        s = np.asarray(s, np.float64)
        assert len(s) == 5 + 3 * len(thr), (len(s), len(thr))
        c = s[5:].reshape(len(thr), 3)
        nan = float("nan")
        P = np.array([_ratio(tp, pp) for tp, pp, _ in c])
        R = np.array([_ratio(tp, gp) for tp, _, gp in c])
        den = P + R
        with np.errstate(all="ignore"):
            f1 = np.where(np.isnan(den), nan, np.where(den > 0, 2.0 * P * R / np.where(den > 0, den, 1.0), 0.0))
        return dict(pen_depth_max=_ratio(s[0], s[3]), pen_depth_ave=_ratio(s[1], s[3]), pen_vertex_rate=_ratio(s[2], 1556.0 * s[3]),
                    surface_contact_precision=P, surface_contact_recall=R, surface_contact_f1=f1)

    def gather_pred(self, pred_results):
        self.pred_results += pred_results

    VERT_KEYS = tuple(f"{mode}_{side}_hand_verts" for mode in ("pred", "gt") for side in ("left", "right"))

    def _meta(self, data_idx):
        dl = self.data_list
        if isinstance(dl, dict):
            return dl.get(data_idx, {})
        return dl[data_idx] if 0 <= data_idx < len(dl) else {}

    def update(self, data_idxs, pred_results, save_verts=True, hand_type="interacting", scale=1.0):
        """evaluator.py:38-97.  One record per sample: the exported arrays, the per-sample metadata with the reference's
        defaults (``annot_type`` 'machine', ``hand_type`` 'interacting', ``hand_type_valid`` 1, ``scale`` 1 -- the two
        keyword arguments override the latter defaults for data without a ``data_list``), with ``save_verts`` the meshes
        present in ``pred_results`` stored as **float16** (``:66-72``), the two joint metrics, and for ``do_flip`` samples
        the flip back to the original image (``:100-134``)."""
        self.save_verts = save_verts
        for i, data_idx in enumerate(np.asarray(data_idxs).tolist()):
            meta = self._meta(data_idx)
            rel = meta.get("img_path", f"synthetic/{data_idx:08d}.jpg")
            single = dict(
                data_idx=data_idx, pred_cam_params=pred_results["pred_cam_params"][i], pred_shape_params=pred_results["pred_shape_params"][i],
                pred_pose_params=pred_results["pred_pose_params"][i], pred_hand_trans=pred_results["pred_hand_trans"][i],
                pred_joints_3d=pred_results["pred_joints_3d"][i], collision_loss_origin_scale=pred_results["collision_loss_origin_scale"][i],
                gt_joints_3d=pred_results["gt_joints_3d"][i],
                img_path=rel if not self.image_root else self.image_root.rstrip("/") + "/" + rel, img_path_relative=rel)
            for key, default in (("annot_type", "machine"), ("hand_type", hand_type), ("hand_type_valid", 1.0), ("scale", scale)):
                single[key] = meta.get(key, default)
            if save_verts:
                for key in self.VERT_KEYS:
                    if key in pred_results:
                        single[key] = np.asarray(pred_results[key][i]).astype(np.float16)
            gt = single["gt_joints_3d"]
            single["j3d_error"] = get_single_joints_error(single["pred_joints_3d"], gt[:, :3], gt[:, 3:], single["scale"])
            single["pa_no_rot_inter_j3d_error"] = get_single_pa_inter_joints_error(
                single["pred_joints_3d"], gt[:, :3], gt[:, 3:], single["scale"])
            hands = list(self._counted_hands(pred_results, i))
            single["v3d_error"] = []
            for h, pv, gv in hands:                                                        # Baseline / MLP exports
                single["v3d_error"] += get_single_verts_error(pv, gv, self.root_weights[h], single["scale"])
            pa, curves = getattr(self, "pa_metrics", False), getattr(self, "curve_metrics", False)
            if curves and not pa:       # the key order of a record: the PA lists come first only where ``pa_metrics`` asks for them
                self._add_curve_joint_list(single)
            if pa or curves:            # the curve metrics count from the PA lists too, under the same keys
                p, sc = single["pred_joints_3d"], single["scale"]
                single["pa_inter_j3d_error"] = get_single_pa_error(p, gt[:, :3], gt[:, 3], sc)
                single["pa_j3d_error"] = get_single_pa_error(p[:21], gt[:21, :3], gt[:21, 3], sc) + get_single_pa_error(p[21:], gt[21:, :3], gt[21:, 3], sc)
                if self._exports_meshes(pred_results):
                    single["pa_v3d_error"] = []
                    for _, pv, gv in hands:
                        single["pa_v3d_error"] += get_single_pa_error(pv, gv, np.ones(len(pv)), sc)
            if curves and pa:
                self._add_curve_joint_list(single)
            if curves and self._exports_meshes(pred_results):
                self._add_nn_lists(single, hands)
            if getattr(self, "interaction_metrics", False):
                single["mrrpe"] = get_single_mrrpe(single["pred_joints_3d"], gt[:, :3], gt[:, 3], single["scale"])
                if all(k in pred_results for k in self.VERT_KEYS + ("mano_params_weight",)) and (np.asarray(pred_results["mano_params_weight"][i])[:2] > 0).all():
                    m = {k: pred_results[k][i] for k in self.VERT_KEYS}
                    s, n, counts, _ = get_single_contact(m["pred_right_hand_verts"], m["pred_left_hand_verts"], m["gt_right_hand_verts"],
                                                         m["gt_left_hand_verts"], single["scale"], self.contact_thresholds)
                    single["contact_pair_sum"], single["contact_pairs"], single["contact_counts"] = s, n, counts
            if "do_flip" in pred_results and pred_results["do_flip"][i]:
                self._flip_back_data(single)
            self.pred_results.append(single)

    NN_KEYS = ("nn_dist_raw_pg", "nn_dist_raw_gp", "nn_dist_pa_pg", "nn_dist_pa_gp")

    def _exports_meshes(self, pred_results):
        return "gt_right_hand_verts" in pred_results and self.root_weights is not None

    def _counted_hands(self, pred_results, i):
        """``(h, predicted mesh, GT mesh)`` of every hand of sample ``i`` that counts: GT meshes are exported and the hand's
        ``mano_params_weight`` is > 0."""
        if self._exports_meshes(pred_results):
            for h, side in enumerate(("right", "left")):
                if pred_results["mano_params_weight"][i][h] > 0:
                    yield h, pred_results[f"pred_{side}_hand_verts"][i], pred_results[f"gt_{side}_hand_verts"][i]

    @staticmethod
    def _add_curve_joint_list(single):
        """``curve_j3d_error``: the float64 form of ``j3d_error``, which keeps its dtype."""
        gt, p = single["gt_joints_3d"], single["pred_joints_3d"]
        single["curve_j3d_error"] = get_single_joints_error(np.asarray(p).astype(np.float64), np.asarray(gt[:, :3]).astype(np.float64),
                                                            gt[:, 3:], single["scale"])

    def _add_nn_lists(self, single, hands):
        """Per counted hand the four nearest-neighbour distance arrays (raw / aligned, p->g / g->p) the F-scores are counted from."""
        for key in self.NN_KEYS:
            single[key] = []
        for h, pv, gv in hands:
            for variant, aligned in (("raw", False), ("pa", True)):
                r = get_single_fscore_counts(pv, gv, self.root_weights[h], single["scale"], self.f_thresholds, aligned)
                if r is not None:
                    single[f"nn_dist_{variant}_pg"].append(r[1])
                    single[f"nn_dist_{variant}_gp"].append(r[2])

    def _flip_back_data(self, single):
        """evaluator.py:100-134: a sample that the loader mirrored (left-only image turned into a right hand) goes back to
        the original image -- camera x and translation x negated, the two hands' pose blocks swapped with the y / z
        axis-angle components negated, joint halves swapped with x negated, the two 778-halves of the per-vertex
        penetration depths swapped, and (with ``save_verts``) the stored meshes swapped and mirrored.  Acts in place on the
        record's arrays like the reference (which are rows of the exported batch arrays); the metrics were taken before."""
        single["pred_cam_params"][1] *= -1
        single["pred_hand_trans"][0] *= -1
        pose = single["pred_pose_params"].copy()
        single["pred_pose_params"][:48], single["pred_pose_params"][48:] = pose[48:], pose[:48]
        single["pred_pose_params"][1::3] *= -1
        single["pred_pose_params"][2::3] *= -1
        for key in ("pred_joints_3d", "gt_joints_3d"):
            j = single[key].copy()
            single[key][:21], single[key][21:] = j[21:], j[:21]
            single[key][:, 0] *= -1
        c = single["collision_loss_origin_scale"].copy()
        single["collision_loss_origin_scale"][:778], single["collision_loss_origin_scale"][778:] = c[778:], c[:778]
        if self.save_verts:
            # the reference indexes all four mesh keys here and raises KeyError when one is missing; this build swaps what
            # is stored (IHMR-OPT exports no GT meshes and never flips: do_flip is all zeros, optimize_model.py:433)
            saved = {k: single[k].copy() for k in self.VERT_KEYS if k in single}
            for key in saved:
                other = key.replace("left", "right") if "left" in key else key.replace("right", "left")
                if other in saved:
                    single[key] = saved[other]
                    single[key][:, 0] *= -1

    def remove_redunc(self):
        """evaluator.py:137-146: drop the padding duplicates (same image id)."""
        seen, out = set(), []
        for d in self.pred_results:
            if d["img_path_relative"] not in seen:
                out.append(d)
                seen.add(d["img_path_relative"])
        self.pred_results = out

    def metric_sums(self):
        """[sum mpjpe, n, sum inter, n, sum coll_ave, sum coll_max, n_interacting, sum mpvpe, n] (float64, additive over ranks)."""
        e = [x for p in self.pred_results for x in p["j3d_error"]]
        pa = [x for p in self.pred_results for x in p["pa_no_rot_inter_j3d_error"]]
        inter = [p for p in self.pred_results if p["hand_type"] == "interacting"]
        ca = [np.mean(p["collision_loss_origin_scale"].astype(np.float64)) * 1000 for p in inter]
        cm = [np.max(p["collision_loss_origin_scale"].astype(np.float64)) * 1000 for p in inter]
        f64 = lambda x: float(np.sum(np.asarray(x, dtype=np.float64)))
        ve = [x for p in self.pred_results for x in p.get("v3d_error", [])]
        sums = np.array([f64(e), len(e), f64(pa), len(pa), f64(ca), f64(cm), len(inter), f64(ve), len(ve)], dtype=np.float64)
        self._add_device_sums(sums[:7], "_device_parts")
        self._add_device_sums(sums[7:9], "_device_vert_parts")
        return sums

    def pa_metric_sums(self):
        """[sum PA error over all valid joints, n, sum per-hand PA error, n, sum PA vertex error, n] (float64, additive over ranks):
        the records of an ``Evaluator(pa_metrics=True)`` plus what :meth:`update_device_pa` / :meth:`update_device_pa_verts` left on
        the device."""
        f64 = lambda x: float(np.sum(np.asarray(x, dtype=np.float64)))
        cols = [[x for p in self.pred_results for x in p.get(k, [])] for k in ("pa_inter_j3d_error", "pa_j3d_error", "pa_v3d_error")]
        sums = np.array([v for c in cols for v in (f64(c), len(c))], dtype=np.float64)
        self._add_device_sums(sums[:4], "_device_pa_parts")
        self._add_device_sums(sums[4:6], "_device_pa_vert_parts")
        return sums

    def curve_sums(self):
        """One flat float64 vector, additive over batches and ranks.  With T = len(thresholds), F = len(f_thresholds) and the C = 50
        thresholds of :func:`calc_collision_auc`:

        * 5 blocks of T + 1, the populations ``j3d, pa_inter_j3d, pa_j3d, v3d, pa_v3d``: [#err <= tau_0 .. #err <= tau_{T-1}, n];
        * 2 blocks of F + 1, ``fscore_raw, fscore_pa``: [sum over the counted hands of the hand's F at tau_0 .. tau_{F-1}, hands];
        * 2 blocks of C + 1, the per-sample max and mean penetration depth [mm] of the interacting samples:
          [#x < tau_0 .. #x < tau_{C-1}, n].

        Everything is a count except the F sums: F is formed per hand from that hand's two counts, and the sum over hands is the
        correctly rounded one (``math.fsum``), so it does not depend on the order or the grouping of the hands.  Records of an
        ``Evaluator(curve_metrics=True)`` plus what :meth:`update_device_curves` / :meth:`update_device_curve_verts` left on the
        device and, with ``curve_metrics`` set, the collision columns of :meth:`update_device`."""
        import math
        thr, fthr = self.thresholds, self.f_thresholds
        T, F, nv = len(thr), len(fthr), 778.0
        recs = [p for p in self.pred_results if "curve_j3d_error" in p]
        blocks = []
        for name in CURVE_POPULATIONS:
            e = [x for p in recs for x in p.get("curve_j3d_error" if name == "j3d" else f"{name}_error", [])]
            blocks.append(np.concatenate([curve_counts(e, thr), [len(e)]]))
        fvals = {"raw": [], "pa": []}                      # per variant the per-hand F rows (F,)
        for variant in ("raw", "pa"):
            for p in recs:
                for d_pg, d_gp in zip(p.get(f"nn_dist_{variant}_pg", []), p.get(f"nn_dist_{variant}_gp", [])):
                    fvals[variant].append(fscore_from_counts(curve_counts(d_pg, fthr, strict=True), curve_counts(d_gp, fthr, strict=True), nv))
        hands = {v: float(len(fvals[v])) for v in fvals}
        inter = [p for p in recs if p["hand_type"] == "interacting"]
        cmax = [[np.max(p["collision_loss_origin_scale"].astype(np.float64)) * 1000 for p in inter]]
        cave = [[np.mean(p["collision_loss_origin_scale"].astype(np.float64)) * 1000 for p in inter]]
        n_inter = float(len(inter))
        d = self._device_column_sums("_device_curve_parts")
        if d is not None:
            blocks[:3] = [blocks[k] + d[k] for k in range(3)]
        d = self._device_column_sums("_device_curve_vert_parts", 0)
        if d is not None:            # the counts, then F per hand from the counts of the hands that were counted and kept
            blocks[3:5] = [blocks[3 + k] + d[k] for k in range(2)]
            counted = self._device_rows("_device_curve_vert_parts", 2).cpu().numpy().reshape(-1, 2)
            fc = self._device_rows("_device_curve_vert_parts", 1).cpu().numpy().reshape(len(counted), 2, 2, F)    # (hands, raw / pa, p->g / g->p, F)
            for k, variant in enumerate(("raw", "pa")):
                rows = fc[counted[:, k] > 0, k]
                fvals[variant] += list(fscore_from_counts(rows[:, 0], rows[:, 1], nv))
                hands[variant] += float(np.sum(counted[:, k] > 0))
        d = self._device_rows("_device_parts") if getattr(self, "curve_metrics", False) else None
        if d is not None:            # columns 4, 5: mean and max depth [mm]; 6: interacting and kept
            d = d[d[:, 6] > 0].cpu().numpy()
            cave.append(d[:, 4])
            cmax.append(d[:, 5])
            n_inter += float(len(d))
        for variant in ("raw", "pa"):
            rows = np.asarray(fvals[variant], np.float64).reshape(-1, F)
            blocks.append(np.array([math.fsum(rows[:, k]) for k in range(F)] + [hands[variant]]))
        for pop in (cmax, cave):
            blocks.append(np.concatenate([sum(curve_counts(x, COLLISION_AUC_THRESHOLDS, strict=True) for x in pop), [n_inter]]))
        return np.concatenate(blocks).astype(np.float64)

    @staticmethod
    def curve_metrics_from_sums(s, thresholds=None, f_thresholds=None):
        """From a (summed) :meth:`curve_sums` vector: ``pck_<name>`` (T,) and ``auc_<name>`` for the five populations, ``fscore_raw`` /
        ``fscore_pa`` (F,), ``collision_auc_max`` / ``collision_auc_ave``.  NaN where nothing was counted; an AUC over one threshold
        is NaN.  The tables are those the sums were counted with (default: the Evaluator's defaults)."""
        thr = check_thresholds(CURVE_THRESHOLDS if thresholds is None else thresholds, MAX_THRESHOLDS)
        fthr = check_thresholds(F_THRESHOLDS if f_thresholds is None else f_thresholds, MAX_F_THRESHOLDS, "f_thresholds", True)
        T, F, C = len(thr), len(fthr), len(COLLISION_AUC_THRESHOLDS)
        s = np.asarray(s, np.float64)
        assert len(s) == 5 * (T + 1) + 2 * (F + 1) + 2 * (C + 1), (len(s), T, F)
        nan = float("nan")
        out, at = {}, 0
        for name in CURVE_POPULATIONS:
            c, n = s[at:at + T], s[at + T]
            out[f"pck_{name}"] = c / n if n > 0 else np.full(T, nan)
            out[f"auc_{name}"] = curve_auc(c, n, thr)
            at += T + 1
        for name in ("fscore_raw", "fscore_pa"):
            out[name] = s[at:at + F] / s[at + F] if s[at + F] > 0 else np.full(F, nan)
            at += F + 1
        for name in ("collision_auc_max", "collision_auc_ave"):
            out[name] = curve_auc(s[at:at + C], s[at + C], COLLISION_AUC_THRESHOLDS)
            at += C + 1
        return out

    @staticmethod
    def pa_metrics_from_sums(s):
        """``pa_inter_mpjpe_3d`` (one alignment over all valid joints of both hands, the reference's ``use_rot=True`` call),
        ``pa_mpjpe_3d`` (one alignment per hand) and, where aligned vertex errors were counted, ``pa_mpvpe_3d``."""
        out = dict(pa_inter_mpjpe_3d=_ratio(s[0], s[1]), pa_mpjpe_3d=_ratio(s[2], s[3]))
        if s[5] > 0:
            out["pa_mpvpe_3d"] = _ratio(s[4], s[5])
        return out

    @staticmethod
    def metrics_from_sums(s):
        out = dict(mpjpe_3d=_ratio(s[0], s[1]), inter_mpjpe_3d=_ratio(s[2], s[3]), collision_ave=_ratio(s[4], s[6]), collision_max=_ratio(s[5], s[6]))
        if len(s) > 8 and s[8] > 0:        # only the models that export GT meshes (IHMR-Baseline / IHMR-MLP) have it
            out["mpvpe_3d"] = _ratio(s[7], s[8])
        return out

    def _metric_families(self):
        """The metric families this Evaluator reports, in the order of the packed vector -- base, PA, volume, curves, interaction, surface -- each as
        ``(its *_sums method, its *_from_sums method, the length of its sums)``."""
        families = [(self.metric_sums, self.metrics_from_sums, 9)]
        if getattr(self, "pa_metrics", False):
            families.append((self.pa_metric_sums, self.pa_metrics_from_sums, 6))
        if getattr(self, "volume_metric", False):
            families.append((self.volume_sums, self.volume_metrics_from_sums, 4))
        if getattr(self, "curve_metrics", False):
            T, F, C = len(self.thresholds), len(self.f_thresholds), len(COLLISION_AUC_THRESHOLDS)
            families.append((self.curve_sums, lambda s: self.curve_metrics_from_sums(s, self.thresholds, self.f_thresholds),
                             5 * (T + 1) + 2 * (F + 1) + 2 * (C + 1)))
        if getattr(self, "interaction_metrics", False):      # the last family: the slices of the others do not move
            families.append((self.interaction_sums, lambda s: self.interaction_metrics_from_sums(s, self.contact_thresholds),
                             5 + 3 * len(self.contact_thresholds)))
        if getattr(self, "surface_metrics", False):          # appended after the interaction family: no existing slice moves
            families.append((self.surface_sums, lambda s: self.surface_metrics_from_sums(s, self.surface_thresholds),
                             5 + 3 * len(self.surface_thresholds)))
        return families

    def packed_sums(self):
        """The sums of every family in one float64 vector: what one all-reduce carries (:func:`ihmr_amd.dist.reduce_metrics`)."""
        parts = [sums() for sums, _, _ in self._metric_families()]
        assert [len(p) for p in parts] == [n for _, _, n in self._metric_families()]
        return np.concatenate(parts)

    def metrics_from_packed(self, s):
        """The metrics dict of a (reduced) :meth:`packed_sums` vector: every family's ``*_from_sums`` of its slice."""
        families = self._metric_families()
        assert len(s) == sum(n for _, _, n in families), (len(s), [n for _, _, n in families])
        out, at = {}, 0
        for _, from_sums, n in families:
            out.update(from_sums(s[at:at + n]))
            at += n
        return out

    @property
    def mpjpe_3d(self): return self.metrics_from_sums(self.metric_sums())["mpjpe_3d"]
    @property
    def inter_mpjpe_3d(self): return self.metrics_from_sums(self.metric_sums())["inter_mpjpe_3d"]
    @property
    def collision_ave(self): return self.metrics_from_sums(self.metric_sums())["collision_ave"]
    @property
    def collision_max(self): return self.metrics_from_sums(self.metric_sums())["collision_max"]
    @property
    def mpvpe_3d(self): return self.metrics_from_sums(self.metric_sums()).get("mpvpe_3d", float("nan"))
    @property
    def pa_inter_mpjpe_3d(self): return self.pa_metrics_from_sums(self.pa_metric_sums())["pa_inter_mpjpe_3d"]
    @property
    def pa_mpjpe_3d(self): return self.pa_metrics_from_sums(self.pa_metric_sums())["pa_mpjpe_3d"]
    @property
    def pa_mpvpe_3d(self): return self.pa_metrics_from_sums(self.pa_metric_sums()).get("pa_mpvpe_3d", float("nan"))

    # ------------------------------------------------------------------------------------------ visualisation (evaluator.py:184-275)
    def _build_dirs(self, res_dir):
        """evaluator.py:184-190: ``img_name`` = the last four components of ``img_path`` (the last two joined by ``_``)."""
        for pred in self.pred_results:
            record = pred["img_path"].split("/")
            pred["img_name"] = osp.join(*(record[-4:-2] + ["_".join(record[-2:])]))
            os.makedirs(osp.dirname(osp.join(res_dir, pred["img_name"])) or ".", exist_ok=True)

    def visualize_result(self, res_vis_dir, res_obj_dir, size_type="double", batch_size=64, image_loader=None, views=(),
                         collision_map=False, collision_range=(0.0, 0.005)):
        """evaluator.py:231-275 for every stored record: the image padded and resized to ``final_size`` (``size_type`` 'double' =
        2 x inputSize, 'normalized' = inputSize, 'origin' = the image's longer side, which the resize kernel needs to be a multiple
        of 4), both hands rendered over it for an interacting sample (right ``light_green``, left ``light_blue``) and the one hand of
        ``hand_type`` otherwise, image stacked over render and written to ``<res_vis_dir>/<img_name>`` as .jpg, the mesh to
        ``<res_obj_dir>/<img_name>.obj``.  ``image_loader(path) -> (H,W,3) uint8 BGR`` replaces the PIL loader.  The reference forks
        16 processes of OpenDR; here the records go through the device in batches of ``batch_size``: one resize launch and one render
        per batch and image size.

        ``views``: ``(axis, deg)`` pairs or (3,3) matrices; one more panel per view, the hands turned about the middle of their
        bounding box and drawn on white (``MeshRenderer.render_views``), is stacked under image and render.  ``collision_map``:
        the hands of an interacting sample are painted from the record's ``collision_loss_origin_scale`` (``render.penetration_colors``:
        the hand's colour at ``collision_range[0]`` metres of penetration or less, red from ``collision_range[1]`` on), in the
        camera's view and in every other; a flipped record's table was swapped back with its hands (``_flip_back_data``).  With
        the defaults the files are what they are without these arguments."""
        import torch

        from . import hip, render, ry_utils
        from .preprocess import DataProcessor
        hip.require_gpu()
        assert size_type in ("origin", "double", "normalized")
        assert self.right_hand_faces is not None and self.left_hand_faces is not None, "Evaluator needs the MANO models' faces"
        loader = image_loader or load_image_bgr
        self._build_dirs(res_vis_dir)
        self._build_dirs(res_obj_dir)
        faces = {"right": np.asarray(self.right_hand_faces).astype(np.int64), "left": np.asarray(self.left_hand_faces).astype(np.int64)}
        nv = hip.NUM_VERTS
        renderer = render.MeshRenderer(faces["right"], faces["left"], nv, nv)
        two = np.array([render.COLORS["light_green"], render.COLORS["light_blue"]], np.float32)
        one = np.array([render.SINGLE_HAND_COLOR, render.SINGLE_HAND_COLOR], np.float32)
        views = list(views)
        for start in range(0, len(self.pred_results), batch_size):
            chunk = self.pred_results[start:start + batch_size]
            images = [loader(r["img_path"]) for r in chunk]
            sizes = [int(np.max(im.shape[:2])) if size_type == "origin" else self.inputSize * (2 if size_type == "double" else 1) for im in images]
            for S in sorted(set(sizes)):
                rows = [i for i, s in enumerate(sizes) if s == S]
                img = DataProcessor(final_size=S)([images[i] for i in rows], return_uint8=True)["img_uint8"]
                zeros = np.zeros((nv, 3), np.float32)
                hand = lambda r, side: np.asarray(r.get(f"pred_{side}_hand_verts", zeros), np.float32)
                recs = [chunk[i] for i in rows]
                inter = [r["hand_type"] == "interacting" for r in recs]
                present = np.array([[1, 1] if it else [r["hand_type"] == "right", r["hand_type"] == "left"] for r, it in zip(recs, inter)], np.uint8)
                colors = np.stack([two if it else one for it in inter])
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                scene = (up(np.stack([hand(r, "right") for r in recs])), up(np.stack([hand(r, "left") for r in recs])),
                         up(np.stack([np.asarray(r["pred_cam_params"], np.float32)[:3] for r in recs])))
                if not views and not collision_map:
                    out = renderer.render(*scene, img, present=up(present), colors=up(colors))
                else:
                    paint = None
                    if collision_map:
                        no_depth = np.zeros(2 * nv, np.float32)            # a depth of zero is the hand's own colour
                        depth = np.stack([np.asarray(r["collision_loss_origin_scale"], np.float32).reshape(2 * nv) if it else no_depth
                                          for r, it in zip(recs, inter)])
                        paint = render.penetration_colors(up(depth), up(colors), lo=collision_range[0], hi=collision_range[1])
                    panels = renderer.render_views(*scene, [None] + views, img, present=up(present), colors=up(colors), vertex_colors=paint)
                    out = panels.reshape(len(recs), (1 + len(views)) * S, S, 3)    # the camera's view, then one panel per view
                res = torch.cat([img, out], dim=1).cpu().numpy()               # image over render (evaluator.py:250)
                for k, r in enumerate(recs):
                    if inter[k]:                                               # evaluator.py:206-221
                        verts = np.concatenate((r["pred_right_hand_verts"], r["pred_left_hand_verts"]), axis=0)
                        f = np.concatenate((faces["right"], faces["left"] + r["pred_right_hand_verts"].shape[0]), axis=0)
                    else:                                                      # evaluator.py:223-229
                        verts, f = r[f"pred_{r['hand_type']}_hand_verts"], faces[r["hand_type"]]
                    write_image_bgr(osp.join(res_vis_dir, r["img_name"]).replace(".png", ".jpg"), res[k])
                    ry_utils.save_mesh_to_obj(osp.join(res_obj_dir, r["img_name"])[:-4] + ".obj", verts, f)


def parse_views(text):
    """``"y:90,x:-90"`` -> ``[("y", 90.0), ("x", -90.0)]`` (the ``--views`` option)."""
    out = []
    for item in filter(None, (t.strip() for t in text.split(","))):
        axis, sep, deg = item.partition(":")
        if not sep or axis not in ("x", "y", "z"):
            raise ValueError(f"a view is axis:degrees with axis x, y or z, not {item!r}")
        out.append((axis, float(deg)))
    return out


def main():
    """evaluator.py:278-291: ``python -m ihmr_amd.evaluator METHOD DATASET [--views y:90,x:-90] [--collision_map]`` visualises
    ``evaluate_results/METHOD/DATASET.pkl``; ``--views`` adds one panel per ``axis:degrees`` entry, ``--collision_map`` paints the
    interacting hands by their per-vertex penetration depth."""
    import argparse
    import shutil

    from . import ry_utils
    ap = argparse.ArgumentParser(prog="python -m ihmr_amd.evaluator")
    ap.add_argument("method")
    ap.add_argument("dataset")
    ap.add_argument("--views", default="", help="comma-separated axis:degrees entries, e.g. y:90,x:-90")
    ap.add_argument("--collision_map", action="store_true")
    args = ap.parse_args()
    method, dataset = args.method, args.dataset
    views = parse_views(args.views)
    pkl_path = osp.join("evaluate_results", method, f"{dataset}.pkl")
    assert osp.exists(pkl_path)
    evaluator = ry_utils.load_pkl(pkl_path)
    res_vis_dir = osp.join("evaluate_results", method, dataset, "images")
    res_obj_dir = osp.join("evaluate_results", method, dataset, "objs")
    for d in (res_vis_dir, res_obj_dir):                                       # ry_utils.renew_dir
        if osp.isdir(d):
            shutil.rmtree(d)
        os.makedirs(d)
    evaluator.visualize_result(res_vis_dir, res_obj_dir, views=views, collision_map=args.collision_map)


if __name__ == "__main__":
    main()

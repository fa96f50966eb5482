"""The Procrustes-aligned metrics stated in float64 numpy with the points in ROWS, the seeded case tables of the CPU and GPU tests and
the conditioning figure of a case.

Statement (utils/metric_utils.py:59-104 read with points in rows): x1 = p - mean p, x2 = g - mean g, K = x1^T x2 (3 x 3), K = U S V^T,
R = V diag(1, 1, d) U^T with d = sign det(U V^T), scale = trace(R K) / sum |x1|^2, aligned = scale * R p + (mean g - scale * R mean p).
Set rules: a point is valid when its weight is > 0; a set is left out when the sum of its weights is < 2.0 or when all its valid
predicted points coincide (var1 == 0).

Conditioning: the rotation is determined up to eps / g with g = (s2 + d * s3) / s1 of K's singular values, so every case with three or
more valid points has g >= GAP_MIN (checked by tests/test_pa_metrics_cpu.py on every set of every case): float64 results are then good
to ~1e-14 m, far inside the 1e-9 m bar.  Two valid points are mapped onto their targets exactly and are exempt.
"""
import numpy as np

GAP_MIN = 1e-2
MIN_WEIGHT_SUM = 2.0
JOINT_SETS = ((0, 42), (0, 21), (21, 42))      # all joints, right hand, left hand


def procrustes_rows(S1, S2):
    """Aligned copy of S1 (n,3) onto S2 (n,3), float64, points in rows."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    m1, m2 = S1.mean(axis=0), S2.mean(axis=0)
    X1, X2 = S1 - m1, S2 - m2
    K = X1.T @ X2
    U, s, Vh = np.linalg.svd(K)
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
    R = Vh.T @ Z @ U.T                       # maps x1 onto x2
    scale = np.trace(R @ K) / np.sum(X1 ** 2)
    return scale * (S1 @ R.T) + (m2 - scale * (R @ m1))


def gap(S1, S2):
    """g = (s2 + d * s3) / s1 of the centred covariance."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    K = (S1 - S1.mean(axis=0)).T @ (S2 - S2.mean(axis=0))
    U, s, Vh = np.linalg.svd(K)
    return float((s[1] + np.sign(np.linalg.det(U @ Vh)) * s[2]) / s[0])


def set_errors(pred, gt, weights, scale=1.0):
    """Per-point aligned errors (n,) of one set, 0 at invalid points; None when the set is left out."""
    pred, gt, w = np.asarray(pred, np.float64), np.asarray(gt, np.float64), np.asarray(weights, np.float64)
    valid = w > 0
    if np.sum(w) < MIN_WEIGHT_SUM or not valid.any():
        return None
    p, g = pred[valid], gt[valid]
    if np.sum((p - p.mean(axis=0)) ** 2) == 0.0:
        return None
    err = np.zeros(len(w))
    err[valid] = np.linalg.norm(procrustes_rows(p, g) - g, axis=1) / float(scale)
    return err


def joints_statement(pred, gt, scale=1.0):
    """One sample: pred (42,3), gt (42,4) -> out (3,2) [sum, count], point_err (3,42)."""
    out, pe = np.zeros((3, 2)), np.zeros((3, 42))
    for s, (lo, hi) in enumerate(JOINT_SETS):
        e = set_errors(pred[lo:hi], gt[lo:hi, :3], gt[lo:hi, 3], scale)
        if e is not None:
            pe[s, lo:hi] = e
            out[s] = [e.sum(), float(np.sum(gt[lo:hi, 3] > 0))]
    return out, pe


def verts_statement(pred, gt, weight, scale=1.0):
    """One hand: pred, gt (778,3) -> out (2,) [sum, count], point_err (778,)."""
    e = set_errors(pred, gt, np.ones(len(pred)), scale) if weight > 0 else None
    if e is None:
        return np.zeros(2), np.zeros(len(pred))
    return np.array([e.sum(), float(len(pred))]), e


def _rotation(rng, angle=None):
    axis = rng.randn(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0.3, 2.5) if angle is None else angle
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def _cloud(rng, n):
    """A hand-sized point set [m] with three clearly different extents, so the singular values of a covariance stay apart."""
    return rng.randn(n, 3) * np.array([0.06, 0.035, 0.015])


def joint_cases():
    """name -> (pred (42,3) float32, gt (42,4) float32, scale_ratio)."""
    rng = np.random.RandomState(20240)
    cases = {}

    def add(name, weights=None, transform=None, noise=0.006, scale_ratio=1.0, pred=None):
        g = np.concatenate([_cloud(rng, 21) + [0.08, 0, 0], _cloud(rng, 21) - [0.08, 0, 0]])
        R, s, t = transform if transform is not None else (_rotation(rng), rng.uniform(0.8, 1.25), rng.randn(3) * 0.05)
        p = s * (g @ R.T) + t + rng.randn(42, 3) * noise if pred is None else pred(g)
        w = np.ones(42) if weights is None else np.asarray(weights, np.float64)
        cases[name] = (p.astype(np.float32), np.concatenate([g, w[:, None]], axis=1).astype(np.float32), float(scale_ratio))

    only = lambda *idx: np.isin(np.arange(42), idx).astype(np.float64)
    add("all_42")
    add("right_hand_only_21", weights=(np.arange(42) < 21))
    add("missing_wrist_41", weights=(np.arange(42) != 0))
    add("four_valid", weights=only(1, 8, 20, 33))
    add("three_valid", weights=only(0, 5, 30))
    add("two_valid", weights=only(3, 25))
    add("one_valid", weights=only(7))
    add("none_valid", weights=np.zeros(42))
    add("weight_sum_1p5", weights=only(2, 4, 6, 9, 11) * 0.3)
    add("fractional_weights", weights=np.where(np.arange(42) % 3 == 0, 0.0, 0.25 + 0.05 * (np.arange(42) % 5)))
    add("mirrored", pred=lambda g: g * np.array([-1.0, 1.0, 1.0]) + rng.randn(42, 3) * 0.002)
    add("exact_similarity", transform=(_rotation(rng), 1.3, np.array([0.2, -0.1, 0.4])), noise=0.0)
    add("rotation_near_pi", transform=(_rotation(rng, np.pi - 5e-5), 1.0, np.zeros(3)), noise=0.002)
    add("scale_half", transform=(_rotation(rng), 0.5, rng.randn(3) * 0.05))
    add("scale_two", transform=(_rotation(rng), 2.0, rng.randn(3) * 0.05))
    add("translated_metres", transform=(_rotation(rng), 1.0, np.array([3.0, -2.0, 5.0])))
    add("scale_ratio_1p7", scale_ratio=1.7)
    add("coincident_prediction", pred=lambda g: np.tile(np.array([[0.1, 0.2, 0.3]]), (42, 1)))
    return cases


def joint_batch():
    """The case table as one batch: names, pred (B,42,3), gt (B,42,4), scale (B), all float32."""
    c = joint_cases()
    names = list(c)
    return (names, np.stack([c[n][0] for n in names]), np.stack([c[n][1] for n in names]),
            np.array([c[n][2] for n in names], np.float32))


def vert_batch():
    """names, pred (B,2,778,3), gt (B,2,778,3) [right, left], mano_params_weight (B,2), scale (B): float32."""
    rng = np.random.RandomState(778)
    names, P, G, W, S = [], [], [], [], []

    def add(name, weight=(1.0, 1.0), mirror=False, noise=0.004, scale=1.0):
        g = np.stack([_cloud(rng, 778), _cloud(rng, 778)])
        p = np.stack([rng.uniform(0.7, 1.4) * (g[h] @ _rotation(rng).T) + rng.randn(3) * 0.1 + rng.randn(778, 3) * noise for h in range(2)])
        if mirror:
            p = g * np.array([1.0, -1.0, 1.0]) + rng.randn(2, 778, 3) * 0.001
        names.append(name); P.append(p); G.append(g); W.append(weight); S.append(scale)

    add("both_hands")
    add("left_without_annotation", weight=(1.0, 0.0), scale=1.4)
    add("right_without_annotation", weight=(0.0, 0.5))
    add("mirrored_mesh", mirror=True)
    add("exact_similarity", noise=0.0)
    return names, np.float32(P), np.float32(G), np.float32(W), np.float32(S)

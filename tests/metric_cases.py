"""The five headline metrics (MPJPE, the aligned "inter" MPJPE, collision_ave, collision_max, MPVPE) stated in float64 numpy for ONE
sample, the seeded case classes of the CPU and GPU tests, and the bar a float32 implementation is held to.  Imports no GPU and nothing
of ``ihmr_amd``.

Statement (utils/metric_utils.py:23-38, 107-143 and utils/evaluator.py:149-181 of the reference, read literally):

* joint error: for root in (0, 21): when the root's weight is > 0, the root's row is subtracted from ALL rows of both copies (the second
  subtraction acts on the already shifted copies), then every joint root .. root + 20 of weight > 0 gives ``|a - b| / scale``;
* aligned error: nothing when the SUM of the 42 weights is < 2.0; otherwise over the joints of weight > 0, per axis
  ``(p - mean p) / std p * std g + mean g`` (population std), then ``|. - g| / scale``.  Where an axis of the selected predictions has no
  spread the division is 0 / 0: every selected joint's error is NaN, and the sample still counts its joints;
* depths: ``mean x 1000`` and ``np.max x 1000`` of the 1556 values in float64 (NaN propagates through both); 0 and not counted unless
  the sample is interacting;
* vertex error of one hand (this build's definition, the joint error's convention): both meshes relative to their own root
  ``root_w . mesh``, ``|p - g| / scale`` per vertex; the hand counts when its weight is > 0.

``mutate`` switches ONE rule to a plausible wrong one; tests/test_metric_cases_cpu.py uses it to show that the cases can tell.

Bar.  The reference is this statement; the yardstick is the float32 route of the reference's own arithmetic (the host functions of
``ihmr_amd/evaluator.py`` on the float32 arrays).  Per case class D = the largest |float32 route - statement| of one point's error over
the class; a device sum over n counted points may be off by ``n * (3 * D + ulp32(largest |coordinate| of the sample) / scale)``.  3 and
not 1.5 (tests/test_gpu_adam.py): a butterfly sum and numpy's running sum round differently, so a per-case 1.5 is not owed.

Weights are dyadic (their float32 and float64 sums agree exactly: the 2.0 threshold is no rounding question), and so is every constant
coordinate of the ``flat`` class: the float32 mean of n equal values c is c only when n * c is representable, otherwise the reference's
own float32 route leaves the 0 / 0 to rounding and there is nothing to pin.
"""
import numpy as np

NV = 778
ND = 2 * NV                      # 1556 per-vertex penetration depths
MIN_WEIGHT_SUM = 2.0
DEPTH_POSITIONS = (0, 19, 20, 63, 64, 777, 778, 1535, 1536, 1555)     # lane 19 / 20: 25 / 24 rounds of a 64-stride loop; 1536 = 24 * 64
MUTATIONS = ("count_rule", "scale_ignored_joint", "scale_ignored_aligned", "scale_ignored_verts", "left_from_right_root",
             "invalid_in_alignment", "depth_mean_778", "depth_max_1536", "interacting_ignored", "weight_ge_0", "verts_no_root")


# ------------------------------------------------------------------------------------------------------------------ statement
def joint_errors(pred, gt, scale=1.0, mutate=None):
    """The per-joint errors (a list, in joint order) of one sample: pred (42,3), gt (42,4)."""
    a, b, w = np.array(pred, np.float64), np.array(gt, np.float64)[:, :3], np.asarray(gt, np.float64)[:, 3]
    sc = 1.0 if mutate == "scale_ignored_joint" else float(scale)
    ok = (lambda x: x >= 0) if mutate == "weight_ge_0" else (lambda x: x > 0)
    out = []
    for root in (0, 21):
        if ok(w[root]):
            if not (mutate == "left_from_right_root" and root == 21):
                a, b = a - a[root], b - b[root]
            out += [float(np.sqrt(np.sum((a[j] - b[j]) ** 2)) / sc) for j in range(root, root + 21) if ok(w[j])]
    return out


def aligned_errors(pred, gt, scale=1.0, mutate=None):
    """The aligned errors of one sample: None when the sample is left out, else an array over the selected joints (NaN at 0 / 0)."""
    p, g, w = np.asarray(pred, np.float64), np.asarray(gt, np.float64)[:, :3], np.asarray(gt, np.float64)[:, 3]
    sel = w >= 0 if mutate == "weight_ge_0" else w > 0
    if (np.sum(sel) < 2 if mutate == "count_rule" else np.sum(w) < MIN_WEIGHT_SUM):
        return None
    stat = np.ones(42, bool) if mutate == "invalid_in_alignment" else sel
    sc = 1.0 if mutate == "scale_ignored_aligned" else float(scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        m1, m2 = p[stat].mean(axis=0), g[stat].mean(axis=0)
        s1, s2 = np.sqrt(np.mean((p[stat] - m1) ** 2, axis=0)), np.sqrt(np.mean((g[stat] - m2) ** 2, axis=0))
        moved = (p[sel] - m1) / s1 * s2 + m2
        return np.sqrt(np.sum((moved - g[sel]) ** 2, axis=1)) / sc


def depth_stats(coll, interacting=True, mutate=None):
    """[mean depth, max depth] in mm of the 1556 float32 values; zeros unless interacting."""
    if not interacting and mutate != "interacting_ignored":
        return np.zeros(2)
    x = np.asarray(coll, np.float32).astype(np.float64).reshape(ND)
    mean = np.mean(x[:NV]) if mutate == "depth_mean_778" else np.mean(x)
    return np.array([mean * 1000.0, np.max(x[:1536] if mutate == "depth_max_1536" else x) * 1000.0])


def joints_statement(pred, gt, coll, interacting=True, scale=1.0, mutate=None):
    """One sample -> (6,): [sum err, n, sum aligned err, n_aligned, depth mean [mm], depth max [mm]]."""
    e = joint_errors(pred, gt, scale, mutate)
    a = aligned_errors(pred, gt, scale, mutate)
    a = np.zeros(0) if a is None else a
    return np.concatenate([[np.sum(np.asarray(e, np.float64)), len(e), np.sum(a), len(a)], depth_stats(coll, interacting, mutate)])


def vert_errors(pred, gt, root_w, scale=1.0, mutate=None):
    """The 778 per-vertex errors of one hand."""
    P, G, rw = np.asarray(pred, np.float64), np.asarray(gt, np.float64), np.asarray(root_w, np.float64)
    if mutate != "verts_no_root":
        P, G = P - rw @ P, G - rw @ G
    return np.sqrt(np.sum((P - G) ** 2, axis=1)) / (1.0 if mutate == "scale_ignored_verts" else float(scale))


def verts_statement(pred, gt, root_w, weight, scale=1.0, mutate=None):
    """One hand: pred, gt (778,3), root_w (778,) -> (2,) [sum, n]; zeros when the hand does not count."""
    if not weight > 0:
        return np.zeros(2)
    return np.array([np.sum(vert_errors(pred, gt, root_w, scale, mutate)), float(NV)])


# ------------------------------------------------------------------------------------------------------------------ the bar
def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def point_allowance(coords, scale):
    """One float32 ulp of the largest |coordinate| among ``coords`` (arrays), divided by the scale."""
    return ulp32(max(float(np.max(np.abs(np.asarray(c, np.float64)))) for c in coords)) / float(scale)


def sum_bar(n, class_max, allowance):
    """What a float32 sum over ``n`` counted points may be off by."""
    return n * (3.0 * class_max + allowance)


def _dist(e32, e64):
    """max |e32 - e64| over the finite entries; lengths and NaN positions must agree."""
    e32, e64 = np.asarray(e32, np.float64).reshape(-1), np.asarray(e64, np.float64).reshape(-1)
    assert e32.shape == e64.shape and np.array_equal(np.isnan(e32), np.isnan(e64)), (e32, e64)
    fin = ~np.isnan(e64)
    return float(np.max(np.abs(e32[fin] - e64[fin]))) if fin.any() else 0.0


def joint_class_maxima(classes, joints_fn, aligned_fn):
    """class -> (D joint, D aligned): the float32 route (``joints_fn(pred, gt3, w (42,1), scale)`` and ``aligned_fn`` of the same
    signature, lists out) against the statement, per point, the largest over the class."""
    out = {}
    for name, samples in classes.items():
        dj = da = 0.0
        for s in samples:
            sc = float(s["scale"])
            dj = max(dj, _dist(joints_fn(s["pred"], s["gt"][:, :3], s["gt"][:, 3:], sc), joint_errors(s["pred"], s["gt"], sc)))
            a = aligned_errors(s["pred"], s["gt"], sc)
            with np.errstate(invalid="ignore", divide="ignore"):
                da = max(da, _dist(aligned_fn(s["pred"], s["gt"][:, :3], s["gt"][:, 3:], sc), [] if a is None else a))
        out[name] = (dj, da)
    return out


def mesh_class_maxima(classes, root_w, verts_fn):
    """class -> D: ``verts_fn(pred, gt, root_w, scale)`` (list out) on the float32 arrays against the statement, per vertex."""
    return {name: max(_dist(verts_fn(s["pred"][h], s["gt"][h], root_w[h], float(s["scale"])),
                            vert_errors(s["pred"][h], s["gt"][h], root_w[h], float(s["scale"])))
                      for s in samples for h in range(2)) for name, samples in classes.items()}


# ------------------------------------------------------------------------------------------------------------------ joint cases
def _depths(rng):
    """A sparse table like a real sample's: most vertices outside the other hand."""
    return (np.abs(rng.randn(ND)) * 1e-3 * (rng.rand(ND) > 0.7)).astype(np.float32)


def _only(*idx, value=1.0):
    w = np.zeros(42)
    w[list(idx)] = value
    return w


def joint_classes():
    """class -> list of samples; a sample is a dict: pred (42,3), gt (42,4), coll (1556,) float32, interacting bool, scale float32,
    name.  Joint spread ~0.05 m, pred-to-gt noise ~0.01 m."""
    rng = np.random.RandomState(20260)
    classes = {}

    def add(cls, name, weights=None, offset=0.0, scale=1.0, interacting=True, coll=None, edit=None):
        p = rng.randn(42, 3) * 0.05
        g = p + rng.randn(42, 3) * 0.01
        p, g = np.float32(p + offset), np.float32(g + offset)
        if edit is not None:
            edit(p, g)
        w = np.ones(42) if weights is None else np.asarray(weights, np.float64)
        assert np.array_equal(np.float32(w), w)
        classes.setdefault(cls, []).append(dict(
            name=f"{cls}/{name}", pred=p, gt=np.concatenate([g, np.float32(w)[:, None]], axis=1),
            coll=_depths(rng) if coll is None else np.asarray(coll, np.float32), interacting=bool(interacting), scale=np.float32(scale)))

    for k in range(4):
        add("plain", str(k))
    for k in range(3):
        add("offset_0p5", str(k), offset=0.5)
        add("offset_2", str(k), offset=2.0)
    for sc in (0.25, 1.7, 1000.0):
        add("scaled", f"{sc:g}", scale=sc)
    add("scaled", "1.7_masked", scale=1.7, weights=(np.arange(42) % 4 != 1))

    j = np.arange(42)
    add("missing", "masks_inside_a_hand", weights=~np.isin(j, (5, 6, 7, 8, 30, 41)))
    add("missing", "right_root", weights=(j != 0))
    add("missing", "left_root", weights=(j != 21))
    add("missing", "both_roots", weights=~np.isin(j, (0, 21)))
    add("missing", "left_hand", weights=(j < 21))
    add("missing", "right_hand", weights=(j >= 21))
    add("missing", "single_joint", weights=_only(7))
    add("missing", "single_root", weights=_only(21))
    add("missing", "none", weights=np.zeros(42))

    add("fractional", "half_x3_sum_1p5", weights=_only(0, 5, 30, value=0.5))            # left out; a count rule keeps three
    add("fractional", "half_x4_sum_2", weights=_only(0, 5, 21, 30, value=0.5))          # exactly 2.0: kept
    add("fractional", "one_joint_of_2", weights=_only(0, value=2.0))                    # kept, one point: no spread, NaN
    add("fractional", "one_joint_of_2_no_root", weights=_only(33, value=2.0))
    add("fractional", "quarter_and_three", weights=np.where(j % 3 == 0, 3.0, 0.25))
    add("fractional", "quarter_x7_sum_1p75", weights=_only(0, 1, 2, 21, 22, 23, 24, value=0.25))
    w = _only(0, 4, 25)
    w[12] = -1.5
    add("fractional", "negative_pulls_sum_to_1p5", weights=w)                          # three joints of weight > 0, sum 1.5: left out
    w = np.ones(42)
    w[21], w[9] = -1.0, -0.25
    add("fractional", "negative_root", weights=w)                                      # the left hand has no root; sum 38.75

    def const(which, axis, value, rows):
        def edit(p, g):
            (p if which == "pred" else g)[rows, axis] = np.float32(value)
        return edit

    add("flat", "pred_two_joints_x", weights=_only(3, 25), edit=const("pred", 0, 0.046875, [3, 25]))
    add("flat", "pred_three_joints_z", weights=_only(0, 5, 30), edit=const("pred", 2, -0.09375, [0, 5, 30]))
    add("flat", "pred_all_joints_y", edit=const("pred", 1, 0.046875, slice(None)))
    add("flat", "pred_three_joints_z_offset", weights=_only(0, 5, 30), offset=2.0, edit=const("pred", 2, 2.125, [0, 5, 30]))
    add("flat", "gt_two_joints_x", weights=_only(3, 25), edit=const("gt", 0, 0.046875, [3, 25]))
    add("flat", "gt_three_joints_z", weights=_only(0, 5, 30), edit=const("gt", 2, -0.09375, [0, 5, 30]))
    add("flat", "gt_all_joints_y", edit=const("gt", 1, 0.046875, slice(None)))

    dense = (np.abs(rng.randn(ND)) * 2e-3 + 1e-4).astype(np.float32)
    nan_table = dense.copy()
    nan_table[100] = np.nan
    add("non_interacting", "sparse", interacting=False)
    add("non_interacting", "dense", interacting=False, coll=dense)
    add("non_interacting", "nan_depth", interacting=False, coll=nan_table)
    add("non_interacting", "masked", interacting=False, weights=(j % 5 != 2), scale=1.7)

    add("depth", "all_zero", coll=np.zeros(ND))
    for v in DEPTH_POSITIONS:
        t = np.zeros(ND, np.float32)
        t[v] = np.float32(3.3e-3)
        add("depth", f"single_at_{v}", coll=t)
    add("depth", "dense", coll=dense)
    for v in (777, 778, 1536, 1555):                  # the maximum of a dense table in the last round / at the seam of the two hands
        t = dense.copy()
        t[v] = np.float32(0.0123)
        add("depth", f"dense_max_at_{v}", coll=t)
    add("depth", "nan_at_100", coll=nan_table)
    t = dense.copy()
    t[1555] = np.nan
    add("depth", "nan_at_1555", coll=t)
    return classes


def flatten(classes):
    """(class name per sample, samples) in class order."""
    return [c for c, ss in classes.items() for _ in ss], [s for ss in classes.values() for s in ss]


def joint_arrays(samples):
    """pred (B,42,3), gt (B,42,4), coll (B,1556) float32, interacting (B,) uint8, scale (B,) float32."""
    return (np.stack([s["pred"] for s in samples]), np.stack([s["gt"] for s in samples]), np.stack([s["coll"] for s in samples]),
            np.array([s["interacting"] for s in samples], np.uint8), np.array([s["scale"] for s in samples], np.float32))


def big_batch_rows(n_samples, B=257, seed=5):
    """Row -> sample index of the position-independence batch: a fixed permutation of the samples repeated up to B rows."""
    return np.random.RandomState(seed).permutation(B) % n_samples


# ------------------------------------------------------------------------------------------------------------------ mesh cases
def mesh_classes():
    """class -> list of samples; a sample is a dict: pred (2,778,3), gt (2,778,3) float32 [right, left], weight (2,) float32,
    scale float32, name.  The roots come from the caller's root_w (2,778): row 0 of each hand's joint regressor."""
    rng = np.random.RandomState(778)
    classes = {}

    def add(cls, name, weight=(1.0, 1.0), offset=0.0, scale=1.0, equal=False):
        g = rng.randn(2, NV, 3) * np.array([0.06, 0.035, 0.015]) + rng.randn(2, 1, 3) * 0.05
        p = g + rng.randn(2, NV, 3) * 0.01 + rng.randn(2, 1, 3) * 0.02
        g = np.float32(g + offset)
        p = g.copy() if equal else np.float32(p + offset)
        classes.setdefault(cls, []).append(dict(name=f"{cls}/{name}", pred=p, gt=g, weight=np.float32(weight), scale=np.float32(scale)))

    add("plain", "0")
    add("plain", "1")
    add("offset_1", "0", offset=1.0)
    add("offset_1", "1", offset=-1.0)
    for sc in (0.25, 1.7, 1000.0):
        add("scaled", f"{sc:g}", scale=sc)
    for k, wt in enumerate(((0.0, 1.0), (1e-8, 1.0), (1.0, -1.0), (0.3, 1e-8), (-1.0, 0.3))):
        add("hand_weight", str(k), weight=wt, scale=(1.0, 1.7)[k % 2])
    add("both_missing", "0", weight=(0.0, 0.0))
    add("both_missing", "negative", weight=(-1.0, 0.0))
    add("equal", "0", equal=True)
    add("equal", "offset", equal=True, offset=1.0)
    return classes


def mesh_arrays(samples):
    """pred (B,2,778,3), gt (B,2,778,3), weight (B,2), scale (B,) float32."""
    return (np.stack([s["pred"] for s in samples]), np.stack([s["gt"] for s in samples]), np.stack([s["weight"] for s in samples]),
            np.array([s["scale"] for s in samples], np.float32))

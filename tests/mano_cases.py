"""The cases of the MANO layer tests, shared by tests/test_mano_cases_cpu.py (which checks on the oracle that they are what they are
meant to be) and tests/test_gpu_mano_layer.py (which compares the HIP layer with the oracle on them).  Seeded generators, no GPU.

A case is a dict of float32 numpy arrays: ``orient`` (N,3), ``pose`` (N,45), ``betas`` (N,10) and the upstream gradients ``gv``
(N,778,3), ``gj`` (N,16,3) ~ N(0,1) of the loss sum(verts gv) + sum(joints gj).  The pose classes are named by the FULL pose
``cat(orient, pose) + [0,0,0, hands_mean]`` the layer turns into rotations; "N(0, s)" below is a normal distribution of standard
deviation s:

  mild    orient 0.8 N(0,1), pose 0.3 N(0,1), betas 0.8 N(0,1): the inputs of the LBS tests in tests/test_gpu_parity.py
  zero    orient 0, pose -hands_mean, betas 0: the full pose is exactly zero (an absent or flat hand), angle = ||0 + 1e-8||
  tiny6   full pose ~ N(0, 1e-6), betas as in mild
  tiny4   full pose ~ N(0, 1e-4): where float32 loses the most of `cos a - sin a / a` in the rotation gradient
  tiny3   full pose ~ N(0, 1e-3)
  large   orient 4 N(0,1), pose 2 N(0,1), betas 3 N(0,1): angles beyond pi, a mesh a few times the template's size
  mixed   hand k takes class CLASSES[k % 6]: a packed pair and a hand group of the skin kernel hold different classes

The hand pose of the tiny classes is ``float32(x) - float32(hands_mean)`` rounded to float32; the layer's ``pose + hands_mean`` is
then exact in float32 wherever |x| is below half the mean's entry (Sterbenz's lemma) and one rounding of the mean's size off
elsewhere, which is part of what a float32 layer does.

The truth is the oracle (``oracle.mano_ref.ManoRef``) in float64 on the asset ROUNDED TO FLOAT32 first -- the constants the float32
oracle and the HIP layer hold -- so that it is the exact value of the function both of them compute and the distances below hold
arithmetic error only.  ``within`` is the one comparison: a float32 implementation may be 1.5 times as far from the truth as the
float32 oracle is (the criterion of ``_arbiter_distances`` in tests/test_gpu_parity.py), or as far as the floor the existing LBS tests
use, whichever is larger."""
import numpy as np

CLASSES = ("mild", "zero", "tiny6", "tiny4", "tiny3", "large")
TINY = {"tiny6": 1e-6, "tiny4": 1e-4, "tiny3": 1e-3}
OUTPUTS = ("verts", "joints", "d_orient", "d_pose", "d_betas")
RATIO = 1.5                # max |got - f64| <= RATIO x max |oracle32 - f64| (round-4 review: `worst_ratio`)
GRAD_FLOOR = 2e-5          # x max |f64 gradient| (test_lbs_backward_matches_autograd)
METRE_FLOOR = 2e-6         # m, for a 0.2 m mesh (test_lbs_forward_matches_oracle, _arbiter_distances)
# the launch forms of the layer change at these hand counts (csrc/mano_lbs.h, lbs_*_launch in csrc/ihmr_hip.hip); each is the smallest
# that reaches its form
N_LIST = (1, 8, 9, 33, 256, 257, 321)
SMALL_MAX_HANDS = 256      # LBS_SMALL_MAX_HANDS: HG = 4 hands per skin workgroup up to it, 8 above


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _class_inputs(name, N, seed, hands_mean):
    rng = np.random.RandomState(seed)
    hm = _f32(hands_mean)
    o, p, b = rng.standard_normal((N, 3)), rng.standard_normal((N, 45)), rng.standard_normal((N, 10))
    if name == "mild":
        return _f32(0.8 * o), _f32(0.3 * p), _f32(0.8 * b)
    if name == "large":
        return _f32(4.0 * o), _f32(2.0 * p), _f32(3.0 * b)
    if name == "zero":
        return np.zeros((N, 3), np.float32), np.repeat(-hm[None], N, 0), np.zeros((N, 10), np.float32)
    s = TINY[name]
    return _f32(s * o), _f32(_f32(s * p) - hm[None]), _f32(0.8 * b)


def inputs(name, N, seed, hands_mean):
    """orient (N,3), pose (N,45), betas (N,10) of a pose class, float32."""
    if name != "mixed":
        return _class_inputs(name, N, seed, hands_mean)
    parts = [_class_inputs(c, N, seed + 101 * (i + 1), hands_mean) for i, c in enumerate(CLASSES)]
    pick = np.arange(N) % len(CLASSES)
    return tuple(np.ascontiguousarray(np.stack([parts[pick[k]][t][k] for k in range(N)])) for t in range(3))


def class_of_hand(name, N):
    """(N,) index into CLASSES of every hand of a case."""
    return np.arange(N) % len(CLASSES) if name == "mixed" else np.full(N, CLASSES.index(name))


def upstream(N, seed):
    """gv (N,778,3), gj (N,16,3) ~ N(0,1), float32."""
    rng = np.random.RandomState(seed + 7919)
    return _f32(rng.standard_normal((N, 778, 3))), _f32(rng.standard_normal((N, 16, 3)))


def case(name, N, seed, hands_mean):
    o, p, b = inputs(name, N, seed, hands_mean)
    gv, gj = upstream(N, seed)
    return dict(name=name, N=N, seed=seed, orient=o, pose=p, betas=b, gv=gv, gj=gj)


def permuted(c, perm):
    """The same hands in another order."""
    return dict(c, **{k: np.ascontiguousarray(c[k][perm]) for k in ("orient", "pose", "betas", "gv", "gj")})


def full_pose(c, hands_mean):
    """(N,48) float32: what the layer hands to Rodrigues, in float32 arithmetic."""
    hm = _f32(hands_mean)
    return np.concatenate([c["orient"], c["pose"] + hm[None]], 1)


def rounded_asset(arrays):
    """The asset with every floating-point array rounded to float32: the constants a float32 implementation holds."""
    return {k: (_f32(v) if np.asarray(v).dtype.kind == "f" else np.asarray(v)) for k, v in arrays.items()}


def reference(arrays, c, dtype, use_gv=True, use_gj=True):
    """verts, joints, d_orient, d_pose, d_betas of the oracle in `dtype` (torch.float32 / torch.float64) on the float32-rounded asset,
    as float64 arrays; the gradients are those of sum(verts gv) + sum(joints gj) (either term can be left out)."""
    import torch
    from oracle.mano_ref import ManoRef
    ref = ManoRef(rounded_asset(arrays), dtype=dtype)
    o, p, b = (torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("orient", "pose", "betas"))
    out = ref(global_orient=o, hand_pose=p, betas=b)
    loss = 0.0
    if use_gv:
        loss = loss + (out.vertices * torch.tensor(c["gv"], dtype=dtype)).sum()
    if use_gj:
        loss = loss + (out.joints * torch.tensor(c["gj"], dtype=dtype)).sum()
    loss.backward()
    f = lambda t: t.detach().numpy().astype(np.float64)
    return dict(verts=f(out.vertices), joints=f(out.joints), d_orient=f(o.grad), d_pose=f(p.grad), d_betas=f(b.grad))


def floor_of(output, f64):
    """The absolute floor of an output's bound.  Gradients: 2e-5 of the largest true gradient.  Metres: 2e-6 m, the round-off of a
    0.2 m mesh, scaled with the mesh where it is larger than that (`large`: betas x 3)."""
    top = float(np.abs(f64).max()) if np.size(f64) else 0.0
    return GRAD_FLOOR * top if output.startswith("d_") else METRE_FLOOR * max(1.0, top / 0.2)


def distances(got, f64, o32):
    """max |got - f64|, max |o32 - f64|."""
    f64 = np.asarray(f64, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - f64).max()), float(np.abs(np.asarray(o32, np.float64) - f64).max())


def within(got, f64, o32, floor, tag=""):
    """Assert max |got - f64| <= max(floor, 1.5 max |o32 - f64|); both distances and their ratio are printed first.  Returns the ratio."""
    assert np.all(np.isfinite(np.asarray(got, np.float64))), (tag, "not finite")
    d_got, d_o32 = distances(got, f64, o32)
    ratio = d_got / max(d_o32, 1e-300)
    bound = max(floor, RATIO * d_o32)
    print(f"[mano] {tag}: |got - f64| {d_got:.3e}  |oracle32 - f64| {d_o32:.3e}  ratio {ratio:.2f}  floor {floor:.3e}  "
          f"max|f64| {float(np.abs(f64).max()):.3e}  ({'ratio' if RATIO * d_o32 > floor else 'floor'} governs)")
    assert d_got <= bound, (tag, "distance from the float64 oracle", d_got, "bound", bound, "float32 oracle's", d_o32)
    return ratio


def check_outputs(tag, got, f64, o32, rows=None):
    """`within` on each of the five outputs (dicts keyed by OUTPUTS), over the hands `rows` if given; {output: ratio}."""
    sel = (lambda a: a) if rows is None else (lambda a: np.asarray(a)[rows])
    return {k: within(sel(got[k]), sel(f64[k]), sel(o32[k]), floor_of(k, sel(f64[k])), f"{tag} {k}") for k in OUTPUTS if k in got}


# ----------------------------------------------------------------------------------- the skin kernel's deal of hands to workgroups
def dense_weight_asset(arr, nnz=7, seed=5):
    """The synthetic asset with up to `nnz` non-zero skinning weights per vertex (rows still sum to 1): MANO's own weights have at
    most four, which is what the kernels' short skinning loops assume -- a denser asset must take their 16-joint form."""
    rng = np.random.default_rng(seed)
    a = dict(arr)
    w = np.array(arr["lbs_weights"], dtype=np.float64)
    for v in range(0, w.shape[0], 3):
        extra = rng.choice(w.shape[1], size=nnz, replace=False)
        w[v, extra] += rng.uniform(0.02, 0.2, size=nnz)
    w /= w.sum(axis=1, keepdims=True)
    a["lbs_weights"] = w.astype(arr["lbs_weights"].dtype)
    assert int((a["lbs_weights"] != 0).sum(axis=1).max()) > 4
    return a


def skin_hands_per_group(N):
    return 4 if N <= SMALL_MAX_HANDS else 8


def lbs_group_hand(HG, x, s, i):
    """Restatement of `lbs_group_hand<HG>` (csrc/mano_lbs.h): hand i of workgroup (x, s)."""
    return x + 8 * (HG * s + i)


def skin_slots(N):
    """(groups, HG) bool: slot i of workgroup (x, s) holds a real hand (< N); the launch has 8 x ceil(N / (8 HG)) workgroups per vertex tile."""
    HG = skin_hands_per_group(N)
    S = (N + 8 * HG - 1) // (8 * HG)
    return np.array([[lbs_group_hand(HG, x, s, i) < N for i in range(HG)] for s in range(S) for x in range(8)])

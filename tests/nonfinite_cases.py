"""Non-finite input: the control batches and the poison kinds of tests/test_gpu_nonfinite.py.  Host only (no GPU is touched on import or
by any function here); tests/test_nonfinite_cases_cpu.py checks the preconditions with the float32 oracle.

A case = a control batch of three samples + ONE sample (the victim) poisoned in ONE place.  Every kind is an input the audit of
DESIGN.md ("Non-finite input") shows to be bounded: no kind is chosen to make a kernel fault.  What a poisoned run is compared with is
always the control run that differs from it in the victim alone."""
import numpy as np
import torch

NAN, INF = float("nan"), float("inf")
B = 3
DEFAULT_SEED = 3022      # oracle_two_hand_verts(mano_arrays, 3, 3022): 155 / 125 / 171 penetrating vertices (float32 oracle), all three two-handed
CONTROL_KINDS = ("deep", "default")

# ------------------------------------------------------------------------------------------------ refinement loop: targets and initial state
# name -> (batch key, index inside the victim's row, value)
TARGET_KINDS = {
    "joints2d-nan": ("init_joints_2d", (7, 0), NAN),
    "joints3d-inf": ("init_joints_3d", (30, 1), INF),
    "trans-target-nan": ("init_hand_trans_j", (0, 2), NAN),
    "wrist-weight-nan": ("init_joints_3d", (0, 3), NAN),
}
STATE_KINDS = {
    "pose-nan": ("init_pose_params", (10,), NAN),
    "shape-neg-inf": ("init_shape_params", (13,), -INF),
    "trans-nan": ("init_hand_trans", (0, 1), NAN),
    "trans-1e30": ("init_hand_trans", (0, 1), 1e30),
    "cam-nan": ("init_cam", (0,), NAN),
}
LOOP_KINDS = dict(TARGET_KINDS, **STATE_KINDS)
# one stage per tail form (stage_cases.stage_for(mask, 3)): translation, translation + camera, both orientations, both finger poses,
# both shapes, every block
LOOP_MASKS = (2, 3, 12, 48, 192, 255)
SAMPLE0_MASKS = (2, 12)       # ... also with the victim at batch position 0, whose workgroup zeroes the shared inside-voxel counters
N_ITERS = 3

# ------------------------------------------------------------------------------------------------ seam B: vertices
VERTEX_KINDS = ("nan-x", "nan-y", "hand-nan", "vertex-inf", "extent-overflow", "vertex-1e30", "all-equal")
HANDS = {"right": (0,), "left": (1,), "both": (0, 1)}
VICTIM = 1                    # the control sample that is poisoned, wherever a case places it


def poison_vertices(hv, b, kind, hands, vertex):
    """A copy of the hand pairs `hv` (B,2,778,3) with sample b's hands `hands` (indices 0 = right, 1 = left) poisoned at the vertices
    `vertex[hand]` (`deepest_vertices`: a vertex far from the other hand would change nothing the kernels look at)."""
    out = hv.clone()
    for h in hands:
        v = out[b, h]
        pv_ = int(vertex[h])
        if kind == "nan-x":
            v[pv_, 0] = NAN
        elif kind == "nan-y":
            v[pv_, 1] = NAN
        elif kind == "hand-nan":
            v[:] = NAN
        elif kind == "vertex-inf":
            v[pv_] = INF
        elif kind == "extent-overflow":              # max - min overflows float32: the box scale is +inf, its centre finite
            v[pv_] = 3e38
            v[(pv_ + 1) % 778] = -3e38
        elif kind == "vertex-1e30":
            v[pv_] = 1e30
        elif kind == "all-equal":                     # the box has extent 0: scale 0, every normalised coordinate 0 / 0
            v[:] = v[pv_].clone()
        else:
            raise ValueError(kind)
    return out


_CONTROL, _DEEPEST = {}, {}


def deepest_vertices(mano_arrays, kind):
    """(right, left): per hand of the control's VICTIM sample, the vertex that lies deepest inside the other hand (float32 oracle, on
    the finite control pair).  Entry h * 778 + v of per_vert samples hand h's grid at vertex v of hand 1 - h."""
    if kind not in _DEEPEST:
        from oracle.sdf_ref import SDFLossRef
        right, left = mano_arrays
        hv, _ = control(mano_arrays, kind)
        _, per_vert, _ = SDFLossRef(right["faces"], left["faces"])(hv, return_per_vert_loss=True, return_origin_scale_loss=True)
        pv = per_vert[VICTIM].view(2, 778)
        assert float(pv[1].max()) > 0 and float(pv[0].max()) > 0, "both hands of the victim must have a vertex inside the other hand"
        _DEEPEST[kind] = (int(pv[1].argmax()), int(pv[0].argmax()))
    return _DEEPEST[kind]


def control(mano_arrays, kind):
    """(hand pairs (3,2,778,3), batch) of a control kind: `deep` = stage_cases.batch(mano_arrays, "deep"), `default` = the default
    geometry of seed DEFAULT_SEED.  Built once, handed out unchanged."""
    if kind not in _CONTROL:
        from helpers import DEEP_SEED, oracle_two_hand_verts
        import stage_cases
        if kind == "deep":
            hv, _ = oracle_two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
            batch = stage_cases.batch(mano_arrays, "deep", B)
        elif kind == "default":
            hv, batch = oracle_two_hand_verts(mano_arrays, B, DEFAULT_SEED)
        else:
            raise ValueError(kind)
        _CONTROL[kind] = (hv, batch)
    return _CONTROL[kind]


def place(batch, victim, position):
    """The batch with the samples `victim` and `position` exchanged (every tensor; a copy): the victim then sits at `position`."""
    order = list(range(B))
    order[victim], order[position] = order[position], order[victim]
    idx = torch.tensor(order)
    return {k: v[idx].clone() for k, v in batch.items()}


def poison_batch(batch, b, kind):
    """A copy of `batch` with sample b poisoned by the loop kind `kind` (LOOP_KINDS) or an (key, index, value) triple."""
    key, index, value = LOOP_KINDS[kind] if isinstance(kind, str) else kind
    out = {k: v.clone() for k, v in batch.items()}
    out[key][(b,) + tuple(index)] = value
    return out


def differs_only_in(a, b_, row):
    """True iff the two batches have the same bytes outside sample `row` (and differ inside it)."""
    same_elsewhere, differ_here = True, False
    for k in a:
        x, y = a[k].contiguous().numpy(), b_[k].contiguous().numpy()
        eq = x.view(np.uint8).reshape(x.shape[0], -1) == y.view(np.uint8).reshape(y.shape[0], -1)
        rows = eq.all(axis=1)
        differ_here = differ_here or not rows[row]
        rows[row] = True
        same_elsewhere = same_elsewhere and bool(rows.all())
    return same_elsewhere and differ_here


def select_replay(snap_loss, use_filter, filter_factor, select_loss):
    """numpy float32 restatement of the product's select rule (include/ihmr_hip.h, ihmr_opt_run_stage) on snap_loss (S,3,B): snapshot 0
    is the first candidate; snapshot s replaces the best so far iff its key -- its select loss when it passes every filter (loss <=
    float32(origin * factor)), float32(1e11) otherwise -- is LESS than the best key.  A NaN never passes a filter and never wins."""
    snap_loss = np.asarray(snap_loss, np.float32)
    S, _, nb = snap_loss.shape
    out = np.zeros(nb, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(nb):
            bar = [np.float32(snap_loss[0, l, b] * np.float32(filter_factor[l])) for l in range(3)]
            best, best_v = 0, snap_loss[0, select_loss, b]
            for s in range(1, S):
                valid = all(bool(snap_loss[s, l, b] <= bar[l]) for l in range(3) if use_filter[l])
                key = snap_loss[s, select_loss, b] if valid else np.float32(100000000000.0)
                if key < best_v:
                    best, best_v = s, key
            out[b] = best
    return out


def reference_select(snap_loss, use_filter, filter_factor, select_loss):
    """The reference's rule on the same snapshots (utils/opt_utils.py:104-153): invalid rows get 1e11, row 0 is restored, torch.argmin
    -- which takes a NaN for the minimum and returns the first one."""
    snap_loss = np.asarray(snap_loss, np.float32)
    S, _, nb = snap_loss.shape
    keys = torch.tensor(snap_loss[:, select_loss, :].copy())
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(3):
            if use_filter[l]:
                bar = (snap_loss[0, l] * np.float32(filter_factor[l])).astype(np.float32)
                bad = ~(snap_loss[:, l] <= bar[None])
                bad[0] = False
                keys[torch.tensor(bad)] = 100000000000.0
    return torch.argmin(keys, dim=0).numpy().astype(np.int32)

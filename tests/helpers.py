"""Helpers shared by the tests and by tests/golden/make_golden.py."""
import numpy as np
import torch


def seeded_state_dict(module, seed, last_scale=None):
    """Deterministic weights reproducible on any side: tensor i of ``state_dict()`` (in order) is drawn
    from RandomState(seed + i); conv/linear weights ~ N(0, 1/fan_in), BN gamma ~ U(0.5,1.5),
    beta / bias ~ N(0, 0.05), running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5)."""
    new = {}
    for i, (k, v) in enumerate(module.state_dict().items()):
        rng = np.random.RandomState(seed + i)
        shp = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            new[k] = torch.zeros_like(v)
        elif k.endswith("running_var"):
            new[k] = torch.tensor(rng.uniform(0.5, 1.5, shp), dtype=torch.float32)
        elif k.endswith("running_mean"):
            new[k] = torch.tensor(rng.normal(0, 0.1, shp), dtype=torch.float32)
        elif v.dim() >= 2:
            fan_in = int(np.prod(shp[1:]))
            new[k] = torch.tensor(rng.normal(0, 1.0 / np.sqrt(fan_in), shp), dtype=torch.float32)
        elif "bn" in k or "downsample.1" in k:
            new[k] = torch.tensor(rng.uniform(0.5, 1.5, shp) if k.endswith("weight") else rng.normal(0, 0.05, shp),
                                  dtype=torch.float32)
        else:
            new[k] = torch.tensor(rng.normal(0, 0.05, shp), dtype=torch.float32)
    if last_scale is not None:  # shrink the output layer (small residual updates, like the trained MLP heads)
        last = [k for k in new if k.endswith('weight')][-1]
        new[last] = new[last] * last_scale
        new[last.replace('weight', 'bias')] = new[last.replace('weight', 'bias')] * last_scale
    return new


def ragged_opt_batch(batch):
    """Turn a synthetic IHMR-OPT batch (>= 8 samples, ``ihmr_amd.synthetic.synthetic_opt_batch``) into a RAGGED one, in
    place, covering the branches the reference's loss code takes on real annotation
    (``loss_utils.py:90-98`` root choice, ``:186-188`` hand-type mask, zero joint weights):

      0  both hands, fully annotated (control)
      1  right hand only  (hand_type [1,0]; left joints unannotated; no translation target)
      2  left hand only   (hand_type [0,1]; right joints unannotated -> root = joint 21)
      3  both hands, right wrist unannotated in both target sets (root = joint 21 twice)
      4  init wrist weight 0.3 (second alignment skipped), GT wrist weight 1
      5  GT wrist weight 0.3 (first alignment skipped), init wrist weight 0 (second one about joint 21), random
         zero-weight joints in every target set
      6  no 3-D target at all (every init 3-D weight 0), a few 2-D weights 0
      7  hands 0.4 m apart: collision term exactly 0 although both hands are present
    Samples >= 8 are left alone."""
    B = batch["init_cam"].shape[0]
    assert B >= 8
    rng = np.random.RandomState(99)
    j2, j3, i2, i3 = batch["joints_2d"], batch["joints_3d"], batch["init_joints_2d"], batch["init_joints_3d"]
    # 1: right only
    batch["hand_type_array"][1] = torch.tensor([1.0, 0.0])
    for t in (j2, j3, i2, i3):
        t[1, 21:, -1] = 0.0
    batch["init_hand_trans_j"][1, 0, 3] = 0.0
    batch["hand_trans"][1, 0, 3] = 0.0
    # 2: left only
    batch["hand_type_array"][2] = torch.tensor([0.0, 1.0])
    for t in (j2, j3, i2, i3):
        t[2, :21, -1] = 0.0
    batch["init_hand_trans_j"][2, 0, 3] = 0.0
    batch["hand_trans"][2, 0, 3] = 0.0
    # 3: no right wrist
    j3[3, 0, 3] = 0.0
    i3[3, 0, 3] = 0.0
    # 4 / 5: in-between weights
    i3[4, 0, 3] = 0.3
    j3[5, 0, 3] = 0.3
    i3[5, 0, 3] = 0.0
    for t in (j2, j3, i2, i3):
        drop = torch.from_numpy(rng.rand(42) < 0.3)
        drop[0] = False
        t[5, drop, -1] = 0.0
    # 6: no 3-D target
    i3[6, :, 3] = 0.0
    i2[6, torch.from_numpy(rng.rand(42) < 0.2), 2] = 0.0
    # 7: separated hands
    batch["init_hand_trans"][7, 0, 0] += 0.4
    return batch


def variant_strategy(epoch):
    """opt_default's stages with filter / select criteria the reference accepts but its default strategy does not use
    (utils/opt_utils.py:57-67: any loss with a `_batch` twin that is not GT-based)."""
    from ihmr_amd.strategies import make_opt_strategy
    st = make_opt_strategy(epoch)
    st[0]["filter_loss"], st[0]["select_loss"] = [("joints_2d_loss_p", "+5")], "collision_loss"
    st[1]["filter_loss"], st[1]["select_loss"] = [("collision_loss", "-10")], "joints_2d_loss_p"
    st[3]["filter_loss"], st[3]["select_loss"] = [("joints_3d_loss_p", "+0"), ("joints_3d_loss_p", "-1"), ("joints_2d_loss_p", "+20")], "joints_3d_loss_p"
    return st


# ----------------------------------------------------------------------------------- collision geometries and what they ask of the kernels
def oracle_two_hand_verts(mano_arrays, B, seed, interlock=False, overlap=None):
    """(B,2,778,3) hand pairs (index 0 = right) from the oracle's forward at the initial parameters of the synthetic batch, and the
    batch itself (``ihmr_amd.synthetic.synthetic_opt_batch``; interlock: the finger asset's generator; overlap="deep": the deep batch)."""
    from oracle.opt_ref import OptimizeRef
    from ihmr_amd.synthetic import synthetic_opt_batch
    right, left = mano_arrays
    orc = OptimizeRef(right, left, B, [], save_mid_freq=1)

    def fwd(pose, shape, trans):
        orc.pred_right_orient, orc.pred_left_orient = pose[:, :3], pose[:, 48:51]
        orc.pred_right_pose_params, orc.pred_left_pose_params = pose[:, 3:48], pose[:, 51:]
        orc.pred_right_shape_params, orc.pred_left_shape_params = shape[:, :10], shape[:, 10:]
        orc.pred_hand_trans = trans.view(-1, 1, 3)
        fwd.out = orc.get_mano_output()
        return fwd.out[2]

    batch = synthetic_opt_batch(B, fwd, seed=seed, interlock=interlock, overlap=overlap)
    with torch.no_grad():
        fwd(batch["init_pose_params"], batch["init_shape_params"], batch["init_hand_trans"][:, 0, :3])
    rv, lv, _ = fwd.out
    return torch.stack([rv, lv], dim=1).detach().contiguous(), batch


def point_cloud_pairs(hv, seed):
    """The left hand's 778 vertices replaced by a seeded uniform point cloud over the right hand's vertex box: the right hand's queries
    then need almost every column of its grid, and the left 'mesh' (the hand's faces over scattered points) is a tangle of long
    triangles.  The oracle's grid is defined for any mesh, so the single-shot collision must still match it."""
    g = torch.Generator().manual_seed(seed)
    r = hv[:, 0]
    lo, hi = r.min(dim=1, keepdim=True)[0], r.max(dim=1, keepdim=True)[0]
    cloud = lo + (hi - lo) * torch.rand(r.shape, generator=g, dtype=r.dtype)
    return torch.stack([r, cloud], dim=1).contiguous()


G = 32
DEEP_SEED = 6475          # the deep batch of the collision tests: at B = 64, 4 of its 128 hands queue more than SDF_RAYQ = 3072 ray pairs
POINT_CLOUD_SEED = 4646


def needed_voxels(hv):
    """(B,2,G,G,G) bool, voxel [k][j][i] = (z, y, x): the voxels of hand h's grid that the other hand's vertices read -- the 8 corners
    of the cell that holds each query (trilinear sampling, align_corners False, zeros padding; a query whose cell lies wholly outside the
    grid reads nothing).  A numpy restatement of the sparse prep kernel's rule (csrc/sdf_collision.h, the `needed` words), float32."""
    from oracle.sdf_ref import hand_boxes
    centre, scale = hand_boxes(hv)
    B = hv.shape[0]
    out = np.zeros((B, 2, G, G, G), bool)
    f = np.float32
    for h in (0, 1):
        q = ((hv[:, 1 - h] - centre[:, h]) / scale[:, h]).numpy().astype(f)              # (B,778,3): x, y, z
        ic = ((q + f(1)) * f(G) - f(1)) / f(2)
        fl = np.floor(ic)
        ok = np.all((fl >= -1) & (fl <= G - 1), axis=-1)
        b_i, v_i = np.nonzero(ok)
        c0 = fl[b_i, v_i].astype(np.int64)                                                  # (n,3) x0, y0, z0
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    x, y, z = c0[:, 0] + dx, c0[:, 1] + dy, c0[:, 2] + dz
                    m = (x >= 0) & (x < G) & (y >= 0) & (y < G) & (z >= 0) & (z < G)
                    out[b_i[m], h, z[m], y[m], x[m]] = True
    return out


def oracle_inside(hv, faces_right, faces_left):
    """(B,2,G,G,G) bool: the oracle's float32 grid of each hand (normalised by its own box) > 0."""
    from oracle import sdf_ref
    centre, scale = sdf_ref.hand_boxes(hv)
    vn = (hv - centre) / scale
    fr, fl = torch.tensor(np.asarray(faces_right, np.int32)), torch.tensor(np.asarray(faces_left, np.int32))
    return torch.stack([sdf_ref.sdf_grid(vn[:, 0].contiguous(), fr), sdf_ref.sdf_grid(vn[:, 1].contiguous(), fl)], dim=1).numpy() > 0


def tri_col_range(y, z):
    """numpy float32 restatement of ``tri_col_range`` (csrc/ihmr_pure.h) over arrays of triangles: y, z (..., 3) -> j0, j1, k0, k1."""
    f = np.float32
    m = f(1e-4)
    lo = lambda a: np.min(a, axis=-1) - m
    hi = lambda a: np.max(a, axis=-1) + m
    idx = lambda a, fn: fn((a + f(1)) * f(16) - f(0.5)).astype(np.int64)
    j0 = np.maximum(0, idx(lo(y), np.ceil)); j1 = np.minimum(G - 1, idx(hi(y), np.floor))
    k0 = np.maximum(0, idx(lo(z), np.ceil)); k1 = np.minimum(G - 1, idx(hi(z), np.floor))
    return j0, j1, k0, k1


def ray_queue_pairs(hv, faces_right, faces_left, needed):
    """(B,2) int: P per hand -- over the hand's triangles that are not degenerate in yz (|det| >= 1e-12 in its normalised frame), the
    number of (triangle, column) pairs whose column (k, j) lies in the triangle's column range and holds a needed voxel: the entries of
    the sparse prep kernel's ray-parity queue, SDF_RAYQ = 3072 per window."""
    from oracle.sdf_ref import hand_boxes
    centre, scale = hand_boxes(hv)
    vn = ((hv - centre) / scale).numpy().astype(np.float32)
    col = needed.any(axis=-1)                                               # (B,2,G(k),G(j))
    cum = np.zeros(col.shape[:2] + (G + 1, G + 1), np.int64)                # 2-D prefix sums: columns in a (k, j) rectangle
    cum[..., 1:, 1:] = col.astype(np.int64).cumsum(-1).cumsum(-2)
    B = hv.shape[0]
    P = np.zeros((B, 2), np.int64)
    for h, faces in ((0, faces_right), (1, faces_left)):
        t = vn[:, h][:, np.asarray(faces, np.int64)]                        # (B,F,3 corners,3)
        y, z = t[..., 1], t[..., 2]
        e1y, e1z, e2y, e2z = y[..., 1] - y[..., 0], z[..., 1] - z[..., 0], y[..., 2] - y[..., 0], z[..., 2] - z[..., 0]
        det = (e1z.astype(np.float64) * e2y - (e1y * e2z).astype(np.float64)).astype(np.float32)    # (fmaf: one rounding)
        j0, j1, k0, k1 = tri_col_range(y, z)
        ok = (np.abs(det) >= np.float32(1e-12)) & (j1 >= j0) & (k1 >= k0)
        bb = np.arange(B)[:, None]
        c = cum[:, h]
        j0, k0, j1, k1 = np.minimum(j0, G), np.minimum(k0, G), np.maximum(j1, -1), np.maximum(k1, -1)     # (masked below when empty)
        n = c[bb, k1 + 1, j1 + 1] - c[bb, k0, j1 + 1] - c[bb, k1 + 1, j0] + c[bb, k0, j0]
        P[:, h] = np.where(ok, n, 0).sum(axis=1)
    return P


def synthetic_mlp_batch(mano_arrays, B, seed):
    """A synthetic IHMR-MLP batch with image features (``synthetic_opt_batch(..., with_feat=True)`` on the oracle's two-hand MANO),
    in the layout MLPModel / MLPRef take: ``init_hand_trans`` (B,3), an 8 x 8 dummy image, no ``init_hand_trans_j``."""
    from ihmr_amd.synthetic import synthetic_opt_batch
    from oracle.opt_ref import OptimizeRef
    right, left = mano_arrays
    helper = OptimizeRef(right, left, B, [], save_mid_freq=1)

    def fwd(pose, shape, trans):
        helper.pred_right_orient, helper.pred_left_orient = pose[:, :3], pose[:, 48:51]
        helper.pred_right_pose_params, helper.pred_left_pose_params = pose[:, 3:48], pose[:, 51:]
        helper.pred_right_shape_params, helper.pred_left_shape_params = shape[:, :10], shape[:, 10:]
        helper.pred_hand_trans = trans.view(-1, 1, 3)
        return helper.get_mano_output()[2]

    batch = synthetic_opt_batch(B, fwd, seed=seed, with_feat=True)
    batch["init_hand_trans"] = batch["init_hand_trans"][:, 0, :3].contiguous()
    batch["img"] = torch.zeros(B, 3, 8, 8)
    batch.pop("init_hand_trans_j")
    return batch

"""GPU parity tests proper: the HIP path, called through the C ABI (ctypes, ``ihmr_amd.hip``), against
the CPU oracle on the same seeded inputs.  Tolerances are written next to each check.

    python -m pytest tests -m gpu -x -q          (on the MI355X box)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _report(name, got, ref, atol, rtol=0.0):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    lim = atol + rtol * np.abs(ref)
    worst = float((err - lim).max())
    print(f"[parity] {name}: max|err|={err.max():.3e} max|ref|={np.abs(ref).max():.3e} (atol {atol:g}, rtol {rtol:g})")
    assert worst <= 0, f"{name}: max err {err.max():.3e} exceeds tolerance (atol {atol}, rtol {rtol})"


# ----------------------------------------------------------------------------------- seam A (MANO LBS)
def _rand_mano_inputs(N, seed):
    g = torch.Generator().manual_seed(seed)
    orient = torch.randn(N, 3, generator=g) * 0.8
    pose = torch.randn(N, 45, generator=g) * 0.3
    betas = torch.randn(N, 10, generator=g) * 0.8
    return orient, pose, betas


def test_lbs_forward_matches_oracle(mano_arrays):
    from ihmr_amd import mano
    from oracle.mano_ref import ManoRef
    right, _ = mano_arrays
    N = 7
    orient, pose, betas = _rand_mano_inputs(N, 0)
    ref = ManoRef(right)(global_orient=orient, hand_pose=pose, betas=betas)
    m = mano.MANO(right).to(_dev())
    out = m(global_orient=orient.cuda(), hand_pose=pose.cuda(), betas=betas.cuda())
    # metres; fp32 round-off of a ~0.2 m mesh -- 1e-6 is 5 ulp-ish, far inside the 1e-4 bar
    _report("lbs verts", out.vertices.cpu(), ref.vertices, atol=2e-6)
    _report("lbs joints", out.joints.cpu(), ref.joints, atol=2e-6)


def test_lbs_zero_pose_is_template(mano_arrays):
    """KAT: zero pose & betas with zero hands_mean => verts == v_template, joints == J_regressor v_template."""
    from ihmr_amd import mano
    right, _ = mano_arrays
    arr = dict(right)
    arr["hands_mean"] = np.zeros(45, np.float32)
    m = mano.MANO(arr).to(_dev())
    z = lambda d: torch.zeros(2, d, device=_dev())
    out = m(global_orient=z(3), hand_pose=z(45), betas=z(10))
    _report("template verts", out.vertices[0].cpu(), arr["v_template"], atol=1e-7)
    _report("template joints", out.joints[0].cpu(), arr["J_regressor"] @ arr["v_template"], atol=1e-7)


@pytest.mark.parametrize("which", ["orient", "pose", "betas", "all"])
def test_lbs_backward_matches_autograd(mano_arrays, which):
    from ihmr_amd import mano
    from oracle.mano_ref import ManoRef
    right, _ = mano_arrays
    N = 5
    orient, pose, betas = _rand_mano_inputs(N, 1)
    g = torch.Generator().manual_seed(2)
    gv = torch.randn(N, 778, 3, generator=g)
    gj = torch.randn(N, 16, 3, generator=g)
    need = dict(orient=which in ("orient", "all"), pose=which in ("pose", "all"), betas=which in ("betas", "all"))

    def run(module, dev):
        o, p, b = (t.clone().to(dev).requires_grad_(need[k]) for t, k in ((orient, "orient"), (pose, "pose"), (betas, "betas")))
        out = module(global_orient=o, hand_pose=p, betas=b)
        loss = (out.vertices * gv.to(dev)).sum() + (out.joints * gj.to(dev)).sum()
        loss.backward()
        return {k: (t.grad.cpu() if t.grad is not None else None) for k, t in (("orient", o), ("pose", p), ("betas", b))}

    ref = run(ManoRef(right), "cpu")
    got = run(mano.MANO(right).to(_dev()), _dev())
    for k in ref:
        if need[k]:
            scale = float(ref[k].abs().max())
            # gradients are sums over 778 vertices of O(1) terms: relative-to-max tolerance 2e-5
            _report(f"lbs d{k} [{which}]", got[k], ref[k], atol=2e-5 * scale)


def test_lbs_dense_weight_asset_matches_oracle(mano_arrays):
    """Forward and all gradients of the LBS kernels on an asset whose vertices have MORE than four non-zero skinning weights (the
    16-joint loops) against the oracle; the same inputs on the 4-sparse asset go through the short loops (tests above)."""
    from ihmr_amd import mano
    from mano_cases import dense_weight_asset
    from oracle.mano_ref import ManoRef
    right, _ = mano_arrays
    arr = dense_weight_asset(right)
    N = 5
    orient, pose, betas = _rand_mano_inputs(N, 11)
    g = torch.Generator().manual_seed(12)
    gv = torch.randn(N, 778, 3, generator=g)
    gj = torch.randn(N, 16, 3, generator=g)

    def run(module, dev):
        o, p, b = (t.clone().to(dev).requires_grad_(True) for t in (orient, pose, betas))
        out = module(global_orient=o, hand_pose=p, betas=b)
        ((out.vertices * gv.to(dev)).sum() + (out.joints * gj.to(dev)).sum()).backward()
        return out.vertices.detach().cpu(), out.joints.detach().cpu(), o.grad.cpu(), p.grad.cpu(), b.grad.cpu()

    ref = run(ManoRef(arr), "cpu")
    got = run(mano.MANO(arr).to(_dev()), _dev())
    _report("dense-weight lbs verts", got[0], ref[0], atol=2e-6)
    _report("dense-weight lbs joints", got[1], ref[1], atol=2e-6)
    for name, a, b in zip(("orient", "pose", "betas"), got[2:], ref[2:]):
        _report(f"dense-weight lbs d{name}", a, b, atol=2e-5 * float(b.abs().max()))


# ----------------------------------------------------------------------------------- seam B (collision)
def _two_hand_verts(mano_arrays, B, seed, interlock=False, overlap=None):
    """(B,2,778,3) penetrating hand pairs from the oracle forward on the synthetic batch (interlock: the finger asset's batch generator;
    overlap="deep": the deeply interpenetrating batch, tests/helpers.py)."""
    from helpers import oracle_two_hand_verts
    return oracle_two_hand_verts(mano_arrays, B, seed, interlock=interlock, overlap=overlap)


@pytest.mark.parametrize("squash", [None, 0.3, 1e-3, 1e-6, "ball"], ids=["hands", "flat", "thin", "sliver", "ball"])
def test_sdf_dense_grid_bit_exact(mano_arrays, squash):
    """The product kernels evaluated on EVERY voxel reproduce the oracle's dense 32^3 grid bit for bit
    (same operation order, contraction off) -- inside/outside decisions and distances alike.  The squashed
    variants flatten the meshes along y, so the yz determinants of the ray test shrink by 1e3 / 1e6: the
    near-degenerate regime in which the kernel's loop-free hit mask must fall back to per-voxel evaluation (no voxel
    centre lies inside those two: the expected grid is all zeros, i.e. the test is that no ray produces a false crossing;
    "flat" = 0.3 keeps an interior).  "ball"
    projects every vertex onto a sphere about the hand's centre: voxels near the centre are (nearly) equidistant from
    all 1538 triangles, so the bounding-sphere cull keeps more triangles than the per-wave survivor list holds and the
    distance kernel takes its overflow path."""
    B = 2
    hv, _ = _two_hand_verts(mano_arrays, B, 77)
    _dense_grid_check(mano_arrays, hv, squash)


@pytest.fixture(scope="module")
def finger_arrays():
    """The geometry-sensitivity asset (round 5): the same MANO-shaped model on a mesh with a palm and five finger tubes."""
    from ihmr_amd.assets import synthetic_mano
    return synthetic_mano(True, kind="fingers"), synthetic_mano(False, kind="fingers")


def test_sdf_dense_grid_bit_exact_on_the_finger_asset(finger_arrays):
    """The same bit-for-bit grid test on the five-finger mesh with interlocked hands (thin tubes, webs between the fingers, many
    more triangles per voxel neighbourhood than the blob) and on the default pose distribution."""
    for interlock in (True, False):
        hv, _ = _two_hand_verts(finger_arrays, 2, 77, interlock=interlock)
        _dense_grid_check(finger_arrays, hv, None)


def _dense_grid_check(mano_arrays, hv, squash):
    import ctypes as C
    from ihmr_amd import hip
    from oracle import sdf_ref
    right, left = mano_arrays
    B = hv.shape[0]
    if squash == "ball":
        c = hv.mean(dim=2, keepdim=True)
        d = hv - c
        hv = (c + 0.08 * d / d.norm(dim=3, keepdim=True).clamp_min(1e-9)).contiguous()
    elif squash is not None:
        hv = (hv * torch.tensor([1.0, squash, 1.0])).contiguous()
    centre, scale = sdf_ref.hand_boxes(hv)
    vn = (hv - centre) / scale
    fr = torch.tensor(right["faces"].astype(np.int32))
    fl = torch.tensor(left["faces"].astype(np.int32))
    ref = torch.stack([sdf_ref.sdf_grid(vn[:, 0].contiguous(), fr), sdf_ref.sdf_grid(vn[:, 1].contiguous(), fl)], dim=1)
    dev = _dev()
    phi = torch.empty(B, 2, 32, 32, 32, device=dev)
    ws = torch.empty(hip.lib().ihmr_sdf_workspace_bytes(B), dtype=torch.uint8, device=dev)
    fr_d, fl_d, hv_d = fr.to(dev), fl.to(dev), hv.to(dev)  # keep the device buffers alive across the async call
    hip.check(hip.lib().ihmr_sdf_dense_grid(hip.ptr(fr_d), hip.ptr(fl_d), hip.ptr(hv_d), B, hip.ptr(phi),
                                            hip.ptr(ws), hip.stream_ptr()), "dense_grid")
    torch.cuda.synchronize()
    got = phi.cpu()
    n_in_ref, n_in_got = int((ref > 0).sum()), int((got > 0).sum())
    mism = int(((ref > 0) != (got > 0)).sum())
    print(f"[parity] dense grid: inside voxels ref={n_in_ref} got={n_in_got} inside/outside mismatches={mism} "
          f"max|diff|={float((ref - got).abs().max()):.3e}")
    assert mism == 0
    assert torch.equal(ref, got), "phi grid differs from the oracle bit pattern"


def test_sdf_collision_matches_oracle(mano_arrays):
    from ihmr_amd.sdf import SDFLoss
    from oracle.sdf_ref import SDFLossRef
    right, left = mano_arrays
    B = 6
    hv, _ = _two_hand_verts(mano_arrays, B, 5)
    ref_mod = SDFLossRef(right["faces"], left["faces"])
    hv_ref = hv.clone().requires_grad_(True)
    l_ref, pv_ref, os_ref = ref_mod(hv_ref, return_per_vert_loss=True, return_origin_scale_loss=True)
    w = torch.linspace(0.5, 1.5, B)
    (l_ref * w).sum().backward()

    mod = SDFLoss(right["faces"], left["faces"]).to(_dev())
    hv_g = hv.clone().to(_dev()).requires_grad_(True)
    l, pv, os_ = mod(hv_g, return_per_vert_loss=True, return_origin_scale_loss=True)
    (l * w.to(_dev())).sum().backward()
    print("[parity] collision loss per sample (ref):", l_ref.detach().numpy().round(4))
    assert int((pv_ref > 0).sum()) > 50, "test batch must actually penetrate"
    # phi is bit-exact; the trilinear blend differs only by summation order: 1e-6 of a O(0.1) value
    _report("sdf per_vert", pv.detach().cpu(), pv_ref.detach(), atol=1e-6)
    _report("sdf origin_scale [m]", os_.detach().cpu(), os_ref.detach(), atol=1e-7)
    _report("sdf loss", l.detach().cpu(), l_ref.detach(), atol=1e-5, rtol=1e-6)
    _report("sdf d/dverts", hv_g.grad.cpu(), hv_ref.grad, atol=1e-4 * float(hv_ref.grad.abs().max()))


@pytest.mark.parametrize("robustifier", [0.05, 1.0])
def test_sdf_collision_robustifier_matches_oracle(mano_arrays, robustifier):
    """The train-time branch of seam B (loss_utils.py:36-38: `SDFLoss(..., robustifier=...)`): per-vertex value
    r^2 / (r^2 + 1), r = phi / robustifier, and its gradient, against the oracle."""
    from ihmr_amd.sdf import SDFLoss
    from oracle.sdf_ref import SDFLossRef
    right, left = mano_arrays
    B = 5
    hv, _ = _two_hand_verts(mano_arrays, B, 11)
    ref_mod = SDFLossRef(right["faces"], left["faces"], robustifier=robustifier)
    hv_ref = hv.clone().requires_grad_(True)
    l_ref, pv_ref, os_ref = ref_mod(hv_ref, return_per_vert_loss=True, return_origin_scale_loss=True)
    w = torch.linspace(0.7, 1.3, B)
    (l_ref * w).sum().backward()
    mod = SDFLoss(right["faces"], left["faces"], robustifier=robustifier).to(_dev())
    hv_g = hv.clone().to(_dev()).requires_grad_(True)
    l, pv, os_ = mod(hv_g, return_per_vert_loss=True, return_origin_scale_loss=True)
    (l * w.to(_dev())).sum().backward()
    assert int((pv_ref > 0).sum()) > 50, "test batch must actually penetrate"
    _report(f"robust {robustifier} per_vert", pv.detach().cpu(), pv_ref.detach(), atol=2e-6, rtol=1e-5)
    _report(f"robust {robustifier} origin_scale", os_.detach().cpu(), os_ref.detach(), atol=2e-7, rtol=1e-5)
    _report(f"robust {robustifier} loss", l.detach().cpu(), l_ref.detach(), atol=1e-5, rtol=1e-5)
    _report(f"robust {robustifier} d/dverts", hv_g.grad.cpu(), hv_ref.grad, atol=1e-4 * float(hv_ref.grad.abs().max()))


def test_sdf_loss_divisor_must_be_positive(mano_arrays):
    from ihmr_amd.sdf import SDFLoss
    right, left = mano_arrays
    for bad in (0.0, -4.0):
        with pytest.raises(ValueError):
            SDFLoss(right["faces"], left["faces"], loss_divisor=bad)


def test_sdf_disjoint_hands_zero(mano_arrays):
    from ihmr_amd.sdf import SDFLoss
    right, left = mano_arrays
    v = torch.tensor(right["v_template"])
    far = v.clone()
    far[:, 0] = -far[:, 0] - 0.5
    hv = torch.stack([v, far])[None].to(_dev())
    l, pv, os_ = SDFLoss(right["faces"], left["faces"]).to(_dev())(hv, return_per_vert_loss=True, return_origin_scale_loss=True)
    assert float(l.abs().max()) == 0.0 and float(pv.abs().max()) == 0.0


# ----------------------------------------------------------------------------------- seam B under deep interpenetration
def _deep_pairs(mano_arrays, geometry, B):
    """The deep batch's initial hand pairs, or ("point cloud") the same with the left hand replaced by a point cloud over the right hand's
    box: the geometries tests/test_collision_geometry_cpu.py shows to reach the second ray-queue window and the long candidate lists."""
    from helpers import DEEP_SEED, POINT_CLOUD_SEED, point_cloud_pairs
    hv, batch = _two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
    return (point_cloud_pairs(hv, POINT_CLOUD_SEED) if geometry == "point cloud" else hv), batch


@pytest.mark.parametrize("geometry,B", [("deep", 8), ("deep", 96), ("point cloud", 8)])
def test_sdf_collision_matches_oracle_under_deep_overlap(mano_arrays, geometry, B):
    """Seam B against the oracle on deeply interpenetrating pairs, with test_sdf_collision_matches_oracle's tolerances.  B = 96 is 192
    hands: more than SDF_PREP_SMALL_MAX_HANDS = 128, so the 512-thread form of the prep kernel runs.  The point cloud needs almost every
    column of the right hand's grid (tens of thousands of ray-queue pairs, many SDF_RAYQ windows), and its own 'mesh' is a tangle of
    long triangles whose ray parity must still be the oracle's bit for bit."""
    from helpers import needed_voxels, ray_queue_pairs
    from ihmr_amd.sdf import SDFLoss
    from oracle.sdf_ref import SDFLossRef
    right, left = mano_arrays
    hv, _ = _deep_pairs(mano_arrays, geometry, B)
    P = ray_queue_pairs(hv, right["faces"], left["faces"], needed_voxels(hv))
    print(f"[parity] {geometry} B={B}: ray-queue pairs per hand max {P.max()}, hands over 3072: {int((P > 3072).sum())} of {P.size}")
    ref_mod = SDFLossRef(right["faces"], left["faces"])
    hv_ref = hv.clone().requires_grad_(True)
    l_ref, pv_ref, os_ref = ref_mod(hv_ref, return_per_vert_loss=True, return_origin_scale_loss=True)
    w = torch.linspace(0.5, 1.5, B)
    (l_ref * w).sum().backward()
    mod = SDFLoss(right["faces"], left["faces"]).to(_dev())
    hv_g = hv.clone().to(_dev()).requires_grad_(True)
    l, pv, os_ = mod(hv_g, return_per_vert_loss=True, return_origin_scale_loss=True)
    (l * w.to(_dev())).sum().backward()
    print(f"[parity] {geometry} B={B}: penetrating vertices (ref) {int((pv_ref > 0).sum())}, mean loss {float(l_ref.detach().mean()):.4f}")
    assert int((pv_ref > 0).sum()) > 300 * B, "the pairs must penetrate deeply"
    _report(f"{geometry} B={B} sdf per_vert", pv.detach().cpu(), pv_ref.detach(), atol=1e-6)
    _report(f"{geometry} B={B} sdf origin_scale [m]", os_.detach().cpu(), os_ref.detach(), atol=1e-7)
    _report(f"{geometry} B={B} sdf loss", l.detach().cpu(), l_ref.detach(), atol=1e-5, rtol=1e-6)
    _report(f"{geometry} B={B} sdf d/dverts", hv_g.grad.cpu(), hv_ref.grad, atol=1e-4 * float(hv_ref.grad.abs().max()))


@pytest.mark.parametrize("B", [64, 96])
def test_sdf_inside_bits_match_the_oracle_grid_under_deep_overlap(mano_arrays, B):
    """The fused loop's collision launch on the deep batch (set_input, init_optimize, forward_losses): the inside-voxel bitmaps it leaves
    in the workspace equal, bit for bit, the oracle's float32 grid > 0 on the voxels the other hand's vertices read (and nothing else),
    computed on the very vertices the launch saw; the boxes equal the oracle's (centre, scale).  B = 96: the 512-thread prep form."""
    from helpers import DEEP_SEED, needed_voxels, oracle_inside
    from ihmr_amd.optimize_model import OptimizeModel
    from oracle.sdf_ref import hand_boxes
    right, left = mano_arrays
    _, batch = _two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
    model = OptimizeModel(_make_opt(B, epoch=2, save_mid_freq=1))
    model.set_input(batch); model.init_optimize(); model.forward_losses()
    torch.cuda.synchronize()
    bits, box = model.sdf_inside_bits()
    hv = torch.stack([model.buf["verts"][0], model.buf["verts"][1]], dim=1).cpu().contiguous()
    want = needed_voxels(hv) & oracle_inside(hv, right["faces"], left["faces"])           # (B,2,k,j,i)
    words = (want.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).reshape(B, 2, 1024)
    words = words.transpose(1, 0, 2)                                                       # (hand, sample, k * 32 + j): bit i
    n_want = int(want.sum())
    n_got = int(sum(bin(int(x)).count("1") for x in bits[bits != 0]))
    n_diff = int(sum(bin(int(x)).count("1") for x in (bits ^ words)[(bits ^ words) != 0]))
    print(f"[parity] deep B={B}: inside voxels read per hand (oracle) {n_want / (2 * B):.1f}, got {n_got / (2 * B):.1f}; voxels that differ {n_diff}")
    assert n_want > 300 * 2 * B
    assert n_diff == 0
    centre, scale = hand_boxes(hv)
    ref_box = torch.cat([centre[:, :, 0, :], scale[:, :, 0, :]], dim=-1).transpose(0, 1).numpy()
    assert np.array_equal(box, ref_box), float(np.abs(box - ref_box).max())


# ----------------------------------------------------------------------------------- seam C (OPT loop)
def _make_opt(B, strategy="opt_default", epoch=4, save_mid_freq=2, model_root=""):
    import types
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root=model_root, strategy=strategy, save_mid_freq=save_mid_freq,
                                 optimizer="adam", opt_epoch=epoch)


def _oracle_and_model(mano_arrays, B, epoch, freq, seed=1234, record=True, fingers=False, overlap=None):
    """fingers: `mano_arrays` is the finger asset -- the product loads the same asset (model_root "synthetic:fingers") and the batch
    comes from the interlocked generator; overlap="deep": the deep-overlap batch."""
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.strategies import make_opt_strategy
    from oracle.opt_ref import OptimizeRef
    right, left = mano_arrays
    _, batch = _two_hand_verts(mano_arrays, B, seed, interlock=fingers, overlap=overlap)
    orc = OptimizeRef(right, left, B, make_opt_strategy(epoch), save_mid_freq=freq, record=record)
    model = OptimizeModel(_make_opt(B, epoch=epoch, save_mid_freq=freq, model_root="synthetic:fingers" if fingers else ""))
    return orc, model, batch


ARBITER_KEYS = (("joints", "pred_joints_3d"), ("right verts", "pred_right_hand_verts"), ("left verts", "pred_left_hand_verts"),
                ("penetration depth", "collision_loss_origin_scale"))


def _f64_arbiter(mano_arrays, B, epoch, freq, batch):
    """The oracle's loop in FLOAT64 (MANO layer, losses, Adam and the voxel grid in double precision; the float32 inputs converted
    exactly) on the same batch: the reference trajectory both float32 implementations are measured against."""
    from ihmr_amd.strategies import make_opt_strategy
    from oracle.opt_ref import OptimizeRef
    right, left = mano_arrays
    arb = OptimizeRef(right, left, B, make_opt_strategy(epoch), save_mid_freq=freq, dtype=torch.float64)
    arb.set_input(batch); arb.init_optimize(); arb.optimize()
    return arb.get_pred_result(), np.stack(arb.selected), arb


def _arbiter_distances(tag, g, r, a, same, max_ratio=None, worst_ratio=None):
    """|hip - f64| and |oracle32 - f64| per key over the samples `same` (every stage picked the same snapshot in all three runs): mean,
    99.9th percentile and maximum of both, printed side by side.  Asserted: the HIP path lies within north_star's 1e-4 of the float64
    trajectory everywhere; `worst_ratio`: max |hip - f64| <= worst_ratio x max |oracle32 - f64| + 2e-6 m per key (the
    round-4 review's criterion: 1.5); `max_ratio`: the same for the MEAN distances (+ 1e-7 m)."""
    out = {}
    for name, key in ARBITER_KEYS:
        e_hip = np.abs(g[key][same].astype(np.float64) - a[key][same]).ravel()
        e_o32 = np.abs(r[key][same].astype(np.float64) - a[key][same]).ravel()
        st = lambda e: (float(e.mean()), float(np.percentile(e, 99.9)), float(e.max()))
        out[name] = (st(e_hip), st(e_o32))
        print(f"[parity] {tag} {name} [m]: |hip - f64| mean {out[name][0][0]:.3e} p99.9 {out[name][0][1]:.3e} max {out[name][0][2]:.3e};  "
              f"|oracle32 - f64| mean {out[name][1][0]:.3e} p99.9 {out[name][1][1]:.3e} max {out[name][1][2]:.3e}  "
              f"(ratios {out[name][0][0] / max(out[name][1][0], 1e-30):.2f} / {out[name][0][1] / max(out[name][1][1], 1e-30):.2f} / "
              f"{out[name][0][2] / max(out[name][1][2], 1e-30):.2f})")
    for name, (h, o) in out.items():
        assert h[2] <= 1e-4, (tag, name, "hip", h)          # (the float32 oracle's own distance is printed, not asserted: it is the checker)
        if worst_ratio is not None:
            assert h[2] <= worst_ratio * o[2] + 2e-6, (tag, name, "max distance from the float64 trajectory", h[2], o[2])
        if max_ratio is not None:
            assert h[0] <= max_ratio * o[0] + 1e-7, (tag, name, "mean distance from the float64 trajectory", h[0], o[0])
    return out


def test_opt_forward_losses_match_oracle(mano_arrays):
    B = 4
    orc, model, batch = _oracle_and_model(mano_arrays, B, 2, 1)
    orc.set_input(batch); orc.init_optimize(); orc.forward(); orc.compute_loss(orc.default_loss_weights)
    model.set_input(batch); model.init_optimize(); model.forward_losses()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    _report("fwd right verts", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=2e-6)
    _report("fwd left verts", g["pred_left_hand_verts"], r["pred_left_hand_verts"], atol=2e-6)
    _report("fwd joints_3d (aligned)", g["pred_joints_3d"], r["pred_joints_3d"], atol=2e-6)
    _report("fwd joints_2d", model.pred_joints_2d.cpu(), orc.pred_joints_2d.detach(), atol=2e-5)
    _report("collision_loss_batch", g["collision_loss"], r["collision_loss"], atol=1e-5, rtol=1e-5)
    _report("collision origin scale", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-6)
    _report("joints_3d_loss_p_batch", model.joints_3d_loss_p_batch.cpu(), orc.joints_3d_loss_p_batch.detach(), atol=1e-6, rtol=1e-4)
    _report("finger_reg_batch", model.buf["loss_batch"][3].cpu(), orc.finger_reg_loss_batch.detach(), atol=1e-9, rtol=1e-3)
    print("[parity] MPJPE-style joint delta (mm):", float(np.abs(g["pred_joints_3d"] - r["pred_joints_3d"]).max() * 1000))


@pytest.mark.parametrize("stage_id", [0, 1, 2, 3])
def test_opt_single_step_gradients(mano_arrays, stage_id):
    """One iteration of one stage from identical state: Adam's first moment after step 1 is
    0.1 * grad, so the analytic HIP gradient of the WHOLE loss is compared with autograd."""
    from ihmr_amd.strategies import make_opt_strategy
    B = 4
    orc, model, batch = _oracle_and_model(mano_arrays, B, 0, 1)
    stage = make_opt_strategy(0)[stage_id]
    orc.strategy = [stage]
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.run_stage(stage)
    torch.cuda.synchronize()
    grads = orc.trace[0]["grads"]
    names = sorted(stage["update_params"])  # left first, then right (or trans)
    m = model.buf["adam_m"].cpu().numpy() / 0.1
    from ihmr_amd.hip import PARAM_BLOCKS
    got = {n: m[:, PARAM_BLOCKS[n][1]:PARAM_BLOCKS[n][1] + PARAM_BLOCKS[n][2]].reshape(grads[n].shape) for n in names}
    for n in names:
        ref = grads[n]
        scale = float(np.abs(ref).max())
        _report(f"stage{stage_id} dL/d{n}", got[n], ref, atol=3e-4 * scale)


def test_opt_trajectory_matches_oracle(mano_arrays):
    """Full 4-stage refinement (5 iterations per stage, snapshot every 2): snapshots, selection indices
    and exported results against the CPU oracle.  Adam normalises gradients, so per-step parameter
    differences stay at fp32 round-off x lr; bars: parameters 2e-4 (lr 1e-2, 5 steps), vertices 1e-4 m,
    per-vertex penetration depth 1e-4 m (BASELINE.json tolerance)."""
    B, epoch, freq = 4, 4, 2
    orc, model, batch = _oracle_and_model(mano_arrays, B, epoch, freq)
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    sel_ref = np.stack(orc.selected)
    sel_got = torch.stack(model.selected_history).cpu().numpy()
    agree = float((sel_ref == sel_got).mean())
    print(f"[parity] selection indices ref={sel_ref.tolist()} got={sel_got.tolist()} agreement={agree:.2f}")
    assert agree == 1.0
    _report("traj pose", g["pred_pose_params"], r["pred_pose_params"], atol=2e-4)
    _report("traj shape", g["pred_shape_params"], r["pred_shape_params"], atol=2e-4)
    _report("traj trans", g["pred_hand_trans"], r["pred_hand_trans"], atol=2e-5)
    _report("traj right verts [m]", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=1e-4)
    _report("traj left verts [m]", g["pred_left_hand_verts"], r["pred_left_hand_verts"], atol=1e-4)
    _report("traj joints [m]", g["pred_joints_3d"], r["pred_joints_3d"], atol=1e-4)
    _report("traj penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)
    mean_pen_ref = float(r["collision_loss_origin_scale"].mean())
    mean_pen_got = float(g["collision_loss_origin_scale"].mean())
    print(f"[parity] mean penetration depth ref={mean_pen_ref:.6e} got={mean_pen_got:.6e}")
    assert abs(mean_pen_ref - mean_pen_got) < 1e-4


def test_opt_fused_batches_are_bit_identical(mano_arrays):
    """``opt.fuse_batches = 2``: one launch sequence over two batches gives, sample for sample, the bits of two
    separate batch-size calls (the batch-mean factors come from ``ihmr_opt_io.norm_batch``, nothing else couples
    samples) -- parameters, meshes, losses and the snapshot selection."""
    from ihmr_amd.optimize_model import OptimizeModel
    B, epoch, freq = 8, 3, 2
    _, b1 = _two_hand_verts(mano_arrays, B, 11)
    _, b2 = _two_hand_verts(mano_arrays, B, 12)
    single = OptimizeModel(_make_opt(B, epoch=epoch, save_mid_freq=freq))
    outs = []
    for bt in (b1, b2):
        single.set_input(bt); single.init_optimize(); single.optimize()
        torch.cuda.synchronize()
        outs.append((single.get_pred_result(), torch.stack(single.selected_history).cpu().numpy()))
    opt = _make_opt(B, epoch=epoch, save_mid_freq=freq)
    opt.fuse_batches = 2
    fused = OptimizeModel(opt)
    both = {k: torch.cat([b1[k], b2[k]], dim=0) for k in b1}
    fused.set_input(both); fused.init_optimize(); fused.optimize()
    torch.cuda.synchronize()
    got, sel = fused.get_pred_result(), torch.stack(fused.selected_history).cpu().numpy()
    for i, (ref, sel_ref) in enumerate(outs):
        sl = slice(i * B, (i + 1) * B)
        assert np.array_equal(sel[:, sl], sel_ref)
        for k in ("pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
                  "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
            assert np.array_equal(got[k][sl], ref[k]), f"{k} of batch {i} differs between the fused and the separate run"


def test_opt_replay_is_deterministic(mano_arrays):
    """A model instance is reused batch after batch (``src/optimize.py`` loop): later passes replay the cached stage
    graphs on the same (default) stream and must reproduce the first pass bit for bit -- and so must a second
    instance.  Batch 64 x 40 iterations on purpose: a lost update between two threads of the chain backward once
    made the shape stage differ from run to run, and it only showed at this size."""
    from ihmr_amd.optimize_model import OptimizeModel
    B = 64
    _, batch = _two_hand_verts(mano_arrays, B, 21)
    models = [OptimizeModel(_make_opt(B, epoch=9, save_mid_freq=5)) for _ in range(2)]
    outs = []
    for r in range(5):
        model = models[r // 4]
        model.set_input(batch); model.init_optimize(); model.optimize()
        torch.cuda.synchronize()
        outs.append(model.get_pred_result())
    for k in ("pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "collision_loss_origin_scale"):
        for o in outs[1:]:
            assert np.array_equal(outs[0][k], o[k]), k


def test_async_export_equals_blocking_export(mano_arrays):
    """get_pred_result_async().wait() hands out exactly what get_pred_result() does (same keys, dtypes, bits)."""
    from ihmr_amd.optimize_model import OptimizeModel
    B = 4
    _, batch = _two_hand_verts(mano_arrays, B, 31)
    model = OptimizeModel(_make_opt(B, epoch=2, save_mid_freq=1))
    model.set_input(batch); model.init_optimize(); model.optimize()
    h = model.get_pred_result_async()
    ref = model.get_pred_result()
    got = h.wait()
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("B", [1, 9, 33])
def test_opt_odd_batch_sizes_match_oracle(mano_arrays, B):
    """Batch sizes that are no multiple of the 8-hand skinning groups, of the 32-hand MFMA tiles of the pose-gradient
    GEMM (2B = 2, 18, 66 hands) or of the XCD count: two iterations of every stage against the oracle."""
    orc, model, batch = _oracle_and_model(mano_arrays, B, 1, 1, seed=100 + B)
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    assert np.array_equal(np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy())
    _report(f"B={B} pose", g["pred_pose_params"], r["pred_pose_params"], atol=1e-4)
    _report(f"B={B} shape", g["pred_shape_params"], r["pred_shape_params"], atol=1e-4)
    _report(f"B={B} verts [m]", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=1e-4)
    _report(f"B={B} penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)


def test_opt_200_iterations_match_oracle(mano_arrays):
    """The benchmark schedule itself (opt_default, epoch = 49: 4 x 50 = 200 refinement iterations, snapshots every 10)
    on 6 samples against the oracle: selection indices, parameters and the BASELINE.json parity figures -- mean
    penetration depth to 1e-4 (metres) and MPJPE-style joint positions to 1e-4."""
    B = 6
    orc, model, batch = _oracle_and_model(mano_arrays, B, 49, 10, seed=4242, record=False)
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    sel_ref, sel_got = np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy()
    print(f"[parity] 200 iterations: selection ref={sel_ref.tolist()} got={sel_got.tolist()}")
    assert np.array_equal(sel_ref, sel_got)
    _report("200it pose", g["pred_pose_params"], r["pred_pose_params"], atol=1e-3)
    # shape coefficients whose gradient is at round-off level take steps of +-lr under Adam (m / sqrt(v) = +-1 whatever the
    # magnitude): after 50 steps at lr 1e-2 they may differ by a few 1e-3 without moving the mesh (checked below to 1e-4 m)
    _report("200it shape", g["pred_shape_params"], r["pred_shape_params"], atol=1e-2)
    _report("200it joints [m]", g["pred_joints_3d"], r["pred_joints_3d"], atol=1e-4)
    _report("200it right verts [m]", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=1e-4)
    _report("200it penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)
    mp_ref, mp_got = float(r["collision_loss_origin_scale"].mean()), float(g["collision_loss_origin_scale"].mean())
    print(f"[parity] 200 iterations: mean penetration depth ref={mp_ref:.6e} got={mp_got:.6e}")
    assert abs(mp_ref - mp_got) < 1e-4


def test_lbs_backward_with_dense_skinning_weights(mano_arrays):
    """A weight matrix without zeros (every vertex bound to all 16 bones): ~960 dA segments, i.e. 46 KB of dynamic LDS
    on top of the static 36 KB of lbs_bwd1 -- beyond the default per-workgroup limit, the library has to raise it.
    Gradients against autograd through the oracle."""
    from ihmr_amd import mano
    from oracle.mano_ref import ManoRef
    right = dict(mano_arrays[0])
    rng = np.random.RandomState(5)
    w = np.abs(rng.rand(778, 16)).astype(np.float32) * 0.02 + right["lbs_weights"]
    right["lbs_weights"] = (w / w.sum(1, keepdims=True)).astype(np.float32)
    N = 3
    g = torch.Generator().manual_seed(9)
    o, p, b = (torch.randn(N, 3, generator=g) * 0.3), (torch.randn(N, 45, generator=g) * 0.2), torch.randn(N, 10, generator=g) * 0.5
    wv, wj = torch.randn(N, 778, 3, generator=g), torch.randn(N, 16, 3, generator=g)

    def run(mod, dev):
        oo, pp, bb = (t.clone().to(dev).requires_grad_(True) for t in (o, p, b))
        out = mod(global_orient=oo, hand_pose=pp, betas=bb)
        ((out.vertices * wv.to(dev)).sum() + (out.joints * wj.to(dev)).sum()).backward()
        return out.vertices.detach().cpu(), [t.grad.cpu() for t in (oo, pp, bb)]

    v_ref, g_ref = run(ManoRef(right), "cpu")
    v_got, g_got = run(mano.MANO(right).to(_dev()), _dev())
    _report("dense-weights verts", v_got, v_ref, atol=2e-6)
    for name, a, r in zip(("orient", "pose", "betas"), g_got, g_ref):
        _report(f"dense-weights d{name}", a, r, atol=3e-5 * float(r.abs().max()))


# ----------------------------------------------------------------------------------- seam C vs the REFERENCE's own runs
import os.path as _osp

_GOLD = _osp.join(_osp.dirname(_osp.abspath(__file__)), "golden")


def _gold(name):
    return dict(np.load(_osp.join(_GOLD, name), allow_pickle=False))


def _run_golden_batch(g, strategy, optimizer="adam"):
    """HIP OptimizeModel over the `in_*` batch of a reference-generated fixture."""
    from ihmr_amd.optimize_model import OptimizeModel
    epoch, freq = (int(x) for x in g["meta_epoch_freq"])
    batch = {k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}
    B = batch["init_cam"].shape[0]
    opt = _make_opt(B, epoch=epoch, save_mid_freq=freq)
    opt.optimizer = optimizer
    model = OptimizeModel(opt)
    if strategy is not None:
        model.strategy = strategy(epoch)
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    return model, model.get_pred_result()


def _check_against_reference(tag, model, got, g, prefix=""):
    """Every key the reference's get_pred_result() exported (tolerances: parameters 2e-4 -- Adam steps of lr 1e-2 are
    sign-like, so round-off in a gradient moves a parameter by lr x 1e-3 at most; metres 1e-4 = BASELINE.json's bar;
    integer keys exact)."""
    tol = dict(pred_cam_params=1e-6, pred_hand_trans=2e-5, pred_shape_params=2e-4, pred_pose_params=2e-4, pred_right_hand_verts=1e-4,
               pred_left_hand_verts=1e-4, mano_params_weight=0, pred_joints_3d=1e-4, gt_joints_3d=0, collision_loss_origin_scale=1e-4)
    for k, v in got.items():
        key = f"{prefix}out_{k}"
        if key not in g:
            continue
        if v.dtype.kind == "i":
            assert np.array_equal(v, g[key]), k
        elif k == "collision_loss":
            _report(f"{tag} {k}", v, g[key], atol=2e-4, rtol=1e-3)
        else:
            _report(f"{tag} {k}", v, g[key], atol=tol[k])
    _report(f"{tag} joints_2d", model.pred_joints_2d.cpu(), g[f"{prefix}out_pred_joints_2d"], atol=1e-3)
    _report(f"{tag} joints_3d_loss_p_batch", model.joints_3d_loss_p_batch.cpu(), g[f"{prefix}out_joints_3d_loss_p_batch"], atol=1e-5, rtol=1e-3)
    _report(f"{tag} joints_2d_loss_p_batch", model.joints_2d_loss_p_batch.cpu(), g[f"{prefix}out_joints_2d_loss_p_batch"], atol=1e-5, rtol=1e-3)


def test_opt_replays_reference_trajectory():
    """tests/golden/opt_traj.npz = the REFERENCE's own OptimizeModel.optimize() (B=3, 4 x 4 iterations, a sample without
    right wrist): the HIP OptimizeModel on the same inputs against the reference's exported results, directly."""
    g = _gold("opt_traj.npz")
    model, got = _run_golden_batch(g, None)
    _check_against_reference("ref-traj", model, got, g)


def test_mesh_export_of_device_result_matches_reference_save_pred_obj(tmp_path):
    """SURVEY 8(f)4.  The reference's own ``save_pred_obj`` (utils/opt_utils.py:45-54) run on the reference's own refinement of
    the opt_traj.npz batch recorded what it hands to the OBJ writer (tests/golden/evaluator.npz: obj_*).  Here the HIP
    OptimizeModel refines the same batch on the device, the result is exported and written by this build's writer, and the FILE is
    read back: the file name and every face index are identical integers (combined index = concat(faces_r, faces_l + 778),
    1-based in the file), the vertices equal the exported device meshes to the writer's print precision and the reference's
    vertices within the trajectory tolerance; the Evaluator stores the same meshes as float16 (evaluator.py:66-72)."""
    import os.path as osp
    from ihmr_amd import ry_utils
    from ihmr_amd.evaluator import Evaluator
    g, ge = _gold("opt_traj.npz"), _gold("evaluator.npz")
    model, got = _run_golden_batch(g, None)
    path = ry_utils.save_pred_obj(str(tmp_path), got, model.mano_models, 7, 2, 30)
    assert osp.basename(path) == osp.basename(str(ge["obj_path"]))
    v, f = [], []
    for line in open(path):
        t = line.split()
        (v if t[0] == "v" else f).append([float(x) if t[0] == "v" else int(x) for x in t[1:]])
    v, f = np.array(v), np.array(f, dtype=np.int64)
    assert np.array_equal(f - 1, ge["obj_faces"]), "combined face index differs from the reference's"
    assert np.array_equal(f[:1538] - 1, np.asarray(model.mano_models["right"].faces)) and f.min() == 1 and f.max() == 1556
    mine = np.concatenate([got["pred_right_hand_verts"][0], got["pred_left_hand_verts"][0]], 0)
    _report("OBJ vertices vs the exported device meshes", v, mine, atol=5.01e-7)
    _report("OBJ vertices vs the reference's export", v, ge["obj_verts"], atol=1e-4)
    ev = Evaluator(model.mano_models)
    ev.update(np.arange(got["pred_cam_params"].shape[0]), got, save_verts=True)
    rec = ev.pred_results[0]
    assert rec["pred_right_hand_verts"].dtype == np.float16
    assert np.array_equal(rec["pred_right_hand_verts"], got["pred_right_hand_verts"][0].astype(np.float16))
    assert np.array_equal(rec["pred_left_hand_verts"], got["pred_left_hand_verts"][0].astype(np.float16))
    assert np.abs(rec["pred_left_hand_verts"].astype(np.float32) - g["out_pred_left_hand_verts"][0]).max() < 1e-4 + 2.5e-4   # fp16 spacing at 0.25 m


def test_opt_replays_reference_ragged_trajectory():
    """tests/golden/opt_traj_ragged.npz = the reference's own run on the ragged batch of tests/helpers.py:ragged_opt_batch
    (single-hand samples -> collision mask 0, right wrist missing -> root = joint 21, half weights -> no alignment,
    zero-weight joints, no 3-D target, separated hands)."""
    g = _gold("opt_traj_ragged.npz")
    model, got = _run_golden_batch(g, None)
    _check_against_reference("ref-ragged", model, got, g)
    ht = g["in_hand_type_array"]
    single = ht.sum(1) < 1.5
    assert single.sum() == 2 and np.all(got["collision_loss"][single] == 0.0)
    assert np.abs(got["collision_loss_origin_scale"][single]).max() > 0     # per-vertex depths stay unmasked (loss_utils.py:189)
    assert got["collision_loss"][7] == 0.0 and np.abs(got["collision_loss_origin_scale"][7]).max() == 0.0


@pytest.mark.parametrize("tag,optimizer", [("crit", "adam"), ("sgd", "sgd")])
def test_opt_replays_reference_variants(tag, optimizer):
    """tests/golden/opt_traj_variants.npz: the reference's run with (crit) filter / select criteria its default strategy
    does not use -- joints_2d_loss_p as filter and as select loss, collision_loss as select loss, ONE filter only (the
    other loss must not be compared at all: sample 2 has origin collision loss 0), two criteria on one loss -- and
    (sgd) torch.optim.SGD(momentum 0.9) instead of Adam."""
    from helpers import variant_strategy
    from ihmr_amd.strategies import make_opt_strategy
    g = _gold("opt_traj_variants.npz")
    model, got = _run_golden_batch(g, variant_strategy if tag == "crit" else make_opt_strategy, optimizer)
    _check_against_reference(f"ref-{tag}", model, got, g, prefix=f"{tag}_")


# ----------------------------------------------------------------------------------- seam C, ragged batch vs the oracle
def _ragged_oracle_and_model(mano_arrays, B, epoch, freq, seed=777):
    from helpers import ragged_opt_batch
    orc, model, batch = _oracle_and_model(mano_arrays, B, epoch, freq, seed=seed)
    return orc, model, ragged_opt_batch(batch)


def test_opt_ragged_forward_losses_match_oracle(mano_arrays):
    B = 9
    orc, model, batch = _ragged_oracle_and_model(mano_arrays, B, 2, 1)
    orc.set_input(batch); orc.init_optimize(); orc.forward(); orc.compute_loss(orc.default_loss_weights)
    model.set_input(batch); model.init_optimize(); model.forward_losses()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    _report("ragged joints_3d (aligned)", g["pred_joints_3d"], r["pred_joints_3d"], atol=2e-6)
    _report("ragged collision_loss_batch", g["collision_loss"], r["collision_loss"], atol=1e-5, rtol=1e-5)
    _report("ragged collision origin scale", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-6)
    _report("ragged joints_3d_loss_p_batch", model.joints_3d_loss_p_batch.cpu(), orc.joints_3d_loss_p_batch.detach(), atol=1e-6, rtol=1e-4)
    _report("ragged joints_2d_loss_p_batch", model.joints_2d_loss_p_batch.cpu(), orc.joints_2d_loss_p_batch.detach(), atol=1e-6, rtol=1e-4)
    _report("ragged finger_reg_batch", model.buf["loss_batch"][3].cpu(), orc.finger_reg_loss_batch.detach(), atol=1e-9, rtol=1e-3)
    lb = model.buf["loss_batch"].cpu().numpy()
    # the GT-side losses the reference prints (optimize_model.py:279-281,291-293,305-307): batch means of rows 4, 5, 7
    _report("ragged gt joints_2d_loss", lb[4].mean(), float(orc.joints_2d_loss), atol=1e-6, rtol=1e-5)
    _report("ragged gt joints_3d_loss", lb[5].mean() * 1000, float(orc.joints_3d_loss), atol=1e-6, rtol=1e-4)
    _report("ragged gt hand_trans_loss", lb[7].mean() * 10, float(orc.hand_trans_loss), atol=1e-7, rtol=1e-4)
    assert g["collision_loss"][1] == 0 and g["collision_loss"][2] == 0 and g["collision_loss"][7] == 0 and g["collision_loss"][0] > 0


_MIXED_STAGE = dict(update_params=["pred_cam_params", "pred_hand_trans", "pred_left_orient", "pred_right_shape_params"],
                    loss_weights=dict(joints_2d_loss=10.0, joints_3d_loss=1000.0, trans_loss_weight=100.0, shape_reg_loss_weight=0.1,
                                      collision_loss_weight=1.0, finger_reg_loss_weight=0.0),
                    lr=2e-4, epoch=0, filter_loss=[("joints_3d_loss_p", "+0")], select_loss="joints_3d_loss_p")


@pytest.mark.parametrize("stage_id", [0, 1, 2, 3, "mixed"])
def test_opt_ragged_single_step_gradients(mano_arrays, stage_id):
    """Whole-loss gradients on the ragged batch (root = joint 21 / no alignment / masked collision / zero weights all
    back-propagate differently), every default stage + a stage over a mixed parameter set the default strategy never
    uses (camera + translation + one hand's orientation + one hand's shape)."""
    from ihmr_amd.hip import PARAM_BLOCKS
    from ihmr_amd.strategies import make_opt_strategy
    B = 8
    orc, model, batch = _ragged_oracle_and_model(mano_arrays, B, 0, 1)
    stage = dict(_MIXED_STAGE) if stage_id == "mixed" else make_opt_strategy(0)[stage_id]
    orc.strategy = [stage]
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.run_stage(stage)
    torch.cuda.synchronize()
    grads = orc.trace[0]["grads"]
    m = model.buf["adam_m"].cpu().numpy() / 0.1
    for n in stage["update_params"]:
        lo, size = PARAM_BLOCKS[n][1], PARAM_BLOCKS[n][2]
        ref = grads[n]
        _report(f"ragged stage {stage_id} dL/d{n}", m[:, lo:lo + size].reshape(ref.shape), ref, atol=3e-4 * float(np.abs(ref).max()))
    untouched = np.ones(122, bool)
    for n in stage["update_params"]:
        untouched[PARAM_BLOCKS[n][1]:PARAM_BLOCKS[n][1] + PARAM_BLOCKS[n][2]] = False
    assert np.all(m[:, untouched] == 0), "optimizer state of parameters outside update_params must stay untouched"


def test_opt_mixed_parameter_stage_trajectory(mano_arrays):
    """A 6-iteration stage over the mixed parameter set, then a default stage: parameters (incl. the camera) against
    the oracle.  (No finger regulariser in the mixed stage: it is invariant to translation and rotation, so for the
    single-hand samples -- whose other gradient terms are exactly zero -- it leaves a pure round-off gradient on
    pred_hand_trans / pred_left_orient, which Adam turns into +-lr steps in the reference and here alike, in
    directions that are noise.)"""
    from ihmr_amd.strategies import make_opt_strategy
    B = 8
    orc, model, batch = _ragged_oracle_and_model(mano_arrays, B, 5, 2, seed=31)
    strategy = [dict(_MIXED_STAGE, epoch=5), make_opt_strategy(5)[2]]
    orc.strategy = strategy
    model.strategy = strategy
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    assert np.array_equal(np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy())
    assert np.abs(r["pred_cam_params"] - batch["init_cam"].numpy()).max() > 1e-4, "the camera must have moved"
    # the 2-D term is an L1 loss: its gradient jumps when a projected joint crosses its target, so a round-off difference
    # can change one Adam step of the parameters it drives (camera, translation) by a fraction of lr = 2e-4
    _report("mixed cam", g["pred_cam_params"], r["pred_cam_params"], atol=1e-4)
    _report("mixed trans", g["pred_hand_trans"], r["pred_hand_trans"], atol=1e-4)
    _report("mixed pose", g["pred_pose_params"], r["pred_pose_params"], atol=2e-4)
    _report("mixed shape", g["pred_shape_params"], r["pred_shape_params"], atol=2e-4)
    _report("mixed joints [m]", g["pred_joints_3d"], r["pred_joints_3d"], atol=1e-4)
    _report("mixed penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)


# ----------------------------------------------------------------------------------- BASELINE.json's batch size
def test_opt_batch64_matches_oracle(mano_arrays):
    """IHMR-OPT at the benchmark's batch size (64 samples = 128 hands: the launch shapes the bench line is measured
    with), 4 stages x 5 iterations, snapshot every 2, against the oracle."""
    _batch64_trajectory(mano_arrays, fingers=False)


def test_opt_batch64_matches_oracle_on_the_finger_asset(finger_arrays):
    """The same trajectory test on the five-finger mesh with interlocked hands (round 5: the geometry the blob cannot show -- thin
    penetration volumes between fingers, long candidate lists, more refused voxels)."""
    _batch64_trajectory(finger_arrays, fingers=True)


def test_opt_batch64_matches_oracle_under_deep_overlap(mano_arrays):
    """The same trajectory test on the deep-overlap batch (tests/test_collision_geometry_cpu.py: ~4 x the default batch's inside voxels
    per hand, hands past the first ray-queue window), same keys and tolerances.  The selections must be the oracle's; a flip is only
    accepted where the float64 arbiter explains it (the headline test's rule: at most 2 more disagreements with the float64 run than the
    float32 oracle has), and the samples that flipped are left out of the element-wise comparison.  The batch must stay deep: its mean
    penetration depth after the schedule is several times the default batch's under the same schedule."""
    from helpers import DEEP_SEED
    from ihmr_amd.optimize_model import OptimizeModel
    B, epoch, freq = 64, 4, 2
    orc, model, batch = _oracle_and_model(mano_arrays, B, epoch, freq, seed=DEEP_SEED, record=False, overlap="deep")
    torch.set_num_threads(max(1, min(32, (__import__("os").cpu_count() or 8))))
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    sel_ref, sel_got = np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy()
    same = np.all(sel_ref == sel_got, axis=0)
    print(f"[parity] deep B=64: selection agreement {float((sel_ref == sel_got).mean()):.4f} ({int((~same).sum())} samples differ)")
    if not same.all():
        _, sel_f64, _ = _f64_arbiter(mano_arrays, B, epoch, freq, batch)
        print(f"[parity] deep B=64 arbiter: hip vs f64 differ at {int((sel_got != sel_f64).sum())}, oracle32 vs f64 at "
              f"{int((sel_ref != sel_f64).sum())} of {sel_f64.size} (stage, sample) pairs")
        assert (sel_got != sel_f64).sum() <= (sel_ref != sel_f64).sum() + 2
    assert same.sum() >= B - 4
    _report("deep B=64 pose", g["pred_pose_params"][same], r["pred_pose_params"][same], atol=2e-4)
    _report("deep B=64 shape", g["pred_shape_params"][same], r["pred_shape_params"][same], atol=2e-4)
    _report("deep B=64 trans", g["pred_hand_trans"][same], r["pred_hand_trans"][same], atol=2e-5)
    _report("deep B=64 right verts [m]", g["pred_right_hand_verts"][same], r["pred_right_hand_verts"][same], atol=1e-4)
    _report("deep B=64 left verts [m]", g["pred_left_hand_verts"][same], r["pred_left_hand_verts"][same], atol=1e-4)
    _report("deep B=64 joints [m]", g["pred_joints_3d"][same], r["pred_joints_3d"][same], atol=1e-4)
    _report("deep B=64 penetration depth [m]", g["collision_loss_origin_scale"][same], r["collision_loss_origin_scale"][same], atol=1e-4)
    _report("deep B=64 collision_loss", g["collision_loss"][same], r["collision_loss"][same], atol=2e-4, rtol=1e-3)
    _, shallow = _two_hand_verts(mano_arrays, B, 6464)            # (the default batch of test_opt_batch64_matches_oracle)
    m2 = OptimizeModel(_make_opt(B, epoch=epoch, save_mid_freq=freq))
    m2.set_input(shallow); m2.init_optimize(); m2.optimize()
    torch.cuda.synchronize()
    deep_pen, shallow_pen = float(r["collision_loss_origin_scale"].mean()), float(m2.get_pred_result()["collision_loss_origin_scale"].mean())
    print(f"[parity] mean penetration depth after 4 x 5 iterations: deep batch {deep_pen:.3e} m, default batch {shallow_pen:.3e} m")
    assert deep_pen >= 3 * shallow_pen          # (oracle: 1.0e-3 against 2.2e-4 m)


def _batch64_trajectory(mano_arrays, fingers):
    B, epoch, freq = 64, 4, 2
    orc, model, batch = _oracle_and_model(mano_arrays, B, epoch, freq, seed=6464, record=False, fingers=fingers)
    torch.set_num_threads(max(1, min(32, (__import__("os").cpu_count() or 8))))
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    sel_ref, sel_got = np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy()
    print(f"[parity] B=64: selection agreement {float((sel_ref == sel_got).mean()):.4f}")
    assert np.array_equal(sel_ref, sel_got)
    _report("B=64 pose", g["pred_pose_params"], r["pred_pose_params"], atol=2e-4)
    _report("B=64 shape", g["pred_shape_params"], r["pred_shape_params"], atol=2e-4)
    _report("B=64 trans", g["pred_hand_trans"], r["pred_hand_trans"], atol=2e-5)
    _report("B=64 right verts [m]", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=1e-4)
    _report("B=64 left verts [m]", g["pred_left_hand_verts"], r["pred_left_hand_verts"], atol=1e-4)
    _report("B=64 joints [m]", g["pred_joints_3d"], r["pred_joints_3d"], atol=1e-4)
    _report("B=64 penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)
    _report("B=64 collision_loss", g["collision_loss"], r["collision_loss"], atol=2e-4, rtol=1e-3)


@pytest.mark.slow
def test_opt_headline_workload_matches_oracle(mano_arrays):
    """BASELINE.json's metric config itself -- IHMR-OPT, batch 64, opt_default at epoch 49 = 4 x 50 = 200 refinement iterations,
    snapshot every 10 (what bench.py times) -- against the oracle (minutes of CPU time): selection indices identical; the metrics
    north_star names (MPJPE, mean per-vertex distance, mean penetration depth) within 1e-4, and every element within 1e-4 (round 5;
    3e-4 before).  A float64 ARBITER -- the same loop in double precision -- says how far each float32 implementation is from the
    exact trajectory: the HIP path at most 1.5 x as far as torch's float32 per key (measured: 0.03-0.5 x)."""
    B, epoch, freq = 64, 49, 10
    orc, model, batch = _oracle_and_model(mano_arrays, B, epoch, freq, seed=1234, record=False)
    torch.set_num_threads(max(1, min(32, (__import__("os").cpu_count() or 8))))
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    sel_ref, sel_got = np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy()
    print(f"[parity] headline: selection agreement {float((sel_ref == sel_got).mean()):.4f}")
    assert np.array_equal(sel_ref, sel_got)
    # north_star's bar (MPJPE / MPVPE / penetration depth within 1e-4) holds ELEMENT BY ELEMENT since round 5: 200 Adam steps amplify
    # summation-order rounding (the update m / sqrt(v) is scale-free), and rounds 1-4 measured a worst vertex of 1.2e-4 m against the
    # float32 oracle (bar: 3e-4 with 99.9 % within 1e-4); with the skinning kernel's blend offsets summed from zero the worst vertex is
    # 3.6e-5 m, the worst joint 2.9e-5 m -- most of which is the float32 ORACLE's own distance from the exact trajectory (arbiter below).
    worst = {}
    for name, key in (("joints", "pred_joints_3d"), ("right verts", "pred_right_hand_verts"), ("left verts", "pred_left_hand_verts"),
                      ("penetration depth", "collision_loss_origin_scale")):
        e = np.abs(g[key].astype(np.float64) - r[key].astype(np.float64))
        worst[name] = float(e.max())
        frac = float((e <= 1e-4).mean())
        print(f"[parity] headline {name} [m]: max|err|={e.max():.3e}, within 1e-4: {100 * frac:.4f} %")
        assert e.max() <= 1e-4, name
    mp_ref, mp_got = float(r["collision_loss_origin_scale"].mean()), float(g["collision_loss_origin_scale"].mean())
    mpjpe = lambda x: float(np.linalg.norm(x["pred_joints_3d"] - x["gt_joints_3d"][..., :3], axis=-1).mean())
    mpvpe = float(np.mean([np.linalg.norm(g[k] - r[k], axis=-1).mean() for k in ("pred_right_hand_verts", "pred_left_hand_verts")]))
    print(f"[parity] headline: mean penetration depth ref={mp_ref:.6e} got={mp_got:.6e}; MPJPE ref={mpjpe(r):.6e} got={mpjpe(g):.6e}; "
          f"mean per-vertex distance HIP vs oracle {mpvpe:.3e}")
    assert abs(mp_ref - mp_got) < 1e-4 and abs(mpjpe(r) - mpjpe(g)) < 1e-4 and mpvpe < 1e-4
    # ---- the arbiter: who is how far from the float64 trajectory?
    a, sel_f64, _ = _f64_arbiter(mano_arrays, B, epoch, freq, batch)
    same = np.all(sel_f64 == sel_ref, axis=0) & np.all(sel_f64 == sel_got, axis=0)
    print(f"[parity] headline arbiter: selections of all three runs agree on {int(same.sum())} of {B} samples "
          f"(hip vs f64 differ at {int((sel_got != sel_f64).sum())}, oracle32 vs f64 at {int((sel_ref != sel_f64).sum())} of {sel_f64.size} (stage, sample) pairs)")
    assert same.sum() >= B - 4 and (sel_got != sel_f64).sum() <= (sel_ref != sel_f64).sum() + 2
    # Round 5 history: the first arbiter run found the HIP path 2.2-2.8 x (mean) and up to 6 x (99.9th percentile) as far from the float64
    # trajectory as torch's float32 (worst vertex 1.17e-4 m) -- the skinning kernel ran its 145 blend-shape FMAs onto a running VERTEX,
    # rounding at the vertex's magnitude each time (scripts/experiments/gradient_error_vs_f64.py: forward 2.9 x torch's error).  With the
    # offsets summed from zero (csrc/mano_lbs.h) the HIP path is CLOSER to the float64 trajectory than the float32 oracle: joints 2.9e-6
    # against 3.0e-5 m, left vertices 1.1e-6 against 3.7e-5 m at the worst element.  Asserted: the review's criterion (max distance
    # <= 1.5 x the oracle's, per key) and the same for the means
    _arbiter_distances("headline arbiter", g, r, a, same, max_ratio=1.5, worst_ratio=1.5)
    assert abs(float(a["collision_loss_origin_scale"].mean()) - mp_got) < 1e-4 and abs(mpjpe(a) - mpjpe(g)) < 1e-4


@pytest.mark.slow
def test_opt_reference_default_schedule_matches_oracle(mano_arrays):
    """The reference's own default schedule (strategies/opt_default.py:15,34,53,73: epoch 300 = 4 x 301 iterations, 31 snapshots
    per stage) at B = 8 against the oracle, with the candidate lists of the collision kernels ON and OFF: the long schedule
    is where stale lists would show (hands drift furthest from the pose their lists were built at).  Lists on / off: bit for bit.
    Against the oracle: the metrics within 1e-4, per element 3e-4; a selection index may differ only between snapshots whose
    select losses are within 1 % of each other in the ORACLE's own table."""
    from ihmr_amd.optimize_model import OptimizeModel
    B, epoch, freq = 8, 300, 10
    orc, model, batch = _oracle_and_model(mano_arrays, B, epoch, freq, seed=808, record=False)
    torch.set_num_threads(max(1, min(32, (__import__("os").cpu_count() or 8))))
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    r = orc.get_pred_result()
    sel_ref = np.stack(orc.selected)
    # the float64 arbiter of the same schedule (round 5): where the two float32 runs pick different snapshots, is either of them "right"?
    a, sel_f64, arb = _f64_arbiter(mano_arrays, B, epoch, freq, batch)
    print(f"[parity] 4x301 arbiter: oracle32 picks another snapshot than float64 at {int((sel_ref != sel_f64).sum())} of {sel_f64.size} (stage, sample) pairs")
    o2 = _make_opt(B, epoch=epoch, save_mid_freq=freq)
    o2.sdf_no_candidate_lists = True
    outs, sels = {}, {}
    for name, m in (("lists", model), ("no lists", OptimizeModel(o2))):
        m.set_input(batch); m.init_optimize(); m.optimize()
        torch.cuda.synchronize()
        g = m.get_pred_result()
        outs[name] = g
        sel = torch.stack(m.selected_history).cpu().numpy()
        sels[name] = sel
        # 31 snapshots of a stage that has long converged carry select losses within a fraction of a percent of each other, and two
        # fp32 implementations of 301 Adam steps do not follow the same trajectory to that precision (measured: 3 of 32 (stage, sample)
        # pairs pick another snapshot; the oracle's own loss at the HIP path's choice is 4e-4 ... 3e-3 above its minimum, relative,
        # i.e. <= 1e-4 absolute).  Where the choice differs, the oracle's loss at that snapshot must be within 1 % (or 2e-4 absolute)
        # of its minimum -- a choice between near-ties, not a wrong one -- and the outputs are compared below either way
        diff = np.argwhere(sel != sel_ref)
        print(f"[parity] 4x301 [{name}]: selection differs from the oracle at {len(diff)} of {sel.size} (stage, sample) pairs")
        for st_i, b_i in diff:
            tab = orc.select_table[st_i][:, b_i]
            print(f"[parity]    stage {st_i} sample {b_i}: oracle loss at the HIP choice {tab[sel[st_i, b_i]]:.6e}, oracle minimum {tab.min():.6e}")
            assert tab[sel[st_i, b_i]] <= tab.min() + max(1e-2 * tab.min(), 2e-4), (name, st_i, b_i, tab[sel[st_i, b_i]], tab.min())
        assert len(diff) <= sel.size // 8
        # against the arbiter: the HIP path disagrees with the float64 run about as often as the float32 oracle does -- near-ties
        # flip either way (measured: HIP 2, oracle32 3 of 32 pairs) --, its choices are near-ties in the arbiter's table as well
        # (every run picks the argmin of its OWN table, and after 301 Adam steps the tables of two runs differ by ~1 % at the same
        # snapshot: 3 % here), and on the samples where all three agree both float32 runs stay within the bars of _arbiter_distances
        d64 = np.argwhere(sel != sel_f64)
        print(f"[parity] 4x301 [{name}]: selection differs from float64 at {len(d64)} pairs (oracle32: {int((sel_ref != sel_f64).sum())})")
        for st_i, b_i in d64:
            tab = arb.select_table[st_i][:, b_i]
            print(f"[parity]    stage {st_i} sample {b_i}: float64 loss at the HIP choice {tab[sel[st_i, b_i]]:.6e}, float64 minimum {tab.min():.6e}")
            assert tab[sel[st_i, b_i]] <= tab.min() + max(3e-2 * tab.min(), 2e-4), (name, "f64", st_i, b_i, tab[sel[st_i, b_i]], tab.min())
        assert len(d64) <= max((sel_ref != sel_f64).sum() + 2, sel.size // 8)
        same3 = np.all(sel == sel_ref, axis=0) & np.all(sel == sel_f64, axis=0)
        if same3.any():
            _arbiter_distances(f"4x301 [{name}] arbiter", g, r, a, same3, max_ratio=4.0, worst_ratio=2.0)
        # element by element only where every stage picked the oracle's snapshot (another snapshot = parameters ten optimizer steps
        # apart: measured 7e-4 m on a joint): 3e-4 after 1204 Adam steps (see test_opt_headline_workload_matches_oracle); the
        # metrics north_star names over ALL samples at its 1e-4
        same = np.all(sel == sel_ref, axis=0)
        assert same.sum() >= B - len(diff)
        _report(f"4x301 [{name}] joints [m]", g["pred_joints_3d"][same], r["pred_joints_3d"][same], atol=1e-4)
        _report(f"4x301 [{name}] right verts [m]", g["pred_right_hand_verts"][same], r["pred_right_hand_verts"][same], atol=1e-4)
        _report(f"4x301 [{name}] left verts [m]", g["pred_left_hand_verts"][same], r["pred_left_hand_verts"][same], atol=1e-4)
        _report(f"4x301 [{name}] penetration depth [m]", g["collision_loss_origin_scale"][same], r["collision_loss_origin_scale"][same], atol=1e-4)
        mpjpe = lambda x: float(np.linalg.norm(x["pred_joints_3d"] - x["gt_joints_3d"][..., :3], axis=-1).mean())
        mpv = float(np.mean([np.linalg.norm(g[k] - r[k], axis=-1).mean() for k in ("pred_right_hand_verts", "pred_left_hand_verts")]))
        pen = abs(float(g["collision_loss_origin_scale"].mean()) - float(r["collision_loss_origin_scale"].mean()))
        print(f"[parity] 4x301 [{name}]: |MPJPE diff| {abs(mpjpe(g) - mpjpe(r)):.3e}, mean per-vertex distance {mpv:.3e}, |mean penetration depth diff| {pen:.3e}")
        assert abs(mpjpe(g) - mpjpe(r)) < 1e-4 and mpv < 1e-4 and pen < 1e-4
    assert np.array_equal(sels["lists"], sels["no lists"])
    for k in ("pred_pose_params", "pred_shape_params", "pred_right_hand_verts", "pred_left_hand_verts", "collision_loss_origin_scale"):
        assert np.array_equal(outs["lists"][k], outs["no lists"][k]), f"candidate lists changed {k}"


# ----------------------------------------------------------------------------------- seams A + B composed (import-swap route)
def test_reference_shaped_loop_over_the_hip_seams_matches_cpu_oracle(mano_arrays):
    """INTEGRATION.md's first route: keep the reference's own loop (autograd, torch.optim.Adam re-created per stage,
    python snapshots / filter / select) and swap only the two third-party imports.  The oracle's OptimizeRef IS that loop
    (pinned to the reference's by opt_traj*.npz); here it runs on the GPU with `ihmr_amd.mano.create` as smplx.create and
    `ihmr_amd.sdf.SDFLoss` as sdf.SDFLoss -- including the in-place `.shapedirs` mutation before `.cuda()`
    (optimize_model.py:109-117) -- against the same loop on the CPU restatements, on the ragged batch."""
    from helpers import ragged_opt_batch
    from ihmr_amd import mano as seam_a
    from ihmr_amd import sdf as seam_b
    from ihmr_amd.strategies import make_opt_strategy
    from oracle.opt_ref import OptimizeRef
    right, left = mano_arrays
    B, epoch, freq = 8, 3, 2
    _, batch = _two_hand_verts(mano_arrays, B, 4711)
    batch = ragged_opt_batch(batch)
    cpu = OptimizeRef(right, left, B, make_opt_strategy(epoch), save_mid_freq=freq)
    gpu = OptimizeRef(None, None, B, make_opt_strategy(epoch), save_mid_freq=freq, smplx_create=seam_a.create,
                      sdf_loss_cls=seam_b.SDFLoss, device="cuda")
    assert isinstance(gpu.mano_right, seam_a.MANO) and isinstance(gpu.sdf, seam_b.SDFLoss)
    assert float((gpu.mano_left.shapedirs[:, 0, :] + gpu.mano_right.shapedirs[:, 0, :]).abs().max()) == 0.0   # mutated in place
    for o in (cpu, gpu):
        o.set_input(batch); o.init_optimize(); o.optimize()
    torch.cuda.synchronize()
    r, g = cpu.get_pred_result(), gpu.get_pred_result()
    assert np.array_equal(np.stack(cpu.selected), np.stack(gpu.selected))
    _report("seams pose", g["pred_pose_params"], r["pred_pose_params"], atol=2e-4)
    _report("seams shape", g["pred_shape_params"], r["pred_shape_params"], atol=2e-4)
    _report("seams trans", g["pred_hand_trans"], r["pred_hand_trans"], atol=2e-5)
    _report("seams right verts [m]", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=1e-4)
    _report("seams left verts [m]", g["pred_left_hand_verts"], r["pred_left_hand_verts"], atol=1e-4)
    _report("seams joints [m]", g["pred_joints_3d"], r["pred_joints_3d"], atol=1e-4)
    _report("seams penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)
    _report("seams collision_loss", g["collision_loss"], r["collision_loss"], atol=2e-4, rtol=1e-3)


# ----------------------------------------------------------------------------------- the reference's own batch size: 512
def test_opt_batch512_matches_oracle_and_is_permutation_equivariant(mano_arrays):
    """bash/optimize.sh:11,33 runs IHMR-OPT at batchSize 512 per process.  One launch sequence over 512 samples (1024
    hands): (a) against the oracle (2 iterations per stage + final forward); (b) size-independent properties on the
    4 x 10-iteration schedule: no sample depends on where it sits in the batch (a permuted batch gives the permuted result,
    bit for bit) nor on its neighbours (duplicated samples give duplicated results)."""
    from ihmr_amd.optimize_model import OptimizeModel
    B = 512
    orc, model, batch = _oracle_and_model(mano_arrays, B, 1, 1, seed=512512, record=False)
    torch.set_num_threads(max(1, min(32, (__import__("os").cpu_count() or 8))))
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    assert np.array_equal(np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy())
    _report("B=512 pose", g["pred_pose_params"], r["pred_pose_params"], atol=1e-4)
    _report("B=512 shape", g["pred_shape_params"], r["pred_shape_params"], atol=1e-4)
    _report("B=512 trans", g["pred_hand_trans"], r["pred_hand_trans"], atol=2e-5)
    _report("B=512 right verts [m]", g["pred_right_hand_verts"], r["pred_right_hand_verts"], atol=1e-4)
    _report("B=512 left verts [m]", g["pred_left_hand_verts"], r["pred_left_hand_verts"], atol=1e-4)
    _report("B=512 joints [m]", g["pred_joints_3d"], r["pred_joints_3d"], atol=1e-4)
    _report("B=512 penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-4)
    # (b) properties, 40 iterations
    long = OptimizeModel(_make_opt(B, epoch=9, save_mid_freq=5))
    dup = {k: torch.cat([v[:256], v[:256]], dim=0) for k, v in batch.items()}
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(7))
    outs = []
    for inp in (dup, {k: v[perm] for k, v in dup.items()}):
        long.set_input(inp); long.init_optimize(); long.optimize()
        torch.cuda.synchronize()
        outs.append((long.get_pred_result(), torch.stack(long.selected_history).cpu().numpy()))
    (a, sel_a), (p, sel_p) = outs
    keys = ("pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
            "pred_joints_3d", "collision_loss", "collision_loss_origin_scale")
    for k in keys:
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k][:256], a[k][256:]), f"{k}: duplicated samples differ"
        assert np.array_equal(p[k], a[k][perm.numpy()]), f"{k}: the result depends on the position in the batch"
    assert np.array_equal(sel_p, sel_a[:, perm.numpy()])
    assert len(np.unique(sel_a)) > 1


# ----------------------------------------------------------------------------------- seam B conventions (ihmr_sdf_options)
@pytest.mark.parametrize("align_corners,loss_divisor,swap_xz", [(False, 4.0, False), (True, 4.0, False), (False, 1.0, False), (True, 1.0, False),
                                                                (False, 4.0, True), (True, 1.0, True)])
def test_sdf_convention_switches_match_oracle(mano_arrays, align_corners, loss_divisor, swap_xz):
    """The three conventions of the absent upstream collision module that nothing in the reference pins -- grid_sample's
    `align_corners`, the normalisation of the per-sample loss and the axis order of the grid as grid_sample sees it (`swap_xz`) --
    are explicit parameters on both sides (oracle:
    SDFLossRef(align_corners=, loss_divisor=, swap_xz=); product: SDFLoss(...) -> ihmr_sdf_collision_ex, and opt.sdf_* ->
    ihmr_opt_io for the fused loop); every combination is compared: values, loss and gradient through seam B, and the
    fused loop's collision term + one Adam step of every stage."""
    import functools
    from ihmr_amd.sdf import SDFLoss
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.strategies import make_opt_strategy
    from oracle.opt_ref import OptimizeRef
    from oracle.sdf_ref import SDFLossRef
    right, left = mano_arrays
    B = 4
    hv, batch = _two_hand_verts(mano_arrays, B, 5)
    ref_mod = SDFLossRef(right["faces"], left["faces"], align_corners=align_corners, loss_divisor=loss_divisor, swap_xz=swap_xz)
    hv_ref = hv.clone().requires_grad_(True)
    l_ref, pv_ref, os_ref = ref_mod(hv_ref, return_per_vert_loss=True, return_origin_scale_loss=True)
    w = torch.linspace(0.5, 1.5, B)
    (l_ref * w).sum().backward()
    mod = SDFLoss(right["faces"], left["faces"], align_corners=align_corners, loss_divisor=loss_divisor, swap_xz=swap_xz).to(_dev())
    hv_g = hv.clone().to(_dev()).requires_grad_(True)
    l, pv, os_ = mod(hv_g, return_per_vert_loss=True, return_origin_scale_loss=True)
    (l * w.to(_dev())).sum().backward()
    assert int((pv_ref > 0).sum()) > (10 if swap_xz else 50)
    _report("conv per_vert", pv.detach().cpu(), pv_ref.detach(), atol=1e-6)
    _report("conv origin_scale [m]", os_.detach().cpu(), os_ref.detach(), atol=1e-7)
    _report("conv loss", l.detach().cpu(), l_ref.detach(), atol=1e-5, rtol=1e-6)
    _report("conv d/dverts", hv_g.grad.cpu(), hv_ref.grad, atol=1e-4 * float(hv_ref.grad.abs().max()))
    # fused loop
    opt = _make_opt(B, epoch=1, save_mid_freq=1)
    opt.sdf_align_corners, opt.sdf_loss_divisor, opt.sdf_swap_xz = align_corners, loss_divisor, swap_xz
    model = OptimizeModel(opt)
    orc = OptimizeRef(right, left, B, make_opt_strategy(1), save_mid_freq=1,
                      sdf_loss_cls=functools.partial(SDFLossRef, align_corners=align_corners, loss_divisor=loss_divisor, swap_xz=swap_xz))
    orc.set_input(batch); orc.init_optimize(); orc.optimize()
    model.set_input(batch); model.init_optimize(); model.optimize()
    torch.cuda.synchronize()
    r, g = orc.get_pred_result(), model.get_pred_result()
    assert np.array_equal(np.stack(orc.selected), torch.stack(model.selected_history).cpu().numpy())
    _report("conv fused collision_loss", g["collision_loss"], r["collision_loss"], atol=1e-5, rtol=1e-5)
    _report("conv fused pose", g["pred_pose_params"], r["pred_pose_params"], atol=1e-4)
    _report("conv fused penetration depth [m]", g["collision_loss_origin_scale"], r["collision_loss_origin_scale"], atol=1e-6)


# ----------------------------------------------------------------------------------- candidate lists are exact
@pytest.mark.parametrize("B,epoch,overlap", [pytest.param(16, 29, None, id="16-29"), pytest.param(64, 9, None, id="64-9"),
                                             pytest.param(64, 14, "deep", id="deep-64-14"), pytest.param(160, 14, "deep", id="deep-160-14")])
def test_candidate_lists_do_not_change_a_bit(mano_arrays, B, epoch, overlap):
    """Inside a stage the distance kernel searches, per voxel, only the candidate triangles recorded when the hand's lists were
    last built (valid while no vertex has moved by more than the slack in the hand's normalised frame; rebuilt otherwise, and at
    a stage start unless the caller vouches for its workspace: ihmr_opt_stage.keep_lists, round 6).  A conservative acceleration: with `opt.sdf_no_candidate_lists` every iteration searches all 1538
    triangles -- both runs must agree bit for bit, on the regular and on the ragged batch, through all four stages (the
    translation / shape stages reuse the lists for many iterations, the orientation / pose stages rebuild every few).  "deep": the
    deep-overlap batch, where lists run long, are refused, and late voxels take fresh slots over 60-iteration stages; the snapshot
    losses and the optimizer state are compared as well."""
    from helpers import DEEP_SEED, ragged_opt_batch
    from ihmr_amd.optimize_model import OptimizeModel
    _, batch = _two_hand_verts(mano_arrays, B, DEEP_SEED if overlap else 900 + B, overlap=overlap)
    if B == 16:
        batch = ragged_opt_batch(batch)
    outs = []
    for off in (False, True):
        opt = _make_opt(B, epoch=epoch, save_mid_freq=5)
        opt.sdf_no_candidate_lists = off
        m = OptimizeModel(opt)
        for rep in range(2):            # the second pass replays the captured graphs over the previous pass's (stale) lists
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
        outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["snap_loss"].cpu().numpy(), m.buf["adam_m"].cpu().numpy()))
    (a, sa, la, ma), (b, sb, lb, mb) = outs
    assert np.array_equal(sa, sb)
    if overlap:
        assert np.array_equal(la, lb) and np.array_equal(ma, mb)
    for k in ("pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: the candidate lists changed the result"
    assert float(a["collision_loss_origin_scale"].max()) > 0


@pytest.mark.parametrize("B,epoch,overlap", [pytest.param(16, 39, None, id="16-39"), pytest.param(64, 14, None, id="64-14"),
                                             pytest.param(64, 14, "deep", id="deep-64-14"), pytest.param(160, 14, "deep", id="deep-160-14")])
def test_static_hand_reuse_does_not_change_a_bit(mano_arrays, B, epoch, overlap):
    """A hand whose vertices cannot change during a stage keeps, from the stage's second iteration on, its box, normalised vertices
    and triangle records, and what earlier iterations found out about its voxels (inside / outside, distance): only voxels that the
    other hand reaches for the first time are tested and searched.  The same vertices give the same grid, so `opt.sdf_no_static_reuse`
    (everything from scratch every iteration) must agree bit for bit.  Stages: opt_default (translation stage: the right hands are
    static) + three that opt_default never runs -- right orientation alone (the left hands are static), left finger pose alone
    (the right hands are static while the other side rebuilds its candidate lists), camera + translation (right static, camera
    gradient on) -- regular, ragged and deep-overlap batch, graphs replayed twice over stale state."""
    from helpers import DEEP_SEED, ragged_opt_batch
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.strategies import make_opt_strategy
    _, batch = _two_hand_verts(mano_arrays, B, DEEP_SEED if overlap else 3100 + B, overlap=overlap)
    if B == 16:
        batch = ragged_opt_batch(batch)
    base = make_opt_strategy(epoch)
    extra = []
    for params, like in ((["pred_right_orient"], 1), (["pred_left_pose_params"], 2), (["pred_cam_params", "pred_hand_trans"], 0)):
        st = dict(base[like]); st["update_params"] = params
        extra.append(st)
    outs = []
    for off in (False, True):
        opt = _make_opt(B, epoch=epoch, save_mid_freq=5)
        opt.sdf_no_static_reuse = off
        opt.sdf_no_translated_reuse = True       # (the round-5 extension is rounding-level, not bit-level: its own test below)
        m = OptimizeModel(opt)
        m.strategy = base + extra
        for rep in range(2):
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
        outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["snap_loss"].cpu().numpy(), m.buf["adam_m"].cpu().numpy()))
    (a, sa, la, ma), (b, sb, lb, mb) = outs
    assert np.array_equal(sa, sb) and np.array_equal(la, lb) and np.array_equal(ma, mb)
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: the static-hand reuse changed the result"
    assert float(a["collision_loss_origin_scale"].max()) > 0


@pytest.mark.parametrize("B,epoch,translated,overlap", [pytest.param(16, 29, False, None, id="16-29-False"),
                                                       pytest.param(64, 14, False, None, id="64-14-False"),
                                                       pytest.param(160, 9, True, None, id="160-9-True"),
                                                       pytest.param(64, 14, False, "deep", id="deep-64-14-False"),
                                                       pytest.param(160, 14, True, "deep", id="deep-160-14-True")])
def test_lists_kept_across_stage_boundaries_do_not_change_a_bit(mano_arrays, B, epoch, translated, overlap):
    """Round 6: `OptimizeModel.run_stage` tells the library (`ihmr_opt_stage.keep_lists`) when the workspace still holds the candidate
    lists of the SAME batch's previous stage; the stage's first iteration then resets only the static-hand bookkeeping and a hand keeps its
    lists while the prep kernel's own displacement test passes -- whether an optimizer step or the previous stage's select step moved
    it.  An exact acceleration: `opt.sdf_no_stage_list_reuse` (every stage rebuilds, rounds 1-5) must agree bit for bit, over
    opt_default + three stages it never runs (so that every kind of stage follows every other kind), on the regular, the ragged and the
    >128-hand batch (the 512-thread form of the prep kernel), graphs replayed twice.  The flag is the caller's guarantee about its
    workspace: set_input / init_optimize / a single-shot forward clear it, a fresh instance never sets it in its first stage.
    "deep": the same on the deep-overlap batch."""
    from helpers import DEEP_SEED, ragged_opt_batch
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.strategies import make_opt_strategy
    _, batch = _two_hand_verts(mano_arrays, B, DEEP_SEED if overlap else 4700 + B, overlap=overlap)
    if B == 16:
        batch = ragged_opt_batch(batch)
    base = make_opt_strategy(epoch)
    extra = []
    for params, like in ((["pred_left_pose_params"], 2), (["pred_right_orient"], 1), (["pred_cam_params", "pred_hand_trans"], 0)):
        st = dict(base[like]); st["update_params"] = params
        extra.append(st)
    outs, rebuilt = [], []
    for off in (False, True):
        opt = _make_opt(B, epoch=epoch, save_mid_freq=5)
        opt.sdf_no_stage_list_reuse = off
        opt.sdf_no_translated_reuse = not translated
        m = OptimizeModel(opt)
        m.strategy = base + extra
        assert m._lists_live is False
        for rep in range(2):
            m.set_input(batch); m.init_optimize()
            assert m._lists_live is False
            m.optimize()                         # (ends with the single-shot final forward)
            assert m._lists_live is False
            torch.cuda.synchronize()
        outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["snap_loss"].cpu().numpy(), m.buf["adam_m"].cpu().numpy()))
        m.set_input(batch); m.init_optimize()
        m.sdf_counters_start()
        for st in m.strategy:
            m.run_stage(st)
            assert m._lists_live is True
        rebuilt.append(m.sdf_counters_stop())
    (a, sa, la, ma), (b, sb, lb, mb) = outs
    assert np.array_equal(sa, sb) and np.array_equal(la, lb) and np.array_equal(ma, mb)
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: keeping the lists across the stage boundary changed the result"
    assert float(a["collision_loss_origin_scale"].max()) > 0
    on, off = rebuilt
    print(f"[stage lists] {overlap or 'regular'} B={B}: lists refused {on['lists_refused']} (kept) vs {off['lists_refused']}; voxels rebuilt {on['voxels_rebuilt']} (kept) vs {off['voxels_rebuilt']} (every stage rebuilds); "
          f"full search {on['voxels_full_search']} vs {off['voxels_full_search']}; inside {on['inside_voxels']} vs {off['inside_voxels']}")
    assert on["inside_voxels"] == off["inside_voxels"]
    assert on["voxels_rebuilt"] < off["voxels_rebuilt"]


@pytest.mark.parametrize("B,epoch", [(16, 39), (64, 49)])
def test_translated_hand_reuse_stays_at_rounding_level(mano_arrays, B, epoch):
    """Round 5: a left hand that a stage only TRANSLATES (opt_default's translation stage; camera + translation) is static in its own
    normalised frame, so the product keeps its grid like a static hand's and lets only the box follow the current vertices
    (SdfWorkspace::moving_box).  Unlike the static reuse this is not bit-identical to the from-scratch path: the kept grid is the first
    iteration's, a recomputation differs from it by the rounding of the translated vertices (~1e-7 m).  `opt.sdf_no_translated_reuse`
    switches it off alone; asserted here: the same selections, every exported length within 5e-6 m and every parameter within 5e-6 of
    the run without it after the full schedule (+ a camera + translation stage) -- a twentieth of the parity bar the headline test
    holds the product to against the oracle.  Measured (scripts/experiments/translated_reuse_probe.py): parameters, meshes, optimizer
    state and final losses come out bit-identical on every batch tried; a stored snapshot loss of a translation stage differs by one
    unit in the last place now and then -- which is why this is not filed under the exact accelerations."""
    from helpers import ragged_opt_batch
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.strategies import make_opt_strategy
    base = make_opt_strategy(epoch)
    st = dict(base[0]); st["update_params"] = ["pred_cam_params", "pred_hand_trans"]
    worst_all = {}
    for seed in (3100 + B, 5200 + B, 77):          # (3100 + B: the batch of the static-reuse test, on which the two paths differ)
        _, batch = _two_hand_verts(mano_arrays, B, seed)
        if B == 16:
            batch = ragged_opt_batch(batch)
        worst = _translated_reuse_diff(batch, B, epoch, base + [st])
        print(f"[parity] translated-hand reuse vs from scratch (B {B}, seed {seed}), max |diff|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        for k, v in worst.items():
            worst_all[k] = max(worst_all.get(k, 0.0), v)
    assert max(worst_all.values()) <= 5e-6, worst_all


def _translated_reuse_diff(batch, B, epoch, strategy):
    from ihmr_amd.optimize_model import OptimizeModel
    outs = []
    for off in (False, True):
        opt = _make_opt(B, epoch=epoch, save_mid_freq=5)
        opt.sdf_no_translated_reuse = off
        m = OptimizeModel(opt)
        m.strategy = strategy
        for rep in range(2):
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
        outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy()))
    (a, sa), (b, sb) = outs
    assert np.array_equal(sa, sb)
    worst = {}
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss_origin_scale"):
        worst[k] = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
    assert float(a["collision_loss_origin_scale"].max()) > 0
    return worst


@pytest.mark.parametrize("asset", ["mitten", "fingers", "deep"])
@pytest.mark.parametrize("B,epoch", [(16, 39), (64, 49)])
def test_translated_hand_reuse_in_numbers(mano_arrays, finger_arrays, asset, B, epoch):
    """Round 6 (review item 5): numbers on the one default-on acceleration that is not exact.  Sixteen batches per asset (the blob and
    the five-finger mesh with interlocked hands; "deep": the blob on the deep-overlap batch, where the collision term dominates) and size (16 ragged, 64): the full schedule + a camera + translation stage with the kept
    grid (default) against `opt.sdf_no_translated_reuse`, counting
      * (stage, sample) pairs that select another snapshot,
      * stored snapshot losses that differ at all, and by how much (relative),
      * after the translation stage alone (its 50th iteration: the kept grid is then 49 iterations old) the voxels of the left hands'
        grids whose inside / outside status differs from the from-scratch evaluation of the same iteration (`ihmr_opt_sdf_inside_bits`).
    A rounding-level change of the normalised vertices can in principle move a voxel centre across the surface, and a 1-ulp snapshot
    loss can flip a `<=` filter: asserted here that on these 64 batches neither happens (0 flips, 0 voxels), and that every export stays
    within 5e-6; the counts are printed for DESIGN.md section 5.0."""
    from helpers import ragged_opt_batch
    from ihmr_amd.optimize_model import OptimizeModel
    from ihmr_amd.strategies import make_opt_strategy
    arrays = finger_arrays if asset == "fingers" else mano_arrays
    base = make_opt_strategy(epoch)
    st = dict(base[0]); st["update_params"] = ["pred_cam_params", "pred_hand_trans"]
    models = []
    for off in (False, True):
        opt = _make_opt(B, epoch=epoch, save_mid_freq=5, model_root="synthetic:fingers" if asset == "fingers" else "")
        opt.sdf_no_translated_reuse = off
        m = OptimizeModel(opt)
        m.strategy = base + [st]
        models.append(m)
    flips = pairs = loss_diff = loss_n = vox_diff = vox_n = 0
    worst_ulp, worst, worst_abs = 0.0, 0.0, 0.0
    for seed in range(9000, 9016):
        _, batch = _two_hand_verts(arrays, B, seed + B, interlock=asset == "fingers", overlap="deep" if asset == "deep" else None)
        if B == 16:
            batch = ragged_opt_batch(batch)
        res = []
        for m in models:
            m.set_input(batch); m.init_optimize(); m.run_stage(m.strategy[0])
            bits, box = m.sdf_inside_bits()
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
            res.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["snap_loss"].cpu().numpy().copy(), bits, box))
        (a, sa, la, ba, xa), (b, sb, lb, bb, xb) = res
        flips += int((sa != sb).sum()); pairs += sa.size
        d = np.abs(la.astype(np.float64) - lb.astype(np.float64))
        loss_diff += int((d != 0).sum()); loss_n += d.size
        worst_ulp = max(worst_ulp, float((d / np.maximum(np.abs(la), 1e-30)).max()))      # (relative, not in units of the last place: see below)
        worst_abs = max(worst_abs, float(d.max()))
        x = ba ^ bb
        vox_diff += int(sum(bin(int(w)).count("1") for w in x[x != 0])); vox_n += int(sum(bin(int(w)).count("1") for w in (ba | bb)[(ba | bb) != 0]))
        assert np.array_equal(xa[0], xb[0]) and np.abs(xa[1] - xb[1]).max() <= 1e-6          # (right hands: static either way; left boxes: rounding)
        for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
                  "pred_joints_3d", "collision_loss_origin_scale"):
            worst = max(worst, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))
    print(f"[parity] translated-hand reuse in numbers ({asset}, B {B}, 16 batches): selection flips {flips} of {pairs} (stage, sample) pairs; "
          f"stored snapshot losses that differ {loss_diff} of {loss_n} (worst relative difference {worst_ulp:.1e}, absolute {worst_abs:.1e}); inside / outside "
          f"status after the translation stage: {vox_diff} of {vox_n} inside voxels differ; worst export difference {worst:.2e}")
    # the stored collision losses of the translation stages are sums of penetration depths (normalised units) evaluated from coordinates
    # that differ in their last bits: every depth moves by ~1e-7, the voxel SET is the same
    # (bound, in the loss's own units -- normalised grid lengths: 5e-6, i.e. ~50 sampled depths each off by one rounding of a coordinate;
    # relative to a loss that is itself ~1e-4 for a pair that barely touches this can be percents)
    assert flips == 0 and vox_diff == 0 and worst <= 5e-6 and worst_abs <= 5e-6, (flips, vox_diff, worst, worst_abs, worst_ulp)


def _tail_run_state(m, selected):
    """What a fused-tail run is compared on: every export, the selections, the optimizer state and the snapshot losses."""
    return m.get_pred_result(), selected.cpu().numpy(), m.buf["adam_m"].cpu().numpy(), m.buf["snap_loss"].cpu().numpy()


def _assert_tail_runs_identical(fused, separate):
    (a, sa, ma, la), (b, sb, mb, lb) = fused, separate
    assert np.array_equal(sa, sb) and np.array_equal(ma, mb) and np.array_equal(la, lb)
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: the fused tail launch changed the result"


@pytest.mark.parametrize("B,optimizer,overlap", [pytest.param(16, "adam", None, id="16-adam"), pytest.param(64, "adam", None, id="64-adam"),
                                                pytest.param(9, "sgd", None, id="9-sgd"), pytest.param(64, "adam", "deep", id="deep-64-adam"),
                                                pytest.param(160, "adam", "deep", id="deep-160-adam")])
def test_fused_tail_launch_does_not_change_a_bit(mano_arrays, B, optimizer, overlap):
    """The stages that do not move the finger pose run the tail of an iteration -- collision sampling + losses, the LBS backward of
    both hands, the optimizer step + the next skeletons -- as ONE launch per sample (`opt_tail_kernel`); `opt.no_fused_tail` runs
    the three launches it replaces.  The same device functions in the same order: bit for bit the same results, on the regular
    and the ragged batch, with Adam and SGD, graphs replayed twice; on the deep-overlap batch over 60-iteration stages."""
    from helpers import DEEP_SEED, ragged_opt_batch
    from ihmr_amd.optimize_model import OptimizeModel
    _, batch = _two_hand_verts(mano_arrays, B, DEEP_SEED if overlap else 1700 + B, overlap=overlap)
    if B == 16:
        batch = ragged_opt_batch(batch)
    outs = []
    for off in (False, True):
        opt = _make_opt(B, epoch=14 if overlap else 7, save_mid_freq=3)
        opt.no_fused_tail = off
        opt.optimizer = optimizer
        m = OptimizeModel(opt)
        for rep in range(2):
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
        outs.append(_tail_run_state(m, torch.stack(m.selected_history)))
    _assert_tail_runs_identical(*outs)


def test_fused_tail_on_a_hand_with_a_degenerate_box_does_not_change_a_bit(mano_arrays):
    """A hand whose box scale lies outside [1e-6, 1e6] takes the plain division (`sdf_div`), and in the cell-word samplers EVERY entry
    that samples it runs the full arithmetic, whatever its corner mask says (`nz` set by `!fast`).  The right hand of sample 1 is shrunk
    towards its centroid: the first shape direction of the right-hand model (which the loop evaluates for both hands) is made
    `centroid - v_template`, so beta_0 = 1 - 5e-6 leaves an extent of ~1e-6 m (a few dozen float32 ulps at hand coordinates: everything
    stays finite) -- the hand's other betas are 0 and its finger pose is the rest pose (no pose-blend offsets); every other hand has
    beta_0 = 0 and is an ordinary hand.  The scale the prep kernel stored is read back and must lie strictly between 0 and 1e-6.  One
    orientation stage of 3 iterations with the fused tail and with `opt.no_fused_tail`: bit for bit the same."""
    from ihmr_amd.optimize_model import OptimizeModel
    B = 2
    _, batch = _two_hand_verts(mano_arrays, B, 1234)
    batch = {k: v.clone() for k, v in batch.items()}
    batch["init_shape_params"][:, [0, 10]] = 0.0
    batch["init_shape_params"][1, :10] = 0.0
    batch["init_shape_params"][1, 0] = 1.0 - 5e-6
    outs = []
    for off in (False, True):
        opt = _make_opt(B, epoch=2, save_mid_freq=1)
        opt.no_fused_tail = off
        m = OptimizeModel(opt)
        right = m.mano_models["right"]
        right.shapedirs[:, :, 0] = right.v_template.mean(dim=0, keepdim=True) - right.v_template      # (in place: re-uploaded by _handle)
        batch["init_pose_params"][1, 3:48] = -right.hand_mean.cpu()
        m.set_input(batch); m.init_optimize()
        m.run_stage(m.strategy[1])
        torch.cuda.synchronize()
        _, box = m.sdf_inside_bits()
        print(f"[parity] degenerate box ({'separate' if off else 'fused'}): scales {box[:, :, 3].tolist()}")
        assert 0.0 < box[0, 1, 3] < 1e-6 and box[0, 0, 3] >= 1e-6 and (box[1, :, 3] >= 1e-6).all(), box[:, :, 3]
        assert np.isfinite(m.buf["snap_loss"].cpu().numpy()).all()
        m.forward_losses()                     # (as optimize() closes: the tail launch does not write the exported per-vertex depths)
        torch.cuda.synchronize()
        outs.append(_tail_run_state(m, m.buf["selected"]))
    _assert_tail_runs_identical(*outs)


def test_lbs_bwd2_forms_are_bit_identical(mano_arrays):
    """The pose-gradient GEMM of the finger-pose stage has two forms: `lbs_bwd2_kernel` (operands streamed; up to 255 hands per launch)
    and `lbs_bwd2_lds_kernel` (operands staged through LDS; from 256 hands on, i.e. every launch of the headline bench).  The same
    k -> MFMA-step assignment and the same fixed-order sum of the split-K partials: the same bits.  B = 160 (320 hands, a ragged
    tail for the 64-hand tiles of the LDS form) through all four stages with either form (`ihmr_debug_force_lbs_bwd2_streaming`):
    the raw pose gradient of the last iteration, the optimizer state, every snapshot loss, the selection and the exports."""
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel
    B = 160
    _, batch = _two_hand_verts(mano_arrays, B, 4242)
    outs = []
    try:
        for force in (0, 1):
            hip.lib().ihmr_debug_force_lbs_bwd2_streaming(force)
            m = OptimizeModel(_make_opt(B, epoch=5, save_mid_freq=2))     # (a fresh instance: the stage graphs are captured under the switch)
            m.set_input(batch); m.init_optimize(); m.optimize()
            torch.cuda.synchronize()
            outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["adam_m"].cpu().numpy(),
                         m.buf["adam_v"].cpu().numpy(), m.buf["snap_loss"].cpu().numpy()))
    finally:
        hip.lib().ihmr_debug_force_lbs_bwd2_streaming(0)
    (a, sa, ma, va, la), (b, sb, mb, vb, lb) = outs
    assert np.abs(ma).max() > 0
    assert np.array_equal(sa, sb) and np.array_equal(ma, mb) and np.array_equal(va, vb) and np.array_equal(la, lb)
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: the two forms of the pose-gradient GEMM differ"


@pytest.mark.parametrize("B", [24, 160])
def test_skin_keeps_pose_offsets_bit_identically(mano_arrays, B):
    """Round 5: a stage that moves the shape but not the finger pose (opt_default's fourth) stores the pose-blend offsets P in its first
    iteration's skinning launch and reuses them after -- `v_posed = (v_template + S) + P` with the stored P is the operation the full
    kernel ends with, on the same bits.  opt_default (the shape stage with and without its snapshots' selection) at a small launch
    (4 hands per skin workgroup) and a large one (8), with the reuse and with `ihmr_debug_force_full_skin`: optimizer state, snapshot
    losses, selection and every export bit for bit."""
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel
    _, batch = _two_hand_verts(mano_arrays, B, 515)
    outs = []
    try:
        for force in (0, 1):
            hip.lib().ihmr_debug_force_full_skin(force)
            m = OptimizeModel(_make_opt(B, epoch=6, save_mid_freq=2))     # (a fresh instance: the stage graphs are captured under the switch)
            m.set_input(batch); m.init_optimize(); m.optimize()
            m.set_input(batch); m.init_optimize(); m.optimize()            # (a second pass replays the graphs over the first pass's stale offsets)
            torch.cuda.synchronize()
            outs.append((m.get_pred_result(), torch.stack(m.selected_history).cpu().numpy(), m.buf["adam_m"].cpu().numpy(),
                         m.buf["adam_v"].cpu().numpy(), m.buf["snap_loss"].cpu().numpy()))
    finally:
        hip.lib().ihmr_debug_force_full_skin(0)
    (a, sa, ma, va, la), (b, sb, mb, vb, lb) = outs
    assert np.abs(ma).max() > 0
    assert np.array_equal(sa, sb) and np.array_equal(ma, mb) and np.array_equal(va, vb) and np.array_equal(la, lb)
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: kept pose offsets change the result"


def test_candidate_lists_are_used_and_accounted_for(mano_arrays):
    """The work counters of the fused loop (`inside_voxels` = the voxels handed to the distance kernel): inside a stage most of them are
    answered from their candidate lists, every one is evaluated exactly once per iteration (list search + full search), the list search
    tests far fewer spheres than the 1538 of a full search; with the lists switched off nothing goes through them; and in the
    translation stage the static right hands hand over only voxels that are new (far fewer evaluations than with `sdf_no_static_reuse`)."""
    from ihmr_amd.optimize_model import OptimizeModel
    B = 16
    _, batch = _two_hand_verts(mano_arrays, B, 77)
    evaluated = {}
    for mode in ("default", "no_static_reuse", "no_lists", "translated"):
        opt = _make_opt(B, epoch=19, save_mid_freq=5)
        opt.sdf_no_candidate_lists = mode == "no_lists"
        opt.sdf_no_static_reuse = mode == "no_static_reuse"
        opt.sdf_no_translated_reuse = mode != "translated"     # "default" here = the exact accelerations alone (lists + static right hands)
        m = OptimizeModel(opt)
        m.set_input(batch); m.init_optimize()
        m.sdf_counters_start()
        m.run_stage(m.strategy[0])
        c = m.sdf_counters_stop()
        evaluated[mode] = c["inside_voxels"]
        assert c["inside_voxels"] > 0
        assert c["voxels_from_lists"] + c["voxels_full_search"] == c["inside_voxels"]
        if mode == "no_lists":
            assert c["voxels_from_lists"] == 0 and c["voxels_without_list"] == 0 and c["voxels_rebuilt"] == 0
            assert c["sphere_tests"] == 1538 * c["inside_voxels"]
        elif mode == "translated":     # the product's default: in the translation stage BOTH hands keep their grids, only new voxels are searched
            assert c["voxels_from_lists"] == 0
        else:
            assert c["voxels_from_lists"] > c["inside_voxels"] // 2
            assert c["sphere_tests"] < 1538 * c["inside_voxels"] // 2
        if mode == "no_static_reuse":
            assert c["voxels_from_lists"] + c["voxels_without_list"] + c["voxels_rebuilt"] == c["inside_voxels"]
    assert evaluated["no_static_reuse"] == evaluated["no_lists"]
    assert evaluated["default"] < 0.75 * evaluated["no_static_reuse"], evaluated
    assert evaluated["translated"] < 0.5 * evaluated["default"], evaluated


@pytest.mark.parametrize("B", [16, 64])
def test_candidate_lists_exact_over_the_reference_schedule_under_deep_overlap(mano_arrays, B):
    """The reference's default schedule (opt_default at epoch 300: 4 x 301 iterations, a snapshot every 10) on the deep-overlap batch,
    candidate lists on and off (`opt.sdf_no_candidate_lists`): bit for bit the same selections, snapshot losses, optimizer state and
    exports.  Long stages with deep overlap are where late voxels keep taking fresh list slots until a hand's SDF_LCAP_V = 1024 run out,
    and where lists longer than SDF_LCAP_L = 192 triangles are refused and the voxel is searched in full from then on.  The counters do
    not tell a refusal for want of slots from one for length, so slot exhaustion is exercised here but not separately shown.  Asserted:
    lists were refused and voxels searched in full, and every inside voxel was answered exactly once; the refused lists per sample and
    iteration and the full-search share are printed per stage, with the default batch's under the same schedule beside them."""
    from helpers import DEEP_SEED
    from ihmr_amd.optimize_model import OptimizeModel
    epoch, freq = 300, 10
    _, deep = _two_hand_verts(mano_arrays, B, DEEP_SEED, overlap="deep")
    _, shallow = _two_hand_verts(mano_arrays, B, DEEP_SEED)
    its = B * (epoch + 1)

    def counted(batch, tag):
        m = OptimizeModel(_make_opt(B, epoch=epoch, save_mid_freq=freq))
        m.set_input(batch); m.init_optimize()
        m.selected_history, per_stage = [], []
        for st in m.strategy:                      # (OptimizeModel.optimize, with the counters read per stage)
            m.sdf_counters_start()
            m.run_stage(st)
            per_stage.append(m.sdf_counters_stop())
            m.selected_history.append(m.buf["selected"].clone())
        m.forward_losses(m.default_loss_weights)
        torch.cuda.synchronize()
        for i, c in enumerate(per_stage):
            print(f"[lists] {tag} B={B} stage {i}: lists refused {c['lists_refused']} ({c['lists_refused'] / its:.3f} per sample and iteration), "
                  f"full-search share {c['voxels_full_search'] / max(c['inside_voxels'], 1):.4f}, inside voxels {c['inside_voxels'] / its:.1f} "
                  f"per sample and iteration")
        return m, per_stage

    m_on, c_deep = counted(deep, "deep")
    _, c_shallow = counted(shallow, "default")
    tot = {k: sum(c[k] for c in c_deep) for k in c_deep[0]}
    ref = {k: sum(c[k] for c in c_shallow) for k in c_shallow[0]}
    print(f"[lists] B={B} whole schedule: refused lists per sample and iteration {tot['lists_refused'] / (4 * its):.3f} (default batch "
          f"{ref['lists_refused'] / (4 * its):.3f}), full-search share {tot['voxels_full_search'] / tot['inside_voxels']:.4f} (default batch "
          f"{ref['voxels_full_search'] / max(ref['inside_voxels'], 1):.4f})")
    assert tot["lists_refused"] > 0 and tot["voxels_full_search"] > 0
    for c in c_deep:
        assert c["voxels_from_lists"] + c["voxels_full_search"] == c["inside_voxels"]
    opt = _make_opt(B, epoch=epoch, save_mid_freq=freq)
    opt.sdf_no_candidate_lists = True
    m_off = OptimizeModel(opt)
    m_off.set_input(deep); m_off.init_optimize(); m_off.optimize()
    torch.cuda.synchronize()
    a, b = m_on.get_pred_result(), m_off.get_pred_result()
    assert np.array_equal(torch.stack(m_on.selected_history).cpu().numpy(), torch.stack(m_off.selected_history).cpu().numpy())
    assert np.array_equal(m_on.buf["snap_loss"].cpu().numpy(), m_off.buf["snap_loss"].cpu().numpy())
    assert np.array_equal(m_on.buf["adam_m"].cpu().numpy(), m_off.buf["adam_m"].cpu().numpy())
    for k in ("pred_cam_params", "pred_pose_params", "pred_shape_params", "pred_hand_trans", "pred_right_hand_verts", "pred_left_hand_verts",
              "pred_joints_3d", "collision_loss", "collision_loss_origin_scale"):
        assert np.array_equal(a[k], b[k]), f"{k}: the candidate lists changed the result over the long schedule"
    assert float(a["collision_loss_origin_scale"].max()) > 0

"""The MANO layer (``ihmr_amd.mano.MANO`` over ``ihmr_mano_lbs_fwd`` / ``ihmr_mano_lbs_bwd``) at every launch form and at the pose
extremes, against the oracle in FLOAT64 (tests/mano_cases.py: the cases, the truth and the one comparison, `within`).

The hand counts 1, 8, 9, 33, 256, 257, 321 are the smallest that reach each form of the launches (csrc/mano_lbs.h):
  1    one hand                                      8    the last launch whose hands all sit in slot 0 of their skin workgroup
  9    the first real slot 1, i.e. the first packed two-hand FMA with two real hands
  33   the second hand group of the small skin form (4 hands per workgroup) and a second 32-row tile of lbs_bwd2_kernel with one row
  256  the last small skin form; the first LDS form of the pose-gradient GEMM (lbs_bwd2_lds_kernel), four full 64-hand tiles
  257  the first 8-hand skin form; a one-row ragged fifth LDS tile
  321  a sixth hand group of the large form with one hand in it; a one-row ragged sixth LDS tile
(tests/test_mano_cases_cpu.py checks on a restatement of `lbs_group_hand` that these fill every slot of some workgroup and leave a
real hand next to an empty slot, for both workgroup sizes.)

No tolerance but `within`'s: max |hip - f64| <= max(floor, 1.5 max |oracle32 - f64|) per output, floors 2e-5 max |f64| (gradients)
and 2e-6 m max(1, max |f64| / 0.2 m) (vertices, joints).  Everything else is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mano_cases as MC

pytestmark = pytest.mark.gpu

SEED = 411
GUARD = 256          # bytes
FILL = 0xA5


@pytest.fixture(scope="module")
def assets(mano_arrays):
    right, left = mano_arrays
    return {"right": right, "left": left, "dense": MC.dense_weight_asset(right)}


@pytest.fixture(scope="module")
def layers(assets):
    from ihmr_amd import mano
    assert torch.cuda.is_available()
    return {k: mano.MANO(a, is_rhand=k != "left").to("cuda:0") for k, a in assets.items()}


@pytest.fixture(scope="module")
def truth(assets):
    """(case, float64 oracle, float32 oracle) per (asset, class, N, seed[, which upstream gradients]): computed once, read-only."""
    @functools.lru_cache(maxsize=None)
    def get(asset, name, N, seed=SEED, use_gv=True, use_gj=True):
        c = MC.case(name, N, seed, assets[asset]["hands_mean"])
        f64 = MC.reference(assets[asset], c, torch.float64, use_gv, use_gj)
        o32 = MC.reference(assets[asset], c, torch.float32, use_gv, use_gj)
        for d in (c, f64, o32):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return c, f64, o32
    return get


def _up(a):
    return torch.from_numpy(np.array(a)).cuda()


def _forward(layer, c, need=(True, True, True)):
    o, p, b = (_up(c[k]).requires_grad_(n) for k, n in zip(("orient", "pose", "betas"), need))
    out = layer(global_orient=o, hand_pose=p, betas=b)
    return out, (o, p, b)


def _backward(out, leaves, c, use_gv=True, use_gj=True):
    loss = 0.0
    if use_gv:
        loss = loss + (out.vertices * _up(c["gv"])).sum()
    if use_gj:
        loss = loss + (out.joints * _up(c["gj"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = dict(verts=out.vertices.detach().cpu().numpy(), joints=out.joints.detach().cpu().numpy())
    for k, t in zip(("d_orient", "d_pose", "d_betas"), leaves):
        if t.grad is not None:
            res[k] = t.grad.cpu().numpy()
    return res


def _run_layer(layer, c, need=(True, True, True), use_gv=True, use_gj=True):
    """The case through the autograd layer: verts, joints and the requested gradients, float32 arrays."""
    out, leaves = _forward(layer, c, need)
    return _backward(out, leaves, c, use_gv, use_gj)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------------- 1. every launch form
@pytest.mark.parametrize("N,asset", [(N, "right") for N in MC.N_LIST] + [(9, "left"), (257, "left")])
def test_forward_and_gradients_at_every_launch_form(layers, truth, N, asset):
    """`mixed` hands (class k % 6 in hand k) through the layer with all three inputs requiring grad: verts, joints, d_orient, d_pose,
    d_betas each `within` the bound -- over all hands, and over the hands of each pose class by themselves, so that a mild hand is
    not judged by the tiny4 hand's ill-conditioned bound next to it."""
    c, f64, o32 = truth(asset, "mixed", N)
    got = _run_layer(layers[asset], c)
    MC.check_outputs(f"N={N} {asset} mixed", got, f64, o32)
    cls = MC.class_of_hand("mixed", N)
    for i, name in enumerate(MC.CLASSES):
        rows = np.nonzero(cls == i)[0]
        if rows.size:
            MC.check_outputs(f"N={N} {asset} mixed/{name}", got, f64, o32, rows)


# ----------------------------------------------------------------------------------- 2. every pose class
@pytest.mark.parametrize("name", MC.CLASSES + ("mixed",))
def test_every_pose_class_at_33_hands(layers, truth, name):
    """Forward and gradients of each pose class at N = 33, `within` the bound.  The rotation gradients near a zero rotation are where
    float32 is ill-conditioned (tests/test_mano_cases_cpu.py::test_conditioning_table): the ratios |hip - f64| / |oracle32 - f64|
    printed here are recorded in DESIGN.md ("MANO layer: distances from the float64 oracle").  Measured on the MI355X, d_orient / d_pose:
    zero 0.80 / 0.53, tiny6 1.00 / 1.03, tiny4 0.92 / 1.00, tiny3 1.00 / 1.01 (mild 1.21 / 0.56 and large 1.00 / 0.72, both far inside the
    floor): near a zero rotation the kernels lose what torch's float32 loses, no more."""
    c, f64, o32 = truth("right", name, 33)
    got = _run_layer(layers["right"], c)
    ratios = MC.check_outputs(f"N=33 right {name}", got, f64, o32)
    print(f"[mano] N=33 {name}: ratio d_orient {ratios['d_orient']:.2f}  d_pose {ratios['d_pose']:.2f}")


# ----------------------------------------------------------------------------------- 3. permutation
@pytest.mark.parametrize("N", [33, 321])
def test_permuted_hands_give_permuted_bits(layers, truth, N):
    """One launch form, one summation order per hand: the hands in another order (other skin slots, other packed-pair partners, other
    GEMM tile rows, other tail positions) give the same bits per hand, in every output."""
    c, _, _ = truth("right", "mixed", N)
    perm = np.random.RandomState(SEED + N).permutation(N)
    assert not np.array_equal(perm, np.arange(N))
    a = _run_layer(layers["right"], c)
    b = _run_layer(layers["right"], MC.permuted(c, perm))
    for k in MC.OUTPUTS:
        bad = [int(i) for i in range(N) if not _same_bits(b[k][i], a[k][perm[i]])]
        assert not bad, (k, "hands whose bits depend on their position", [(i, int(perm[i])) for i in bad[:8]], len(bad))


# ----------------------------------------------------------------------------------- C ABI helpers (4, 5)
class _Buf:
    """`nbytes` of device memory followed directly by a guard region, all filled with FILL, in one ordinary allocation."""

    def __init__(self, nbytes, guard=GUARD):
        self.nbytes = nbytes
        self.t = torch.full((nbytes + guard,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def floats(self):
        return self.t[:self.nbytes].cpu().numpy().view(np.float32)

    def untouched(self):
        return bool((self.t[:self.nbytes] == FILL).all().item())

    def guard_intact(self):
        return bool((self.t[self.nbytes:] == FILL).all().item())


def _abi_forward(layer, c):
    """ihmr_mano_lbs_fwd on fresh guarded buffers; the workspace is exactly ihmr_mano_workspace_bytes(N) bytes (+ its guard)."""
    from ihmr_amd import hip
    L, N = hip.lib(), c["N"]
    st = dict(N=N, handle=layer._handle().handle, inputs=[_up(c[k]) for k in ("orient", "pose", "betas")],
              verts=_Buf(N * 778 * 3 * 4), joints=_Buf(N * 16 * 3 * 4), ws=_Buf(int(L.ihmr_mano_workspace_bytes(N))))
    hip.check(L.ihmr_mano_lbs_fwd(st["handle"], *(hip.ptr(t) for t in st["inputs"]), N, st["verts"].ptr, st["joints"].ptr, st["ws"].ptr,
                                  hip.stream_ptr()), "ihmr_mano_lbs_fwd")
    return st


def _abi_backward(st, c, mask):
    from ihmr_amd import hip
    N = st["N"]
    gv, gj = _up(c["gv"]), _up(c["gj"])
    g = dict(d_orient=_Buf(N * 3 * 4), d_pose=_Buf(N * 45 * 4), d_betas=_Buf(N * 10 * 4))
    hip.check(hip.lib().ihmr_mano_lbs_bwd(st["handle"], N, st["ws"].ptr, hip.ptr(gv), hip.ptr(gj), g["d_orient"].ptr, g["d_pose"].ptr,
                                          g["d_betas"].ptr, mask, hip.stream_ptr()), "ihmr_mano_lbs_bwd")
    torch.cuda.synchronize()
    return g


MASK_BIT = {"d_orient": 1, "d_pose": 2, "d_betas": 4}


# ----------------------------------------------------------------------------------- 4. need_mask
@pytest.mark.parametrize("asset", ["right", "dense"])
def test_need_mask_requested_bits_and_untouched_buffers(layers, truth, asset):
    """ihmr_mano_lbs_bwd with each of the seven non-empty masks on one forward's workspace, N = 33: a requested gradient has the bits of
    the all-mask run, an unrequested buffer keeps its fill.

    `dense` (up to seven weights per vertex, the 16-joint loops): need_mask only leaves work out, all seven masks bit for bit.
    `right` (the 4-sparse asset, short loops): the same for masks 2 - 7.  Mask 1 there is not the same sum with work left out:
    lbs_bwd1_hand takes its orientation-stage form (d L / d R0 as one 3 x 3 reduction over the re-skinned vertices instead of the
    per-joint segmented sums and the chain backward; `(need_mask & 7) == 1 && m.sparse4`), another summation order by design, whose
    bits are not the all-mask run's (measured: 1.4e-6 apart at a largest gradient of 6.6).  That one gradient is held to `within` against float64 instead, and to the bits of the same
    form reached through the layer (only `global_orient` requiring grad); its distance from the all-mask bits is printed."""
    c, f64, o32 = truth(asset, "mixed", 33)
    sparse4 = int((np.asarray(layers[asset]._arrays["lbs_weights"], np.float32) != 0).sum(axis=1).max()) <= 4
    assert sparse4 == (asset == "right")
    st = _abi_forward(layers[asset], c)
    full = {k: b.floats() for k, b in _abi_backward(st, c, 7).items()}
    shaped = dict(full, verts=st["verts"].floats(), joints=st["joints"].floats())
    MC.check_outputs(f"N=33 {asset} C ABI mask 7", {k: v.reshape(f64[k].shape) for k, v in shaped.items()}, f64, o32)
    wrong = []
    for mask in (1, 2, 3, 4, 5, 6, 7):
        g = _abi_backward(st, c, mask)
        for k, b in g.items():
            assert b.guard_intact(), (mask, k)
            if mask == 1 and k == "d_orient" and sparse4:
                got = b.floats().reshape(33, 3)
                print(f"[mano] {asset} need_mask 1 d_orient (orientation-stage form): max distance from the all-mask bits "
                      f"{np.abs(got.astype(np.float64) - full[k].reshape(33, 3)).max():.3e}")
                MC.within(got, f64[k], o32[k], MC.floor_of(k, f64[k]), f"N=33 {asset} C ABI mask 1 {k}")
                via_layer = _run_layer(layers[asset], c, need=(True, False, False))
                assert set(via_layer) == {"verts", "joints", "d_orient"} and _same_bits(got, via_layer[k])
            elif mask & MASK_BIT[k]:
                if not _same_bits(b.floats(), full[k]):
                    d = np.abs(b.floats().astype(np.float64) - full[k]).max()
                    print(f"[mano] {asset} need_mask {mask} {k}: differs from the all-mask run by {d:.3e} (max|.| {np.abs(full[k]).max():.3e})")
                    wrong.append((mask, k, float(d)))
            else:
                assert b.untouched(), (mask, k, "an unrequested buffer was written")
    assert not wrong, ("requested gradients that are not the all-mask run's bits", wrong)


@pytest.mark.parametrize("which", ["joints only", "verts only"])
def test_loss_on_one_output_only(layers, truth, which):
    """A loss on the joints alone (autograd hands the layer no vertex gradient) and on the vertices alone, N = 33, against the oracle."""
    use_gv, use_gj = which == "verts only", which == "joints only"
    c, f64, o32 = truth("right", "mixed", 33, SEED, use_gv, use_gj)
    got = _run_layer(layers["right"], c, use_gv=use_gv, use_gj=use_gj)
    MC.check_outputs(f"N=33 right mixed, loss on the {which}", got, f64, o32)


def test_absent_output_gradients_are_zeros(layers, truth):
    """`_LbsFunction.backward` with d_verts = None / d_joints = None (a caller that does not materialise absent gradients): the bits of the
    same backward with explicit zeros."""
    from ihmr_amd.mano import _LbsFunction
    c, _, _ = truth("right", "mixed", 33)
    layer = layers["right"]

    class Once(torch.autograd.Function):
        """The layer's function with materialisation of absent output gradients switched off."""
        @staticmethod
        def forward(ctx, o, p, b):
            ctx.set_materialize_grads(False)
            return _LbsFunction.forward(ctx, o, p, b, layer)

        @staticmethod
        def backward(ctx, dv, dj):
            seen.append((dv is None, dj is None))
            return _LbsFunction.backward(ctx, dv, dj)[:3]

    for use_gv, use_gj in ((False, True), (True, False)):
        seen = []
        o, p, b = (_up(c[k]).requires_grad_(True) for k in ("orient", "pose", "betas"))
        v, j = Once.apply(o, p, b)
        ((v * _up(c["gv"])).sum() if use_gv else (j * _up(c["gj"])).sum()).backward()
        torch.cuda.synchronize()
        assert seen == [(not use_gv, not use_gj)]
        ref = _run_layer(layer, c, use_gv=use_gv, use_gj=use_gj)
        for k, t in zip(("d_orient", "d_pose", "d_betas"), (o, p, b)):
            assert _same_bits(t.grad.cpu().numpy(), ref[k]), (use_gv, use_gj, k)


# ----------------------------------------------------------------------------------- 5. guards
@pytest.mark.parametrize("N", [9, 257])
def test_guard_regions_behind_every_buffer_stay_intact(layers, truth, N):
    """verts, joints, the three gradients and the workspace (exactly ihmr_mano_workspace_bytes(N) bytes, filled with 0xA5 like its guard)
    each with a guard region directly behind them: after forward + backward every guard byte is intact, every output byte was written
    by the kernels' own arithmetic (the layer's bits), and nothing depends on what the workspace held before."""
    c, _, _ = truth("right", "mixed", N)
    st = _abi_forward(layers["right"], c)
    g = _abi_backward(st, c, 7)
    for k, b in dict(g, verts=st["verts"], joints=st["joints"], ws=st["ws"]).items():
        assert b.guard_intact(), (N, k, "guard region written")
    ref = _run_layer(layers["right"], c)
    for k in ("verts", "joints"):
        assert _same_bits(st[k].floats(), ref[k].reshape(-1)), k
    for k, b in g.items():
        assert _same_bits(b.floats(), ref[k].reshape(-1)), k


# ----------------------------------------------------------------------------------- 6. two autograd graphs alive
def test_two_forwards_alive_backward_in_reverse_order(layers, truth):
    """Two forwards (N = 9 and N = 33, different inputs) before either backward, the backwards in reverse order: each forward owns its
    workspace, so each gradient has the bits of its single run."""
    layer = layers["right"]
    ca, cb = truth("right", "mild", 9, SEED + 1)[0], truth("right", "mild", 33, SEED + 2)[0]
    single_a, single_b = _run_layer(layer, ca), _run_layer(layer, cb)
    out_a, leaves_a = _forward(layer, ca)
    out_b, leaves_b = _forward(layer, cb)
    got_b = _backward(out_b, leaves_b, cb)
    got_a = _backward(out_a, leaves_a, ca)
    for got, single, tag in ((got_a, single_a, "N=9"), (got_b, single_b, "N=33")):
        for k in MC.OUTPUTS:
            assert _same_bits(got[k], single[k]), (tag, k)
    _, f64, o32 = truth("right", "mild", 33, SEED + 2)
    MC.check_outputs("N=33 right mild (second graph)", got_b, f64, o32)


# ----------------------------------------------------------------------------------- 7. dense weights
def test_dense_weight_asset_at_a_ragged_hand_count(layers, truth):
    """The 16-joint skinning loops (an asset with up to seven weights per vertex) at N = 33: real neighbours in the slots, two hand groups."""
    c, f64, o32 = truth("dense", "mixed", 33)
    got = _run_layer(layers["dense"], c)
    MC.check_outputs("N=33 dense mixed", got, f64, o32)
    cls = MC.class_of_hand("mixed", 33)
    for i, name in enumerate(MC.CLASSES):
        MC.check_outputs(f"N=33 dense mixed/{name}", got, f64, o32, np.nonzero(cls == i)[0])

"""The pose-gradient GEMM of the MANO backward, LDS form (`lbs_bwd2_lds_kernel`, csrc/mano_lbs.h) against the streaming form
(`lbs_bwd2_kernel`, unchanged, selected with `ihmr_debug_force_lbs_bwd2_streaming(1)`): bit for bit.

The LDS form gives a workgroup of four waves a unit of T = 32 hands x one K group: one 32-feature tile per wave on
v_mfma_f32_32x32x2_f32 and the seven leftover features 128..134 as a 16-row tile on v_mfma_f32_16x16x4_f32, whose four k values per step
are fed in the order the 32-row chain meets them.  Both are k-ordered fmaf chains, so every bit of d hand_pose must be the streaming
form's.  The upstream vertex gradient here is DENSE (the refinement loop's own d v_posed is about 94 % zeros and would hide a wrong k
assignment or a dropped chunk); d global_orient and d betas come from the per-hand launch in front of the GEMM and are compared too.

Hand counts: 256 the smallest LDS launch, all tiles full; 257 one real hand in a ragged tile; 256 + T - 1 and 256 + T + 1 the last row of
one tile and the first row of the next; 321.  One more case has the upstream gradient non-zero only in the last vertex (columns
2331..2333: the half-valid last group of four columns) of the last of 257 hands (the ragged tile).
Every output sits in front of a guard region (as in tests/test_gpu_mano_layer.py), the workspace is exactly its stated size."""
import ctypes as C

import numpy as np
import pytest
import torch

import mano_cases as MC

pytestmark = pytest.mark.gpu

SEED = 1907
GUARD = 256          # bytes
FILL = 0xA5
T = 32               # csrc/mano_lbs.h: LBS_B2_HANDS


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

    def guard_intact(self):
        return bool((self.t[self.nbytes:] == FILL).all().item())


@pytest.fixture(scope="module")
def layer(mano_arrays):
    from ihmr_amd import mano
    assert torch.cuda.is_available()
    return mano.MANO(mano_arrays[0], is_rhand=True).to("cuda:0")


def _up(a):
    return torch.from_numpy(np.array(a)).cuda()


def _abi_gradients(layer, c, streaming):
    """Forward + backward through the C ABI on fresh guarded buffers with the form switch set; the switch is put back."""
    from ihmr_amd import hip
    L, N = hip.lib(), c["N"]
    handle = layer._handle().handle
    inputs = [_up(c[k]) for k in ("orient", "pose", "betas")]
    gv, gj = _up(c["gv"]), _up(c["gj"])
    bufs = dict(verts=_Buf(N * 778 * 3 * 4), joints=_Buf(N * 16 * 3 * 4), ws=_Buf(int(L.ihmr_mano_workspace_bytes(N))),
                d_orient=_Buf(N * 3 * 4), d_pose=_Buf(N * 45 * 4), d_betas=_Buf(N * 10 * 4))
    L.ihmr_debug_force_lbs_bwd2_streaming(1 if streaming else 0)
    try:
        hip.check(L.ihmr_mano_lbs_fwd(handle, *(hip.ptr(t) for t in inputs), N, bufs["verts"].ptr, bufs["joints"].ptr, bufs["ws"].ptr,
                                      hip.stream_ptr()), "ihmr_mano_lbs_fwd")
        hip.check(L.ihmr_mano_lbs_bwd(handle, N, bufs["ws"].ptr, hip.ptr(gv), hip.ptr(gj), bufs["d_orient"].ptr, bufs["d_pose"].ptr,
                                      bufs["d_betas"].ptr, 7, hip.stream_ptr()), "ihmr_mano_lbs_bwd")
        torch.cuda.synchronize()
    finally:
        L.ihmr_debug_force_lbs_bwd2_streaming(0)
    for k, b in bufs.items():
        assert b.guard_intact(), (N, streaming, k, "guard region written")
    return {k: bufs[k].floats() for k in ("d_orient", "d_pose", "d_betas")}


def _layer_gradients(layer, c):
    """The same case through the autograd layer (default form)."""
    o, p, b = (_up(c[k]).requires_grad_(True) for k in ("orient", "pose", "betas"))
    out = layer(global_orient=o, hand_pose=p, betas=b)
    ((out.vertices * _up(c["gv"])).sum() + (out.joints * _up(c["gj"])).sum()).backward()
    torch.cuda.synchronize()
    return dict(d_orient=o.grad.cpu().numpy().reshape(-1), d_pose=p.grad.cpu().numpy().reshape(-1), d_betas=b.grad.cpu().numpy().reshape(-1))


def _compare(tag, N, got, ref):
    for k in ("d_pose", "d_orient", "d_betas"):
        a, b = got[k].view(np.uint32), ref[k].view(np.uint32)
        assert a.shape == b.shape, (tag, k)
        bad = np.flatnonzero(a != b)
        width = a.size // N
        d = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        print(f"[bwd2] {tag} {k}: {bad.size} of {a.size} words differ from the streaming form, max |difference| {d:.3e}, "
              f"max |value| {np.abs(ref[k]).max():.3e}")
        assert bad.size == 0, (tag, k, "first (hand, column) that differ", [(int(i) // width, int(i) % width) for i in bad[:8]])


@pytest.mark.parametrize("N", [256, 257, 256 + T - 1, 256 + T + 1, 321])
def test_lds_form_has_the_streaming_forms_bits_on_a_dense_gradient(layer, mano_arrays, N):
    c = MC.case("mixed", N, SEED, mano_arrays[0]["hands_mean"])
    assert float((c["gv"] != 0).mean()) > 0.99
    ref = _abi_gradients(layer, c, streaming=True)
    got = _abi_gradients(layer, c, streaming=False)
    assert np.isfinite(ref["d_pose"]).all() and np.abs(ref["d_pose"]).max() > 0
    _compare(f"N={N}", N, got, ref)
    via_layer = _layer_gradients(layer, c)
    _compare(f"N={N} autograd layer", N, via_layer, ref)


def test_last_vertex_of_the_last_ragged_hand(layer, mano_arrays):
    N = 257
    c = MC.case("mixed", N, SEED + 1, mano_arrays[0]["hands_mean"])
    gv = np.zeros_like(c["gv"])
    gv[N - 1, 777] = c["gv"][N - 1, 777]
    c = dict(c, gv=gv, gj=np.zeros_like(c["gj"]))
    ref = _abi_gradients(layer, c, streaming=True)
    got = _abi_gradients(layer, c, streaming=False)
    pose = ref["d_pose"].reshape(N, 45)
    assert np.abs(pose[N - 1]).max() > 0, "the one non-zero gradient must reach the last hand's pose"
    assert not pose[:N - 1].any(), "and nobody else's"
    _compare("last vertex, last hand of 257", N, got, ref)

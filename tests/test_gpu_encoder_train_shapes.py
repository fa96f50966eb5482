"""Every launch of the training BACKWARD pass at its real batch-64 shape, through the wrappers of ``ihmr_amd.encoder_train`` with the
strides the trainer passes.  The table, the restated ``ihmr_conv_wgrad`` selection and the operand draws come from
tests/encoder_train_shapes.py (checked on the CPU by tests/test_encoder_train_shapes_cpu.py); guards, NaN workspace and fingerprint
helpers are those of tests/test_gpu_encoder_shapes.py.  Per weight-gradient and input-gradient geometry:

* small-integer operands -> every partial sum of any order is exact in fp32 -> float64 ``conv2d_weight`` / ``conv2d_input`` of the
  same numbers, cast back, must equal the kernel's output in EVERY element, and a second launch must give the same bits;
* the output lives inside a larger buffer pre-filled with a NaN bit pattern: everything outside it comes back untouched (for dW that
  includes the padding columns Cout..ldw and the rows K..ceil16(K));
* the workspace is pre-filled with the NaN pattern: no NaN reaches the output and the words that changed are exactly the predicted
  ones (msplit * K * Cout floats for the weight gradient; nothing, or the Stream-K slots, for an input-gradient launch); dW is bit for
  bit the predicted reduce kernel's fixed-order sum of the partials left there;
* random operands against float64: the weight gradient under the project's rule (no further from float64 than 3 x CPU torch-fp32 +
  1e-6 max|ref|, ratio printed), the input gradient at the forward test's allowance 3e-5 + 1e-5 |ref|.

Then the pooling / mask backward kernels and the four heads at their real sizes, and the composed step: two fresh trainers at B = 64
give bit-identical, finite gradients with zeros in every padding position of the flat layout."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_shapes as E  # noqa: E402
import encoder_train_shapes as TS  # noqa: E402
import test_gpu_encoder_shapes as G  # noqa: E402
from test_gpu_encoder_train import _vs_float64  # noqa: E402

pytestmark = pytest.mark.gpu

B = 64
NAN32, GUARD_ROWS = G.NAN32, G.GUARD_ROWS
WGRAD = TS.wgrad_table(B)
DGRAD = TS.dgrad_table(B)
_ids = lambda s: s.name
_dids = lambda d: f"{d.kind}-{d.unit.name}"


def _ceil(x, m):
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def _wgrad_workspace():
    """The 256 MB buffer conv_wgrad keeps per (device, stream), as an int32 view; a tiny first call allocates it as the trainer's does."""
    from ihmr_amd import encoder_train as T
    dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    if key not in T._WG_WS:
        z = torch.zeros(16, 64, device=dev)
        T.conv_wgrad(z, z, 1, 4, 4, 64, 64, 1, 1, 0)
        torch.cuda.synchronize()
    ws = T._WG_WS[key]
    assert ws.numel() * 4 == TS.WGRAD_WORKSPACE_BYTES
    return ws.view(torch.int32)


def _outside_touched(raw, rows, ld, r_used, c_used):
    """Words of a [GUARD_ROWS + rows + GUARD_ROWS][ld] NaN-pattern buffer outside [r_used][c_used] that no longer hold the pattern."""
    chk = raw.clone().view(rows + 2 * GUARD_ROWS, ld)
    chk[GUARD_ROWS:GUARD_ROWS + r_used, :c_used] = NAN32
    return int((chk != NAN32).sum())


def _restated_reduce(part, kind):
    """The fixed summation order of the two reduce kernels applied to the partials [msplit][K][Cout] a launch left in the workspace
    (plain fp32 additions, so torch reproduces them bit for bit).  wgrad_reduce_kernel: sixteen group sums (group g: partials g, g + 16,
    ... added to 0 in ascending order), then the groups in ascending order; conv_splitk_reduce_kernel: the partials in ascending order,
    then + 0 (its absent bias).  The two orders coincide up to 16 partials and differ above."""
    if kind == "wgrad_reduce":
        groups = []
        for g in range(16):
            s = torch.zeros_like(part[0])
            for z in range(g, part.shape[0], 16):
                s = s + part[z]
            groups.append(s)
        t = groups[0]
        for q in range(1, 16):
            t = t + groups[q]
        return t
    v = part[0].clone()
    for z in range(1, part.shape[0]):
        v = v + part[z]
    return v + 0.0


def _wgrad_launch(u, xd, dyd, other_order=None):
    """One ihmr_conv_wgrad launch through encoder_train.conv_wgrad into dW [ceil16(K)][ldw] inside a guarded NaN-pattern buffer, over the
    NaN-filled workspace; asserts guards, absence of NaN, the workspace fingerprint, and that dW is bit for bit the predicted reduce
    kernel's sum of the partials in the workspace (which pins WHICH reduce kernel ran wherever the two orders differ; `other_order`: a
    list that receives whether the other kernel's order gives different bits).  Returns the [K][Cout] view."""
    from ihmr_amd import encoder_train as T
    _, K = E.gemm_dims(u)
    Kp, ldw = _ceil(K, 16), E.packed_ldw(u.Cout)
    plan = TS.plan_wgrad(u)
    raw, out = G._guarded(Kp, ldw, "fp32", 0, ldw)
    wsi = _wgrad_workspace()
    wsi.fill_(NAN32)
    got = T.conv_wgrad(xd, dyd, u.N, u.H, u.W, u.Cin, u.Cout, u.k, u.stride, u.pad, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and out.shape == (Kp, ldw)
    dw = out[:K, :u.Cout]
    touched = _outside_touched(raw, Kp, ldw, K, u.Cout)
    nans = int(torch.isnan(dw).sum())
    changed = wsi != NAN32
    fperr = int((~changed[:plan["prefix"]]).sum()) + int(changed[plan["prefix"]:].sum())
    assert touched == 0, f"{u.name}: {touched} words outside dW [K][Cout] were written (padding rows / columns / guards)"
    assert nans == 0, f"{u.name}: {nans} NaN in dW (an unwritten partial was read)"
    assert fperr == 0, f"{u.name}: workspace fingerprint differs from the plan {plan} in {fperr} words"
    part = wsi.view(torch.float32)[:plan["prefix"]].view(plan["msplit"], K, u.Cout)
    assert G._same_bits(dw, _restated_reduce(part, plan["reduce"])), f"{u.name}: dW is not {plan['reduce']}'s sum of the {plan['msplit']} partials"
    if other_order is not None:
        other = "splitk_reduce4" if plan["reduce"] == "wgrad_reduce" else "wgrad_reduce"
        other_order.append(not G._same_bits(dw, _restated_reduce(part, other)))
    return dw


@pytest.mark.parametrize("u", WGRAD, ids=_ids)
def test_wgrad_exact_on_integers(u):
    """Zero mismatching elements out of K * Cout against float64 conv2d_weight; the same bits on a second launch; guards, NaN and
    workspace fingerprint on both launches (``_wgrad_launch``)."""
    torch.set_num_threads(16)
    plan = TS.plan_wgrad(u)
    x, dy = TS.draw_wgrad_integers(u)
    ref = TS.wgrad_reference(u, x, dy)                                  # float64, CPU
    top = float(ref.abs().max())
    assert top <= TS.wgrad_integer_bound(u) < 2 ** 24, (u.name, top)
    ref = ref.float().cuda()
    xd, dyd = x.view(-1, u.Cin).cuda(), dy.view(-1, u.Cout).cuda()
    assert (xd.shape[1], dyd.shape[1]) == (u.ldx, u.ldy)
    dw = _wgrad_launch(u, xd, dyd)
    dw2 = _wgrad_launch(u, xd, dyd)
    bad = int((dw != ref).sum())
    print(f"[parity] encoder wgrad {u.name} B={B} form={plan['form']} (tile {plan['tile'][0]}x{plan['tile'][1]}, msplit={plan['msplit']}, last slice "
          f"{plan['last']} of {plan['chunks_per']} chunks, {plan['reduce']}): exact on integers, max|dW|={top:.0f} mismatches={bad} of {ref.numel()}")
    assert bad == 0, (u.name, bad, float((dw - ref).abs().max()))
    assert G._same_bits(dw, dw2), f"{u.name}: second launch differs"


def test_wgrad_refuses_2_23_pixels():
    """N * Ho * Wo >= 2^23 is outside the range of the kernel's reciprocal pixel division: the launcher returns an error before any
    launch and hip.check raises.  (The buffers have the full size the shape claims.)"""
    from ihmr_amd import encoder_train as T
    u = WGRAD[0]._replace(N=669)
    M, _ = E.gemm_dims(u)
    assert u.name == "stem" and M >= TS.WGRAD_MAX_PIXELS > E.gemm_dims(u._replace(N=668))[0] and TS.plan_wgrad(u) is None
    x = torch.empty(u.N * u.H * u.W, u.Cin, device="cuda")
    dy = torch.empty(M, u.Cout, device="cuda")
    with pytest.raises(RuntimeError, match="ihmr_conv_wgrad"):
        T.conv_wgrad(x, dy, u.N, u.H, u.W, u.Cin, u.Cout, u.k, u.stride, u.pad)
    torch.cuda.synchronize()


@pytest.mark.parametrize("u", WGRAD, ids=_ids)
def test_wgrad_random_against_float64(u):
    """The project's rule (``_vs_float64``): max |dW - float64| <= 3 x that of CPU torch-fp32 conv2d_weight + 1e-6 max|ref|, on randn
    operands at unit output scale.  The bar is tied to torch-fp32, never to the kernel's own error.  Printed: the ratio and the
    length of the kernel's fp32 chain per slice (chunks_per * 16 pixels).  Also: dW carries the bits of the predicted reduce kernel's
    summation order and, above 16 partials, not those of the other kernel's."""
    torch.set_num_threads(16)
    plan = TS.plan_wgrad(u)
    x, dy = TS.draw_wgrad_random(u)
    ref = TS.wgrad_reference(u, x, dy)
    t32 = TS.wgrad_reference(u, x, dy, torch.float32)
    e_torch = float((t32.double() - ref).abs().max())
    differs = []
    dw = _wgrad_launch(u, x.view(-1, u.Cin).cuda(), dy.view(-1, u.Cout).cuda(), other_order=differs)
    # above 16 partials the two reduce kernels add in different orders: on random operands the bits tell which one ran
    assert differs[0] == (plan["msplit"] > 16), (u.name, plan["msplit"], differs)
    e_kernel = float((dw.double().cpu() - ref).abs().max())
    top = float(ref.abs().max())
    print(f"[parity] encoder wgrad {u.name} B={B} form={plan['form']}: random operands, chain {plan['chunks_per'] * 16} pixels x {plan['msplit']} "
          f"slices, max|err|={e_kernel:.3e} max|ref|={top:.3e} torch-fp32 max|err|={e_torch:.3e} ratio={e_kernel / e_torch:.2f}")
    _vs_float64(f"encoder wgrad {u.name}", e_kernel, e_torch, 1e-6 * top)


# ---------------------------------------------------------------------------------------------------------------- input gradient
def _turned_launch(s, xd, wpk, rd):
    """One ihmr_conv_igemm launch of the backward pass into a guarded buffer over the NaN-filled split-K workspace, with the argument
    list of encoder_train.conv_forward (square filters: the wrapper itself) / conv_dgrad_s2_3x3 (phase filters: restated, the wrapper
    allocates its own outputs); asserts guards, NaN and the workspace fingerprint for this device's CU count."""
    from ihmr_amd import encoder_train as T, hip
    M, _ = E.gemm_dims(s)
    Ho, Wo = E.out_hw(s)
    kh, kw = E.filter_hw(s)
    plan = E.plan_fp32(s, G._cus())
    assert (xd.shape[1], wpk.shape[1], 0 if rd is None else rd.shape[1]) == (s.ldx, E.packed_ldw(s.Cout), s.ldr)
    raw, y = G._guarded(M, s.ldy, "fp32", 0, s.Cout)
    assert s.ldy == s.Cout and y.is_contiguous()
    wsi = G._workspace()
    wsi.fill_(NAN32)
    if kh == kw and s.Ho is None:
        out, ho, wo = T.conv_forward(xd, wpk, s.N, s.H, s.W, s.Cin, s.Cout, kh, 1, s.pad, out=y, residual=rd)
        assert (ho, wo) == (Ho, Wo) and out.data_ptr() == y.data_ptr()
    else:
        assert rd is None and s.pad == 0 and (Ho, Wo) == (s.H, s.W)
        ws = wsi.view(torch.float32)
        hip.check(hip.lib().ihmr_conv_igemm(hip.ptr(xd), hip.ptr(wpk), None, None, hip.ptr(y), s.N, s.H, s.W, s.Cin, Ho, Wo, s.Cout, kh, kw, 1, 0,
                                            xd.shape[1], wpk.shape[1], s.Cout, 0, 0, ws.data_ptr(), ws.numel() * 4, hip.stream_ptr()), "ihmr_conv_igemm")
    torch.cuda.synchronize()
    touched = G._guards_intact(raw, M, s.ldy, 0, s.Cout)
    nans = int(torch.isnan(y).sum())
    fperr = G._footprint_errors(wsi, E.workspace_footprint(s, plan))
    assert touched == 0, f"{s.name}: {touched} words outside [M][Cout] were written"
    assert nans == 0, f"{s.name}: {nans} NaN in the output (unwritten workspace or output read)"
    assert fperr == 0, f"{s.name}: workspace fingerprint differs from the plan {plan} in {fperr} words"
    return y, plan["form"]


def _dgrad_weights(u, w):
    """The operands the trainer derives from the forward-packed master weight (``_refresh_derived``): the flipped, transposed filter by
    ihmr_pack_dgrad_weight (checked against the host packing), and for a 3 x 3 / stride-2 unit the four phase filters."""
    from ihmr_amd import encoder_train as T, hip
    wf = T.pack_forward_weight(w).cuda()
    wd = torch.zeros(_ceil(u.k * u.k * u.Cout, 16), E.packed_ldw(u.Cin), device="cuda")
    hip.check(hip.lib().ihmr_pack_dgrad_weight(hip.ptr(wf), hip.ptr(wd), u.k, u.k, u.Cin, u.Cout, wf.shape[1], wd.shape[1], hip.stream_ptr()),
              "ihmr_pack_dgrad_weight")
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu(), T.pack_dgrad_weight(w)), f"{u.name}: ihmr_pack_dgrad_weight differs from the host packing"
    phases = None
    if TS.dgrad_route(u) == "phase":
        phases = [p.cuda() for p in T.pack_dgrad_phase_weights(T.unpack_wgrad(wf, (u.Cout, u.Cin, 3, 3)))]
    return wd, phases


def _mismatches(name, route, form, got, ref):
    bad = int((got != ref).sum())
    print(f"[parity] encoder dgrad {name} B={B} route={route} form={form}: exact on integers, max|dx|={float(ref.abs().max()):.0f} "
          f"mismatches={bad} of {ref.numel()}")
    return bad


@pytest.mark.parametrize("d", DGRAD, ids=_dids)
def test_dgrad_exact_on_integers(d):
    """Zero mismatching elements out of N * H * W * Cin against float64 conv2d_input (+ the skip gradient where the trainer adds one),
    for every route: the stride-1 turned convolution; the downsample GEMM + dilate2 (odd pixels exactly zero); the four parity phases
    + interleave2 AND the zero-insertion route of conv_dgrad for the 3 x 3 / stride-2 units.  Each igemm launch: guards, NaN,
    workspace fingerprint, the same bits on a second launch; the trainer's own wrapper gives the same bits as the guarded launches."""
    from ihmr_amd import encoder_train as T, hip
    torch.set_num_threads(16)
    u = d.unit
    dy, w, r = TS.draw_dgrad(d, "int")
    ref = TS.dgrad_reference(u, dy, w, r)
    top = float(ref.abs().max())
    assert top <= TS.dgrad_integer_bound(u) < 2 ** 24
    ref = ref.float().cuda()
    dyd = dy.view(-1, u.Cout).cuda()
    rd = None if r is None else r.cuda()
    wd, phases = _dgrad_weights(u, w)
    Ho, Wo = E.out_hw(u)
    args = (u.N, u.H, u.W, u.Cin, u.Cout)
    if d.kind == "s1":
        s, = d.shapes
        y, form = _turned_launch(s, dyd, wd, rd)
        y2, _ = _turned_launch(s, dyd, wd, rd)
        dx = T.conv_dgrad(dyd, wd, *args, u.k, u.stride, u.pad, residual=rd)
        torch.cuda.synchronize()
        assert _mismatches(u.name, "stride-1" + ("+skip" if s.residual else ""), form, y, ref) == 0
        assert G._same_bits(y, y2) and G._same_bits(y, dx), f"{u.name}: second launch / conv_dgrad differ"
    elif d.kind == "ds":
        s, = d.shapes
        small, form = _turned_launch(s, dyd, wd, None)
        small2, _ = _turned_launch(s, dyd, wd, None)
        dx = T.conv_dgrad(dyd, wd, *args, u.k, u.stride, u.pad)
        torch.cuda.synchronize()
        assert _mismatches(u.name, "gemm+dilate2", form, dx, ref) == 0
        v = dx.view(u.N, u.H, u.W, u.Cin)
        assert G._same_bits(small, small2) and G._same_bits(v[:, ::2, ::2].reshape(-1, u.Cin), small), f"{u.name}: even pixels differ from the GEMM"
        nz = int((dx.view(torch.int32) != 0).sum()) - int((v[:, ::2, ::2].contiguous().view(torch.int32) != 0).sum())
        print(f"[parity] encoder dgrad {u.name} dilate2: non-zero words at odd pixels={nz}")
        assert nz == 0
    else:
        outs, forms = [], []
        for s, wp in zip(d.shapes, phases):
            y, form = _turned_launch(s, dyd, wp, None)
            y2, _ = _turned_launch(s, dyd, wp, None)
            assert G._same_bits(y, y2), f"{s.name}: second launch differs"
            outs.append(y.contiguous()); forms.append(f"{E.filter_hw(s)[0]}x{E.filter_hw(s)[1]}:{form}")
        dx_a = torch.empty(u.N * u.H * u.W, u.Cin, device="cuda")
        hip.check(hip.lib().ihmr_interleave2(*(hip.ptr(p) for p in outs), hip.ptr(dx_a), u.N, Ho, Wo, u.Cin, hip.stream_ptr()), "ihmr_interleave2")
        dx_b = T.conv_dgrad_s2_3x3(dyd, phases, *args)
        dx_c = T.conv_dgrad(dyd, wd, *args, u.k, u.stride, u.pad)
        torch.cuda.synchronize()
        bad_a = _mismatches(u.name, "4 phases+interleave2", ",".join(forms), dx_a, ref)
        bad_b = _mismatches(u.name, "conv_dgrad_s2_3x3", ",".join(forms), dx_b, ref)
        bad_c = _mismatches(u.name, "zero insertion", E.plan_fp32(TS.zero_insertion_shape(u), G._cus())["form"], dx_c, ref)
        assert (bad_a, bad_b, bad_c) == (0, 0, 0), (u.name, bad_a, bad_b, bad_c)
        assert G._same_bits(dx_a, dx_b) and G._same_bits(dx_a, dx_c)


@pytest.mark.parametrize("d", DGRAD, ids=_dids)
def test_dgrad_random_against_float64(d):
    """The trainer's route on randn operands at unit output scale, whole output: |got - ref64| <= 3e-5 + 1e-5 |ref64| (the forward
    test's allowance).  Printed beside it: CPU torch-fp32 conv2d_input's own error."""
    from ihmr_amd import encoder_train as T
    torch.set_num_threads(16)
    u = d.unit
    dy, w, r = TS.draw_dgrad(d, "rnd")
    ref = TS.dgrad_reference(u, dy, w, r)
    e_torch = float((TS.dgrad_reference(u, dy, w, r, torch.float32).double() - ref).abs().max())
    dyd = dy.view(-1, u.Cout).cuda()
    wd, phases = _dgrad_weights(u, w)
    args = (u.N, u.H, u.W, u.Cin, u.Cout)
    if d.kind == "phase":
        dx = T.conv_dgrad_s2_3x3(dyd, phases, *args)
    else:
        dx = T.conv_dgrad(dyd, wd, *args, u.k, u.stride, u.pad, residual=None if r is None else r.cuda())
    torch.cuda.synchronize()
    refd = ref.cuda()
    err, bound = (dx.double() - refd).abs(), 3e-5 + 1e-5 * refd.abs()
    e_kernel = float(err.max())
    print(f"[parity] encoder dgrad {u.name} B={B} route={d.kind} forms={[E.plan_fp32(s, G._cus())['form'] for s in d.shapes]}: random operands, "
          f"max|err|={e_kernel:.3e} max|ref|={float(refd.abs().max()):.3e} torch-fp32 max|err|={e_torch:.3e} ratio={e_kernel / e_torch:.2f}")
    assert bool((err <= bound).all()), (u.name, float((err - bound).max()))


# ---------------------------------------------------------------------------------------------------------------- pooling and masks
def test_maxpool_backward_at_the_stem_shape():
    """ihmr_maxpool3x3s2_backward on 64 x 112 x 112 x 64 with a ReLU-ed integer input (about half of the values tie at zero, the rest
    tie often too) and integer dy: every element equal to torch autograd's (which gives the gradient to the first maximum of a window)."""
    from ihmr_amd import encoder_train as T
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(21)
    N, H, W, C = B, 112, 112, 64
    x = torch.relu(torch.randint(-4, 5, (N, H, W, C), generator=g, dtype=torch.int8).float())
    xa = x.permute(0, 3, 1, 2).requires_grad_(True)
    y = F.max_pool2d(xa, 3, 2, 1)
    dy = torch.randint(-8, 9, tuple(y.shape), generator=g, dtype=torch.int8).float()
    y.backward(dy)
    ref = xa.grad.permute(0, 2, 3, 1).reshape(-1, C)
    dx = T.maxpool_backward(x.view(-1, C).cuda(), dy.permute(0, 2, 3, 1).reshape(-1, C).contiguous().cuda(), N, H, W, C)
    torch.cuda.synchronize()
    bad = int((dx.cpu() != ref).sum())
    print(f"[parity] encoder maxpool backward B={B} 112x112x64: zeros in x {float((x == 0).float().mean()):.2f}, mismatches={bad} of {ref.numel()}")
    assert bad == 0 and float((x == 0).float().mean()) > 0.4


def test_avgpool_relu_backward_at_the_trunk_output_shape():
    """ihmr_avgpool_relu_backward on 64 x 49 x 2048: dx = y > 0 ? dy / 49 : 0 for each of the 49 pixels.  Exact where dy is an integer
    multiple of 49; within one fp32 ulp of the correctly rounded dy / 49 on random dy."""
    from ihmr_amd import encoder_train as T
    g = torch.Generator().manual_seed(22)
    N, HW, C = B, 49, 2048
    y = torch.relu(torch.randn(N, C, generator=g))
    for kind in ("multiples of 49", "random"):
        dy = (torch.randint(-40, 41, (N, C), generator=g).float() * 49.0) if kind.startswith("mult") else torch.randn(N, C, generator=g)
        q = (dy.double() / 49.0).float()                                # fl(dy / 49)
        ref = torch.where(y > 0, q, torch.zeros(())).view(N, 1, C).expand(N, HW, C).reshape(-1, C)
        dx = T.avgpool_relu_backward(y.cuda(), dy.cuda(), N, HW, C).cpu()
        torch.cuda.synchronize()
        bad = int((dx != ref).sum())
        ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -126)).double().log2().floor().exp2() * 2.0 ** -23
        off = int(((dx.double() - ref.double()).abs() > ulp).sum())
        print(f"[parity] encoder avgpool+relu backward B={B} 49x2048 {kind}: differing from fl(dy/49)={bad}, beyond one ulp={off} of {ref.numel()}, "
              f"masked={float((y <= 0).float().mean()):.2f}")
        assert off == 0 and (bad == 0 or kind == "random")


def test_relu_backward_at_the_layer1_shape():
    """ihmr_relu_backward in place on (200 704, 256): g where y > 0, else 0, every element."""
    from ihmr_amd import encoder_train as T
    g = torch.Generator().manual_seed(23)
    M, C = 200704, 256
    y = torch.relu(torch.randn(M, C, generator=g))
    grad = torch.randn(M, C, generator=g)
    ref = torch.where(y > 0, grad, torch.zeros(()))
    got = T.relu_backward_(grad.cuda(), y.cuda())
    torch.cuda.synchronize()
    bad = int((got.cpu() != ref).sum())
    print(f"[parity] encoder relu backward {M}x{C}: mismatches={bad} of {ref.numel()}")
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------- heads
def _linear(name, in_f, out_f, g):
    from ihmr_amd.encoder_train import _Flat, _Linear
    dev = torch.device("cuda")
    flat = _Flat()
    lin = _Linear(flat, name, in_f, out_f)
    flat.allocate(dev)
    lin.bind(flat, B, dev)
    W = torch.randint(-5, 8, (out_f, in_f), generator=g).float()
    lin.w[:in_f, :out_f].copy_(W.t())
    lin.refresh()
    return lin, W


def test_head_gradients_at_batch64():
    """_Linear.backward of fc1, feat_encoder, regressor_ih and hand_classifier at B = 64 on integers: gw = x^T dy (a GEMM whose
    reduction runs over the batch), gb = column sums, dx = dy W, every element, against float64; padding rows / columns of gw, gb and
    dx stay zero.  The regressor: three accumulated calls as backward() makes them (the shared weights' gradients add up)."""
    heads = [("fc1", 2048, 1024, 2048), ("feat", 1024, 1024, 1024), ("reg", 1146, 122, 1152), ("cls", 1024, 2, 1152)]
    assert [(n, s.Cout) for n, *_ in heads for s in E.head_table(B) if s.name == n] == [(n, o) for n, _, o, _ in heads]
    g = torch.Generator().manual_seed(31)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    for name, in_f, out_f, ldx in heads:
        lin, W = _linear(name, in_f, out_f, g)
        assert lin.kpad == _ceil(in_f, 16) and lin.ldw == E.packed_ldw(out_f) and lin.kpad <= ldx
        calls = 3 if name == "reg" else 1
        gw_ref, gb_ref = torch.zeros(in_f, out_f, dtype=torch.float64), torch.zeros(out_f, dtype=torch.float64)
        for c in range(calls):
            x = torch.zeros(B, ldx)
            x[:, :in_f] = ri(-8, 8, (B, in_f))
            if ldx > lin.kpad:
                x[:, lin.kpad:] = 3.0                                  # cls reads 1024 of the IEF buffer's 1152 columns: the rest must not matter
            dy = torch.zeros(_ceil(B, 16), lin.ldw)
            dy[:B, :out_f] = ri(-7, 9, (B, out_f))
            dx = lin.backward(x.cuda(), dy.cuda(), accumulate=(c != 0))
            torch.cuda.synchronize()
            gw_ref += x[:, :in_f].double().t() @ dy[:B, :out_f].double()
            gb_ref += dy[:B, :out_f].double().sum(0)
            dx_ref = dy[:B, :out_f].double() @ W.double()
            assert float(gw_ref.abs().max()) < 2 ** 24 and float(dx_ref.abs().max()) < 2 ** 24
            dxc = dx.cpu()
            bad_dx = int((dxc[:B, :in_f].double() != dx_ref).sum())
            assert dxc.shape == (_ceil(B, 16), E.packed_ldw(in_f))
            pad_dx = int((dxc[:, in_f:] != 0).sum()) + int((dxc[B:] != 0).sum())
            gw, gb = lin.gw.cpu(), lin.gb.cpu()
            bad_gw, bad_gb = int((gw[:in_f, :out_f].double() != gw_ref).sum()), int((gb[:out_f].double() != gb_ref).sum())
            pad_gw = int((gw[in_f:] != 0).sum()) + int((gw[:, out_f:] != 0).sum()) + int((gb[out_f:] != 0).sum())
            print(f"[parity] encoder head {name} backward B={B} call {c + 1} of {calls}: exact on integers, mismatches gw={bad_gw} of {gw_ref.numel()} "
                  f"gb={bad_gb} of {out_f} dx={bad_dx} of {dx_ref.numel()}, non-zero padding gw/gb={pad_gw} dx={pad_dx}")
            assert (bad_gw, bad_gb, bad_dx, pad_gw, pad_dx) == (0, 0, 0, 0, 0), name
        if name == "reg":
            assert gw.shape == (1152, 128) and in_f + 6 == 1152 and out_f + 6 == 128


# ---------------------------------------------------------------------------------------------------------------- the composed step
def _trainer_route(tr, u):
    if "w_phase" in u:
        return "phase"
    if "w_dgrad" not in u:
        return "none"
    return "ds" if (u["stride"] == 2 and u["k"] == 1 and u["pad"] == 0) else "s1"      # conv_dgrad's own case split


def _padding_mask(tr):
    """True at every position of the flat layout that is no parameter: the alignment gaps between views, rows K.. and columns Cout..
    of the packed convolution weights, rows in_f.. and columns out_f.. of the packed Linear weights, entries out_f.. of their biases."""
    mask = torch.ones(tr.flat.n, dtype=torch.bool)
    real = {}
    for u in tr.units:
        real[u["name"] + ".w"] = (u["k"] * u["k"] * u["cin"], u["cout"])
    for l in (tr.fc1, tr.feat, tr.reg, tr.cls):
        real[l.name + ".weight"] = (l.in_f, l.out_f)
        real[l.name + ".bias"] = (l.out_f,)
    for name, shape, off, size in tr.flat.specs:
        v = mask[off:off + size].view(shape)
        if name in real:
            v[tuple(slice(0, n) for n in real[name])] = False
        else:
            v[...] = False
    return mask


def test_composed_step_is_deterministic_at_batch64():
    """EncoderTrainer at B = 64: its units are exactly the table of tests/encoder_train_shapes.py (name, cin, cout, k, stride, pad,
    input-gradient route); two fresh trainers on the same seeded weights and images, one forward + backward each: bit-identical flat
    gradients (every kernel has a fixed summation order), all finite, zero in every padding position of the flat layout."""
    from helpers import seeded_state_dict
    from ihmr_amd.encoder_train import EncoderTrainer
    from ihmr_amd.networks import InterHandEncoder
    rng = np.random.RandomState(5)
    mean_params = torch.tensor(rng.normal(0, 0.2, (1, 122)), dtype=torch.float32)
    img = torch.tensor(rng.uniform(-1, 1, (B, 3, 224, 224)), dtype=torch.float32).cuda()
    A = torch.tensor(rng.normal(0, 1, (B, 122)), dtype=torch.float32).cuda()
    Bm = torch.tensor(rng.normal(0, 1, (B, 2)), dtype=torch.float32).cuda()
    sd = None
    runs = []
    for _ in range(2):
        enc = InterHandEncoder(types.SimpleNamespace(total_params_dim=122), mean_params.repeat(B, 1))
        sd = seeded_state_dict(enc, 100) if sd is None else sd
        enc.load_state_dict(sd)
        tr = EncoderTrainer(enc.cuda(), B, 1e-4, torch.device("cuda"))
        got = [(u["name"], u["cin"], u["cout"], u["k"], u["stride"], u["pad"], _trainer_route(tr, u)) for u in tr.units]
        assert got == TS.unit_rows(B), [(a, b) for a, b in zip(got, TS.unit_rows(B)) if a != b]
        p, h = tr.forward(img)
        tr.backward(A, Bm)
        torch.cuda.synchronize()
        runs.append((tr.flat.grads.clone(), p.clone(), h.clone()))
        mask = _padding_mask(tr).cuda()
        n_units = len(tr.units)
        n_real = sum(p_.numel() for p_ in enc.parameters()) + 64 * 7 * 7          # + the stem's fourth (padding) input channel
        del tr, enc
        torch.cuda.empty_cache()
    (g1, p1, h1), (g2, p2, h2) = runs
    same = G._same_bits(g1, g2) and G._same_bits(p1, p2) and G._same_bits(h1, h2)
    finite = bool(torch.isfinite(g1).all())
    pad_nz = int((g1[mask] != 0).sum())
    print(f"[parity] encoder training step B={B}: {n_units} units, {g1.numel()} gradient words ({int(mask.sum())} padding), two fresh trainers "
          f"bit-identical={same}, finite={finite}, non-zero padding={pad_nz}, |grad| max={float(g1.abs().max()):.3e}")
    assert same, int((g1.view(torch.int32) != g2.view(torch.int32)).sum())
    assert finite and pad_nz == 0 and float(g1.abs().max()) > 0
    assert int(mask.sum()) > 0 and int((~mask).sum()) == n_real

"""Every layer of the inference encoder at its real batch-64 shape, fp32 (csrc/encoder.h) and bf16 (csrc/encoder_bf16.h), through
``conv_igemm`` / ``conv_igemm_bf16`` with the strides ``networks.py`` passes.  The table and the restated launcher selection come
from tests/encoder_shapes.py (checked on the CPU by tests/test_encoder_shapes_cpu.py).  Per case:

* small-integer operands -> every product and partial sum is exact in fp32 in any order -> the float64 ``F.conv2d`` of the same
  numbers, cast back, must equal the kernel's output in EVERY element, and a second launch must give the same bits;
* the output lives inside a larger buffer pre-filled with a NaN bit pattern: everything outside [M][Cout] comes back untouched;
* the split-K / Stream-K workspace is pre-filled with a NaN bit pattern: the output holds no NaN (nothing unwritten was read) and
  the set of workspace words that changed is exactly what the restated launcher predicts for this device's CU count -- nothing for
  a one-pass layer, ksplit * M * Cout floats for split-K, the predicted (worker, slot) 64 KB slots for Stream-K;
* random operands against float64, whole output, at the allowance the small-shape tests already use; the kernel's max error is
  printed beside that of CPU torch-fp32 on the same operands (reported, DESIGN.md records the measured ratios)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_shapes as E  # noqa: E402

pytestmark = pytest.mark.gpu

B = 64
NAN32 = 0x7FC0BEEF            # quiet NaNs with a payload no kernel produces
NAN16 = 0x7FC1
GUARD_ROWS = 8
TRUNK = E.trunk_table(B)
HEADS = {s.name: s for s in E.head_table(B)}
# The launcher's own 2-way split-K branch (64 <= tiles < 384, >= 64 K steps, not Stream-K eligible: Cout % 128 != 0) is reached by no
# batch-64 layer and by no small case of tests/test_gpu_encoder.py; one small shape takes it here.
EXTRA_SHAPES = [E.Shape("extra.split2", 8, 32, 32, 1024, 192, 1, 1, 0, 1024, 192, 192, True, 1, ())]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(s, prec):
    return E.plan_fp32(s, _cus()) if prec == "fp32" else E.plan_bf16(s, _cus())


def _dt(prec):
    return torch.float32 if prec == "fp32" else torch.bfloat16


def _pack(s, prec, w, b):
    from ihmr_amd.networks import _Packed, _PackedBF16
    return (_Packed if prec == "fp32" else _PackedBF16)(w.cuda(), b.cuda(), stride=s.stride, pad=s.pad)


def _guarded(M, ld, prec, col, cout):
    """A [GUARD_ROWS + M + GUARD_ROWS][ld] buffer of the NaN pattern; returns (raw integer view, the [M][cout] output view at column col)."""
    it, pat = (torch.int32, NAN32) if prec == "fp32" else (torch.int16, NAN16)
    raw = torch.full(((M + 2 * GUARD_ROWS) * ld,), pat, dtype=it, device="cuda")
    y = raw.view(_dt(prec)).view(M + 2 * GUARD_ROWS, ld)[GUARD_ROWS:GUARD_ROWS + M, col:col + cout]
    return raw, y


def _guards_intact(raw, M, ld, col, cout):
    pat = NAN32 if raw.dtype == torch.int32 else NAN16
    chk = raw.clone().view(M + 2 * GUARD_ROWS, ld)
    chk[GUARD_ROWS:GUARD_ROWS + M, col:col + cout] = pat
    return int((chk != pat).sum())


def _workspace():
    from ihmr_amd.networks import _splitk_workspace
    ws = _splitk_workspace(torch.device("cuda", torch.cuda.current_device()))
    assert ws.numel() * 4 == E.WORKSPACE_BYTES
    return ws.view(torch.int32)


def _footprint_errors(wsi, fp):
    """Words of the workspace that changed although the plan says they stay + words that stayed although the plan says they change."""
    changed = wsi != NAN32
    if fp[0] == "none":
        return int(changed.sum())
    if fp[0] == "prefix":
        return int((~changed[:fp[1]]).sum()) + int(changed[fp[1]:].sum())
    want = torch.zeros(wsi.numel() // E.SLOT_FLOATS, dtype=torch.bool, device=wsi.device)
    want[torch.tensor(sorted(fp[1]), device=wsi.device)] = True
    return int((changed.view(-1, E.SLOT_FLOATS) != want[:, None]).sum())


def _launch(s, prec, xd, pk, rd, act, col=0):
    """One launch as networks.py makes it (same ldx / ldy / ldr), into a guarded buffer and over a NaN-filled workspace.  Returns the
    [M][Cout] output view; asserts the guards, the absence of NaN and the workspace fingerprint."""
    from ihmr_amd.networks import conv_igemm, conv_igemm_bf16
    M, _ = E.gemm_dims(s)
    plan = _plan(s, prec)
    raw, y = _guarded(M, s.ldy, prec, col, s.Cout)
    wsi = _workspace()
    wsi.fill_(NAN32)
    fn = conv_igemm if prec == "fp32" else conv_igemm_bf16
    _, Ho, Wo = fn(xd, pk, s.N, s.H, s.W, ldx=s.ldx, out=y, ldy=s.ldy, residual=rd, ldr=s.ldr, act=act)
    torch.cuda.synchronize()
    assert (Ho, Wo) == E.out_hw(s)
    touched = _guards_intact(raw, M, s.ldy, col, s.Cout)
    nans = int(torch.isnan(y).sum())
    fperr = _footprint_errors(wsi, E.workspace_footprint(s, plan))
    assert touched == 0, f"{s.name} {prec} act={act}: {touched} words outside [M][Cout] were written"
    assert nans == 0, f"{s.name} {prec} act={act}: {nans} NaN in the output (unwritten workspace or output read)"
    assert fperr == 0, f"{s.name} {prec} act={act}: workspace fingerprint differs from the plan {plan} in {fperr} words"
    return y


def _form(s, prec):
    p = _plan(s, prec)
    return p["form"] if prec == "fp32" else f"128x{p['tile'][1]}_{p['mode']}" + (f"_splitk{p['ksplit']}" if p["ksplit"] > 1 else "")


def _device_operands(s, prec, x, r):
    xd = x.to(_dt(prec)).cuda().view(-1, s.Cin)
    rd = None if r is None else r.to(_dt(prec)).cuda()
    return xd, rd


def _same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


_ids = lambda s: s.name


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("s", TRUNK + EXTRA_SHAPES, ids=_ids)
def test_layer_exact_on_integers(s, prec):
    """Zero mismatching elements out of all N * Ho * Wo * Cout, with the network's activation and with act = 0, residual where the
    network has one; the same bits on a second launch; guards, NaN and workspace fingerprint on every launch (``_launch``)."""
    torch.set_num_threads(16)
    x, w, b, r = E.draw_integers(s, prec)
    pre = E.reference(s, x, w, b, r)                                   # float64, CPU
    top = float(pre.abs().max())
    assert top < 2 ** 24 and (prec == "fp32" or 8 <= top <= 256), (s.name, prec, top)
    pre = pre.float().cuda()
    pk = _pack(s, prec, w, b)
    xd, rd = _device_operands(s, prec, x, r)
    for act in (s.act, 0) if s.act else (0, 1):
        ref = E.activate(pre, act)
        y = _launch(s, prec, xd, pk, rd, act)
        y2 = _launch(s, prec, xd, pk, rd, act)
        bad = int((y.float() != ref).sum())
        print(f"[parity] encoder layer {s.name} {prec} B={B} act={act} form={_form(s, prec)}: exact on integers, max|y|={top:.0f} "
              f"mismatches={bad} of {ref.numel()}")
        assert bad == 0, (s.name, prec, act, bad, float((y.float() - ref).abs().max()))
        assert _same_bits(y, y2), f"{s.name} {prec} act={act}: second launch differs"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("s", TRUNK, ids=_ids)
def test_layer_random_against_float64(s, prec):
    """Whole output, the network's residual and activation.  fp32: |got - ref64| <= 3e-5 + 1e-5 |ref64| (the allowance of
    test_conv_streamk_matches_torch: K up to 4608 at unit output scale, w ~ N(0, 1/K)).  bf16: |got - bf16(ref64)| <= 2^-7 |ref64| + 3e-5
    (test_conv_bf16_layers_random).  Printed: the kernel's max error and that of CPU torch-fp32 F.conv2d against the same reference."""
    torch.set_num_threads(16)
    x, w, b, r = E.draw_random(s, prec)
    ref = E.activate(E.reference(s, x, w, b, r), s.act)                # float64
    t32 = E.activate(E.reference(s, x, w, b, r, dtype=torch.float32), s.act)
    e_torch = float((t32.double() - ref).abs().max())
    pk = _pack(s, prec, w, b)
    xd, rd = _device_operands(s, prec, x, r)
    y = _launch(s, prec, xd, pk, rd, s.act)
    refd = ref.cuda()
    if prec == "fp32":
        err, bound = (y.double() - refd).abs(), 3e-5 + 1e-5 * refd.abs()
    else:
        err, bound = (y.double() - refd.float().bfloat16().double()).abs(), 2.0 ** -7 * refd.abs() + 3e-5
    e_kernel = float(err.max())
    tail = (f"ratio={e_kernel / e_torch:.2f} elements differing from torch-fp32: {int((y.cpu() != t32).sum())} of {t32.numel()}" if prec == "fp32"
            else f"differing from bf16(ref): {int((err > 0).sum())} of {err.numel()}")
    print(f"[parity] encoder layer {s.name} {prec} B={B} form={_form(s, prec)}: random operands, max|err|={e_kernel:.3e} "
          f"max|ref|={float(refd.abs().max()):.3e} torch-fp32 max|err|={e_torch:.3e} {tail}")
    assert bool((err <= bound).all()), (s.name, prec, float((err - bound).max()))


def test_heads_at_batch64_with_the_networks_strides():
    """fc1, feat_encoder (ldy = 1152), three chained regressor_ih launches ping-ponging between two [64][1152] buffers as forward()
    does (output and residual are column slices at offset 1024, the 6 padding columns stay zero), hand_classifier with act = 0 exact
    and with the sigmoid against float64 at 1e-5.  fp32 only: the heads stay fp32 in the bf16 encoder."""
    from ihmr_amd.networks import _Packed
    torch.set_num_threads(16)
    col = E.HEAD_COL
    for name in ("fc1", "feat", "cls"):
        s = HEADS[name]
        for kind in ("integers", "random"):
            x, w, b, _ = E.draw_integers(s, "fp32") if kind == "integers" else E.draw_random(s, "fp32")
            xw = torch.full((B, s.ldx), 3.0)                           # cls reads 1024 of the buffer's 1152 columns: the rest must not matter
            xw[:, :s.Cin] = x.view(B, s.Cin)
            pre = E.reference(s, x, w, b, None)
            pk = _pack(s, "fp32", w, b)
            for act in ((s.act, 0) if kind == "integers" else (s.act,)):
                ref = E.activate(pre, act).cuda()
                y = _launch(s, "fp32", xw.cuda(), pk, None, act)
                y2 = _launch(s, "fp32", xw.cuda(), pk, None, act)
                assert _same_bits(y, y2)
                err = float((y.double() - ref).abs().max())
                if kind == "integers" and act != 2:
                    bad = int((y.double() != ref).sum())
                    print(f"[parity] encoder head {name} B={B} act={act} form={_form(s, 'fp32')}: exact on integers, mismatches={bad} of {ref.numel()}")
                    assert bad == 0, (name, act, bad, err)
                elif kind == "random":
                    atol, rtol = (1e-5, 0.0) if act == 2 else (3e-5, 1e-5)
                    print(f"[parity] encoder head {name} B={B} act={act}: random operands, max|err|={err:.3e}")
                    assert bool(((y.double() - ref).abs() <= atol + rtol * ref.abs()).all()), (name, act, err)
    # ---- the IEF iterations: params += Linear([feat | params | 0]) three times
    s = HEADS["reg"]
    feat, params, W, bias, refs = E.reg_chain(B)
    assert max(float(r_.abs().max()) for r_ in refs) < 2 ** 24 and E.reg_chain_partial_bound(feat, params, W, bias, refs) < 2 ** 24
    pk = _Packed(W.cuda()[:, :, None, None], bias.cuda(), k_extra=s.Cin - W.shape[1])
    assert pk.cin == s.Cin == s.ldx and pk.cout == s.Cout
    raws, bufs = [], []
    for i in range(2):
        raw = torch.full(((B + 2 * GUARD_ROWS) * s.ldy,), NAN32, dtype=torch.int32, device="cuda")
        buf = raw.view(torch.float32).view(B + 2 * GUARD_ROWS, s.ldy)[GUARD_ROWS:GUARD_ROWS + B]
        buf.zero_()
        buf[:, :col].copy_(feat)
        raws.append(raw); bufs.append(buf)
    bufs[0][:, col:col + s.Cout].copy_(params)
    from ihmr_amd.networks import conv_igemm
    wsi = _workspace()
    plan = _plan(s, "fp32")
    cur = 0
    for it in range(3):
        src, dst = bufs[cur], bufs[1 - cur]
        wsi.fill_(NAN32)
        conv_igemm(src, pk, B, 1, 1, ldx=s.ldx, out=dst[:, col:], ldy=s.ldy, residual=src[:, col:], ldr=s.ldr, act=0)
        torch.cuda.synchronize()
        fperr = _footprint_errors(wsi, E.workspace_footprint(s, plan))
        got = dst[:, col:col + s.Cout]
        bad = int((got.double().cpu() != refs[it]).sum())
        print(f"[parity] encoder head reg iteration {it} B={B} form={plan['form']}: exact on integers, max|y|={float(refs[it].abs().max()):.0f} "
              f"mismatches={bad} of {got.numel()}")
        assert bad == 0 and fperr == 0, (it, bad, fperr)
        for i in range(2):
            full = raws[i].view(B + 2 * GUARD_ROWS, s.ldy)
            assert bool((full[:GUARD_ROWS] == NAN32).all()) and bool((full[GUARD_ROWS + B:] == NAN32).all()), "guard rows written"
            assert torch.equal(bufs[i][:, :col].cpu(), feat), "the feature columns changed"
            assert not bool(bufs[i][:, col + s.Cout:].any()), "the padding columns 1146..1151 are no longer zero"
        cur = 1 - cur


def _maxpool(x, prec):
    from ihmr_amd import hip
    N, H, W, C = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    raw, y = _guarded(N * Ho * Wo, C, prec, 0, C)
    fn = hip.lib().ihmr_maxpool3x3s2 if prec == "fp32" else hip.lib().ihmr_maxpool3x3s2_bf16
    hip.check(fn(hip.ptr(x.to(_dt(prec)).cuda()), y.data_ptr(), N, H, W, C, Ho, Wo, hip.stream_ptr()), "ihmr_maxpool3x3s2")
    torch.cuda.synchronize()
    assert _guards_intact(raw, N * Ho * Wo, C, 0, C) == 0
    return y.view(N, Ho, Wo, C)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_maxpool_at_the_stem_shape(prec):
    """MaxPool2d(3, 2, 1) on 64 x 112 x 112 x 64, bit for bit against torch on the CPU; a negative-only input too (a maximum that
    starts from zero instead of -inf, or padding that counts as zero, fails it)."""
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(11)
    for kind in ("randn", "negative"):
        x = torch.randn(B, 112, 112, 64, generator=g)
        if kind == "negative":
            x = -x.abs() - 0.5
        x = x.to(_dt(prec))
        ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(_dt(prec))
        y = _maxpool(x, prec)
        bad = int((y.cpu() != ref).sum()) + (0 if _same_bits(y.cpu(), ref) else 1)
        print(f"[parity] encoder maxpool {prec} B={B} 112x112x64 {kind}: mismatches={bad} of {ref.numel()}")
        assert bad == 0 and (kind != "negative" or float(y.float().max()) < 0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_avgpool_relu_at_the_trunk_output_shape(prec):
    """AvgPool2d(7) + ReLU on 64 x 49 x 2048 into rows wider than C.  Integer inputs: the column sum is exact in fp32; where it is a
    multiple of 49 (half of the columns, by construction) the mean is exact, elsewhere the correctly rounded quotient is within one
    fp32 ulp of the float64 mean.  Columns C.. of the output rows stay untouched."""
    from ihmr_amd import hip
    C, HW, ldy = 2048, 49, 2048 + 64
    g = torch.Generator().manual_seed(13)
    x = torch.randint(-2, 7, (B, HW, C), generator=g).double()
    fix = torch.arange(C) % 2 == 0
    part = x[:, :HW - 1, :].sum(1)
    x[:, HW - 1, :] = torch.where(fix[None, :], -(part % 49) + 49 * (part % 3 == 0), x[:, HW - 1, :])     # |last| <= 49: exact in bf16 too
    total = x.sum(1)
    assert bool((total[:, fix] % 49 == 0).all()) and float(x.abs().max()) <= 49
    ref = torch.relu(total / 49.0)
    raw, y = _guarded(B, ldy, "fp32", 0, C)
    fn = hip.lib().ihmr_avgpool_relu if prec == "fp32" else hip.lib().ihmr_avgpool_relu_bf16
    hip.check(fn(hip.ptr(x.to(_dt(prec)).cuda()), y.data_ptr(), B, HW, C, ldy, hip.stream_ptr()), "ihmr_avgpool_relu")
    torch.cuda.synchronize()
    assert _guards_intact(raw, B, ldy, 0, C) == 0
    got = y.cpu().double()
    exact_bad = int((got[:, fix] != ref[:, fix]).sum())
    ulp = torch.maximum(ref.float(), torch.tensor(2.0 ** -126)).double().log2().floor().exp2() * 2.0 ** -23
    off = int(((got - ref).abs() > ulp).sum())
    print(f"[parity] encoder avgpool+relu {prec} B={B} 49x2048 ldy={ldy}: exact columns mismatching={exact_bad}, others beyond one ulp={off}, "
          f"positive means={int((ref > 0).sum())} of {ref.numel()}")
    assert exact_bad == 0 and off == 0 and int((ref > 0).sum()) > ref.numel() // 2


@pytest.mark.parametrize("name,BIG", [("stem", 512), ("l1.0.c3", 512), ("l1.0.c3", 1024)])
def test_large_batch_probe_fp32(name, BIG):
    """B = 512: 6.4 M rows (stem) and 1.6 M rows x 256 channels (l1.0.c3, with its residual): outputs of 1.64 GB each -- 411 M
    elements, byte offsets up to 0.77 x 2^31, so these two stay below 2^31 bytes -- and l1.0.c3 once more at B = 1024, whose output and
    residual (3.3 GB each) do cross 2^31 bytes while `dr * a.ldy` and the gather's `an * H + hi` are formed in 32 bits before widening.
    Integer-exact against float64 in 64-image chunks, every element; guards, workspace untouched (one-pass forms at these sizes)."""
    torch.set_num_threads(16)
    CH = 64
    s = next(t for t in TRUNK if t.name == name)._replace(N=BIG)
    M, _ = E.gemm_dims(s)
    Mc = M // (BIG // CH)
    plan = _plan(s, "fp32")
    assert plan["ksplit"] == 1 and not plan["streamk"] and (M * s.Cout * 4 > 2 ** 31) == (BIG == 1024)
    _, w, b, _ = E.draw_integers(s, "fp32", images=1)
    pk = _pack(s, "fp32", w, b)
    xd = torch.empty(BIG * s.H * s.W, s.Cin, device="cuda")
    rd = torch.empty(M, s.Cout, device="cuda") if s.residual else None
    chunk = lambda c: E.draw_integers(s._replace(name=f"{name}#{c}"), "fp32", images=CH)       # drawn again below: 3 GB less on the host
    for c in range(BIG // CH):
        x, _, _, r = chunk(c)
        xd[c * CH * s.H * s.W:(c + 1) * CH * s.H * s.W].copy_(x.view(-1, s.Cin))
        if rd is not None:
            rd[c * Mc:(c + 1) * Mc].copy_(r)
    y = _launch(s, "fp32", xd, pk, rd, s.act)
    y2 = _launch(s, "fp32", xd, pk, rd, s.act)
    assert torch.equal(y, y2), "second launch differs"
    del y2
    bad = 0
    for c in range(BIG // CH):
        x, _, _, r = chunk(c)
        ref = E.activate(E.reference(s._replace(N=CH), x, w, b, r), s.act).float().cuda()
        bad_c = int((y[c * Mc:(c + 1) * Mc] != ref).sum())
        bad += bad_c
        if bad_c or c in (0, BIG // CH - 1):
            print(f"[parity] encoder layer {name} fp32 B={BIG} form={plan['form']} images {c * CH}..{(c + 1) * CH - 1}: mismatches={bad_c} of {ref.numel()}")
    print(f"[parity] encoder layer {name} fp32 B={BIG} form={plan['form']} tiles={plan['tiles']}: exact on integers, mismatches={bad} of {y.numel()}")
    assert bad == 0, (name, bad)

"""GPU tests of the opt-in bf16 encoder path (``encoder_precision = "bf16"``; csrc/encoder_bf16.h): every kernel against plain torch
on the CPU -- bit for bit where the arithmetic is exact -- the encoder against the reference's golden outputs and against the fp32
path of the same module, and the model-level switch.  The numerics contract is restated in tests/bf16_emulation.py."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

# the shapes of tests/test_gpu_encoder.py: test_conv_igemm_matches_torch (fp32 allowance 2e-5) ...
IGEMM_SHAPES = [
    dict(N=2, H=14, W=14, Cin=64, Cout=64, k=3, s=1, p=1),      # 3x3, M = 392 (tail tile), narrow tile
    dict(N=3, H=15, W=13, Cin=32, Cout=160, k=3, s=2, p=1),     # odd sizes, stride 2, Cout not a tile multiple
    dict(N=2, H=28, W=28, Cin=128, Cout=256, k=1, s=2, p=0),    # strided 1x1 (downsample)
    dict(N=2, H=32, W=32, Cin=3, Cout=64, k=7, s=2, p=3),       # stem-like, Cin = 3 (generic gather)
    dict(N=3, H=30, W=34, Cin=4, Cout=64, k=7, s=2, p=3),       # the stem on a 4-channel image (two 8-byte pixel loads per 8 k)
    dict(N=1, H=9, W=9, Cin=4, Cout=40, k=5, s=1, p=2),         # 4-channel form, taps wrapping inside a chunk (kw = 5), Cout not a tile multiple
    dict(N=1, H=6, W=5, Cin=2064, Cout=32, k=3, s=1, p=1),      # Cin not a multiple of 32 and long: generic gather, padding still zero
    dict(N=1, H=24, W=24, Cin=32, Cout=320, k=1, s=1, p=0),     # 5 x 3 = 15 tiles: the XCD-aware tile order with a remainder, last row and column tiles partial
    dict(N=5, H=20, W=20, Cin=48, Cout=192, k=3, s=1, p=1),     # Cin = 48: generic gather; 16 x 2 tiles, last row tile partial
]
# ... and of test_conv_streamk_matches_torch (fp32 allowance 3e-5): the K-parallel forms, residual + ReLU in the second launch's epilogue
KPAR_SHAPES = [
    dict(N=33, H=14, W=14, Cin=256, Cout=256, k=3, s=1, p=1, res=True),
    dict(N=96, H=10, W=10, Cin=1024, Cout=1024, k=1, s=1, p=0, res=True),
    dict(N=64, H=7, W=7, Cin=512, Cout=512, k=3, s=1, p=1, res=False),
    dict(N=40, H=28, W=28, Cin=128, Cout=128, k=3, s=2, p=1, res=False),
]
ALL_SHAPES = [dict(c, res=c.get("res", i % 2 == 1), a=2e-5) for i, c in enumerate(IGEMM_SHAPES)] + [dict(c, a=3e-5) for c in KPAR_SHAPES]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run_conv(x, w, b, res, cfg, relu=True):
    """x [N][Cin][H][W], w [Cout][Cin][k][k], b [Cout] fp32, res [N][Cout][Ho][Wo] or None -- x, w, res hold bf16-exact values.
    Returns the kernel's output as fp32 NCHW (two launches, asserted bit-identical)."""
    from ihmr_amd.networks import _PackedBF16, conv_igemm_bf16
    pk = _PackedBF16(w.cuda(), b.cuda(), stride=cfg["s"], pad=cfg["p"])
    assert torch.equal(pk.unpack().float().cpu(), w.permute(2, 3, 1, 0).reshape(-1, cfg["Cout"]))      # the operands are bf16-exact
    xn = x.permute(0, 2, 3, 1).contiguous().bfloat16().cuda()
    rn = None if res is None else res.permute(0, 2, 3, 1).reshape(-1, cfg["Cout"]).contiguous().bfloat16().cuda()
    outs = []
    for _ in range(2):
        y, Ho, Wo = conv_igemm_bf16(xn, pk, cfg["N"], cfg["H"], cfg["W"], ldx=cfg["Cin"], residual=rn, ldr=cfg["Cout"], act=1 if relu else 0)
        outs.append(y)
    torch.cuda.synchronize()
    assert outs[0].dtype == torch.bfloat16 and torch.equal(_bits(outs[0]), _bits(outs[1])), "second launch differs"
    return outs[0].view(cfg["N"], Ho, Wo, cfg["Cout"]).permute(0, 3, 1, 2).float().cpu()


@pytest.mark.parametrize("cfg", ALL_SHAPES, ids=lambda c: f"{c['N']}x{c['H']}x{c['W']}_c{c['Cin']}_o{c['Cout']}_k{c['k']}s{c['s']}")
def test_conv_bf16_layers_exact_on_integers(cfg):
    """Small-integer operands: every product and every partial sum is an exact fp32 integer whatever the order, and -- the draw is
    thinned so that |y| <= 256, checked below -- every output is a bf16-exact integer.  Required: the bits of F.conv2d on the same
    numbers, residual and ReLU included, and the same bits on a second launch.  The weight tensor is a random draw (asymmetric), so
    a transposed fragment map cannot pass."""
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(21)
    K = cfg["Cin"] * cfg["k"] ** 2
    # Var(sum) = K * px * E[x^2 = 2] * E[w^2 = 2/3]; px keeps it <= 667 (sd 26: 256 is almost 10 sd away)
    px = min(1.0, 500.0 / K)
    x = torch.randint(-2, 3, (cfg["N"], cfg["Cin"], cfg["H"], cfg["W"]), generator=g).float()
    x = x * (torch.rand(x.shape, generator=g) < px)
    w = torch.randint(-1, 2, (cfg["Cout"], cfg["Cin"], cfg["k"], cfg["k"]), generator=g).float()
    b = torch.randint(-3, 4, (cfg["Cout"],), generator=g).float()
    pre = F.conv2d(x, w, b, stride=cfg["s"], padding=cfg["p"])
    res = None
    if cfg["res"]:
        res = torch.randint(-3, 4, pre.shape, generator=g).float()
        pre = pre + res
    assert float(pre.abs().max()) <= 256, "the draw leaves the range bf16 holds exactly: thin it further"
    assert float(pre.abs().max()) >= 8                          # and is not trivial
    for relu in (True, False):
        ref = torch.relu(pre) if relu else pre
        got = _run_conv(x, w, b, res, cfg, relu=relu)
        bad = int((got != ref).sum())
        print(f"[parity] bf16 conv exact {cfg} relu={relu}: max|y|={float(ref.abs().max()):.0f} mismatches={bad}")
        assert bad == 0, (cfg, relu, bad, float((got - ref).abs().max()))


@pytest.mark.parametrize("cfg", ALL_SHAPES, ids=lambda c: f"{c['N']}x{c['H']}x{c['W']}_c{c['Cin']}_o{c['Cout']}_k{c['k']}s{c['s']}")
def test_conv_bf16_layers_random(cfg):
    """randn operands rounded to bf16 first; reference = fp32 F.conv2d of those rounded operands + the epilogue in fp32.  Bound per
    element: |got - bf16(ref)| <= 2^-7 |ref| + a -- one bf16 ulp (two correctly rounded values of sums that differ only by fp32
    reordering can sit on either side of a tie) plus the allowance `a` the fp32 tests use for the same shape."""
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(1)
    K = cfg["Cin"] * cfg["k"] ** 2
    x = torch.randn(cfg["N"], cfg["Cin"], cfg["H"], cfg["W"], generator=g).bfloat16().float()
    w = (torch.randn(cfg["Cout"], cfg["Cin"], cfg["k"], cfg["k"], generator=g) / np.sqrt(K)).bfloat16().float()
    b = torch.randn(cfg["Cout"], generator=g)
    ref = F.conv2d(x, w, b, stride=cfg["s"], padding=cfg["p"])
    res = None
    if cfg["res"]:
        res = torch.randn(ref.shape, generator=g).bfloat16().float()
        ref = ref + res
    ref = torch.relu(ref)
    got = _run_conv(x, w, b, res, cfg, relu=True)
    err = (got - ref.bfloat16().float()).abs()
    bound = 2.0 ** -7 * ref.abs() + cfg["a"]
    print(f"[parity] bf16 conv random {cfg}: max|err|={float(err.max()):.3e} max|ref|={float(ref.abs().max()):.3e} "
          f"differing from bf16(ref): {int((err > 0).sum())} of {err.numel()}")
    assert bool((err <= bound).all()), (cfg, float((err - bound).max()))


def test_cast_image_pack_and_pools_match_torch_bit_for_bit():
    from ihmr_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(3)
    # cast: random values, ties, specials
    special = torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38, -3.3895314e38, 3.4028235e38, float("inf"), -float("inf"), 1e-40, -1e-45])
    x = torch.cat([torch.randn(100003, generator=g) * 10.0 ** torch.randint(-20, 20, (100003,), generator=g).float(), special]).cuda()
    y = torch.empty(x.numel(), dtype=torch.bfloat16, device="cuda")
    hip.check(L.ihmr_cast_f32_bf16(hip.ptr(x), hip.ptr(y), x.numel(), hip.stream_ptr()), "ihmr_cast_f32_bf16")
    assert torch.equal(_bits(y).cpu(), _bits(x.cpu().bfloat16()))
    nan = torch.tensor([float("nan")], device="cuda")
    yn = torch.empty(1, dtype=torch.bfloat16, device="cuda")
    hip.check(L.ihmr_cast_f32_bf16(hip.ptr(nan), hip.ptr(yn), 1, hip.stream_ptr()), "ihmr_cast_f32_bf16")
    assert bool(torch.isnan(yn.float()).all())
    # image pack: NCHW fp32 -> NHWC4 bf16, channel 3 zero
    img = torch.rand(3, 3, 30, 34, generator=g) * 2 - 1
    out = torch.full((3, 30, 34, 4), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.check(L.ihmr_pack_image_bf16(hip.ptr(img.cuda()), hip.ptr(out), 3, 30, 34, hip.stream_ptr()), "ihmr_pack_image_bf16")
    ref = torch.zeros(3, 30, 34, 4, dtype=torch.bfloat16)
    ref[..., :3] = img.permute(0, 2, 3, 1).bfloat16()
    assert torch.equal(_bits(out).cpu(), _bits(ref))
    # max-pool 3x3 / 2 / 1 on bf16 (odd sizes: the border windows are clipped)
    a = torch.randn(2, 64, 15, 13, generator=g).bfloat16()
    Ho, Wo = (15 + 2 - 3) // 2 + 1, (13 + 2 - 3) // 2 + 1
    yo = torch.empty(2 * Ho * Wo, 64, dtype=torch.bfloat16, device="cuda")
    hip.check(L.ihmr_maxpool3x3s2_bf16(hip.ptr(a.permute(0, 2, 3, 1).contiguous().cuda()), hip.ptr(yo), 2, 15, 13, 64, Ho, Wo, hip.stream_ptr()),
              "ihmr_maxpool3x3s2_bf16")
    ref = F.max_pool2d(a.float(), 3, 2, 1).bfloat16()
    assert torch.equal(_bits(yo.view(2, Ho, Wo, 64).permute(0, 3, 1, 2)).cpu(), _bits(ref))
    # avg-pool 7 x 7 + ReLU: bf16 in, fp32 sum in pixel order, fp32 out -- the order reproduced on the CPU, compared exactly
    a = torch.randn(5, 49, 2048, generator=g).bfloat16()
    yo = torch.empty(5, 2048, device="cuda")
    hip.check(L.ihmr_avgpool_relu_bf16(hip.ptr(a.cuda()), hip.ptr(yo), 5, 49, 2048, 2048, hip.stream_ptr()), "ihmr_avgpool_relu_bf16")
    s = torch.zeros(5, 2048)
    for p in range(49):
        s = s + a[:, p, :].float()
    ref = torch.relu(s / 49.0)
    assert yo.dtype == torch.float32 and torch.equal(yo.cpu(), ref)
    torch.cuda.synchronize()


def _golden_encoder(precision, B=2):
    from helpers import seeded_state_dict
    from ihmr_amd.networks import InterHandEncoder
    g = dict(np.load(os.path.join(GOLD, "encoder.npz")))
    enc = InterHandEncoder(types.SimpleNamespace(total_params_dim=122, encoder_precision=precision), torch.tensor(g["mean_params"]).repeat(B, 1))
    enc.load_state_dict(seeded_state_dict(enc, 100))
    img = torch.tensor(np.random.RandomState(7).uniform(-1, 1, (B, 3, 224, 224)), dtype=torch.float32)
    return enc.cuda(), img.cuda(), g


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def test_encoder_bf16_matches_reference_golden():
    """B = 2, the weights and image of tests/golden/encoder.npz (the reference's own fp32 outputs).  Upper bounds: twice what the CPU
    emulation of the contract measures against the same golden (tests/test_encoder_bf16_cpu.py: 5.36e-3 of max|main_feat|, 0.0469 on
    params, 4.1e-3 on hand_class) -- the factor covers the summation-order effect (about a quarter of the quantisation error).  Floor:
    rms(d main_feat) / rms(main_feat) >= 1e-4 -- the fp32 path sits below 1e-5, so a switch that silently runs fp32 fails."""
    enc, img, g = _golden_encoder("bf16")
    p, h = enc(img)
    torch.cuda.synchronize()
    mf = enc.main_feat.cpu().numpy()
    d_mf = np.abs(mf - g["main_feat"]).max() / np.abs(g["main_feat"]).max()
    rms = _rms(mf - g["main_feat"]) / _rms(g["main_feat"])
    d_p = np.abs(p.cpu().numpy() - g["params"]).max()
    d_h = np.abs(h.cpu().numpy() - g["hand_class"]).max()
    print(f"[parity] bf16 encoder vs reference golden: max|d main_feat|/max|main_feat|={d_mf:.3e} rms ratio={rms:.3e} "
          f"max|d params|={d_p:.3e} max|d hand_class|={d_h:.3e}")
    assert d_mf <= 2 * 5.36e-3 and d_p <= 2 * 0.0469 and d_h <= 2 * 4.1e-3, (d_mf, d_p, d_h)
    assert rms >= 1e-4, rms
    # and against the CPU emulation of the contract itself (same operands, other summation order): reported
    import bf16_emulation as E
    torch.set_num_threads(16)
    e_mf, e_p, e_h = E.encoder(enc.cpu(), img.cpu())
    print(f"[parity] bf16 encoder vs CPU emulation: max|d main_feat|/max|main_feat|={float((torch.tensor(mf) - e_mf).abs().max() / e_mf.abs().max()):.3e} "
          f"max|d params|={float((p.cpu() - e_p).abs().max()):.3e}")


def test_encoder_bf16_at_the_baseline_batch_size():
    """B = 64 (seeded weights 100, image seed 7): bf16 against the fp32 path of the same weights.  rms(d main_feat) / rms(main_feat)
    between 1e-4 and 2 x 3.4e-3 (the ratio was 3.1-3.4e-3 on three CPU cases and does not grow with the number of elements);
    main_feat / feat are fp32 tensors of the fp32 path's shapes; two forwards are bit-identical; forwards on two streams at once equal
    the single-stream result."""
    B = 64
    enc, img, _ = _golden_encoder("bf16", B)
    ref, _, _ = _golden_encoder("fp32", B)
    p32, h32 = ref(img)
    mf32, f32 = ref.main_feat.clone(), ref.feat.clone()
    p, h = enc(img)
    mf, f = enc.main_feat.clone(), enc.feat.clone()
    torch.cuda.synchronize()
    for t, t32 in ((mf, mf32), (f, f32), (p, p32), (h, h32)):
        assert t.dtype == torch.float32 and t.shape == t32.shape
    assert mf.shape == (B, 1024) and f.shape == (B, 1024) and p.shape == (B, 122) and h.shape == (B, 2)
    ratio = _rms((mf - mf32).cpu().numpy()) / _rms(mf32.cpu().numpy())
    print(f"[parity] bf16 vs fp32 encoder, B=64: rms(d main_feat)/rms(main_feat)={ratio:.3e} max|d params|={float((p - p32).abs().max()):.3e} "
          f"max|d hand_class|={float((h - h32).abs().max()):.3e}")
    assert 1e-4 <= ratio <= 2 * 3.4e-3, ratio
    p2, h2 = enc(img)
    torch.cuda.synchronize()
    assert torch.equal(p, p2) and torch.equal(h, h2) and torch.equal(mf, enc.main_feat) and torch.equal(f, enc.feat)
    # two instances in flight: the same module on two streams at once
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    imgs = [img, img.clone()]
    torch.cuda.synchronize()
    outs = []
    for s_, im in zip(streams, imgs):
        with torch.cuda.stream(s_):
            o = enc(im)
            outs.append((o[0], o[1], enc.main_feat))
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o[0], p) and torch.equal(o[1], h) and torch.equal(o[2], mf)


def _opt(B, **kw):
    d = dict(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, input_nc=3, num_joints=42,
             total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20, trans_params_dim=3,
             model_root="", mean_param_file="mean_mano_params.pkl", checkpoints_dir="./checkpoints", strategy="mlp_default")
    d.update(kw)
    return types.SimpleNamespace(**d)


def _seeded(model, seed=100):
    from helpers import seeded_state_dict
    sd = seeded_state_dict(model.encoder, seed)
    sd["regressor_ih.0.weight"] *= 0.05; sd["regressor_ih.0.bias"] *= 0.05      # the predicted pose stays hand-like
    model.encoder.load_state_dict(sd)
    return model.eval()


def test_model_switch_graph_replay_keys_and_no_leak(mano_arrays):
    """InterHandModel with encoder_precision = "bf16": test() through the captured graph equals the eager bf16 run bit for bit;
    get_pred_result() has the keys, shapes and dtypes of the fp32 model; an fp32 encoder built afterwards in the same process still
    meets the bounds of test_encoder_matches_reference_golden; training + bf16 and an unknown precision name are refused, and so is
    training with an sdf_robustifier (by InterHandModel and MLPModel)."""
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    B = 4
    graph = _seeded(InterHandModel(_opt(B, encoder_precision="bf16")))
    eager = _seeded(InterHandModel(_opt(B, encoder_precision="bf16", use_test_graph=False)))
    fp32 = _seeded(InterHandModel(_opt(B)))
    assert graph.encoder.encoder_precision == "bf16" and fp32.encoder.encoder_precision == "fp32"
    fwd = lambda p, s, t: two_hand.forward_from_packed(graph.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    for seed in (5, 6):
        batch = synthetic_opt_batch(B, fwd, seed=seed, with_image=True)
        outs = []
        for m in (graph, eager, fp32):
            m.set_input(batch); m.test(); torch.cuda.synchronize()
            outs.append(m.get_pred_result())
        assert graph._test_graph is not None and getattr(eager, "_test_graph", None) is None
        assert list(outs[0]) == list(outs[1]) == list(outs[2])
        for k in outs[0]:
            a, b, c = (np.asarray(o[k]) for o in outs)
            assert np.array_equal(a, b), (seed, k)
            assert a.shape == c.shape and a.dtype == c.dtype, (k, a.shape, c.shape, a.dtype, c.dtype)
        assert not np.array_equal(outs[0]["pred_pose_params"], outs[2]["pred_pose_params"])     # the switch does switch
    # the switch leaks nothing: the fp32 path afterwards, on the golden case, within the fp32 test's own bounds
    enc, img, g = _golden_encoder("fp32")
    p, h = enc(img)
    torch.cuda.synchronize()

    def within(name, got, ref, atol, rtol):
        err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
        print(f"[parity] fp32 after bf16, {name}: max|err|={err.max():.3e}")
        assert np.all(err <= atol + rtol * np.abs(ref)), (name, err.max())
    within("golden params", p.cpu().numpy(), g["params"], 1e-4, 1e-4)
    within("golden hand_class", h.cpu().numpy(), g["hand_class"], 1e-5, 0)
    within("golden main_feat", enc.main_feat.cpu().numpy(), g["main_feat"], 1e-4 * float(np.abs(g["main_feat"]).max()), 1e-4)
    with pytest.raises(ValueError):
        InterHandModel(_opt(B, isTrain=True, encoder_precision="bf16"))
    with pytest.raises(ValueError):
        InterHandModel(_opt(B, encoder_precision="fp16"))
    # the reference's train-mode robustifier (loss_utils.py:36) is not what the training launches evaluate: refused, by both trainable models
    from ihmr_amd.mlp_model import MLPModel
    for cls in (InterHandModel, MLPModel):
        with pytest.raises(ValueError, match="sdf_robustifier"):
            cls(_opt(B, isTrain=True, sdf_robustifier=0.05))
    InterHandModel(_opt(B, sdf_robustifier=0.05))             # inference never reads it


def test_report_what_bf16_costs_downstream(mano_arrays):
    """Reported, not gated: the difference between the fp32 and the bf16 model's exported pred_joints_3d on a 64-image synthetic batch.
    With seeded RANDOM weights this is not an accuracy claim about a trained checkpoint."""
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    B = 64
    m16, m32 = _seeded(InterHandModel(_opt(B, encoder_precision="bf16"))), _seeded(InterHandModel(_opt(B)))
    fwd = lambda p, s, t: two_hand.forward_from_packed(m32.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    batch = synthetic_opt_batch(B, fwd, seed=1234, with_image=True)
    res = []
    for m in (m16, m32):
        m.set_input(batch); m.test(); torch.cuda.synchronize()
        res.append(m.get_pred_result())
    d = np.linalg.norm(res[0]["pred_joints_3d"][..., :3] - res[1]["pred_joints_3d"][..., :3], axis=-1) * 1000.0
    print(f"[report] bf16 vs fp32 pred_joints_3d on seeded random weights, B=64: mean {d.mean():.3f} mm, max {d.max():.3f} mm")
    assert np.isfinite(d).all()

"""The opt-in bf16 encoder path (``encoder_precision = "bf16"``), checked without a GPU: the cross-compiled kernels (matrix
instruction present, no spills), the C ABI, the weight packing, the rounding helper of csrc/ihmr_pure.h under the sanitizers, and the
CPU emulation of the numerics contract (tests/bf16_emulation.py) against the reference's own outputs."""
import ctypes
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402
import hostbuild  # noqa: E402

NEW_SYMBOLS = ["ihmr_conv_igemm_bf16", "ihmr_pack_image_bf16", "ihmr_maxpool3x3s2_bf16", "ihmr_avgpool_relu_bf16", "ihmr_cast_f32_bf16"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_bf16_conv_kernel_uses_the_bf16_matrix_cores_and_does_not_spill():
    """Device assembly of the product build (as tests/test_build_cpu.py reads it): `conv_igemm_bf16_kernel` is instantiated, the code
    object holds a bf16 matrix instruction, and no instantiation of the kernel uses scratch."""
    seen = {name: (r["vgpr_count"], r["vgpr_spill_count"], r["private_segment_fixed_size"])
            for name, r in codeobj.records().items() if "conv_igemm_bf16_kernel" in name}
    assert seen, "no conv_igemm_bf16_kernel instantiation in the code object"
    for name, (vgpr, spill, scratch) in seen.items():
        print(f"[build] {name}: {vgpr} VGPRs, {spill} spilled, {scratch} B scratch")
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        # the kernel's own body issues the bf16 matrix instruction
        body = "\n".join(codeobj.body(name))
        assert "v_mfma_f32_32x32x16_bf16" in body or "v_mfma_f32_16x16x32_bf16" in body, name


def test_library_exports_the_bf16_entry_points():
    """The five new symbols resolve in the built library (it loads without a GPU) and the version string says 0.2."""
    from ihmr_amd import hip
    L = hip.bind(ctypes.CDLL(hip.build()))
    for sym in NEW_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in hip.EXPORTED_SYMBOLS, sym
    assert b"0.2" in L.ihmr_version() and b"gfx950" in L.ihmr_version()


@pytest.mark.parametrize("cfg", [
    dict(cout=64, cin=64, k=3, stride=1, pad=1, k_extra=0),      # a 3 x 3 layer
    dict(cout=256, cin=128, k=1, stride=2, pad=0, k_extra=0),    # a strided 1 x 1 (downsample)
    dict(cout=64, cin=3, k=7, stride=2, pad=3, k_extra=1),       # the stem: Cin 3 -> 4, K = 196 padded to 224
    dict(cout=40, cin=32, k=3, stride=1, pad=1, k_extra=0),      # Cout not a tile multiple
    dict(cout=160, cin=48, k=3, stride=2, pad=1, k_extra=0),     # Cout not a wide-tile multiple, K = 432 padded to 448
])
def test_packed_bf16_weights_unpack_to_the_folded_rounded_matrix(cfg):
    """`_PackedBF16(w, b).unpack()` is fold -> `.bfloat16()` bit for bit, in K-major order (tap-major, channel-minor); the padding rows
    and columns of the packed image are zero; the bias stays fp32."""
    from ihmr_amd.networks import _PackedBF16, _fold_bn
    g = torch.Generator().manual_seed(11)
    conv = torch.nn.Conv2d(cfg["cin"], cfg["cout"], cfg["k"], stride=cfg["stride"], padding=cfg["pad"], bias=False)
    bn = torch.nn.BatchNorm2d(cfg["cout"])
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        bn.weight.copy_(torch.rand(cfg["cout"], generator=g) + 0.5); bn.bias.copy_(torch.randn(cfg["cout"], generator=g))
        bn.running_mean.copy_(torch.randn(cfg["cout"], generator=g)); bn.running_var.copy_(torch.rand(cfg["cout"], generator=g) + 0.5)
    w, b = _fold_bn(conv, bn)
    pk = _PackedBF16(w, b, stride=cfg["stride"], pad=cfg["pad"], k_extra=cfg["k_extra"])
    cin = cfg["cin"] + cfg["k_extra"]
    K = cfg["k"] ** 2 * cin
    wk = w.permute(2, 3, 1, 0)
    if cfg["k_extra"]:
        wk = torch.cat([wk, torch.zeros(cfg["k"], cfg["k"], cfg["k_extra"], cfg["cout"])], dim=2)
    ref = wk.reshape(K, cfg["cout"]).bfloat16()
    got = pk.unpack()
    assert got.dtype == torch.bfloat16 and got.shape == (K, cfg["cout"])
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    full = pk.unpack(padded=True)
    assert full.shape[0] % 32 == 0 and full.shape[0] >= K and full.shape[1] % 64 == 0 and full.shape[1] >= cfg["cout"]
    assert pk.w.shape == (full.shape[0] // 8, pk.ldw, 8) and pk.w.is_contiguous()
    assert not full[K:].view(torch.int16).any() and not full[:, cfg["cout"]:].view(torch.int16).any()
    # the documented address: element (k, n) at ((k // 8) * ldw + n) * 8 + k % 8
    flat = pk.w.reshape(-1).view(torch.int16)
    for k, n in [(0, 0), (7, 1), (8, 0), (K - 1, cfg["cout"] - 1), (K // 2 + 3, cfg["cout"] // 2)]:
        assert flat[((k // 8) * pk.ldw + n) * 8 + k % 8] == ref.view(torch.int16)[k, n]
    assert pk.b.dtype == torch.float32 and torch.equal(pk.b, b)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rounding_helper_has_the_bits_of_torch(tmp_path):
    """`ihmr_f32_to_bf16` / `ihmr_bf16_to_f32` of csrc/ihmr_pure.h on the host under AddressSanitizer / UBSan: all 65 536 bf16 patterns
    widen exactly and round-trip (NaNs to the quiet NaN torch gives), every tie with even and odd neighbours, +-0, subnormals, the
    largest finite float (rounds to inf), +-inf, NaNs; bits equal `torch.tensor(x).bfloat16()`."""
    exe = hostbuild.build("pure_bf16_driver.cpp", tmp_path, hostbuild.X86_V3)

    def run(op, words, out_dtype):
        words = np.ascontiguousarray(words, np.uint32)
        fin, fout = str(tmp_path / f"{op}.in"), str(tmp_path / f"{op}.out")
        with open(fin, "wb") as fh:
            fh.write(np.int32(words.size).tobytes())
            fh.write(words.tobytes())
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, out_dtype)

    def torch_bits(words):
        """torch's bits.  For a NaN torch has no single answer: `torch.tensor(x).bfloat16()` of a scalar gives the quiet NaN 0x7FC0 (c10's
        scalar rounding), the vectorised conversion of a longer CPU tensor gives 0xFFFF.  The helper follows the scalar form -- the
        expression this test is specified by -- so NaN inputs take their reference from a scalar conversion."""
        words = np.ascontiguousarray(words, np.uint32)
        f = torch.from_numpy(words.view(np.int32).copy()).view(torch.float32)
        out = f.bfloat16().view(torch.int16).numpy().view(np.uint16).copy()
        nan = (words & 0x7fffffff) > 0x7f800000
        scalar_nan = torch.tensor(float("nan")).bfloat16().view(torch.int16).item() & 0xffff
        assert scalar_nan == 0x7fc0
        out[nan] = scalar_nan
        return out

    pats = np.arange(65536, dtype=np.uint32)
    # widening is a 16-bit shift
    assert np.array_equal(run("widen", pats, np.uint32), pats << 16)
    # every bf16 value round-trips (a NaN comes back as the quiet NaN, as in torch)
    got = run("narrow", pats << 16, np.uint16)
    assert np.array_equal(got, torch_bits(pats << 16))
    notnan = (pats & 0x7fff) <= 0x7f80
    assert np.array_equal(got[notnan], pats[notnan].astype(np.uint16)) and np.all(got[~notnan] == 0x7fc0)
    # every tie (low half 0x8000) -- the neighbour below is even or odd with the pattern's bit 16 -- and its two neighbours
    ties = (pats << 16) | 0x8000
    cases = np.concatenate([ties, ties - 1, ties + 1,
                            np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00007fff, 0x00008000, 0x00008001, 0x007fffff, 0x00800000,
                                      0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001,
                                      0x7fffffff, 0x3f800000, 0x3f808000, 0x3f818000], np.uint32)])
    rng = np.random.default_rng(0)
    cases = np.concatenate([cases, rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)])
    got, ref = run("narrow", cases, np.uint16), torch_bits(cases)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, [(hex(int(cases[i])), hex(int(got[i])), hex(int(ref[i]))) for i in bad[:5]]
    # overflow rounds to inf, ties go to even
    one = lambda w: int(run("narrow", np.array([w], np.uint32), np.uint16)[0])
    assert one(0x7f7fffff) == 0x7f80 and one(0xff7fffff) == 0xff80
    assert one(0x3f808000) == 0x3f80 and one(0x3f818000) == 0x3f82


def test_bf16_emulation_against_the_reference_golden():
    """tests/bf16_emulation.py (the checker of the GPU tests) on the weights and image of tests/golden/encoder.npz, against the
    REFERENCE's fp32 outputs stored there.  What bf16 operands cost on this case, measured with torch CPU when the feature was written:

        max|d main_feat| / max|main_feat| = 5.36e-3     rms(d main_feat) / rms(main_feat) = 3.36e-3
        max|d params| = 0.0469                          max|d hand_class| = 4.1e-3

    asserted within +-10 % (deterministic on one torch build; the slack is for another CPU's conv summation order).  The GPU test's
    end-to-end bounds are twice these values."""
    import bf16_emulation as E
    from helpers import seeded_state_dict
    from ihmr_amd.networks import InterHandEncoder
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "encoder.npz")))
    enc = InterHandEncoder(types.SimpleNamespace(total_params_dim=122), torch.tensor(g["mean_params"]).repeat(2, 1))
    enc.load_state_dict(seeded_state_dict(enc, 100))
    img = torch.tensor(np.random.RandomState(7).uniform(-1, 1, (2, 3, 224, 224)), dtype=torch.float32)
    torch.set_num_threads(8)
    mf, p, h = (t.numpy() for t in E.encoder(enc, img))
    d = np.abs(mf - g["main_feat"])
    got = dict(main_feat_max=d.max() / np.abs(g["main_feat"]).max(),
               main_feat_rms=np.sqrt((d ** 2).mean()) / np.sqrt((g["main_feat"] ** 2).mean()),
               params_max=np.abs(p - g["params"]).max(), hand_class_max=np.abs(h - g["hand_class"]).max())
    want = dict(main_feat_max=5.36e-3, main_feat_rms=3.36e-3, params_max=0.0469, hand_class_max=4.1e-3)
    for k, v in want.items():
        print(f"[parity] bf16 emulation vs reference golden: {k} = {got[k]:.4e} (recorded {v:.3e})")
    for k, v in want.items():
        assert 0.9 * v <= got[k] <= 1.1 * v, (k, got[k], v)


def test_encoder_precision_option_is_validated_without_a_gpu():
    from ihmr_amd.networks import InterHandEncoder
    mp = torch.zeros(1, 122)
    assert InterHandEncoder(types.SimpleNamespace(), mp).encoder_precision == "fp32"
    assert InterHandEncoder(types.SimpleNamespace(encoder_precision="bf16"), mp).encoder_precision == "bf16"
    with pytest.raises(ValueError):
        InterHandEncoder(types.SimpleNamespace(encoder_precision="fp16"), mp)

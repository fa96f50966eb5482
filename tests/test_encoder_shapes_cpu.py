"""CPU side of the per-layer batch-64 encoder pass (tests/test_gpu_encoder_shapes.py): the shape table derived from
``InterHandEncoder`` is the ResNet-50 one, the restated launcher selection (tests/encoder_shapes.py) gives each layer the expected
kernel form, every form the fp32 launcher can select is taken by some tested case, and the integer operand draws stay in the range
where fp32 (and, for the bf16 path, bf16) holds every value exactly -- so the GPU test never has to skip or thin a case."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_shapes as E  # noqa: E402

MI355X_CUS = 256

# (first layer of the geometry, H, Cin, Cout, k, stride, M at B = 64, K steps of 16, form at 256 CUs / 128 MiB, tiles)
TRUNK_B64 = [
    ("stem",    224,    4,   64, 7, 2, 802816,  13, "128x64_c4",    6272),
    ("l1.0.c1",  56,   64,   64, 1, 1, 200704,   4, "128x64_fast",  1568),
    ("l1.0.c2",  56,   64,   64, 3, 1, 200704,  36, "128x64_fast",  1568),
    ("l1.0.c3",  56,   64,  256, 1, 1, 200704,   4, "128x128_fast", 3136),
    ("l1.1.c1",  56,  256,   64, 1, 1, 200704,  16, "128x64_fast",  1568),
    ("l2.0.c1",  56,  256,  128, 1, 1, 200704,  16, "128x128_fast", 1568),
    ("l2.0.c2",  56,  128,  128, 3, 2,  50176,  72, "streamk",       392),
    ("l2.0.c3",  28,  128,  512, 1, 1,  50176,   8, "128x128_fast", 1568),
    ("l2.0.ds",  56,  256,  512, 1, 2,  50176,  16, "128x128_fast", 1568),
    ("l2.1.c1",  28,  512,  128, 1, 1,  50176,  32, "128x128_fast",  392),     # 392 >= 384: no split
    ("l2.1.c2",  28,  128,  128, 3, 1,  50176,  72, "streamk",       392),
    ("l3.0.c1",  28,  512,  256, 1, 1,  50176,  32, "64x128_fast",  1568),
    ("l3.0.c2",  28,  256,  256, 3, 2,  12544, 144, "streamk",       196),
    ("l3.0.c3",  14,  256, 1024, 1, 1,  12544,  16, "64x128_fast",  1568),
    ("l3.0.ds",  28,  512, 1024, 1, 2,  12544,  32, "64x128_fast",  1568),
    ("l3.1.c1",  14, 1024,  256, 1, 1,  12544,  64, "streamk",       196),
    ("l3.1.c2",  14,  256,  256, 3, 1,  12544, 144, "streamk",       196),
    ("l4.0.c1",  14, 1024,  512, 1, 1,  12544,  64, "streamk",       392),
    ("l4.0.c2",  14,  512,  512, 3, 2,   3136, 288, "streamk",       100),
    ("l4.0.c3",   7,  512, 2048, 1, 1,   3136,  32, "128x128_fast",  400),
    ("l4.0.ds",  14, 1024, 2048, 1, 2,   3136,  64, "streamk",       400),
    ("l4.1.c1",   7, 2048,  512, 1, 1,   3136, 128, "streamk",       100),
    ("l4.1.c2",   7,  512,  512, 3, 1,   3136, 288, "streamk",       100),
]
# (name, Cin, Cout, ldx, ldy, ldr, act, K steps, form, ksplit).  `cls` reads the first 1024 columns of the 1152-wide IEF buffer:
# K = 1024, 64 steps, split 16 (a restatement that takes K = 1152 for it arrives at 72 steps and 18 -- the containers say 1024).
HEADS_B64 = [
    ("fc1",  2048, 1024, 2048, 1024,    0, 1, 128, "64x128_fast_splitk_reduce4", 32),
    ("feat", 1024, 1024, 1024, 1152,    0, 1,  64, "64x128_fast_splitk_reduce4", 16),
    ("reg",  1152,  122, 1152, 1152, 1152, 0,  72, "64x128_fast_splitk_reduce1", 18),
    ("cls",  1024,    2, 1152,    2,    0, 2,  64, "64x64_fast_splitk_reduce1",  16),
]


def test_the_table_is_resnet50_at_any_batch_size():
    """23 trunk geometries, the ones typed in above; a layer added to or dropped from the trunk changes the list.  Every one of the
    53 convolutions of the trunk lands in exactly one entry."""
    for B in (1, 7, 64, 512):
        T = E.trunk_table(B)
        assert [(s.name, s.H, s.Cin, s.Cout, s.k, s.stride) for s in T] == [t[:6] for t in TRUNK_B64], B
        assert all(s.N == B and s.W == s.H and s.ldx == s.Cin and s.ldy == s.Cout for s in T)
        assert sorted(n for s in T for n in (s.name,) + s.also) == sorted(s.name for s in E.trunk_layers(B))
        assert sum(1 + len(s.also) for s in T) == 53
    T = {s.name: s for s in E.trunk_table(64)}
    assert [E.gemm_dims(T[t[0]])[0] for t in TRUNK_B64] == [t[6] for t in TRUNK_B64]
    # residual and activation as forward() passes them: conv3 adds the block's input (or its projection) and applies ReLU, the
    # projection itself has neither; l1.0.ds shares l1.0.c3's geometry (the GPU test runs every entry with act = 0 as well)
    for s in E.trunk_layers(64):
        role = s.name.rsplit(".", 1)[-1]
        assert (s.residual, s.act, s.ldr) == {"c3": (True, 1, s.Cout), "ds": (False, 0, 0)}.get(role, (False, 1, 0)), s
    assert T["l1.0.c3"].also[0] == "l1.0.ds"
    H = E.head_table(64)
    assert [(s.name, s.Cin, s.Cout, s.ldx, s.ldy, s.ldr, s.act) for s in H] == [h[:7] for h in HEADS_B64]
    assert all(E.gemm_dims(s)[0] == 64 for s in H) and [s.residual for s in H] == [False, False, True, False]


def test_plan_fp32_gives_the_batch64_forms():
    for s, t in zip(E.trunk_table(64), TRUNK_B64):
        p = E.plan_fp32(s, MI355X_CUS, E.WORKSPACE_BYTES)
        assert (p["nk"], p["form"], p["tiles"], p["ksplit"]) == (t[7], t[8], t[9], 1), (s.name, p)
        if p["streamk"]:
            slots, whole = E.streamk_slots(p)
            # at batch 64 no worker owns a whole tile: at most 56 K steps per worker against nk >= 64
            assert p["workers"] == 512 and not whole and p["tiles"] * p["nk"] // 512 <= 56 < 64 <= p["nk"], (s.name, p)
            assert E.workspace_footprint(s, p) == ("slots", {2 * w + sl for w, sl in slots}) and len(slots) >= p["workers"]
        else:
            assert E.workspace_footprint(s, p) == ("none",)
    for s, h in zip(E.head_table(64), HEADS_B64):
        p = E.plan_fp32(s, MI355X_CUS, E.WORKSPACE_BYTES)
        assert (p["nk"], p["form"], p["ksplit"]) == (h[7], h[8], h[9]), (s.name, p)
        assert E.workspace_footprint(s, p) == ("prefix", h[9] * 64 * s.Cout)
    # the selection follows the device: other CU counts give other worker counts, recomputed, never skipped
    s = E.trunk_table(64)[6]
    assert E.plan_fp32(s, 304)["workers"] == 512 and E.plan_fp32(s, 120)["workers"] == 240 and E.plan_fp32(s, 3)["workers"] == 8
    assert E.plan_fp32(s, 256, workspace_bytes=32 << 20)["form"] == "128x128_fast"     # below the 64 MiB of slots: one workgroup per tile


def test_plan_bf16_at_batch64():
    """ihmr_conv_igemm_bf16: 128 x 64 tiles for Cout <= 64, 128 x 128 otherwise; the 4-channel form for the stem, the fast gather
    elsewhere; split-K (up to 8 pieces of >= 4 steps) exactly where a layer has fewer than two tiles per CU."""
    want = {"l2.0.c2": 2, "l2.1.c1": 2, "l2.1.c2": 2, "l3.0.c2": 3, "l3.1.c1": 3, "l3.1.c2": 3, "l4.0.c1": 2, "l4.0.c2": 6, "l4.0.c3": 2,
            "l4.0.ds": 2, "l4.1.c1": 6, "l4.1.c2": 6}
    for s in E.trunk_table(64):
        p = E.plan_bf16(s, MI355X_CUS)
        assert p["tile"] == (128, 64 if s.Cout <= 64 else 128) and p["mode"] == ("c4" if s.name == "stem" else "fast"), (s.name, p)
        assert p["ksplit"] == want.get(s.name, 1), (s.name, p)
        assert (p["ksplit"] > 1) == (p["tiles"] < 2 * MI355X_CUS and p["nk"] >= 8)
        assert E.workspace_footprint(s, p) == (("prefix", p["ksplit"] * E.gemm_dims(s)[0] * s.Cout) if p["ksplit"] > 1 else ("none",))


def _small_case_plans(test_name):
    import test_gpu_encoder as G
    out = []
    for c in getattr(G, test_name).pytestmark[0].args[1]:
        s = E.Shape("small", c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["s"], c["p"], c["Cin"], c["Cout"], c["Cout"], bool(c.get("res")), 1, ())
        out.append((c, s, E.plan_fp32(s, MI355X_CUS)))
    return out


def test_every_fp32_form_has_a_covering_case():
    """Every form ihmr_conv_igemm can select for a Cin % 16 == 0 layer (and the stem's) is taken by an entry of table + heads at batch
    64; the three it has that batch 64 does NOT reach are named here with the small-shape case of tests/test_gpu_encoder.py that
    covers each.  Losing the last covering case of a form fails this test."""
    plans = {s.name: E.plan_fp32(s, MI355X_CUS) for s in E.trunk_table(64) + E.head_table(64)}
    forms = {}
    for name, p in plans.items():
        forms.setdefault(p["form"], []).append(name)
    reachable = {"128x128_fast", "64x128_fast", "128x64_fast", "128x64_c4", "streamk",
                 "64x128_fast_splitk_reduce4", "64x128_fast_splitk_reduce1", "64x64_fast_splitk_reduce1"}
    assert set(forms) == reachable, forms
    assert any(plans[n]["tile"] == (64, 64) for n in plans)                        # the 64 x 64 tile: cls
    assert {plans[n]["reduce"] for n in plans} == {None, 4, 1}                     # both reduce kernels: fc1 / feat and reg / cls
    # full grids of the forms the small cases only touch with a handful of tiles
    assert plans["stem"]["tiles"] == 6272 and plans["l1.0.c3"]["tiles"] == 3136 and plans["l3.0.c1"]["tiles"] == 1568
    # --- not reached at batch 64, covered by small shapes:
    igemm, sk = _small_case_plans("test_conv_igemm_matches_torch"), _small_case_plans("test_conv_streamk_matches_torch")
    # (1) 2-way split-K of the 128 x 128 tile: "strided 1x1 (downsample)", N=2 28x28 128 -> 256 (8 tiles, 8 K steps -> 2 pieces).  The
    #     launcher's OWN 2-way branch (64 <= tiles < 384, >= 64 K steps, not Stream-K) is taken by no case there: the GPU file adds one.
    c, _, p = igemm[2]
    assert (c["Cin"], c["Cout"], c["s"]) == (128, 256, 2) and p["form"] == "128x128_fast_splitk_reduce4" and p["ksplit"] == 2, p
    # (2) Stream-K workers that own whole tiles: N=96 10x10 1024 -> 1024 (600 tiles x 64 steps over 512 workers = 75 steps each)
    c, s, p = sk[1]
    assert c["N"] == 96 and p["streamk"] and E.streamk_slots(p)[1], p
    assert [q["streamk"] for _, _, q in sk] == [True, True, True, False] and sk[3][2]["ksplit"] == 18
    # (3) the generic gather (Cin not a multiple of 16): the Cin = 3 stem and the Cin = 2064 case beyond the zero page
    assert [(c["Cin"], p["mode"]) for c, _, p in igemm if p["mode"] == "generic"] == [(3, "generic"), (2064, "generic")]
    from test_gpu_encoder_shapes import EXTRA_SHAPES
    p = E.plan_fp32(EXTRA_SHAPES[0], MI355X_CUS)
    assert p["form"] == "128x128_fast_splitk_reduce4" and p["ksplit"] == 2 and 64 <= p["tiles"] < 384 and p["nk"] >= 64, p


def test_integer_draws_stay_exact():
    """The float64 reference of the GPU test's integer operands, whole batch of 64, every table entry: max |y| < 2^24 for the fp32
    draw (and its a-priori bound K * 8 * 7 + 16 too, at any batch size: the B = 512 probes), 8 <= max |y| <= 256 for the bf16 draw."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for s in E.trunk_table(64) + E.head_table(64):
        assert E.fp32_integer_bound(s) < 2 ** 24
        x, w, b, r = E.draw_integers(s, "fp32")
        y = E.reference(s, x, w, b, r)
        top = float(y.abs().max())
        assert y.dtype == torch.float64 and top <= E.fp32_integer_bound(s) < 2 ** 24 and top >= 64, (s.name, top)
        assert bool((y == y.round()).all()) and float(w.min()) == -5 and float(w.max()) == 7
        if s.name in ("fc1", "feat", "reg", "cls"):
            continue                                                               # the heads stay fp32 in the bf16 encoder
        x, w, b, r = E.draw_integers(s, "bf16")
        top = float(E.reference(s, x, w, b, r).abs().max())
        print(f"[draw] {s.name}: bf16 max|y|={top:.0f}")
        assert 8 <= top <= 256, (s.name, top)
    # the three chained IEF iterations feed on their own output: their narrower draw, bounded over the whole chain
    feat, params, W, bias, refs = E.reg_chain(64)
    bound = E.reg_chain_partial_bound(feat, params, W, bias, refs)
    print(f"[draw] reg chain: max|params| per iteration {[float(r.abs().max()) for r in refs]}, partial-sum bound {bound:.0f}")
    assert bound < 2 ** 24 and all(bool((r == r.round()).all()) for r in refs) and float(refs[2].abs().max()) > float(refs[0].abs().max())

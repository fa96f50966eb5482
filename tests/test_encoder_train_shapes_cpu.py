"""CPU side of the per-launch batch-64 pass over the training backward kernels (tests/test_gpu_encoder_train_shapes.py): the table of
weight-gradient and input-gradient launches derived from the module is the ResNet-50 one, the restated ``ihmr_conv_wgrad`` selection
(tests/encoder_train_shapes.py) gives each layer the expected form, the integer draws stay where fp32 holds every partial sum of any
summation order exactly, and the kernel's float-reciprocal pixel division is exact on its whole range for every divisor the table
produces -- so the GPU test never has to skip or thin a case."""
import collections
import inspect
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_shapes as E  # noqa: E402
import encoder_train_shapes as TS  # noqa: E402

MI355X_CUS = 256

# (first unit of the geometry, M at B = 64, K, tile over K x Cout, msplit, chunks per slice, chunks of the last slice, reduce kernel)
WGRAD_B64 = [
    ("stem",    802816,  196, (128,  64), 256, 196, 196, "wgrad_reduce"),
    ("l1.0.c1", 200704,   64, ( 64,  64), 256,  49,  49, "wgrad_reduce"),
    ("l1.0.c2", 200704,  576, (128,  64), 203,  62,  20, "wgrad_reduce"),
    ("l1.0.c3", 200704,   64, ( 64, 128), 256,  49,  49, "wgrad_reduce"),
    ("l1.1.c1", 200704,  256, (128,  64), 256,  49,  49, "wgrad_reduce"),
    ("l2.0.c1", 200704,  256, (128, 128), 256,  49,  49, "wgrad_reduce"),
    ("l2.0.c2",  50176, 1152, (128, 128), 112,  28,  28, "wgrad_reduce"),
    ("l2.0.c3",  50176,  128, (128, 128), 242,  13,   3, "wgrad_reduce"),
    ("l2.0.ds",  50176,  256, (128, 128), 126,  25,  11, "wgrad_reduce"),
    ("l2.1.c1",  50176,  512, (128, 128), 242,  13,   3, "wgrad_reduce"),
    ("l2.1.c2",  50176, 1152, (128, 128), 112,  28,  28, "wgrad_reduce"),
    ("l3.0.c1",  50176,  512, (128, 128), 126,  25,  11, "wgrad_reduce"),
    ("l3.0.c2",  12544, 2304, (128, 128),  28,  28,  28, "splitk_reduce4"),
    ("l3.0.c3",  12544,  256, (128, 128),  61,  13,   4, "wgrad_reduce"),
    ("l3.0.ds",  12544,  512, (128, 128),  32,  25,   9, "wgrad_reduce"),       # exactly on the reduce kernels' boundary
    ("l3.1.c1",  12544, 1024, (128, 128),  61,  13,   4, "wgrad_reduce"),
    ("l3.1.c2",  12544, 2304, (128, 128),  28,  28,  28, "splitk_reduce4"),
    ("l4.0.c1",  12544, 1024, (128, 128),  32,  25,   9, "wgrad_reduce"),       # exactly on the boundary
    ("l4.0.c2",   3136, 4608, (128, 128),   8,  25,  21, "splitk_reduce4"),
    ("l4.0.c3",   3136,  512, (128, 128),  16,  13,   1, "splitk_reduce4"),     # one chunk of 13 in the last slice
    ("l4.0.ds",   3136, 1024, (128, 128),   8,  25,  21, "splitk_reduce4"),
    ("l4.1.c1",   3136, 2048, (128, 128),  16,  13,   1, "splitk_reduce4"),
    ("l4.1.c2",   3136, 4608, (128, 128),   8,  25,  21, "splitk_reduce4"),
]
# (kind, first unit, [(kh, kw, M, K steps of 16, form at 256 CUs)] per launch, residual)
DGRAD_B64 = [
    ("s1",    "l1.0.c1", [(1, 1, 200704,   4, "128x64_fast")], True),
    ("s1",    "l1.0.c2", [(3, 3, 200704,  36, "128x64_fast")], False),
    ("s1",    "l1.0.c3", [(1, 1, 200704,  16, "128x64_fast")], False),
    ("s1",    "l1.1.c1", [(1, 1, 200704,   4, "128x128_fast")], True),
    ("s1",    "l2.0.c1", [(1, 1, 200704,   8, "128x128_fast")], True),
    ("phase", "l2.0.c2", [(1, 1, 50176, 8, "128x128_fast"), (1, 2, 50176, 16, "128x128_fast"), (2, 1, 50176, 16, "128x128_fast"),
                          (2, 2, 50176, 32, "128x128_fast")], False),
    ("s1",    "l2.0.c3", [(1, 1,  50176,  32, "128x128_fast")], False),
    ("ds",    "l2.0.ds", [(1, 1,  50176,  32, "64x128_fast")], False),
    ("s1",    "l2.1.c1", [(1, 1,  50176,   8, "128x128_fast")], True),
    ("s1",    "l2.1.c2", [(3, 3,  50176,  72, "streamk")], False),
    ("s1",    "l3.0.c1", [(1, 1,  50176,  16, "128x128_fast")], True),
    ("phase", "l3.0.c2", [(1, 1, 12544, 16, "128x128_fast"), (1, 2, 12544, 32, "128x128_fast"), (2, 1, 12544, 32, "128x128_fast"),
                          (2, 2, 12544, 64, "streamk")], False),
    ("s1",    "l3.0.c3", [(1, 1,  12544,  64, "streamk")], False),
    ("ds",    "l3.0.ds", [(1, 1,  12544,  64, "streamk")], False),
    ("s1",    "l3.1.c1", [(1, 1,  12544,  16, "64x128_fast")], True),
    ("s1",    "l3.1.c2", [(3, 3,  12544, 144, "streamk")], False),
    ("s1",    "l4.0.c1", [(1, 1,  12544,  32, "64x128_fast")], True),
    ("phase", "l4.0.c2", [(1, 1, 3136, 32, "128x128_fast"), (1, 2, 3136, 64, "streamk"), (2, 1, 3136, 64, "streamk"),
                          (2, 2, 3136, 128, "streamk")], False),
    ("s1",    "l4.0.c3", [(1, 1,   3136, 128, "streamk")], False),
    ("ds",    "l4.0.ds", [(1, 1,   3136, 128, "streamk")], False),
    ("s1",    "l4.1.c1", [(1, 1,   3136,  32, "128x128_fast")], True),
    ("s1",    "l4.1.c2", [(3, 3,   3136, 288, "streamk")], False),
]


def test_the_backward_table_is_resnet50():
    """53 weight-gradient launches in 23 geometries; 46 stride-1 turned convolutions, 3 downsample GEMMs and 3 x 4 parity phases in
    16 + 3 + 3 geometries; nothing for the stem; every c1 (and nothing else) carries the skip gradient as a residual."""
    for B in (1, 7, 64):
        units, table = TS.wgrad_units(B), TS.wgrad_table(B)
        assert len(units) == 53 and len(table) == 23 and [u.name for u in table] == [t[0] for t in WGRAD_B64]
        assert sum(1 + len(u.also) for u in table) == 53
        du, dt = TS.dgrad_units(B), TS.dgrad_table(B)
        assert collections.Counter(d.kind for d in du) == {"s1": 46, "ds": 3, "phase": 3}
        assert collections.Counter(d.kind for d in dt) == {"s1": 16, "ds": 3, "phase": 3}
        assert sum(len(d.shapes) for d in du) == 46 + 3 + 12 and sum(len(d.shapes) for d in dt) == 16 + 3 + 12
        assert sorted(n for d in dt for n in (d.unit.name,) + d.also) == sorted(u.name for u in units if u.name != "stem")
        assert [(d.kind, d.unit.name, d.shapes[0].residual) for d in dt] == [(t[0], t[1], t[3]) for t in DGRAD_B64]
        for d in du:
            u = d.unit
            assert all(s.residual == u.name.endswith(".c1") and s.ldr == (u.Cin if s.residual else 0) for s in d.shapes), u.name
            assert all((s.N, s.Cin, s.Cout, s.stride, s.ldx, s.ldy, s.act) == (B, u.Cout, u.Cin, 1, u.Cout, u.Cin, 0) for s in d.shapes)
            Ho, Wo = E.out_hw(u)
            if d.kind == "s1":
                s, = d.shapes
                assert E.out_hw(s) == (u.H, u.W) and (s.H, s.W, s.pad, E.filter_hw(s)) == (Ho, Wo, u.k - 1 - u.pad, (u.k, u.k))
            elif d.kind == "ds":
                s, = d.shapes
                assert E.out_hw(s) == (s.H, s.W) == (Ho, Wo) == (u.H // 2, u.W // 2) and E.filter_hw(s) == (1, 1) and s.pad == 0
            else:
                assert [E.filter_hw(s) for s in d.shapes] == [(1, 1), (1, 2), (2, 1), (2, 2)]
                assert all(E.out_hw(s) == (s.H, s.W) == (Ho, Wo) == (u.H // 2, u.W // 2) and s.pad == 0 for s in d.shapes)
    rows = TS.unit_rows(64)
    assert rows[0] == ("stem", 4, 64, 7, 2, 3, "none") and [r[0] for r in rows if r[6] == "phase"] == ["l2.0.c2", "l3.0.c2", "l4.0.c2"]
    assert [r[0] for r in rows if r[6] == "ds"] == ["l2.0.ds", "l3.0.ds", "l4.0.ds"]


def test_plan_wgrad_gives_the_batch64_forms():
    from ihmr_amd import encoder_train
    assert "64 * 1024 * 1024" in inspect.getsource(encoder_train.conv_wgrad) and TS.WGRAD_WORKSPACE_BYTES == 256 << 20
    plans = {}
    for u, t in zip(TS.wgrad_table(64), WGRAD_B64):
        p = plans[u.name] = TS.plan_wgrad(u)
        M, K = E.gemm_dims(u)
        assert (M, K, p["tile"], p["msplit"], p["chunks_per"], p["last"], p["reduce"]) == t[1:], (u.name, p)
        assert p["nchunks"] == M // 16 == (p["msplit"] - 1) * p["chunks_per"] + p["last"] and p["prefix"] * 4 <= TS.WGRAD_WORKSPACE_BYTES
        assert p["prefix"] == p["msplit"] * K * u.Cout
    assert {p["tile"] for p in plans.values()} == {(64, 64), (64, 128), (128, 64), (128, 128)}       # all four template forms
    assert {p["reduce"] for p in plans.values()} == {"wgrad_reduce", "splitk_reduce4"}               # both reduce kernels
    assert sorted(n for n, p in plans.items() if p["msplit"] == 32) == ["l3.0.ds", "l4.0.c1"]         # on the boundary, on the wide side
    assert all((p["reduce"] == "wgrad_reduce") == (p["msplit"] >= 32) for p in plans.values())
    ragged = [n for n, p in plans.items() if p["last"] < p["chunks_per"]]
    assert len(ragged) >= 5 and {"l4.0.c3", "l4.1.c1", "l2.0.c3", "l3.0.c3"} <= set(ragged), ragged
    assert plans["stem"]["msplit"] * plans["stem"]["chunks_per"] * 16 == 802816                       # 256 slices x 196 chunks
    assert plans["l4.0.c2"]["prefix"] * 4 == 72 << 20
    # the largest pixel count of the table is far inside the division's range; the launcher refuses what is outside it
    assert max(E.gemm_dims(u)[0] for u in TS.wgrad_table(64)) == 802816 < TS.WGRAD_MAX_PIXELS
    assert TS.plan_wgrad(TS.wgrad_table(64)[0]._replace(N=669)) is None and TS.plan_wgrad(TS.wgrad_table(64)[0]._replace(N=668)) is not None


def test_plan_fp32_gives_the_input_gradient_forms():
    """The turned launches through the generalised plan_fp32 (kh != kw, output map given): 7 of the 19 stride-1 launches and 4 of the
    12 phase filters are Stream-K at 256 CUs, three of those with kh != kw and taps that run off the map's edge."""
    table = TS.dgrad_table(64)
    sk_square, sk_phase = [], []
    for d, t in zip(table, DGRAD_B64):
        got = []
        for s in d.shapes:
            p = E.plan_fp32(s, MI355X_CUS)
            M, K = E.gemm_dims(s)
            kh, kw = E.filter_hw(s)
            assert K == kh * kw * s.Cin and p["nk"] == (K + 15) // 16 and p["ksplit"] == 1 and p["mode"] == "fast", (s.name, p)
            got.append((kh, kw, M, p["nk"], p["form"]))
            if p["streamk"]:
                (sk_phase if d.kind == "phase" else sk_square).append(s.name)
                assert E.workspace_footprint(s, p)[0] == "slots"
            else:
                assert E.workspace_footprint(s, p) == ("none",)
        assert got == t[2], (d.unit.name, got)
    assert len(sk_square) == 7 and sk_phase == ["l3.0.c2.dx.p11", "l4.0.c2.dx.p01", "l4.0.c2.dx.p10", "l4.0.c2.dx.p11"]
    assert any(E.filter_hw(s)[0] != E.filter_hw(s)[1] and E.plan_fp32(s, MI355X_CUS)["streamk"] for d in table for s in d.shapes)
    # the zero-insertion route of the three stride-2 3 x 3 units (the GPU test runs it beside the phases)
    for d in table:
        if d.kind == "phase":
            z = TS.zero_insertion_shape(d.unit)
            assert E.out_hw(z) == (d.unit.H, d.unit.W) and E.gemm_dims(z) == (64 * d.unit.H * d.unit.W, 9 * d.unit.Cout)


def test_integer_draws_stay_exact():
    """M * max|x| * max|dy| < 2^24 for every weight-gradient geometry (no partial sum of any order leaves the exact range), the
    ranges are as wide as that allows, asymmetric in dy; on three layers float64 and float32 conv2d_weight agree in every element
    of the draw.  Input gradients: K * 8 * 7 + 9 < 2^24."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for u in TS.wgrad_table(64):
        xr, dr = TS.wgrad_ranges(u)
        assert TS.wgrad_integer_bound(u) < 2 ** 24 and dr[0] == -(dr[1] - 2) and xr[0] == -xr[1], u.name
        assert (xr, dr) == (((-4, 4), (-3, 5)) if u.name == "stem" else ((-8, 8), (-7, 9))), (u.name, xr, dr)
    assert TS.wgrad_integer_bound(TS.wgrad_table(64)[0]) == 802816 * 20 == 16056320
    for d in TS.dgrad_table(64):
        assert TS.dgrad_integer_bound(d.unit) < 2 ** 18
    for name in ("stem", "l3.0.ds", "l4.0.c3"):
        u = next(t for t in TS.wgrad_table(64) if t.name == name)
        x, dy = TS.draw_wgrad_integers(u)
        xr, dr = TS.wgrad_ranges(u)
        assert (float(x.min()), float(x.max()), float(dy.min()), float(dy.max())) == (*xr, *dr)
        assert all(bool((x[..., c] != 0).any()) for c in range(u.Cin))
        r64, r32 = TS.wgrad_reference(u, x, dy), TS.wgrad_reference(u, x, dy, torch.float32)
        top = float(r64.abs().max())
        print(f"[draw] wgrad {name}: max|dW|={top:.0f}, bound {TS.wgrad_integer_bound(u)}")
        assert r64.dtype == torch.float64 and bool((r64 == r64.round()).all()) and 256 <= top <= TS.wgrad_integer_bound(u)
        assert int((r32.double() != r64).sum()) == 0, name
    d = next(t for t in TS.dgrad_table(64) if t.unit.name == "l4.0.c2")
    dy, w, r = TS.draw_dgrad(d, "int")
    r64 = TS.dgrad_reference(d.unit, dy, w, r)
    assert bool((r64 == r64.round()).all()) and 64 <= float(r64.abs().max()) <= TS.dgrad_integer_bound(d.unit)
    assert int((TS.dgrad_reference(d.unit, dy, w, r, torch.float32).double() != r64).sum()) == 0


def test_the_reciprocal_pixel_division_is_exact_below_2_23():
    """conv_wgrad_kernel decodes a pixel index with ``q = (int)((float)v * rd)`` and a +-1 correction, rd = 1.0f / d.  Restated in
    numpy float32 and checked for EVERY v in [0, 2^23) and every divisor a batch-64 step produces (Ho * Wo and Wo of every layer),
    with rd one ulp above and below the correctly rounded reciprocal as well: the guarantee does not hang on how the device rounds the
    division.  What the correction is for: with the correctly rounded reciprocal (what the build's IEEE division gives) the raw quotient
    is already right for every v and every one of these divisors; with a reciprocal one ulp low (an approximate reciprocal instruction)
    it is one short for some v, and the correction repairs exactly that.  So no device test at any admissible size can tell whether the
    correction is there -- this test is what guards it."""
    divisors = TS.sdiv_divisors(64)
    assert divisors == [7, 14, 28, 49, 56, 112, 196, 784, 3136, 12544]
    v = np.arange(1 << 23, dtype=np.int32)
    uncorrected_wrong = [0, 0, 0]                                       # per reciprocal: correctly rounded, one ulp low, one ulp high
    for d in divisors:
        want = v // np.int32(d)
        rd = np.float32(1.0) / np.float32(d)
        for i, r in enumerate((rd, np.nextafter(rd, np.float32(0)), np.nextafter(rd, np.float32(1)))):
            assert r.dtype == np.float32
            bad = int((TS.sdiv_f32(v, d, r) != want).sum())
            assert bad == 0, (d, float(r), bad)
            raw = TS.sdiv_f32(v, d, r, correct=False)
            assert int(np.abs(raw - want).max()) <= 1, d
            uncorrected_wrong[i] += int((raw != want).sum())
    print(f"[sdiv] {len(divisors)} divisors x 3 reciprocals x 2^23 values: 0 mismatches; quotients that need the correction with the "
          f"reciprocal correctly rounded / one ulp low / one ulp high: {uncorrected_wrong}")
    assert uncorrected_wrong[0] == 0 and uncorrected_wrong[1] > 0

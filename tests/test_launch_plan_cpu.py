"""The launch selection of the convolution and BatchNorm launchers (ihmr_amd/csrc/launch_plan.h: plan_conv_fp32, plan_conv_bf16,
plan_conv_wgrad, plan_bn_chunks -- the very functions ihmr_hip.hip dispatches on) compiled for the HOST by g++ with
-fsanitize=address,undefined and compared field for field with the Python restatements the GPU tests predict kernel forms and
workspace fingerprints from (tests/encoder_shapes.py, tests/encoder_train_shapes.py, tests/test_gpu_encoder_train.py).  The
restatements stay the independent oracle; this file is what ties them to the C++ at every batch size, CU count and workspace size,
not only at the shapes and the one device the GPU tests run on.  A threshold edited on either side fails here, without a GPU."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_shapes as E  # noqa: E402
import encoder_train_shapes as T  # noqa: E402
import hostbuild  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

BATCHES = (1, 7, 64, 128, 512)
CUS = (3, 120, 256, 304)
MiB = 1 << 20
WORKSPACES = (0, 32 * MiB, 128 * MiB)
MODES = {"generic": 0, "fast": 1, "c4": 2}
TILES = [(128, 128), (64, 128), (128, 64), (64, 64)]
NO_TUNING = (-2, 0, 0, 0, 0)
SWEEP = 3000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    exe = hostbuild.build("launch_plan_driver.cpp", d, hostbuild.X86_V3)

    def run(op, records):
        records = np.ascontiguousarray(records, np.int64)
        assert records.ndim == 2 and len(records)
        fin, fout = str(d / f"{op}.in"), str(d / f"{op}.out")
        with open(fin, "wb") as fh:
            fh.write(np.int64(records.shape[0]).tobytes())
            fh.write(records.tobytes())
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, np.int64).reshape(records.shape[0], -1)
    return run


def _cdiv(a, b):
    return -(-a // b)


def _geometry(s):
    Ho, Wo = E.out_hw(s)
    kh, kw = E.filter_hw(s)
    return [s.N, s.Cin, Ho, Wo, s.Cout, kh, kw]


# ---------------------------------------------------------------------------------------------------------------- records and expectations
def fp32_record(s, cus, ws, y16=True, tuning=NO_TUNING):
    return _geometry(s) + [s.ldx, E.packed_ldw(s.Cout), s.ldy, cus, ws, int(y16)] + list(tuning)


def fp32_fields(s, p):
    """A plan_fp32 dict as the ConvPlan fields (ok, bm, bn, mode, threads, grid x y z, ksplit, reduce, streamk, sk_workers, sk_tiles,
    tiles_m, nk).  threads: one wave per 64 x 32 sub-tile; the grid: one workgroup per tile and K piece, or the Stream-K workers."""
    M, _ = E.gemm_dims(s)
    bm, bn = p["tile"]
    if p["streamk"]:
        assert (bm, bn, p["ksplit"], p["reduce"]) == (128, 128, 1, None)
        grid, sk = (p["workers"], 1, 1), (1, p["workers"], p["tiles"], _cdiv(M, 128))
    else:
        grid, sk = (_cdiv(M, bm), _cdiv(s.Cout, bn), p["ksplit"]), (0, 0, 0, 0)
        assert grid[0] * grid[1] == p["tiles"]
    return (1, bm, bn, MODES[p["mode"]], (bm // 64) * (bn // 32) * 64) + grid + (p["ksplit"], p["reduce"] or 0) + sk + (p["nk"],)


def bf16_record(s, cus, ws):
    return _geometry(s) + [s.ldx, E.packed_ldw(s.Cout), s.ldy, s.ldr, min(s.act, 1), cus, ws, 1, 1, 1, int(s.residual), 1]


def bf16_fields(s, p):
    """(ok, bn, mode, grid x y z, ksplit, vec, nk); vec (not part of plan_bf16) by hand: four-channel epilogue stores need Cout and the
    row strides of y and of the residual to be multiples of 4 (every pointer of these records is aligned)."""
    M, _ = E.gemm_dims(s)
    bn = p["tile"][1]
    assert p["tile"][0] == 128 and _cdiv(M, 128) * _cdiv(s.Cout, bn) == p["tiles"]
    vec = int(s.Cout % 4 == 0 and s.ldy % 4 == 0 and (not s.residual or s.ldr % 4 == 0))
    return (1, bn, MODES[p["mode"]], _cdiv(M, 128), _cdiv(s.Cout, bn), p["ksplit"], p["ksplit"], vec, p["nk"])


def wgrad_record(u, ws):
    return _geometry(u) + [u.ldx, u.Cout, E.packed_ldw(u.Cout), ws]


def wgrad_fields(u, p):
    """(ok, bm, bn, threads, grid x y z, msplit, chunks_per, reduce)."""
    _, K = E.gemm_dims(u)
    bm, bn = p["tile"]
    assert _cdiv(K, bm) * _cdiv(u.Cout, bn) == p["tiles"]
    reduce = {"wgrad_reduce": 0, "splitk_reduce4": 4, "splitk_reduce1": 1}[p["reduce"]]
    return (1, bm, bn, (bm // 64) * (bn // 32) * 64, _cdiv(K, bm), _cdiv(u.Cout, bn), p["msplit"], p["msplit"], p["chunks_per"], reduce)


def _compare(got, cases, want):
    """got: the driver's rows; want[i]: the expected fields, or None for a refusal (then only ok = 0 is compared)."""
    bad = []
    for row, case, w in zip(got.tolist(), cases, want):
        if (row[0] != 0) if w is None else (tuple(row) != tuple(w)):
            bad.append((case, row, w))
    assert not bad, (len(bad), len(cases), bad[:5])


def _small_cases(test_name):
    import test_gpu_encoder as G
    return [E.Shape("small", c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["s"], c["p"], c["Cin"], c["Cout"], c["Cout"], bool(c.get("res")), 1, ())
            for c in getattr(G, test_name).pytestmark[0].args[1]]


def _random_shapes(seed, n):
    """N 1-96, maps 1-64, Cin from {3, 4} and the multiples of 16 up to 2064, Cout 1-2048, k in {1, 3, 7} with 'same' padding, stride
    1-2; strides as networks.py packs them (ldx = Cin, ldy = ldr = Cout).  Every drawn shape is a case: none is filtered out."""
    rng = np.random.default_rng(seed)
    cins = [3, 4] + list(range(16, 2065, 16))
    out = []
    for i in range(n):
        k = int(rng.choice([1, 3, 7]))
        cin = int(rng.choice([3, 4])) if rng.random() < 0.15 else int(rng.choice(cins))
        # Cout: uniform, with the tile and vector-width boundaries over-represented
        cout = int(rng.integers(1, 2049)) if rng.random() < 0.6 else int(rng.choice([1, 2, 4, 40, 63, 64, 65, 122, 128, 192, 256, 320, 512, 1024, 2048]))
        res = bool(rng.integers(0, 2))
        out.append(E.Shape(f"rnd{i}", int(rng.integers(1, 97)), int(rng.integers(1, 65)), int(rng.integers(1, 65)), cin, cout, k,
                           int(rng.integers(1, 3)), k // 2, cin, cout, cout if res else 0, res, 1, ()))
    return out


def _boundary_shapes():
    """1 x 1 layers placed ON the thresholds of the selections, one step below and one above: 128-pixel images, so N images are N row
    tiles (the 64 / 384 / 768-896 tile counts, with one, two and a narrow column of tiles); 63, 64, 65 K steps of 16 (31-33 of 32);
    single-image-row layers of 63, 64, 65 pixels; for the bf16 split the tile counts around two per CU and 7, 8, 9 K steps of 32."""
    lin = lambda name, N, H, W, cin, cout: E.Shape(name, N, H, W, cin, cout, 1, 1, 0, cin, cout, cout, True, 1, ())
    out = []
    for T in (63, 64, 65, 383, 384, 385, 767, 768, 769, 770, 894, 895, 896, 897):
        for cin in (1008, 1024, 1040, 2048, 2064):
            out += [lin(f"edge.t{T}.c{cin}", T, 8, 16, cin, cout) for cout in (64, 128)]
            if T % 2 == 0:
                out.append(lin(f"edge.t{T}.c{cin}.o256", T // 2, 8, 16, cin, 256))
    for M in (63, 64, 65):
        out += [lin(f"edge.m{M}.c{cin}.o{cout}", 1, 1, M, cin, cout) for cin in (16, 64, 240, 256, 272, 2048, 2064) for cout in (64, 65, 122, 128)]
    for cus in CUS:
        for T in (2 * cus - 1, 2 * cus, 2 * cus + 1):
            out += [lin(f"edge.bf16.t{T}.c{cin}", T, 8, 16, cin, 128) for cin in (224, 256, 288, 512, 1024)]
    return out


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_plan_conv_fp32_equals_plan_fp32(driver):
    shapes = [s for B in BATCHES for s in E.trunk_table(B) + E.head_table(B)]
    for d in T.dgrad_table(64):
        shapes += list(d.shapes)
        if d.kind == "phase":
            shapes.append(T.zero_insertion_shape(d.unit))
    from test_gpu_encoder_shapes import EXTRA_SHAPES
    shapes += _small_cases("test_conv_igemm_matches_torch") + _small_cases("test_conv_streamk_matches_torch") + list(EXTRA_SHAPES)
    # the forms a single image row of odd layers takes, which no network launch and few swept shapes reach: the 4-channel and the
    # generic gather on the 64-row tiles
    shapes += [E.Shape("row.c4", 1, 8, 8, 4, 40, 5, 1, 2, 4, 40, 0, False, 1, ()), E.Shape("row.c3", 1, 8, 8, 3, 40, 5, 1, 2, 3, 40, 0, False, 1, ()),
               E.Shape("row.c48", 2, 5, 5, 48, 192, 3, 1, 1, 48, 192, 0, False, 1, ())]
    shapes += _boundary_shapes()
    cases = [(s, cus, ws, True) for s in shapes for cus in CUS for ws in WORKSPACES]
    rng = np.random.default_rng(11)
    cases += [(s, int(rng.choice(CUS + (8, 64, 80, 228))), int(rng.choice(WORKSPACES + (MiB, 64 * MiB))), bool(rng.random() < 0.9))
              for s in _random_shapes(1, SWEEP)]
    got = driver("fp32", [fp32_record(*c) for c in cases])
    _compare(got, cases, [fp32_fields(s, E.plan_fp32(s, cus, ws, y16)) for s, cus, ws, y16 in cases])
    # the sweep is not idle: every mode, tile, reduce width and Stream-K itself occur in it
    assert {tuple(r[1:4]) for r in got.tolist()} >= {(bm, bn, m) for bm, bn in TILES for m in (0, 1)} | {(128, 64, 2), (64, 64, 2)}
    assert set(got[:, 9].tolist()) == {0, 1, 4} and set(got[:, 10].tolist()) == {0, 1} and len(cases) >= 2000 + len(shapes) * 12


def test_plan_conv_fp32_refuses_what_the_launcher_refused(driver):
    s = E.trunk_table(64)[6]
    rec = lambda **kw: [kw.get(k, v) for k, v in zip("N Cin Ho Wo Cout kh kw ldx ldw ldy cus ws y16 ft fk skt sknk skw".split(),
                                                     fp32_record(s, 256, 128 * MiB))]
    got = driver("fp32", [rec(), rec(N=0), rec(Cout=0), rec(Cout=64, ldw=96), rec(Cout=128, ldw=192), rec(Cout=128, ldw=64), rec(ft=-1, skw=12),
                          rec(ft=-1, skw=0, skt=768, sknk=64, fk=1)])
    # (Cout = 128 on a 192-wide weight: not wide, but 192 = 3 x 64: the 64-column tile; on a 64-wide one likewise -- the launcher
    # never compared ldw with Cout)
    assert got[:, 0].tolist() == [1, 0, 0, 0, 1, 1, 0, 1] and got[4, 2] == 64 and got[0].tolist() == got[7].tolist()


def _forced_by_hand(s, cus, ws, ft, fk):
    """plan_fp32 with IHMR_CONV_FORCE = "<ft> <fk>" applied by hand (ft != 0: a forced 128 x 128 tile could still go to Stream-K): a tile
    the weight stride cannot carry is ignored; otherwise that tile, never Stream-K, the split capped by the workspace and by 4 K steps
    per piece.  The gather mode does not depend on the tile."""
    p = E.plan_fp32(s, cus, ws)
    M, _ = E.gemm_dims(s)
    bm, bn = TILES[ft]
    if bn == 128 and not s.Cout > 64:
        return p
    cap = ws // (M * s.Cout * 4) if ws else 1
    ksplit = max(1, min(fk, cap, max(1, p["nk"] // 4)))
    return dict(p, tile=(bm, bn), ksplit=ksplit, streamk=False, workers=0, tiles=_cdiv(M, bm) * _cdiv(s.Cout, bn),
                reduce=None if ksplit == 1 else 4 if s.Cout % 4 == 0 else 1)


def test_conv_tuning_overrides_are_plan_fp32_with_the_values_applied_by_hand(driver):
    from test_gpu_encoder_shapes import EXTRA_SHAPES
    shapes = E.trunk_table(64) + E.head_table(64) + list(EXTRA_SHAPES) + _small_cases("test_conv_igemm_matches_torch")
    ws = 128 * MiB
    settings = [
        # Stream-K switched off (no tile count passes "at most 0"): the plan of an unaligned y, which is refused Stream-K and nothing else
        ((-1, 1, 0, 64, 512), lambda s: E.plan_fp32(s, 256, ws, y_aligned16=False)),
        # 64 workers on a 256-CU device: the plan of a 32-CU device (the CU count enters plan_fp32 through the worker count alone)
        ((-1, 1, 768, 64, 64), lambda s: E.plan_fp32(s, 32, ws)),
        ((3, 1, 768, 64, 0), lambda s: _forced_by_hand(s, 256, ws, 3, 1)),
        ((1, 4, 768, 64, 0), lambda s: _forced_by_hand(s, 256, ws, 1, 4)),
        ((2, 64, 768, 64, 0), lambda s: _forced_by_hand(s, 256, ws, 2, 64)),
    ]
    for tuning, by_hand in settings:
        got = driver("fp32", [fp32_record(s, 256, ws, True, tuning) for s in shapes])
        _compare(got, [(s.name, tuning) for s in shapes], [fp32_fields(s, by_hand(s)) for s in shapes])
    # the defaults of the struct are the product values
    a = driver("fp32", [fp32_record(s, 256, ws) for s in shapes])
    b = driver("fp32", [fp32_record(s, 256, ws, True, (-1, 1, 768, 64, 0)) for s in shapes])
    c = driver("fp32", [fp32_record(s, 256, ws, True, (-1, 1, 768, 64, 512)) for s in shapes])
    assert (a == b).all() and (a == c).all()


def test_plan_conv_bf16_equals_plan_bf16(driver):
    cases = [(s, cus, ws) for s in [s for B in BATCHES for s in E.trunk_table(B)] + _boundary_shapes() for cus in CUS for ws in WORKSPACES]
    n_table = len(cases)
    rng = np.random.default_rng(12)
    cases += [(s, int(rng.choice(CUS + (8, 64, 80, 228))), int(rng.choice(WORKSPACES + (MiB, 64 * MiB)))) for s in _random_shapes(2, SWEEP)]
    got = driver("bf16", [bf16_record(*c) for c in cases])
    _compare(got, cases, [bf16_fields(s, E.plan_bf16(s, cus, ws)) for s, cus, ws in cases])
    assert set(got[:, 2].tolist()) == {0, 1, 2} and set(got[:, 1].tolist()) == {64, 128} and set(got[:, 7].tolist()) == {0, 1}
    assert set(got[:, 6].tolist()) == set(range(1, 9)) and len(cases) >= 2000 + n_table


def test_plan_conv_bf16_alignment_flags_and_refusals(driver):
    s = E.trunk_table(64)[6]                                                   # l2.0.c2: fast gather, vector epilogue
    names = "N Cin Ho Wo Cout kh kw ldx ldw ldy ldr act cus ws x16 x8 y8 has_r r8".split()
    rec = lambda **kw: [kw.get(k, v) for k, v in zip(names, bf16_record(s, 256, 128 * MiB))]
    got = driver("bf16", [rec(), rec(x16=0), rec(y8=0), rec(has_r=1, ldr=128, r8=0), rec(has_r=1, ldr=130), rec(has_r=1, ldr=128),
                          rec(Cin=4, ldx=4, x16=0), rec(Cin=4, ldx=4, x16=0, x8=0),
                          rec(act=2), rec(Cin=0), rec(ldw=96), rec(Cout=192, ldw=128), rec(Cout=192, ldw=192), rec(N=0)])
    assert got[:, 0].tolist() == [1] * 8 + [0] * 4 + [1, 0]
    assert got[:8, 2].tolist() == [1, 0, 1, 1, 1, 1, 2, 0]                      # mode: fast needs x on 16 bytes, the 4-channel form on 8
    assert got[:8, 7].tolist() == [1, 1, 0, 0, 0, 1, 1, 1]                      # vec: y and the residual on 8 bytes, ldr % 4
    assert got[12, 1] == 64                                                    # 192 columns on a 192-wide weight: three 64-column tiles


def test_plan_conv_wgrad_equals_plan_wgrad(driver):
    cases = [(u, ws) for B in BATCHES for u in T.wgrad_table(B) for ws in (T.WGRAD_WORKSPACE_BYTES, 8 * MiB)]
    n_table = len(cases)
    # what the launcher refuses: 2^23 pixels, Cin % 4, a workspace below one copy of dw
    big = E.Shape("pixels", 512, 128, 128, 64, 64, 1, 1, 0, 64, 64, 0, False, 1, ())
    refused = [(big, T.WGRAD_WORKSPACE_BYTES), (big._replace(Cin=6, ldx=6, N=1), T.WGRAD_WORKSPACE_BYTES), (big._replace(N=1), 64 * 64 * 4 - 1)]
    assert E.gemm_dims(big)[0] == T.WGRAD_MAX_PIXELS and all(T.plan_wgrad(u, ws) is None for u, ws in refused)
    assert T.plan_wgrad(big._replace(N=511), T.WGRAD_WORKSPACE_BYTES) is not None and T.plan_wgrad(big._replace(N=1), 64 * 64 * 4) is not None
    cases += refused + [(big._replace(N=511), T.WGRAD_WORKSPACE_BYTES), (big._replace(N=1), 64 * 64 * 4)]
    # on the thresholds: 8 chunks of 16 pixels per range, the 256-range cap, 32 ranges (the reduce kernel), 1024 tiles x ranges
    for M in (127, 128, 129, 16 * 8 * 31, 16 * 8 * 32, 16 * 8 * 32 + 1, 16 * 8 * 33, 16 * 8 * 256, 16 * 8 * 257):
        for cin, cout in ((64, 64), (64, 256), (256, 512), (512, 2048), (16, 64)):
            cases += [(E.Shape(f"edge.m{M}", 1, 1, M, cin, cout, 1, 1, 0, cin, cout, 0, False, 1, ()), ws) for ws in (T.WGRAD_WORKSPACE_BYTES, 8 * MiB)]
    rng = np.random.default_rng(13)
    cases += [(u, int(rng.choice([T.WGRAD_WORKSPACE_BYTES, 64 * MiB, 8 * MiB, MiB]))) for u in _random_shapes(3, SWEEP)]
    want = [T.plan_wgrad(u, ws) for u, ws in cases]
    got = driver("wgrad", [wgrad_record(*c) for c in cases])
    _compare(got, cases, [None if p is None else wgrad_fields(u, p) for (u, _), p in zip(cases, want)])
    ok = got[got[:, 0] == 1]
    assert {tuple(r) for r in ok[:, 1:3].tolist()} == set(TILES) and set(ok[:, 9].tolist()) == {0, 4}
    refusals = sum(p is None for p in want)                                    # (Cin = 3, Cout % 4 and the small workspaces)
    assert refusals > 500 and len(cases) - refusals > 500 and len(cases) >= 2000 + n_table
    # lddy and ldw, which plan_wgrad takes from the shape: dy rows must be a multiple of 4 floats, dw rows at least Cout wide
    u = T.wgrad_table(64)[3]
    rec = wgrad_record(u, T.WGRAD_WORKSPACE_BYTES)
    got = driver("wgrad", [rec, rec[:8] + [u.Cout + 2] + rec[9:], rec[:9] + [u.Cout - 1] + rec[10:]])
    assert got[:, 0].tolist() == [1, 0, 0]


def test_plan_bn_chunks_equals_bn_rows_per_chunk(driver):
    from test_gpu_encoder_train import _bn_rows_per_chunk
    Ms = sorted({E.gemm_dims(s)[0] for B in BATCHES for s in E.trunk_layers(B)} | {1, 15, 16, 17, 16383, 16384, 16385, 16 * 1024 + 1024})
    Ms += np.random.default_rng(14).integers(1, 1 << 24, SWEEP).tolist()
    got = driver("bn", [[M] for M in Ms])
    for M, (rows_per, chunks) in zip(Ms, got.tolist()):
        assert rows_per == _bn_rows_per_chunk(M) and chunks == _cdiv(M, rows_per) and 1 <= chunks <= 1024, (M, rows_per, chunks)
    with open(os.path.join(hostbuild.ROOT, "ihmr_amd", "csrc", "launch_plan.h")) as fh:
        assert "#define BN_MAX_CHUNKS 1024\n" in fh.read()                      # the 1024 of ihmr_bn_workspace_bytes

"""The arithmetic of the training-time augmentation without a GPU: ``ihmr_amd/csrc/augment_pure.h`` -- the functions the kernels of
``csrc/augment.h`` inline -- compiled for the HOST by g++ with -fsanitize=address,undefined and compared byte for byte with
``tests/augment_ref.py``; ``augment_ref`` itself against the installed Pillow; the distributions of ``TrainDataProcessor.draw``; the
ABI of the new entry points."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
import hostbuild  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "augment.npz")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("augment")
    exe = hostbuild.build("augment_host_driver.cpp", d, hostbuild.X86_V3)

    def run(op, payload=None, dtype=np.uint8):
        fout = str(d / f"{op}.out")
        args = [op]
        if payload is not None:
            fin = str(d / f"{op}.in")
            with open(fin, "wb") as fh:
                fh.write(payload)
            args.append(fin)
        hostbuild.run(exe, *args, fout)
        return np.fromfile(fout, dtype)
    return run


@pytest.fixture(scope="module")
def all_triples():
    v = np.arange(256, dtype=np.uint8)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(4096, 4096, 3)


def _chunked(fn, arr, step=256):
    return np.concatenate([fn(arr[i:i + step]) for i in range(0, arr.shape[0], step)])


@pytest.fixture(scope="module")
def ref_tables(all_triples):
    return _chunked(A.rgb2hsv, all_triples), _chunked(A.hsv2rgb, all_triples)


@needs_gxx
def test_hsv_conversions_over_all_triples(driver, ref_tables):
    """RGB -> HSV and HSV -> RGB of augment_pure.h over all 2^24 triples equal augment_ref in every byte."""
    fwd = driver("rgb2hsv").reshape(4096, 4096, 3)
    assert np.array_equal(fwd, ref_tables[0])
    back = driver("hsv2rgb").reshape(4096, 4096, 3)
    assert np.array_equal(back, ref_tables[1])


@needs_gxx
def test_blend_over_all_pairs(driver):
    """Image.blend's arithmetic over all (value, degenerate) pairs at eight factors on both sides of 1 (truncating and clipping branch)."""
    factors = np.array([0.0, 0.4, 0.8, 0.9, 1.0, 1.0000001, 1.3, 1.6], np.float32)
    got = driver("blend", np.int32(len(factors)).tobytes() + factors.tobytes()).reshape(len(factors), 256, 256)
    a, d = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for i, f in enumerate(factors):
        assert np.array_equal(got[i], A.blend(a, d, f).astype(np.uint8)), f
    # brightness / contrast / saturation are this blend against 0 / a constant / the grey value: spot-check the grey value
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    assert np.array_equal(A.saturation(img, 1.3), A.blend(img, np.repeat(A.gray(img)[..., None], 3, -1), 1.3).astype(np.uint8))


@needs_gxx
@pytest.mark.parametrize("S", [8, 64, 224])
def test_warp_coordinates_and_weights(driver, S):
    """The fixed-point source coordinate and the four weights of every destination pixel for the ten angles; weights sum to 32768."""
    for k in range(10):
        m = A.warp_matrix(18 * k - 90, S)
        got = driver("warp", np.int32(S).tobytes() + m.tobytes(), np.int32).reshape(S, S, 8)
        sx, sy, fx, fy = A.warp_coords(m, S)
        assert np.array_equal(got[..., 0], sx) and np.array_equal(got[..., 1], sy), k
        assert np.array_equal(got[..., 2], fx) and np.array_equal(got[..., 3], fy), k
        assert np.array_equal(got[..., 4:], A.warp_weights(fx, fy)), k
        assert (got[..., 4:].sum(-1) == 32768).all()


@needs_gxx
def test_reflect_and_orientation(driver):
    """BORDER_REFLECT_101 indices for every length up to 40, and rotate_orient's float32 formulas against their float64 restatement."""
    got = driver("reflect", None, np.int32).reshape(40, 120)
    for n in range(1, 41):
        assert np.array_equal(got[n - 1], A.reflect101(np.arange(-40, 80), n)), n
    rng = np.random.RandomState(3)
    rec = []
    while len(rec) < 400:
        o, ang = rng.normal(0, 0.9, 3), 18 * rng.randint(0, 10) - 90
        if 0.3 <= np.linalg.norm(o) <= 2.8 and 0.3 <= A.composed_rotation_angle(o.astype(np.float32), ang) <= 2.8:
            rec.append(list(o) + [float(A.rot_z_f32(ang))])
    rec = np.array(rec, np.float32)
    got = driver("orient", np.int32(len(rec)).tobytes() + rec.tobytes(), np.float32).reshape(-1, 3)
    want = np.stack([A._rotmat_to_aa64(A._aa_to_rotmat64(np.array([0, 0, float(r[3])])) @ A._aa_to_rotmat64(r[:3].astype(np.float64))) for r in rec])
    # float32 formulas of ~40 operations on values <= pi, away from the branch points: 1e-5 is ~40 ulp at pi
    assert np.abs(got - want).max() < 1e-5, np.abs(got - want).max()


def test_augment_ref_equals_pillow_on_the_hsv_tables(all_triples, ref_tables):
    pytest.importorskip("PIL")
    from PIL import Image
    assert np.array_equal(np.asarray(Image.fromarray(all_triples).convert("HSV")), ref_tables[0])
    assert np.array_equal(np.asarray(Image.fromarray(all_triples, "HSV").convert("RGB")), ref_tables[1])


def test_augment_ref_equals_pillow_on_the_golden_colour_cases():
    pytest.importorskip("PIL")
    g = np.load(GOLDEN)
    n_colour = 0
    for i in range(int(g["n"])):
        d = g[f"draw{i}"]
        if not d[8]:
            continue
        n_colour += 1
        before = next(g[f"u8_{s}{i}"] for s in ("rotate", "rescale", "flip") if f"u8_{s}{i}" in g)
        order, (b, c, s, h) = g[f"order{i}"], d[9:13]
        pil = A.pil_color_jitter(before, order, b, c, s, h)
        assert np.array_equal(pil, g[f"u8_color{i}"])                         # the golden was made with Pillow
        assert np.array_equal(A.color_jitter(before, order, b, c, s, A.hue_shift_byte(h)), pil), i
    assert n_colour >= 6
    rng = np.random.RandomState(5)                                            # every operation alone, both blend branches
    for it in range(40):
        img = rng.randint(0, 256, (24, 24, 3)).astype(np.uint8)
        b, c, s, h = rng.uniform(0.9, 1.3), rng.uniform(0.8, 1.3), rng.uniform(0.4, 1.6), rng.uniform(-0.1, 0.1)
        for op in range(4):
            assert np.array_equal(A.color_jitter(img, [op], b, c, s, A.hue_shift_byte(h)), A.pil_color_jitter(img, [op], b, c, s, h)), (it, op)


def test_draw_distributions():
    """``TrainDataProcessor.draw`` over 20 000 samples: the reference's ranges, angles, orders, position bounds and flip rules."""
    import types
    from ihmr_amd import augment as G
    opt = types.SimpleNamespace(use_random_flip=True, use_random_rescale=True, use_random_position=True, use_random_rotation=True,
                                use_color_jittering=True, use_motion_blur=True, motion_blur_prob=0.3, inputSize=224)
    bank = G.line_blur_kernels()
    N, S = 20000, 224
    types_ = np.array([[1, 1], [1, 0], [0, 1]], np.float32)[np.random.RandomState(0).randint(0, 3, N)]
    p = G.TrainDataProcessor(opt, bank, seed=7).draw(types_)
    assert p.dtype == G.PARAMS_DTYPE and p.shape == (N,)
    inter, left, right = types_.sum(1) > 1.5, (types_[:, 0] < 0.5), (types_[:, 1] < 0.5)
    assert (p["flip"][left] == 1).all() and (p["flip"][right] == 0).all()
    assert 0.45 < p["flip"][inter].mean() < 0.55
    assert (p["flags"] == (G.RESCALE | G.ROTATE | G.COLOR)).all()
    assert (p["scale"] >= 0.6).all() and (p["scale"] < 1.0).all() and p["scale"].min() < 0.61 and p["scale"].max() > 0.99
    assert np.array_equal(p["new_size"], (S * p["scale"].astype(np.float64)).astype(np.int64)) or \
        (np.abs(p["new_size"] - S * p["scale"].astype(np.float64)) <= 1).all()
    end = S - p["new_size"] - 1
    for k in ("x_pos", "y_pos"):
        assert (p[k] >= 0).all() and (p[k] <= end).all() and (p[k] == end).any() and (p[k] == 0).any()
    assert sorted(set(p["angle"].tolist())) == [18.0 * k - 90 for k in range(10)]
    for i in (0, 1, N - 1):
        assert np.array_equal(p["warp"][i], A.warp_matrix(float(p["angle"][i]), S))
        assert p["rot_z"][i] == A.rot_z_f32(float(p["angle"][i]))
    for k, (lo, hi) in dict(brightness=(0.9, 1.3), contrast=(0.8, 1.3), saturation=(0.4, 1.6)).items():
        assert (p[k] >= np.float32(lo)).all() and (p[k] <= np.float32(hi)).all() and p[k].min() < lo + 0.01 and p[k].max() > hi - 0.01
    shifts = set(p["hue_shift"].tolist())
    assert shifts == set(range(0, 26)) | set(range(231, 256))                  # (uint8)(int)(U(-0.1, 0.1) * 255)
    assert len({tuple(o) for o in p["order"].tolist()}) == 24
    blurred = p["blur_kernel"] >= 0
    assert 0.27 < blurred.mean() < 0.33 and set(p["blur_kernel"][blurred].tolist()) == set(range(len(bank)))
    # the same seed gives the same table; an explicit generator too
    assert G.TrainDataProcessor(opt, bank, seed=7).draw(types_).tobytes() == p.tobytes()
    assert G.TrainDataProcessor(opt, bank, seed=8).draw(types_).tobytes() != p.tobytes()
    q = G.TrainDataProcessor(opt, bank).draw(types_[:50], np.random.default_rng(3))
    assert q.tobytes() == G.TrainDataProcessor(opt, bank).draw(types_[:50], np.random.default_rng(3)).tobytes()
    # every switch off: only left-only samples are touched
    off = G.TrainDataProcessor(types.SimpleNamespace(inputSize=64)).draw(types_[:100])
    assert (off["flags"] == 0).all() and (off["blur_kernel"] == -1).all() and np.array_equal(off["flip"] == 1, left[:100])
    with pytest.raises(ValueError):
        G.TrainDataProcessor(opt, [np.ones((34, 3), np.float32)])
    with pytest.raises(ValueError):
        G.TrainDataProcessor(opt, [np.ones((2, 40), np.float32)])
    assert len(G.TrainDataProcessor(opt, [np.ones((33, 33), np.float32), np.ones(5, np.float32)]).blur_kernels) == 2


def test_header_binding_and_library_agree_on_the_new_entry_points():
    """include/ihmr_hip.h declares the ihmr_augment_* functions, hip.EXPORTED_SYMBOLS lists them, the built library exports them, and
    the numpy record of the parameter table has the layout of the C struct."""
    from ihmr_amd import augment as G
    from ihmr_amd import hip
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    declared = set(re.findall(r"\b(ihmr_augment_[a-z0-9_]+)\s*\(", header))
    assert declared == {"ihmr_augment_images", "ihmr_augment_labels"}
    assert declared <= set(hip.EXPORTED_SYMBOLS)
    if shutil.which("hipcc") is not None:
        L = ctypes.CDLL(hip.build())
        for sym in declared:
            assert hasattr(L, sym), sym
    body = re.search(r"typedef struct ihmr_aug_params \{(.*?)\} ihmr_aug_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(ctype, re.sub(r"\[.*", "", n.strip())) for n in names.split(",")]
    assert [n for _, n in fields] == list(G.PARAMS_DTYPE.names)
    kinds = dict(double="f8", float="f4", int32_t="i4")
    assert all(G.PARAMS_DTYPE[n].base == np.dtype(kinds[t]) for t, n in fields)
    if shutil.which("g++") is not None:                                       # sizeof / offsetof as the compiler lays the struct out
        size, offsets = hostbuild.struct_layouts({"ihmr_aug_params": G.PARAMS_DTYPE.names})["ihmr_aug_params"]
        assert size == G.PARAMS_DTYPE.itemsize and offsets == {n: G.PARAMS_DTYPE.fields[n][1] for n in G.PARAMS_DTYPE.names}

"""The MANO layer's pose space and output stage without a GPU: include/ihmr_mano_ext.h against ``hip.SIGNATURES_EXT`` argument by
argument, ``assets.get_hand_components``, csrc/mano_pose_space_pure.h built for the host with ASan / UBSan (tests/mano_space_driver.cpp
walks the four kernels in their own order and is run as a program), the statement of tests/mano_space_ref.py checked on itself, and the
build: the four kernels without scratch memory or spills, the LDS the header names, every declared symbol exported.

The bounds are derived, not measured: a chain of K fused multiply-adds from 0 has |fl - exact| <= gamma_K sum_k |c_k C_ki|, gamma_n =
n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; the fused form rounds once per term, so
the bound of the unfused sum holds with room); the translation is one IEEE addition, equal to numpy's; d_transl is one rounding of a
float64 sum whose own error (799 additions of float32 terms, 799 x 2^-53 relative to the sum of magnitudes) is far below half a float32
ulp, hence within ONE float32 ulp of the correctly rounded exact sum."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj  # noqa: E402
import hostbuild  # noqa: E402
import mano_cases as MC  # noqa: E402
import mano_space_ref as SP  # noqa: E402

from ihmr_amd import assets, hip  # noqa: E402

NEW = ["ihmr_mano_pca_fwd", "ihmr_mano_pca_bwd", "ihmr_mano_post_fwd", "ihmr_mano_post_bwd"]
SCALARS = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_size_t: "size_t", ctypes.c_long: "long"}


# ------------------------------------------------------------------------------------------------------------------ fails without the feature
def test_create_takes_a_pca_pose_space_and_the_second_table_exists():
    from ihmr_amd import mano
    layer = mano.create("", "mano", use_pca=True)
    assert isinstance(layer, mano.MANO) and layer.use_pca and layer.num_pca_comps == 6 and not layer.flat_hand_mean
    assert tuple(layer.hand_components.shape) == (6, 45) and sorted(hip.SIGNATURES_EXT) == sorted(NEW)
    flat = mano.create("", "mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True, is_rhand=False)
    assert tuple(flat.hand_components.shape) == (45, 45) and not flat.hand_mean.any() and layer.hand_mean.any()
    assert np.array_equal(flat.hand_components.numpy(), assets.get_hand_components("", False))
    plain = mano.create("", "mano", use_pca=False, is_rhand=True, batch_size=3)
    assert plain.hand_components is None and not plain.use_pca and plain.batch_size == 3
    assert list(plain.state_dict()) == ["shapedirs", "J_regressor", "v_template", "hand_mean"] == list(layer.state_dict())
    assert mano.ManoOutput._fields == ("vertices", "joints", "betas", "global_orient", "hand_pose")
    assert mano.ManoOutputFullPose._fields == mano.ManoOutput._fields + ("full_pose",)
    for bad in (0, 46, -1, 2.5):
        with pytest.raises(ValueError):
            mano.create("", "mano", use_pca=True, num_pca_comps=bad)
    with pytest.raises(ValueError):
        mano.create("", "smplh")


# ------------------------------------------------------------------------------------------------------------------ the ABI
def _prototypes(header_name):
    """{name: (return class, [parameter classes])} of every ihmr_* function a public header declares, comments stripped: "int" |
    "float" | "size_t" | "long" | "ptr" (the rule of tests/test_abi_cpu.py; the second header has no struct)."""
    with open(os.path.join(ROOT, "include", header_name)) as fh:
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S))
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))

    def c_class(decl, is_parameter):
        if "*" in decl:
            return "ptr"
        tokens = [t for t in decl.split() if t != "const"]
        kind = tokens[:-1] if is_parameter and len(tokens) > 1 else tokens
        assert kind in (["int"], ["float"], ["size_t"], ["long"]), decl
        return kind[0]
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(ihmr_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in protos, name
        protos[name] = (c_class(ret, False), [c_class(p, True) for p in ([] if params.strip() in ("", "void") else params.split(","))])
    return protos


def _ctypes_class(t):
    return SCALARS[t] if t in SCALARS else "ptr"


def test_every_prototype_of_the_second_header_agrees_with_its_table():
    protos = _prototypes("ihmr_mano_ext.h")
    assert sorted(protos) == sorted(NEW) == sorted(hip.SIGNATURES_EXT)
    for name, (c_ret, c_args) in protos.items():
        restype, argtypes = hip.SIGNATURES_EXT[name]
        assert all(t in SCALARS or t is ctypes.c_void_p for t in [restype] + argtypes), name
        assert c_ret == _ctypes_class(restype) == "int", name
        assert c_args == [_ctypes_class(t) for t in argtypes], (name, c_args, argtypes)
    assert protos["ihmr_mano_pca_fwd"][1] == ["ptr", "ptr", "int", "int", "ptr", "ptr"]
    assert protos["ihmr_mano_post_fwd"][1] == ["ptr"] * 4 + ["int"] + ["ptr"] * 3
    assert protos["ihmr_mano_post_bwd"][1] == ["ptr"] * 3 + ["int"] + ["ptr"] * 4
    # the comparison sees a wrong table: an int bound as a pointer, a missing argument
    wrong = dict(hip.SIGNATURES_EXT, ihmr_mano_pca_fwd=(ctypes.c_int, [ctypes.c_void_p] * 6))
    assert protos["ihmr_mano_pca_fwd"][1] != [_ctypes_class(t) for t in wrong["ihmr_mano_pca_fwd"][1]]
    assert len(protos["ihmr_mano_post_bwd"][1]) == 8 != len(hip.SIGNATURES_EXT["ihmr_mano_pca_bwd"][1])


def test_the_tables_are_disjoint_and_the_first_header_is_as_it_was():
    assert not set(hip.SIGNATURES) & set(hip.SIGNATURES_EXT)
    assert hip.EXPORTED_SYMBOLS == list(hip.SIGNATURES) and len(hip.SIGNATURES) == 77
    with open(os.path.join(ROOT, "include", "ihmr_hip.h")) as fh:
        first = fh.read()
    assert not any(name in first for name in NEW) and "ihmr_mano_ext" not in first
    assert sorted(_prototypes("ihmr_hip.h")) == sorted(hip.SIGNATURES)
    with open(os.path.join(ROOT, "include", "ihmr_mano_ext.h")) as fh:
        assert int(re.search(r"#define IHMR_MANO_POSE_DIM (\d+)", fh.read()).group(1)) == hip.MANO_POSE_DIM == 45


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_the_library_exports_the_four_and_binds_both_tables():
    L = ctypes.CDLL(hip.build())
    for name in NEW + ["ihmr_mano_lbs_fwd"]:
        getattr(L, name)
    hip.bind(hip.bind(L), hip.SIGNATURES_EXT)
    assert L.ihmr_mano_pca_fwd.argtypes == hip.SIGNATURES_EXT["ihmr_mano_pca_fwd"][1]
    assert L.ihmr_mano_lbs_fwd.argtypes == hip.SIGNATURES["ihmr_mano_lbs_fwd"][1]
    # refusals need no GPU: nothing is launched
    assert L.ihmr_mano_pca_fwd(None, None, 1, 6, None, None) == -1 and L.ihmr_mano_pca_bwd(None, None, 1, 6, None, None) == -1
    assert L.ihmr_mano_post_fwd(None, None, None, None, 1, None, None, None) == -1
    assert L.ihmr_mano_post_bwd(None, None, None, 1, None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------------ the asset
PARENT_KEYS = ["v_template", "faces", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "parents", "hands_mean"]


def test_the_synthetic_basis_is_orthonormal_seeded_and_mirrored():
    right, left = assets.get_hand_components("", True), assets.get_hand_components(None, False)
    assert right.shape == left.shape == (45, 45) and right.dtype == left.dtype == np.float32
    for basis in (right, left):
        assert np.abs(basis.astype(np.float64) @ basis.astype(np.float64).T - np.eye(45)).max() <= 1e-6
    assert np.array_equal(right, assets.get_hand_components("", True, seed=0)) and np.array_equal(right, assets.synthetic_hand_components())
    assert not np.array_equal(right, assets.get_hand_components("", True, seed=1))
    # the mirror rule of hands_mean: the y and z components of every joint's rotation vector change sign
    sign = np.tile(np.array([1.0, -1.0, -1.0], np.float32), 15)
    assert np.array_equal(left, right * sign[None])
    mean_r, mean_l = assets.synthetic_mano(True)["hands_mean"], assets.synthetic_mano(False)["hands_mean"]
    assert np.array_equal(mean_l, mean_r * sign) and mean_r.any()
    assert np.array_equal(assets.get_hand_components("synthetic:fingers/MANO_RIGHT.pkl", True), right)


def test_the_asset_dict_keeps_its_keys_and_its_numbers(tmp_path):
    for is_rhand in (True, False):
        before = assets.get_mano_arrays("", is_rhand)
        assert list(before) == PARENT_KEYS
        assets.get_hand_components("", is_rhand)                                      # draws from a RandomState of its own
        after = assets.get_mano_arrays("", is_rhand)
        assert all(np.array_equal(before[k], after[k]) for k in PARENT_KEYS)
    # a real file: its own hands_components, whichever hand
    import pickle
    arr = assets.synthetic_mano(True)
    comps = np.arange(45 * 45, dtype=np.float64).reshape(45, 45) / 7.0
    data = dict(v_template=arr["v_template"], f=arr["faces"].astype(np.uint32), shapedirs=arr["shapedirs"],
                posedirs=arr["posedirs"].T.reshape(778, 3, 135), J_regressor=arr["J_regressor"], weights=arr["lbs_weights"],
                kintree_table=np.stack([np.where(arr["parents"] < 0, 2 ** 32 - 1, arr["parents"]).astype(np.int64), np.arange(16)]),
                hands_mean=arr["hands_mean"], hands_components=comps)
    path = tmp_path / "MANO_RIGHT.pkl"
    with open(path, "wb") as fh:
        pickle.dump(data, fh)
    assert np.array_equal(assets.get_hand_components(str(path), False), comps.astype(np.float32))
    assert list(assets.get_mano_arrays(str(path), True)) == PARENT_KEYS


# ------------------------------------------------------------------------------------------------------------------ the host driver
def _dyadic(shape, rng, lo=-8, hi=8, scale=0.125):
    """Multiples of 1/8 of small magnitude: every product and partial sum below is exact in float32."""
    return (rng.randint(lo, hi + 1, size=shape) * scale).astype(np.float32)


def _drive(exe, tmp_path, tag, N, K, J, transl, rng, dyadic=False):
    draw = (lambda s: _dyadic(s, rng)) if dyadic else (lambda s: rng.standard_normal(s).astype(np.float32))
    a = dict(coeffs=draw((N, K)), comps=draw((K, 45)) if dyadic else assets.get_hand_components("", True)[:K].copy(), d_pose45=draw((N, 45)),
             verts=draw((N, 778, 3)), joints16=draw((N, 16, 3)), transl=draw((N, 3)), tip_ids=np.asarray(assets.TIP_VERTEX_IDS, np.int32),
             d_verts_out=draw((N, 778, 3)), d_joints_out=draw((N, J, 3)))
    src, dst = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    with open(src, "wb") as fh:
        fh.write(np.array([N, K, J, int(transl)], np.int32).tobytes())
        for k in ("coeffs", "comps", "d_pose45", "verts", "joints16", "transl", "tip_ids", "d_verts_out", "d_joints_out"):
            fh.write(np.ascontiguousarray(a[k]).tobytes())
    hostbuild.run(exe, src, dst)
    flat = np.fromfile(dst, np.float32)
    shapes = [("pose45", (N, 45)), ("d_coeffs", (N, K)), ("verts_out", (N, 778, 3)), ("joints_out", (N, J, 3)), ("inplace", (N, 778, 3)),
              ("d_verts_in", (N, 778, 3)), ("d_joints16", (N, 16, 3)), ("d_transl", (N, 3))]
    assert flat.size == sum(int(np.prod(s)) for _, s in shapes)
    got, at = {}, 0
    for name, s in shapes:
        got[name] = flat[at:at + int(np.prod(s))].reshape(s)
        at += int(np.prod(s))
    return a, got


def _check_driver(a, got, K, J, transl, dyadic):
    exact, mag = SP.pca_exact(a["coeffs"], a["comps"])
    assert (np.abs(got["pose45"] - exact) <= SP.gamma(K) * mag).all()
    b_exact, b_mag = SP.pca_bwd_exact(a["d_pose45"], a["comps"])
    assert (np.abs(got["d_coeffs"] - b_exact) <= SP.gamma(45) * b_mag).all()
    if dyadic:
        assert np.array_equal(got["pose45"].astype(np.float64), exact) and np.array_equal(got["d_coeffs"].astype(np.float64), b_exact)
    t = a["transl"][:, None] if transl else None
    want_v = a["verts"] + t if transl else a["verts"]
    want_j = a["joints16"] + t if transl else a["joints16"]
    assert want_v.dtype == np.float32 and got["verts_out"].tobytes() == want_v.tobytes() == got["inplace"].tobytes()
    assert got["joints_out"][:, :16].tobytes() == np.ascontiguousarray(want_j).tobytes()
    tips = a["tip_ids"].astype(np.int64)
    want_dv = a["d_verts_out"].copy()
    if J == 21:
        assert got["joints_out"][:, 16:].tobytes() == np.ascontiguousarray(want_v[:, tips]).tobytes()
        want_dv[:, tips] += a["d_joints_out"][:, 16:]
    assert got["d_verts_in"].tobytes() == want_dv.tobytes() and got["d_joints16"].tobytes() == np.ascontiguousarray(a["d_joints_out"][:, :16]).tobytes()
    total = SP.transl_sum(a["d_verts_out"], a["d_joints_out"])
    assert (np.abs(got["d_transl"] - total) <= SP.one_ulp_of(total)).all()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    return hostbuild.build("mano_space_driver.cpp", tmp_path_factory.mktemp("mano_space"))


@pytest.mark.parametrize("K", [1, 6, 44, 45])
def test_the_host_driver_meets_the_derived_bounds(driver, tmp_path, K):
    rng = np.random.RandomState(100 + K)
    for J, transl, dyadic in ((21, True, False), (16, False, False), (21, True, True), (16, True, True)):
        a, got = _drive(driver, tmp_path, f"k{K}_{J}_{int(transl)}_{int(dyadic)}", 9, K, J, transl, rng, dyadic)
        _check_driver(a, got, K, J, transl, dyadic)


def test_the_host_driver_crosses_a_tile_and_refuses_bad_sizes(driver, tmp_path):
    a, got = _drive(driver, tmp_path, "n33", 33, 6, 21, True, np.random.RandomState(5))       # three tiles of 16, the last of one hand
    _check_driver(a, got, 6, 21, True, False)
    for head in ((0, 6, 16, 0), (1, 0, 16, 0), (1, 46, 16, 0), (1, 6, 17, 0)):
        src = tmp_path / "bad.in"
        src.write_bytes(np.array(head, np.int32).tobytes())
        hostbuild.run(driver, src, tmp_path / "bad.out", ok=False)


# ------------------------------------------------------------------------------------------------------------------ the statement on itself
def _orthonormal64(is_rhand=True):
    """The synthetic basis re-orthonormalised in float64 (its float32 rows are orthonormal to 1e-7 only)."""
    q, r = np.linalg.qr(assets.get_hand_components("", is_rhand).astype(np.float64).T)
    return (q * np.sign(np.diag(r))[None]).T


def test_the_statement_with_all_45_components_is_the_oracle_on_pose45(mano_arrays):
    import torch
    right = mano_arrays[0]
    C = _orthonormal64()
    assert np.abs(C @ C.T - np.eye(45)).max() < 1e-14 and np.abs(C - assets.get_hand_components("", True)).max() < 1e-6
    c = MC.case("mild", 3, 11, right["hands_mean"])
    plain = MC.reference(right, c, torch.float64)
    wide = dict(orient=c["orient"], hand_pose=c["pose"].astype(np.float64) @ C.T, betas=c["betas"], transl=None, gv=c["gv"], gj=c["gj"])
    got = SP.reference(right, wide, torch.float64, comps=C)
    for k in ("verts", "joints", "d_orient", "d_betas"):
        assert np.abs(got[k] - plain[k]).max() <= 1e-12 * max(1.0, np.abs(plain[k]).max()), k
    assert np.abs(got["d_hand_pose"] - plain["d_pose"] @ C.T).max() <= 1e-12 * np.abs(plain["d_pose"]).max()
    assert np.abs(got["full_pose"][:, 3:] - (c["pose"].astype(np.float64) + MC._f32(right["hands_mean"]))).max() <= 1e-12
    # flat_hand_mean: the mean is gone from the full pose, and the zero pose is the template's skeleton
    flat = SP.reference(right, dict(wide, hand_pose=np.zeros((3, 45))), torch.float64, comps=C, flat_hand_mean=True)
    assert not flat["full_pose"][:, 3:].any() and np.abs(flat["verts"] - plain["verts"]).max() > 1e-3
    # translation and tips: the statement's own definitions
    t = np.array([[0.5, -0.25, 1.0]] * 3)
    moved = SP.reference(right, dict(wide, transl=t, gj=np.concatenate([c["gj"], c["gj"][:, :5]], 1)), torch.float64, comps=C)
    assert np.abs(moved["verts"] - (plain["verts"] + t[:, None])).max() <= 1e-12
    assert np.array_equal(moved["joints"][:, 16:], moved["verts"][:, SP.tip_ids()]) and moved["joints"].shape == (3, 21, 3)
    assert SP.tip_ids().tolist() == [744, 320, 443, 554, 671]
    total = SP.transl_sum(c["gv"], np.concatenate([c["gj"], c["gj"][:, :5]], 1))
    assert np.abs(moved["d_transl"] - total).max() <= 1e-12 * np.abs(total).max()


def test_the_statements_gradients_are_central_differences(mano_arrays):
    right = mano_arrays[0]
    comps = assets.get_hand_components("", True)[:6]
    import torch
    c = SP.case("mild", 2, 6, 23, right["hands_mean"])
    c = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    grad = SP.reference(right, c, torch.float64, comps=comps)
    rng = np.random.RandomState(1)
    for key, name in (("orient", "d_orient"), ("hand_pose", "d_hand_pose"), ("betas", "d_betas"), ("transl", "d_transl")):
        for _ in range(2):
            d = rng.standard_normal(c[key].shape)
            eps = 1e-6
            num = (SP.loss(right, dict(c, **{key: c[key] + eps * d}), comps) - SP.loss(right, dict(c, **{key: c[key] - eps * d}), comps)) / (2 * eps)
            ana = float((grad[name] * d).sum())
            assert abs(num - ana) <= 1e-6 * max(1.0, abs(ana)), (name, num, ana)


# ------------------------------------------------------------------------------------------------------------------ the build
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_the_four_kernels_use_no_scratch_and_the_lds_the_header_names():
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("mano_pca_fwd_kernel", "mano_pca_bwd_kernel", "mano_post_fwd_kernel", "mano_post_bwd_kernel"):
            if k + "PK" in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert len(seen) == 4, sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    with open(os.path.join(ROOT, "ihmr_amd", "csrc", "mano_pose_space_pure.h")) as fh:
        pure = fh.read()
    const = {k: int(v) for k, v in re.findall(r"#define (MPS_POSE|MPS_TILE|MPS_C_STRIDE|MPS_THREADS) (\d+)", pure)}
    assert const == dict(MPS_POSE=45, MPS_TILE=16, MPS_C_STRIDE=45, MPS_THREADS=256)
    lds = {k: eval(v, {"__builtins__": {}}, const) for k, v in re.findall(r"#define (MPS_PCA_LDS_BYTES|MPS_POST_BWD_LDS_BYTES) \((.*)\)\s+//", pure)}
    assert lds == dict(MPS_PCA_LDS_BYTES=45 * 45 * 4 + 16 * 45 * 4, MPS_POST_BWD_LDS_BYTES=320)
    assert seen["mano_pca_fwd_kernel"]["group_segment_fixed_size"] == seen["mano_pca_bwd_kernel"]["group_segment_fixed_size"] == lds["MPS_PCA_LDS_BYTES"]
    assert seen["mano_post_fwd_kernel"]["group_segment_fixed_size"] == 0
    assert seen["mano_post_bwd_kernel"]["group_segment_fixed_size"] == lds["MPS_POST_BWD_LDS_BYTES"]

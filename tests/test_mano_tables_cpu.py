"""The asset tables of the MANO layer (ihmr_amd/csrc/mano_tables.h: build_mano_tables, build_shape_tables -- the very functions
ihmr_mano_create and ihmr_mano_update_shapedirs upload from) compiled for the HOST by g++ with -fsanitize=address,undefined and checked
against a numpy statement of the layouts written at `struct ihmr_mano` (csrc/ihmr_common.h): every table bit for bit, the CSR and its
cut into single-joint segments by their invariants, the three refusals.  A wrong segment boundary or a wrong `sparse4` fails here,
without a GPU; every comparison is exact."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mano_cases as MC  # noqa: E402
import hostbuild  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

NV, NF, NJ, NPF, NVP, NFP, SEG, SEG_CAP = 778, 1538, 16, 135, 832, 1600, 13, 1024
TIPS = (744, 320, 443, 554, 671)
IN_ORDER = (("v_template", np.float32), ("shapedirs", np.float32), ("posedirs", np.float32), ("J_regressor", np.float32),
            ("lbs_weights", np.float32), ("parents", np.int32), ("hands_mean", np.float32), ("faces", np.int32))
OUT_ORDER = (("v_template", "f4"), ("shapedirs_t", "f4"), ("posedirs", "f4"), ("pd4", "f4"), ("sd4", "f4"), ("vt4", "f4"), ("J_template", "f4"),
             ("J_shapedirs", "f4"), ("weights", "f4"), ("w4_w", "f4"), ("w4_j", "u4"), ("pose_mean", "f4"), ("parents", "i4"), ("depth", "i4"),
             ("tip_ids", "i4"), ("wj_start", "i4"), ("wj_vert", "i4"), ("wj_w", "f4"), ("seg_q", "i4"), ("jseg_start", "i4"), ("faces", "i4"),
             ("faces_pk", "u4"), ("J_regressor", "f4"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("mano_tables")
    exe = hostbuild.build("mano_tables_driver.cpp", d, hostbuild.X86_V3)
    count = [0]

    def run(asset, second_shapedirs=None):
        """The driver's tables as a dict (with "rc"); rc != 0: {"rc": rc} alone."""
        count[0] += 1
        fin, fout = str(d / f"{count[0]}.in"), str(d / f"{count[0]}.out")
        with open(fin, "wb") as fh:
            for k, dt in IN_ORDER:
                fh.write(np.ascontiguousarray(asset[k], dt).tobytes())
            fh.write(np.asarray(TIPS, np.int32).tobytes())
            if second_shapedirs is not None:
                fh.write(np.ascontiguousarray(second_shapedirs, np.float32).tobytes())
        op = "build" if second_shapedirs is None else "update"
        assert not hostbuild.run(exe, op, fin, fout).stderr
        raw = open(fout, "rb").read()
        out = {"rc": int(np.frombuffer(raw, np.int32, 1)[0])}
        if out["rc"]:
            assert len(raw) == 4
            return out
        out.update(zip(("sparse4", "max_depth", "nnz", "nseg"), map(int, np.frombuffer(raw, np.int32, 4, 4))))
        at = 20
        for k, dt in OUT_ORDER:
            n = int(np.frombuffer(raw, np.int64, 1, at)[0])
            out[k] = np.frombuffer(raw, dt, n, at + 8)
            at += 8 + 4 * n
        assert at == len(raw)
        return out
    return run


@pytest.fixture(scope="module")
def right():
    from ihmr_amd.assets import synthetic_mano
    return synthetic_mano(True)


def _with_weights(asset, w):
    a = dict(asset)
    a["lbs_weights"] = np.ascontiguousarray(w, np.float32)
    return a


def boundary_asset(asset, five):
    """Weights at the edges of the segment cut and of the 4-sparse form: joints 1, 2, 3 with exactly 13, 14 and 26 entries (one full
    segment; one full + one of 1; two full), joint 0 with all 778, joint 9 with one entry between empty joints, joints 8 and 10 - 15
    empty (the last joint too); vertex 100 with exactly four weights and vertex 101 with four, or with `five` exactly five -- the only
    vertex above four."""
    w = np.zeros((NV, NJ), np.float64)
    w[:, 0] = 1.0
    w[0:13, 1] = 1.0
    w[13:27, 2] = 1.0
    w[27:53, 3] = 1.0
    w[100, 4:7] = 1.0
    w[101, 4:8 if five else 7] = 1.0
    w[200, 9] = 1.0
    w /= w.sum(axis=1, keepdims=True)
    a = _with_weights(asset, w)
    nz = a["lbs_weights"] != 0
    per_joint, per_vertex = nz.sum(axis=0), nz.sum(axis=1)
    assert per_joint[:4].tolist() == [778, 13, 14, 26] and per_joint[9] == 1 and not per_joint[8] and not per_joint[10:].any()
    assert per_vertex[100] == 4 and per_vertex[101] == (5 if five else 4) and np.delete(per_vertex, 101).max() == 4
    return a


def all_nonzero_asset(asset):
    rng = np.random.default_rng(17)
    w = rng.uniform(0.05, 1.0, size=(NV, NJ))
    a = _with_weights(asset, w / w.sum(axis=1, keepdims=True))
    assert (a["lbs_weights"] != 0).all()
    return a


def second_shapedirs(asset):
    rng = np.random.default_rng(23)
    return (asset["shapedirs"] + 1e-3 * rng.standard_normal(asset["shapedirs"].shape)).astype(np.float32)


@pytest.fixture(scope="module")
def assets(right):
    from ihmr_amd.assets import synthetic_mano
    return {"right": right, "left": synthetic_mano(False), "dense7": MC.dense_weight_asset(right), "all_nonzero": all_nonzero_asset(right),
            "boundary4": boundary_asset(right, False), "boundary5": boundary_asset(right, True)}


ASSETS = ("right", "left", "dense7", "all_nonzero", "boundary4", "boundary5")


@pytest.fixture(scope="module")
def tables(driver, assets):
    return {k: driver(a) for k, a in assets.items()}


# ----------------------------------------------------------------------------------- the numpy statement (struct ihmr_mano's comments)
def _pack4(rows):
    """[rows][2334] -> [rows][NVP] (x, y, z, 0), zero rows behind the last vertex."""
    rows = np.asarray(rows, np.float32).reshape(-1, NV, 3)
    out = np.zeros((rows.shape[0], NVP, 4), np.float32)
    out[:, :NV, :3] = rows
    return out.reshape(-1)


def _regress(Jreg, x):
    """J_regressor . x as the float32 rounding of a float64 sum accumulated in vertex order: x (778, ...) -> (16, ...)."""
    Jreg, x = np.asarray(Jreg, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    acc = np.zeros((NJ,) + x.shape[1:], np.float64)
    for v in range(NV):
        acc += Jreg[:, v].reshape((NJ,) + (1,) * (x.ndim - 1)) * x[v][None]
    return acc.astype(np.float32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def check_shape_tables(t, asset, shapedirs):
    sd = np.asarray(shapedirs, np.float32)
    sd_t = np.ascontiguousarray(sd.reshape(NV * 3, 10).T)                  # [10][2334]
    assert _same(t["shapedirs_t"], sd_t.reshape(-1)) and _same(t["sd4"], _pack4(sd_t))
    assert _same(t["J_template"], _regress(asset["J_regressor"], asset["v_template"]).reshape(-1))          # [48]
    assert _same(t["J_shapedirs"], _regress(asset["J_regressor"], sd).reshape(-1))                          # [48][10]


@pytest.mark.parametrize("name", ASSETS)
def test_dense_tables_are_the_layouts_of_the_struct(tables, assets, name):
    t, a = tables[name], assets[name]
    assert t["rc"] == 0
    for k, src in (("v_template", "v_template"), ("posedirs", "posedirs"), ("weights", "lbs_weights"), ("J_regressor", "J_regressor")):
        assert _same(t[k], np.asarray(a[src], np.float32).reshape(-1)), k
    assert _same(t["parents"], np.asarray(a["parents"], np.int32)) and _same(t["tip_ids"], np.asarray(TIPS, np.int32))
    check_shape_tables(t, a, a["shapedirs"])
    assert _same(t["pd4"], _pack4(a["posedirs"])) and _same(t["vt4"], _pack4(a["v_template"]))
    assert _same(t["pose_mean"], np.concatenate([np.zeros(3, np.float32), np.asarray(a["hands_mean"], np.float32)]))
    faces = np.asarray(a["faces"], np.int32)
    padded = np.concatenate([faces, np.repeat(faces[:1], NFP - NF, axis=0)])           # [NFP][3], padded with face 0
    assert _same(t["faces"], padded.T) and t["faces"].size == 3 * NFP
    pk = padded.astype(np.uint32)
    assert _same(t["faces_pk"], pk[:, 0] | pk[:, 1] << 10 | pk[:, 2] << 20)
    depth = np.zeros(NJ, np.int32)
    for j in range(1, NJ):
        depth[j] = depth[a["parents"][j]] + 1
    assert _same(t["depth"], depth) and t["max_depth"] == depth.max()


@pytest.mark.parametrize("name", ASSETS)
def test_csr_by_joint_scatters_back_to_the_weights(tables, assets, name):
    t, w = tables[name], np.asarray(assets[name]["lbs_weights"], np.float32)
    start = t["wj_start"]
    assert start.size == NJ + 1 and start[0] == 0 and start[NJ] == t["nnz"] == t["wj_vert"].size == t["wj_w"].size == np.count_nonzero(w)
    back = np.zeros_like(w)
    for j in range(NJ):
        verts = t["wj_vert"][start[j]:start[j + 1]]
        assert (np.diff(verts) > 0).all() and (verts >= 0).all() and (verts < NV).all(), j          # ascending: no vertex twice
        back[verts, j] = t["wj_w"][start[j]:start[j + 1]]
    assert _same(back, w)


@pytest.mark.parametrize("name", ASSETS)
def test_segments_tile_the_csr_inside_single_joints(tables, name):
    t = tables[name]
    seg, jseg, start, nseg, nnz = t["seg_q"], t["jseg_start"], t["wj_start"], t["nseg"], t["nnz"]
    assert seg.size == nseg + 1 and seg[0] == 0 and seg[nseg] == nnz and nseg <= SEG_CAP
    length = np.diff(seg)
    assert ((1 <= length) & (length <= SEG)).all()                         # with seg[0] and seg[nseg]: an exact tiling of [0, nnz)
    assert jseg.size == NJ + 1 and jseg[0] == 0 and jseg[NJ] == nseg and (np.diff(jseg) >= 0).all()
    for j in range(NJ):
        s0, s1 = jseg[j], jseg[j + 1]
        n = start[j + 1] - start[j]
        assert s1 - s0 == -(-n // SEG), j                                   # an empty joint: an empty range
        if n:
            assert seg[s0] == start[j] and seg[s1] == start[j + 1]         # inside one joint's CSR range
            assert (length[s0:s1 - 1] == SEG).all(), j                     # every segment of a joint but its last is full


@pytest.mark.parametrize("name", ASSETS)
def test_w4_is_the_weights_when_sparse4(tables, assets, name):
    t, w = tables[name], np.asarray(assets[name]["lbs_weights"], np.float32)
    per_vertex = (w != 0).sum(axis=1)
    assert t["sparse4"] == int(per_vertex.max() <= 4)
    w4w, w4j = t["w4_w"].reshape(NV, 4), (t["w4_j"][:, None] >> (8 * np.arange(4, dtype=np.uint32))[None]) & 0xFF
    back = np.zeros_like(w)
    for v in range(NV):
        n = min(int(per_vertex[v]), 4)
        assert (np.diff(w4j[v, :n].astype(np.int64)) > 0).all() and (w4j[v, :n] < NJ).all() and (w4w[v, :n] != 0).all(), v      # joints ascending
        assert not w4j[v, n:].any() and _same(w4w[v, n:], np.zeros(4 - n, np.float32)), v         # padding: joint 0, weight +0
        back[v, w4j[v, :n]] = w4w[v, :n]
        assert _same(back[v, w4j[v, :n]], w[v, w4j[v, :n]]), v             # the first (up to) four non-zero weights, sparse4 or not
        assert n == 0 or (w[v, :int(w4j[v, n - 1])] != 0).sum() == n - 1, v          # ... with no non-zero weight skipped between them
    if t["sparse4"]:
        assert _same(back, w)


def test_the_assets_are_the_cases_they_stand_for(tables):
    assert [tables[k]["sparse4"] for k in ASSETS] == [1, 1, 0, 0, 1, 0]
    assert tables["all_nonzero"]["nnz"] == NV * NJ == 12448 and tables["all_nonzero"]["nseg"] == NJ * -(-NV // SEG) == 960       # the largest there is
    b4, b5 = tables["boundary4"], tables["boundary5"]
    assert np.diff(b4["jseg_start"]).tolist() == [60, 1, 2, 2, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert np.diff(b5["jseg_start"]).tolist() == [60, 1, 2, 2, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0]
    # the fifth weight of vertex 101 alone flips sparse4: every other vertex has the same joints in both
    same = np.delete(np.arange(NV), 101)
    assert _same(b4["w4_j"][same], b5["w4_j"][same]) and b4["w4_j"][101] == b5["w4_j"][101] == 0x06050400


@pytest.mark.parametrize("what", ["parents[5] = 5", "parents[3] = -1", "face id -1", "face id 778"])
def test_refusals(driver, right, what):
    a = dict(right)
    if what.startswith("parents"):
        a["parents"] = np.array(right["parents"], np.int32)
        a["parents"][5 if "[5]" in what else 3] = 5 if "[5]" in what else -1
    else:
        a["faces"] = np.array(right["faces"], np.int32)
        a["faces"][700, 1] = -1 if what.endswith("-1") else NV
    assert driver(a) == {"rc": -1}


def test_the_largest_face_id_and_the_deepest_chain_are_accepted(driver, right):
    a = dict(right, faces=np.array(right["faces"], np.int32), parents=np.arange(-1, NJ - 1, dtype=np.int32))
    a["faces"][700, 1] = NV - 1
    t = driver(a)
    assert t["rc"] == 0 and t["max_depth"] == NJ - 1 and _same(t["depth"], np.arange(NJ, dtype=np.int32))
    assert t["faces"].reshape(3, NFP)[1, 700] == NV - 1 and t["faces_pk"][700] >> 10 & 1023 == NV - 1


def test_shape_update_is_a_full_build_with_the_second_shapedirs(driver, assets, tables):
    for name in ("right", "dense7"):
        a = assets[name]
        sd2 = second_shapedirs(a)
        assert not _same(sd2, a["shapedirs"])
        updated, full = driver(a, sd2), driver(dict(a, shapedirs=sd2))
        check_shape_tables(updated, a, sd2)
        for k, _ in OUT_ORDER:
            assert _same(updated[k], full[k]), k
        assert all(updated[k] == full[k] for k in ("rc", "sparse4", "max_depth", "nnz", "nseg"))
        assert not _same(updated["sd4"], tables[name]["sd4"]) and _same(updated["J_template"], tables[name]["J_template"])

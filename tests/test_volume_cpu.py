"""The two-hand intersection volume without a GPU: the statement of tests/volume_ref.py against itself in float64 (a condition on the
case table) and against the lens formula; ``close_boundary``; csrc/volume_pure.h built for the host with ASan / UBSan
(tests/volume_host_driver.cpp, run as a program) against the statement word for word; the build (no spills, no scratch, the LDS
size of the header, the exported symbols); the Evaluator's volume sums, its unchanged pickle and the refused option pair."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj  # noqa: E402
import hostbuild  # noqa: E402
import volume_ref as VR  # noqa: E402

DIFF_CAP = 1e-4          # share of the counted voxels on which the float32 and the float64 grids may differ


def _subdivs(name):
    return (1, 2, 4) if name in VR.SUBDIV_2_4_CASES else (1,)


def test_case_table_has_every_class_and_the_stated_statuses():
    t = VR.case_table()
    for name in ("hand_default_0", "hand_deep_0", "fingers_0", "hand_open", "sphere162", "sphere642", "tetra", "sphere_vs_hand", "disjoint",
                 "touching", "nan_vertex", "tiny_cube", "shifted_2m", "far_vertex"):
        assert name in t, name
    assert t["sphere162"].va.shape == (162, 3) and t["sphere162"].fa.shape == (320, 3)
    assert t["sphere642"].va.shape == (642, 3) and t["sphere642"].fa.shape == (1280, 3)
    assert t["tetra"].va.shape == (4, 3) and t["tetra"].fa.shape == (4, 3)
    assert t["sphere_vs_hand"].va.shape[0] != t["sphere_vs_hand"].vb.shape[0]
    assert t["hand_default_0"].fa.shape == (1552, 3) and t["hand_open"].fa.shape == (1538, 3)
    for name, c in t.items():
        s = VR.statement(c, 1)
        assert s["status"] == c.status, (name, s["status"])
        if c.status != VR.COUNTED:
            assert not s["box"].any() and not s["counts"].any() and not s["bits"].any()
    # the counted cases count something, the far vertex really lies a metre outside the cube
    for name in ("hand_default_0", "hand_deep_0", "fingers_0", "sphere162", "tetra", "sphere_vs_hand", "shifted_2m", "far_vertex"):
        assert VR.statement(t[name], 1)["counts"].sum() > 0, name
    box = VR.statement(t["far_vertex"], 1)["box"]
    assert np.abs(t["far_vertex"].va[100, 1:] - box[1:3]).min() >= 1.0


def test_float32_and_float64_grids_agree_on_the_case_table():
    """A condition on the inputs, not a measurement of the kernel: over every case and every subdivision used, the float32 and the
    float64 grids of the voxels inside both meshes differ on at most 1e-4 of the counted voxels; on the known-answer cases no voxel
    of either mesh's inside grid differs.  (Per mesh, over all voxels examined, the figure is printed: a hand's surface passes
    through far more voxels than the intersection holds.)"""
    counted = differ = examined = differ_any = 0
    for name, c in VR.case_table().items():
        if c.status != VR.COUNTED:
            continue
        for n in _subdivs(name):
            a, b = VR.statement(c, n), VR.statement(c, n, f64=True)
            assert a["box"].tobytes() == b["box"].tobytes()
            d_any = int((a["inside_a"] != b["inside_a"]).sum() + (a["inside_b"] != b["inside_b"]).sum())
            d = int((a["bits"] != b["bits"]).sum() and ((a["inside_a"] & a["inside_b"]) != (b["inside_a"] & b["inside_b"])).sum())
            both = int(a["counts"].sum())
            print(f"[volume] {name} subdiv {n}: counted {both}, float32 != float64 on {d} of them; per mesh on {d_any} of "
                  f"{2 * a['inside_a'].size} voxels examined")
            if c.known_answer:
                assert d_any == 0, (name, n, d_any)
            counted, differ, examined, differ_any = counted + both, differ + d, examined + 2 * a["inside_a"].size, differ_any + d_any
    print(f"[volume] case table: {counted} counted voxels, float32 != float64 on {differ} of them; per mesh on {differ_any} of {examined} examined")
    assert counted > 1e5 and differ <= DIFF_CAP * counted, (differ, counted)


def test_lens_volume_of_the_sphere_pair():
    c = VR.case_table()["sphere642"]
    want = VR.lens_volume()
    vols = {n: VR.volume_m3(c, n) for n in (1, 2, 4)}
    for n, v in vols.items():
        print(f"[volume] sphere642 subdiv {n}: {v * 1e6:.4f} cm^3, lens {want * 1e6:.4f} cm^3, {100 * (v / want - 1):+.2f} %")
        assert abs(v / want - 1.0) <= 0.025, (n, v, want)
    assert abs(vols[2] / vols[4] - 1.0) <= 0.002, vols


# ------------------------------------------------------------------------------------------------------------------ close_boundary
def _directed_edges(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return [tuple(x) for x in e.tolist()]


@pytest.mark.parametrize("kind", ["mitten", "fingers"])
def test_close_boundary_closes_the_wrist(kind):
    from ihmr_amd.assets import synthetic_mano
    from ihmr_amd.sdf import close_boundary
    for is_right in (True, False):
        faces = np.asarray(synthetic_mano(is_right, kind=kind)["faces"], np.int32)
        assert faces.shape == (1538, 3) and len(VR.boundary_edges(faces)) == 16
        closed = close_boundary(faces, 778)
        assert closed.dtype == faces.dtype and closed.shape == (1552, 3) and np.array_equal(closed[:1538], faces)
        assert closed.max() < 778 and closed.min() >= 0                       # no new vertex
        edges = _directed_edges(closed)
        assert len(set(edges)) == len(edges)                                   # every directed edge once ...
        assert all((b, a) in set(edges) for a, b in edges)                     # ... and its opposite too: each edge twice, opposed
        assert np.array_equal(closed, VR.close_boundary(faces, 778))           # the statement's own restatement
        assert np.array_equal(close_boundary(closed, 778), closed)             # a closed mesh is returned unchanged
    v, f = VR.icosphere(1)
    assert np.array_equal(close_boundary(f, len(v)), f)


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("volume_pure")
    exe = hostbuild.build("volume_host_driver.cpp", d)
    count = [0]

    def run(case, n):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        with open(fin, "wb") as fh:
            fh.write(np.array([len(case.va), len(case.fa), len(case.vb), len(case.fb), n], np.int32).tobytes())
            for v, f in ((case.va, case.fa), (case.vb, case.fb)):
                fh.write(v.tobytes())
                fh.write(f.tobytes())
        hostbuild.run(exe, fin, fout)
        raw = open(fout, "rb").read()
        T = n ** 3
        assert len(raw) == 16 + 4 + 4 * T + 4 * T * 1024
        return dict(box=np.frombuffer(raw, np.float32, 4, 0), status=int(np.frombuffer(raw, np.int32, 1, 16)[0]),
                    counts=np.frombuffer(raw, np.uint32, T, 20), bits=np.frombuffer(raw, np.uint32, T * 1024, 20 + 4 * T).reshape(T, 1024))
    return run


def _assert_equal(got, want, what):
    assert got["status"] == want["status"], what
    assert got["box"].tobytes() == want["box"].tobytes(), (what, got["box"], want["box"])
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
    assert np.array_equal(got["bits"], want["bits"]), (what, int((got["bits"] != want["bits"]).sum()))


def test_pure_header_equals_the_statement_word_for_word(driver):
    """Every AND-word, count, status and the bits of the box: the whole case table at subdiv 1, four cases at subdiv 2 and 4."""
    tiles = 0
    for name, c in VR.case_table().items():
        for n in _subdivs(name):
            _assert_equal(driver(c, n), VR.statement(c, n), f"{name} subdiv {n}")
            tiles += n ** 3
    assert tiles >= len(VR.case_table()) + 4 * (8 + 64)


def test_column_range_clamp_and_record_packing(tmp_path):
    """vol_index_lo / vol_index_hi for far and non-finite coordinates (UBSan: no undefined conversion) and the list record round trip."""
    src = tmp_path / "clamp.cpp"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main() {\n'
                   '  const float xs[] = {-3e38f, -1e9f, -100.f, -1.2f, -1.f, 0.f, 0.97f, 1.f, 1.2f, 100.f, 1e9f, 3e38f, INFINITY, -INFINITY, NAN};\n'
                   '  for (float x : xs) printf("%%d %%d\\n", vol_index_lo(x), vol_index_hi(x));\n'
                   '  int ia, ib, ic, m; vol_unpack_record(vol_pack_record(1023u, 0u, 517u, 1), ia, ib, ic, m);\n'
                   '  printf("%%d %%d %%d %%d\\n", ia, ib, ic, m);\n'
                   '  int a, b, c, d; printf("%%d\\n", (int)vol_col_range(-500.f, 700.f, 3.f, 1e5f, -1e5f, 0.f, a, b, c, d)); printf("%%d %%d %%d %%d\\n", a, b, c, d);\n'
                   '  printf("%%d\\n", (int)vol_col_range(5.f, 7.f, 6.f, 0.f, 0.1f, 0.2f, a, b, c, d));\n'
                   '  return 0; }\n' % os.path.join(ROOT, "ihmr_amd", "csrc", "volume_pure.h"))
    r = hostbuild.run(hostbuild.build(src, tmp_path))
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.strip().splitlines()]
    f = np.float32
    for x, (lo, hi) in zip([-3e38, -1e9, -100.0, -1.2, -1.0, 0.0, 0.97, 1.0, 1.2, 100.0, 1e9, 3e38], rows):
        # inside the range that matters the clamp changes nothing: the indices are tri_col_range's (tests/helpers.py)
        with np.errstate(over="ignore"):
            want_lo = max(0, int(np.clip(np.ceil((f(x) + f(1)) * f(16) - f(0.5)), -4, 36)))
            want_hi = min(31, int(np.clip(np.floor((f(x) + f(1)) * f(16) - f(0.5)), -4, 36)))
        assert (lo, hi) == (want_lo, want_hi), (x, lo, hi)
    assert rows[12] == (36, 31) and rows[13] == (0, -4) and rows[14] == (0, -4)          # +Inf, -Inf, NaN (fmaxf drops the NaN)
    assert rows[15] == (1023, 0, 517, 1)
    assert rows[16] == (1,) and rows[17] == (0, 31, 0, 31) and rows[18] == (0,)


# ------------------------------------------------------------------------------------------------------------------ the build
def test_volume_kernels_use_no_scratch_and_the_symbol_is_exported():
    import ctypes

    from ihmr_amd import hip
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("vol_box_kernel", "vol_count_kernel"):
            if k in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == ["vol_box_kernel", "vol_count_kernel"], sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    # VOL_LDS_BYTES of csrc/volume_pure.h, which the kernel's struct is static_asserted against
    pure = open(os.path.join(ROOT, "ihmr_amd", "csrc", "volume_pure.h")).read()
    assert re.search(r"#define VOL_LDS_BYTES \(2 \* VOL_MAX_VERTS \* 3 \* 4 \+ 2 \* VOL_COLS \* 4 \+ 2 \* VOL_MAX_FACES \* 4 \+ \(VOL_THREADS / 64\) \* 4 \+ 4\)", pure)
    lds = 2 * hip.VOLUME_MAX_VERTS * 3 * 4 + 2 * 1024 * 4 + 2 * hip.VOLUME_MAX_FACES * 4 + 4 * 4 + 4
    assert seen["vol_count_kernel"]["group_segment_fixed_size"] == lds <= 64 * 1024
    assert seen["vol_box_kernel"]["group_segment_fixed_size"] == 4 * 13 * 4
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    assert f"#define IHMR_VOLUME_MAX_VERTS {hip.VOLUME_MAX_VERTS}\n" in header and f"#define IHMR_VOLUME_MAX_FACES {hip.VOLUME_MAX_FACES}\n" in header
    declared = set(re.findall(r"^\s*(?:[A-Za-z_][\w ]*?[\s*]+)(ihmr_\w+)\s*\(", header, flags=re.M))
    assert "ihmr_sdf_volume" in declared
    assert declared == set(hip.EXPORTED_SYMBOLS), declared ^ set(hip.EXPORTED_SYMBOLS)
    L = ctypes.CDLL(hip.build())
    for sym in declared:
        getattr(L, sym)


# ------------------------------------------------------------------------------------------------------------------ Evaluator
def _mano():
    import types
    one_hot = np.zeros(778, np.float32)
    one_hot[0] = 1.0
    m = types.SimpleNamespace(faces=np.zeros((1538, 3), np.int64), J_regressor=np.stack([one_hot] * 16))
    return dict(right=m, left=m)


def _rows(seed, B):
    """What update_device_volume leaves behind for one batch, made up on the host: (B,4) float64 [cm^3, interacting and kept,
    of those with count > 0, invalid]."""
    import torch
    rng = np.random.RandomState(seed)
    kept = rng.rand(B) < 0.8
    counted = kept & (rng.rand(B) < 0.6)
    vol = np.where(counted, rng.rand(B) * 7.0, 0.0)
    invalid = kept & ~counted & (rng.rand(B) < 0.3)
    return torch.from_numpy(np.stack([vol, kept.astype(np.float64), counted.astype(np.float64), invalid.astype(np.float64)], axis=1))


def test_volume_sums_are_additive_over_split_batches():
    from ihmr_amd import evaluator as E
    whole, split = E.Evaluator(_mano(), volume_metric=True), E.Evaluator(_mano(), volume_metric=True)
    assert np.array_equal(whole.volume_sums(), np.zeros(4)) and whole.volume_sums().dtype == np.float64
    rows = _rows(3, 13)
    whole._device_volume_parts.append(rows)
    for lo, hi in ((0, 4), (4, 5), (5, 13)):
        split._device_volume_parts.append(rows[lo:hi])
    a, b = whole.volume_sums(), split.volume_sums()
    assert np.array_equal(a[1:], b[1:]) and np.array_equal(a[1:], rows[:, 1:].sum(dim=0).numpy())
    assert abs(a[0] - b[0]) <= 1e-12 * a[0] and a[0] > 0
    two = E.Evaluator(_mano(), volume_metric=True)
    two._device_volume_parts.append(_rows(4, 6))
    m = E.Evaluator.volume_metrics_from_sums(a + two.volume_sums())                # over ranks: the sums add
    tot = a + two.volume_sums()
    assert m == dict(pen_volume=tot[0] / tot[1], pen_rate=tot[2] / tot[1])
    nothing = E.Evaluator.volume_metrics_from_sums(np.zeros(4))
    assert np.isnan(nothing["pen_volume"]) and np.isnan(nothing["pen_rate"])
    whole.clear()
    assert np.array_equal(whole.volume_sums(), np.zeros(4))
    # the existing sums know nothing of the volume
    assert len(whole.metric_sums()) == 9 and len(whole.pa_metric_sums()) == 6
    with pytest.raises(RuntimeError):
        E.Evaluator(_mano()).update_device_volume(None, None)                      # the metric is off by default


def test_default_evaluator_pickles_byte_for_byte_as_before():
    from ihmr_amd import evaluator as E
    ev = E.Evaluator(_mano())
    before = ["pa_metrics", "curve_metrics", "thresholds", "f_thresholds", "inputSize", "left_hand_faces", "right_hand_faces", "root_weights",
              "data_list", "image_root", "save_verts", "pred_results", "_device_parts", "_device_vert_parts", "_device_pa_parts",
              "_device_pa_vert_parts", "_device_curve_parts", "_device_curve_vert_parts"]
    assert list(ev.__dict__) == before                       # the attributes, in order, of an Evaluator from before the metric
    blob = pickle.dumps(ev)
    assert b"volume" not in blob
    # the same bytes as an object given exactly the earlier attributes
    twin = E.Evaluator.__new__(E.Evaluator)
    for k in before:
        twin.__dict__[k] = ev.__dict__[k]
    assert pickle.dumps(twin) == blob
    ev.clear()
    assert list(ev.__dict__) == before
    back = pickle.loads(blob)
    assert np.array_equal(back.volume_sums(), np.zeros(4)) and list(back.__dict__) == before
    on = E.Evaluator(_mano(), volume_metric=True, volume_subdiv=4)
    assert on.volume_metric and on.volume_subdiv == 4 and list(on.__dict__)[:len(before)] == before
    with pytest.raises(ValueError):
        E.Evaluator(_mano(), volume_metric=True, volume_subdiv=3)


def test_run_optimize_refuses_volume_metric_with_host_eval():
    r = subprocess.run([sys.executable, "-m", "ihmr_amd.run_optimize", "--volume_metric", "--host_eval"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "--volume_metric" in r.stderr and "--host_eval" in r.stderr, (r.returncode, r.stderr[-2000:])

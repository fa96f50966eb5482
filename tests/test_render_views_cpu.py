"""Rotated views and the penetration heat map of the mesh renderer without a GPU: the ABI of ``ihmr_view_vertices`` /
``ihmr_heat_colours`` / ``ihmr_paint_meshes``, the resource budget of their kernels, the new functions of ``ihmr_amd/csrc/render_pure.h``
compiled for the host (g++ -fsanitize=address,undefined, ``tests/view_host_driver.cpp``) against ``tests/render_views_ref.py`` bit for
bit, known answers written out by hand, and the input conditions of what tests/test_gpu_render_views.py renders."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402
import hostbuild  # noqa: E402
import render_cases as RC  # noqa: E402
import render_ref as R  # noqa: E402
import render_views_ref as V  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
f32 = np.float32
NEW = ("ihmr_view_vertices", "ihmr_heat_colours", "ihmr_paint_meshes")
LO, HI = f32(0.0), f32(0.005)


def edge_depths(lo=LO, hi=HI):
    """Negative, 0, lo, hi, their float neighbours, above hi, NaN and the infinities."""
    up, down = lambda x: np.nextafter(f32(x), f32(np.inf)), lambda x: np.nextafter(f32(x), f32(-np.inf))
    return np.array([-1.0, -1e-3, -0.0, 0.0, lo, up(lo), down(lo), hi, up(hi), down(hi), 0.5 * (lo + hi), 0.001, 0.0049, 0.01, 1.0, 3e38,
                     np.nan, np.inf, -np.inf, 1e-45, -1e-45], f32)


# ------------------------------------------------------------------------------------------------------------------ ABI and build
def test_header_binding_and_library_agree_on_the_view_entry_points():
    from ihmr_amd import hip
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    for sym in NEW:
        assert len(re.findall(rf"\bint {sym}\s*\(", header)) == 1, sym
        assert hip.EXPORTED_SYMBOLS.count(sym) == 1, sym
    if shutil.which("hipcc") is None:
        return
    L = hip.bind(ctypes.CDLL(hip.build()))
    for sym in NEW:
        assert hasattr(L, sym), sym
    # bad shapes, missing pointers and overlapping buffers are refused before anything is launched (no GPU is touched here)
    one = ctypes.c_void_p(1 << 20)
    nbytes = 2 * 1556 * 12
    far = ctypes.c_void_p((1 << 20) + nbytes)                                    # the first byte behind `verts`: no overlap
    good = [one, None, 1556, 778, one, 0, None, far, 2, None]
    for at, bad in ((0, None), (4, None), (7, None), (2, 0), (2, (1 << 24) + 1), (3, -1), (3, 1557), (5, 2), (5, -1), (8, 0), (8, 65536),
                    (7, one), (7, ctypes.c_void_p((1 << 20) + nbytes - 4)), (7, ctypes.c_void_p((1 << 20) - nbytes + 4)), (7, ctypes.c_void_p((1 << 20) + 12))):
        args = list(good)
        args[at] = bad
        assert L.ihmr_view_vertices(*args) == -1, (at, bad)
    hot = (ctypes.c_float * 3)(0, 0, 1)
    good = [one, one, hot, 0.0, 0.005, 1556, 778, 1, one, 2, None]
    for at, bad in ((0, None), (1, None), (2, None), (8, None), (4, 0.0), (4, -1.0), (3, 0.005), (3, float("nan")), (4, float("nan")),
                    (4, float("inf")), (3, float("-inf")), (5, 0), (5, 1555), (5, 1557), (6, 777), (6, -1), (7, 2), (7, -1), (9, 0), (9, 65536)):
        args = list(good)
        args[at] = bad
        assert L.ihmr_heat_colours(*args) == -1, (at, bad)
    args = list(good)
    args[5], args[6], args[7] = 1555, 1556, 0                                    # n_split beyond n_verts, also under layout 0
    assert L.ihmr_heat_colours(*args) == -1
    lights = hip.RenderLights()
    good = [one, one, one, one, 1556, 3076, 1538, None, one, one, ctypes.byref(lights), None, 64, one, None, one, 1, None]
    for at, bad in ((0, None), (1, None), (8, None), (10, None), (13, None), (15, None), (4, 0), (5, 0), (6, 3077), (12, 15), (12, 2049), (16, 0)):
        args = list(good)
        args[at] = bad
        assert L.ihmr_paint_meshes(*args) == -1, (at, bad)


@needs_hipcc
def test_view_kernels_use_no_scratch_and_the_render_kernels_keep_their_budget():
    """The three new kernels spill nothing and have no private segment; the three kernels of the plain render keep the registers, the
    LDS and the empty private segment they had before the vertex stage became a function two kernels call."""
    names = ("render_vertex_kernel", "render_raster_kernel", "draw_keypoints_kernel", "paint_vertex_kernel", "view_vertices_kernel",
             "heat_colours_kernel")
    seen = {}
    for name, rec in codeobj.records().items():
        for k in names:
            if k in name:
                assert k not in seen, name
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == sorted(names), sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    # what the parent commit's code object reports for the three existing kernels
    parent = dict(render_vertex_kernel=(27, 0), render_raster_kernel=(94, 18448), draw_keypoints_kernel=(14, 0))
    for name, (vgpr, lds) in parent.items():
        assert (seen[name]["vgpr_count"], seen[name]["agpr_count"], seen[name]["group_segment_fixed_size"]) == (vgpr, 0, lds), (name, seen[name])
    assert seen["view_vertices_kernel"]["group_segment_fixed_size"] == 4 * 6 * 4                # one box per wave
    assert seen["heat_colours_kernel"]["group_segment_fixed_size"] == 0 and seen["paint_vertex_kernel"]["group_segment_fixed_size"] == 0
    assert seen["paint_vertex_kernel"]["vgpr_count"] <= 32


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("views")
    exe = hostbuild.build("view_host_driver.cpp", d)
    count = [0]

    def run(op, payload, ok=True):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        with open(fin, "wb") as fh:
            fh.write(payload)
        hostbuild.run(exe, op, fin, fout, ok=ok)
        return open(fout, "rb").read()

    class D:
        @staticmethod
        def view(verts, rots, n_split, present=(1, 1), pivot=None):
            verts, rots = np.ascontiguousarray(verts, f32), np.ascontiguousarray(rots, f32).reshape(-1, 3, 3)
            nV, nR = verts.shape[0], rots.shape[0]
            raw = run("view", b"".join([np.array([nV, n_split, present[0], present[1], pivot is not None, nR], np.int32).tobytes(),
                                        np.asarray(pivot if pivot is not None else np.zeros(3), f32).tobytes(), rots.tobytes(), verts.tobytes()]))
            a = np.frombuffer(raw, f32)
            return a[:3].copy(), a[3:].reshape(nR, nV, 3)

        @staticmethod
        def heat(depth, albedo, hot, lo, hi, n_split, layout, ok=True):
            depth = np.ascontiguousarray(depth, f32)
            raw = run("heat", b"".join([np.array([depth.shape[0], n_split, layout], np.int32).tobytes(), np.array([lo, hi], f32).tobytes(),
                                        np.asarray(hot, f32).tobytes(), np.asarray(albedo, f32).tobytes(), depth.tobytes()]), ok)
            return np.frombuffer(raw, f32).reshape(-1, 3)
    return D


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rotations():
    """50 matrices as float32: the five views of the GPU tests, turns of 0, +-90, 180 and 720 degrees about every axis, random angles."""
    rng = np.random.RandomState(5)
    views = list(V.VIEWS) + [(a, d) for a in "xyz" for d in (0, 90, -90, 180, 720)]
    views += [("xyz"[k % 3], float(rng.uniform(-400, 400))) for k in range(50 - len(views))]
    assert len(views) == 50
    return np.stack([V.view_rotation(a, d) for a, d in views]).astype(f32)


@needs_gxx
def test_host_view_points_match_the_restatement(driver):
    """20 000 random points x 50 rotations about a given pivot, and about the default pivot of the same cloud."""
    rng = np.random.RandomState(6)
    p = (rng.normal(0, 0.1, (20000, 3)) * np.array([1.0, 3.0, 0.2])).astype(f32)
    rots = rotations()
    for pivot in (np.array([0.013, -0.4, 2.0], f32), None):
        c, q = driver.view(p, rots, 12000, pivot=pivot)
        want_c = V.bbox_mid(p, 12000) if pivot is None else pivot
        assert same_bits(c, want_c)
        for k in range(50):
            assert same_bits(q[k], V.view_points(p, want_c, rots[k])), k
    # the restatement's matrices are the product's, and the identity does not give the points back: "no view" must skip the transform
    from ihmr_amd import render
    for a, d in list(V.VIEWS) + [("x", 0), ("q", 720), ("z", -90)]:
        assert np.array_equal(render.view_rotation(a, d), V.view_rotation(a, d)), (a, d)
    moved = V.view_points(p, V.bbox_mid(p, 12000), np.eye(3))
    assert not same_bits(moved, p) and np.abs(moved - p).max() < 1e-6


@needs_gxx
def test_host_default_pivot_matches_the_restatement(driver):
    """Hands with NaN / Inf vertices, no finite vertex at all, one hand drawn, none drawn, a split at either end, signed zeros."""
    rng = np.random.RandomState(7)
    base = RC.hand_verts()[0]
    eye = np.eye(3, dtype=f32)
    cases = []
    for present in ((1, 1), (1, 0), (0, 1), (0, 0)):
        cases.append((base, 778, present))
    bad = base.copy()
    bad[rng.choice(1556, 200, replace=False), rng.randint(0, 3, 200)] = rng.choice([np.nan, np.inf, -np.inf], 200)
    bad[np.argmax(base[:, 0]), 1] = np.nan                                       # the vertex that held the x maximum no longer counts
    bad[np.argmin(base[:778, 2]), 0] = np.inf
    for present in ((1, 1), (1, 0), (0, 1)):
        cases.append((bad, 778, present))
    none = np.full((300, 3), np.nan, f32)
    none[::2, 1] = 1.0                                                           # one finite coordinate is not enough
    cases += [(none, 150, (1, 1)), (base[:778], 0, (1, 1)), (base[:778], 0, (1, 0)), (base[:778], 778, (1, 0)), (base[:1], 1, (1, 1))]
    zeros = np.array([[0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, -0.0], [-1.0, -2.0, -0.0]], f32)
    cases += [(zeros[:3], 3, (1, 1)), (zeros[:3][::-1], 3, (1, 1)), (zeros, 2, (1, 0)), (zeros, 2, (0, 1))]
    for k, (verts, n_split, present) in enumerate(cases):
        c, q = driver.view(verts, eye, n_split, present)
        want = V.bbox_mid(verts, n_split, present)
        assert same_bits(c, want), (k, c, want)
        assert same_bits(q[0], V.view_points(verts, want, eye)), k               # every vertex is transformed, drawn or not, NaN or not
    assert same_bits(V.bbox_mid(none, 150), np.zeros(3, f32)) and same_bits(V.bbox_mid(base, 778, (0, 0)), np.zeros(3, f32))
    assert not same_bits(V.bbox_mid(bad, 778), V.bbox_mid(base, 778))
    assert not same_bits(V.bbox_mid(base, 778, (1, 0)), V.bbox_mid(base, 778, (0, 1)))
    # the deviation from the reference is real: the middle of the box is not the mean
    assert np.abs(V.bbox_mid(base, 778) - base.mean(0)).max() > 1e-3


@needs_gxx
def test_host_heat_colours_match_the_restatement(driver):
    rng = np.random.RandomState(8)
    hot = np.array([0, 0, 1], f32)
    for lo, hi in ((LO, HI), (f32(0.001), f32(0.0035)), (f32(-0.002), f32(1e-3))):
        edges = edge_depths(lo, hi)
        depth = np.concatenate([edges, rng.uniform(-0.002, 0.008, 1556 - 2 * len(edges)).astype(f32), edges[::-1]])
        assert depth.shape == (1556,)
        for layout in (0, 1):
            got = driver.heat(depth, RC.TWO_HAND, hot, lo, hi, 778, layout)
            assert same_bits(got, V.heat_colours(depth, RC.TWO_HAND, hot, lo, hi, 778, layout)), (lo, hi, layout)
    got = driver.heat(edge_depths(), RC.TWO_HAND, (0.25, 0.5, 0.75), LO, HI, 9, 0)                 # n_verts odd, an uneven split
    assert same_bits(got, V.heat_colours(edge_depths(), RC.TWO_HAND, (0.25, 0.5, 0.75), LO, HI, 9, 0))
    driver.heat(edge_depths(), RC.TWO_HAND, hot, LO, HI, 9, 1, ok=False)                           # layout 1 needs two equal halves
    # what the edges mean: base colour up to lo and for NaN, hot from hi on, strictly between them between
    c = V.heat_colours(edge_depths(), RC.TWO_HAND, hot, LO, HI, 21, 0)
    d = edge_depths()
    with np.errstate(invalid="ignore"):
        is_base, is_hot = ~(d > LO), d >= HI
    assert is_base.sum() >= 8 and is_hot.sum() >= 6 and (~is_base & ~is_hot).sum() >= 5
    assert same_bits(c[is_base], np.repeat(RC.TWO_HAND[:1], is_base.sum(), 0)) and same_bits(c[is_hot], np.repeat(hot[None], is_hot.sum(), 0))
    mid = c[(d > 1e-4) & (d < HI)]                                                # (a depth of 1e-45 blends by less than a rounding)
    assert len(mid) >= 4
    assert ((mid[:, 2] > RC.TWO_HAND[0, 2]) & (mid[:, 2] < 1)).all() and ((mid[:, 0] < RC.TWO_HAND[0, 0]) & (mid[:, 0] > 0)).all()


# ------------------------------------------------------------------------------------------------------------------ known answers
def test_quarter_turn_about_y_of_dyadic_points_is_exact():
    """R = Ry(90 degrees) written with exact 0 and +-1: q = (d0 R[0] + d1 R[1] + d2 R[2]) + c = (-d2, d1, d0) + c.  With dyadic points and a
    dyadic pivot every operation is exact:  p = (1.5, 0.25, -2), c = (0.5, 0.25, 1) -> d = (1, 0, -3) -> (3, 0, 1) + c = (3.5, 0.25, 2)."""
    ry = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], f32)
    c = np.array([0.5, 0.25, 1.0], f32)
    p = np.array([[1.5, 0.25, -2.0], [0.5, 0.25, 1.0], [0.5, 4.25, 1.0], [-0.25, -1.0, 1.125]], f32)
    want = np.array([[3.5, 0.25, 2.0], [0.5, 0.25, 1.0], [0.5, 4.25, 1.0], [0.375, -1.0, 0.25]], f32)
    assert np.array_equal(V.view_points(p, c, ry), want)
    # four quarter turns come back, and the pivot of a dyadic box is its middle: x in [-0.25, 1.5], y in [-1, 4.25], z in [-2, 1.125]
    q = p
    for _ in range(4):
        q = V.view_points(q, c, ry)
    assert np.array_equal(q, p)
    assert np.array_equal(V.bbox_mid(p, 4), np.array([0.625, 1.625, -0.4375], f32))
    assert np.array_equal(V.bbox_mid(p, 2, (0, 1)), np.array([0.125, 1.625, 1.0625], f32))
    # Ry(90) as the product builds it differs from the exact matrix only by cos(pi / 2) = 6.1e-17
    assert np.abs(V.view_rotation("y", 90) - ry).max() < 1e-16 and V.view_rotation("y", 90)[0, 2] == 1.0


@pytest.mark.parametrize("entry", [0, 5, 777, 778, 1000, 1555])
def test_collision_layout_lights_the_named_vertex_of_the_other_hand(entry):
    """Entry h * 778 + v of the collision module's table was sampled at vertex v of hand 1 - h: exactly that vertex of the merged mesh
    turns hot, every other keeps its hand's colour."""
    depth = np.zeros(1556, f32)
    depth[entry] = 0.01
    h, v = divmod(entry, 778)
    lit = (1 - h) * 778 + v
    hot = np.array([0, 0, 1], f32)
    c = V.heat_colours(depth, RC.TWO_HAND, hot, LO, HI, 778, 1)
    want = np.repeat(RC.TWO_HAND, 778, 0)
    want[lit] = hot
    assert np.array_equal(c, want)
    c0 = V.heat_colours(depth, RC.TWO_HAND, hot, LO, HI, 778, 0)
    want = np.repeat(RC.TWO_HAND, 778, 0)
    want[entry] = hot
    assert np.array_equal(c0, want)


def test_painting_every_vertex_in_its_hands_colour_is_the_plain_render():
    sc, f = RC.scene("s64"), RC.faces()
    for b in range(3):
        img, ids = V.render_sample_painted(sc["verts"][b], f, sc["cam"][b], 64, np.repeat(sc["albedo"][b], 778, 0), RC.SPLIT, sc["present"][b], sc["bg"][b])
        assert np.array_equal(img, RC.reference("s64")[0][b]) and np.array_equal(ids, RC.reference("s64")[1][b])


def test_evaluator_command_line_parses_views():
    from ihmr_amd import evaluator as E
    assert E.parse_views("y:90,x:-90") == [("y", 90.0), ("x", -90.0)] and E.parse_views("") == [] and E.parse_views(" z:37.5 ") == [("z", 37.5)]
    for bad in ("y", "w:90", "y:abc"):
        with pytest.raises(ValueError):
            E.parse_views(bad)


def test_new_render_options_are_keyword_only_and_raise_without_a_gpu(monkeypatch):
    import inspect
    import torch
    from ihmr_amd import render
    p = inspect.signature(render.MeshRenderer.render).parameters
    for name in ("view", "pivot", "vertex_colors", "return_alpha"):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default in (None, False), name
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fr, fl = RC.hand_faces()
    r = render.MeshRenderer(fr, fl)
    z = torch.zeros(1, 778, 3)
    with pytest.raises(RuntimeError):
        r.render(z, z, torch.ones(1, 3), size=64, view=("y", 90))
    with pytest.raises(RuntimeError):
        r.render_views(z, z, torch.ones(1, 3), [None, ("y", 90)], size=64)
    with pytest.raises(RuntimeError):
        render.penetration_colors(torch.zeros(1, 1556))
    with pytest.raises(RuntimeError):
        render.rotated(np.zeros((778, 3)), fr, 90, np.ones(3), 64)


# ------------------------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", ["s64", "s50", "deep"])
def test_rotated_scenes_stay_in_the_image_and_differ_from_the_front_view(name):
    """Asserted on the restatement: under each of the five views, about the default pivot, every sample covers at least 1.5 % of the
    image, touches no border pixel, and differs from the camera's own view in at least 100 face-id pixels."""
    _, front = RC.reference(name)
    for view in V.VIEWS:
        _, ids = V.view_reference(name, view)
        for b in range(ids.shape[0]):
            cov = ids[b] >= 0
            changed = int((ids[b] != front[b]).sum())
            print(f"[views] {name}[{b}] {view}: {cov.mean():.3f} covered, {changed} face-id pixels differ from the front view")
            assert cov.mean() >= 0.015, (name, b, view, cov.mean())
            assert not (cov[0].any() or cov[-1].any() or cov[:, 0].any() or cov[:, -1].any()), (name, b, view)
            assert changed >= 100, (name, b, view, changed)


def test_deep_hands_exercise_base_colour_ramp_and_saturation():
    """The oracle's per-vertex penetration depth of the four deep-overlap hands: each half of each sample has at least 200 positive
    entries, at least 10 at or above 5 mm and at least 100 strictly between -- the default range (0, 5 mm) reaches all three parts."""
    import torch
    from ihmr_amd.assets import synthetic_mano
    from oracle.sdf_ref import SDFLossRef
    right, left = synthetic_mano(True), synthetic_mano(False)
    hv = torch.from_numpy(RC.hand_verts().reshape(4, 2, 778, 3))
    _, _, osc = SDFLossRef(right["faces"], left["faces"])(hv, return_per_vert_loss=True, return_origin_scale_loss=True)
    osc = osc.detach().numpy().reshape(4, 2, 778)
    for b in range(4):
        for h in range(2):
            d = osc[b, h]
            pos, sat, ramp = int((d > 0).sum()), int((d >= HI).sum()), int(((d > 0) & (d < HI)).sum())
            print(f"[depth] sample {b} half {h}: {pos} positive, {sat} at or above 5 mm, {ramp} between")
            assert pos >= 200 and sat >= 10 and ramp >= 100, (b, h, pos, sat, ramp)

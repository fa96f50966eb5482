"""The mesh renderer without a GPU: the ABI of its entry points, the resource budget of its kernels, ``ihmr_amd/csrc/render_pure.h``
compiled for the host (g++ -fsanitize=address,undefined, ``tests/render_host_driver.cpp``) against ``tests/render_ref.py`` bit for bit,
known answers worked out by hand on the restatement, the host half of ``ihmr_amd/render.py`` against what the reference handed to OpenDR
(``tests/golden/render.npz``), and the input conditions of the scenes the GPU tests render (``tests/render_cases.py``)."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cases as RC  # noqa: E402
import codeobj  # noqa: E402
import hostbuild  # noqa: E402
import render_ref as R  # noqa: E402

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
f32 = np.float32
GREY = np.full((2, 3), 0.5, f32)


# ------------------------------------------------------------------------------------------------------------------ ABI and build
def test_header_binding_and_library_agree_on_the_render_entry_points():
    from ihmr_amd import hip
    header = open(os.path.join(ROOT, "include", "ihmr_hip.h")).read()
    declared = set(re.findall(r"\b(ihmr_render_[a-z0-9_]+|ihmr_draw_keypoints)\s*\(", header))
    assert declared == {"ihmr_render_workspace_bytes", "ihmr_render_meshes", "ihmr_draw_keypoints"}
    assert declared <= set(hip.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(hip.RenderLights) == 72
    if shutil.which("hipcc") is not None:
        L = hip.bind(ctypes.CDLL(hip.build()))
        for sym in declared:
            assert hasattr(L, sym), sym
        assert L.ihmr_render_workspace_bytes(3, 1556) == 3 * 1556 * 24 and L.ihmr_render_workspace_bytes(0, 1556) == 0
        # bad shapes and missing pointers are refused before anything is launched (no GPU is touched here)
        lights = hip.RenderLights()
        one = ctypes.c_void_p(64)
        good = [one, one, one, one, 1556, 3076, 1538, None, one, one, ctypes.byref(lights), None, 64, one, None, one, 1, None]
        for at, bad in ((0, None), (1, None), (8, None), (10, None), (13, None), (15, None), (4, 0), (5, 0), (6, 3077), (12, 15), (12, 2049), (16, 0)):
            args = list(good)
            args[at] = bad
            assert L.ihmr_render_meshes(*args) == -1, (at, bad)
        assert L.ihmr_draw_keypoints(None, one, one, b"\0\0\0", 1, 64, 42, None) == -1
        assert L.ihmr_draw_keypoints(one, one, one, b"\0\0\0", 1, 64, 0, None) == -1


@needs_hipcc
def test_render_kernels_use_no_scratch():
    """The z-buffer, the face record a thread sets up and the four pixels' winners live in registers: a spill would put them in memory."""
    seen = {}
    for name, rec in codeobj.records().items():
        for k in ("render_vertex_kernel", "render_raster_kernel", "draw_keypoints_kernel"):
            if k in name:
                seen[k] = {key: rec[key] for key in
                           ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    assert sorted(seen) == ["draw_keypoints_kernel", "render_raster_kernel", "render_vertex_kernel"], sorted(seen)
    for name, m in sorted(seen.items()):
        print(f"[build] {name}: {m}")
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
    assert seen["render_raster_kernel"]["group_segment_fixed_size"] <= 256 * 72 + 64         # the chunk list and the four wave counts
    assert seen["render_raster_kernel"]["vgpr_count"] <= 128                                # two workgroups of 256 per SIMD quartet


# ------------------------------------------------------------------------------------------------------------------ host build of the header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("render")
    exe = hostbuild.build("render_host_driver.cpp", d)
    count = [0]

    def run(op, payload):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        with open(fin, "wb") as fh:
            fh.write(payload)
        hostbuild.run(exe, op, fin, fout)
        return open(fout, "rb").read()

    def render(verts, faces, cam, S, albedo, split, present=(1, 1), bg=None, light=None):
        verts, faces = np.ascontiguousarray(verts, f32), np.ascontiguousarray(faces, np.int32)
        nV, nF = verts.shape[0], faces.shape[0]
        off, ids = R.build_csr(faces, nV)
        pos, col = light if light is not None else R.lights()
        payload = b"".join([np.array([nV, nF, split, S, present[0], present[1], bg is not None], np.int32).tobytes(),
                            np.asarray(cam, f32).tobytes(), np.asarray(albedo, f32).tobytes(), np.asarray(pos, f32).tobytes(),
                            np.asarray(col, f32).tobytes(), verts.tobytes(), faces.tobytes(), off.tobytes(), ids.tobytes(),
                            b"" if bg is None else np.ascontiguousarray(bg, np.uint8).tobytes()])
        raw = run("render", payload)
        rec = np.frombuffer(raw[:nV * 36], np.uint32).reshape(nV, 9)
        img = np.frombuffer(raw[nV * 36:nV * 36 + S * S * 3], np.uint8).reshape(S, S, 3)
        fid = np.frombuffer(raw[nV * 36 + S * S * 3:], np.int32).reshape(S, S)
        return rec, img, fid
    render.raw = run
    return render


def ref_vertex_records(verts, faces, cam, S, albedo, split):
    """What the driver writes per vertex, from the restatement: normal, colour (float32 bits), X, Y, 1/z bits."""
    verts = np.asarray(verts, f32)
    nV = verts.shape[0]
    off, ids = R.build_csr(faces, nV)
    hand = np.zeros(nV, np.int64)
    has = off[1:] > off[:-1]
    hand[has] = ids[off[:-1][has]] >= split
    n = R.vertex_normals(verts, faces, (off, ids))
    p = R.translate(verts, cam)
    c = R.shade(n, p, np.asarray(albedo, f32)[hand])
    X, Y, iz, _ = R.project(p, S)
    return np.concatenate([n.view(np.uint32), c.view(np.uint32), X.view(np.uint32)[:, None], Y.view(np.uint32)[:, None], iz.view(np.uint32)[:, None]], 1)


def soup(seed, nV, nF, S, spread=1.6):
    """Random triangles: vertices over more than the view (faces partly and wholly off screen, both windings), depths from in front of
    the near distance to far behind it."""
    rng = np.random.RandomState(seed)
    cam = np.array([2.0, 0.05, -0.03], f32)                                          # t_z = 2.5
    verts = np.stack([rng.uniform(-spread, spread, nV) * 0.5, rng.uniform(-spread, spread, nV) * 0.5, rng.uniform(-2.45, 1.5, nV)], 1).astype(f32)
    faces = rng.randint(0, nV, (nF, 3)).astype(np.int32)
    return verts, faces, cam


@needs_gxx
def test_host_build_matches_the_restatement_on_random_vertices(driver):
    """2 000 random vertices under 3 000 random faces: normals, shaded colours and 1/z bitwise equal as float32, snapped coordinates exact
    -- and the image and the face ids of the soup with them."""
    verts, faces, cam = soup(1, 2000, 3000, 48)
    rec, img, fid = driver(verts, faces, cam, 48, RC.TWO_HAND, 1500)
    want = ref_vertex_records(verts, faces, cam, 48, RC.TWO_HAND, 1500)
    for name, cols in (("normal", slice(0, 3)), ("colour", slice(3, 6)), ("X", 6), ("Y", 7), ("1/z", 8)):
        assert np.array_equal(rec[:, cols], want[:, cols]), name
    assert (want[:, 6].view(np.int32) == R.BAD).any() and (want[:, 6].view(np.int32) != R.BAD).any()
    ri, rf = R.render_sample(verts, faces, cam, 48, RC.TWO_HAND, 1500)
    assert np.array_equal(img, ri) and np.array_equal(fid, rf)


@needs_gxx
def test_host_build_matches_the_restatement_on_a_triangle_soup_with_degenerate_faces(driver):
    """300 faces at S = 48 over a background: faces partly and wholly off screen, both windings, zero-area faces (a repeated vertex,
    three collinear vertices, three coincident ones), a face with one vertex in front of the near distance over the middle of the image."""
    rng = np.random.RandomState(2)
    cam = np.array([2.0, 0.05, -0.03], f32)                                          # t_z = 2.5
    centre = np.stack([rng.uniform(-0.7, 0.7, 290), rng.uniform(-0.7, 0.7, 290), rng.uniform(-1.5, 1.5, 290)], 1)
    off = rng.uniform(-0.1, 0.1, (290, 3, 3))
    centre[:12, 2], off[:12, :, :2] = -2.4, off[:12, :, :2] * 0.03               # twelve small faces across the near distance (z = 0.1 +- 0.1)
    verts = (centre[:, None, :] + off).reshape(-1, 3).astype(f32)                 # 290 small triangles of their own vertices
    faces = np.arange(870, dtype=np.int32).reshape(290, 3)
    p = lambda col, row, z: [(col - 24) / 120.0 * (z + 2.5) - 0.05, (row - 24) / 120.0 * (z + 2.5) + 0.03, z]      # projects to (col, row): F = 120, t_z = 2.5
    extra_v = np.array([p(10, 10, 0), p(30, 10, 0), p(20, 30, 0),              # 870..872: a plain face in view
                        p(5, 40, 0), p(15, 40, 0), p(25, 40, 0),               # 873..875: collinear
                        p(24, 20, -2.45), p(10, 35, 0.2), p(40, 35, 0.2)], f32)  # 876..878: 876 lies at z = 0.05 < 0.1
    extra_f = np.array([[870, 871, 872], [870, 872, 871], [870, 870, 871], [873, 874, 875], [872, 872, 872], [876, 877, 878],
                        [871, 870, 872], [877, 878, 872], [878, 877, 872], [870, 871, 872]], np.int32)
    verts, faces = np.concatenate([verts, extra_v]), np.concatenate([faces, extra_f])
    assert faces.shape[0] == 300
    bg = RC.background(1, 48, 5)[0]
    rec, img, fid = driver(verts, faces, cam, 48, RC.TWO_HAND, 150, bg=bg)
    ri, rf = R.render_sample(verts, faces, cam, 48, RC.TWO_HAND, 150, background=bg)
    assert np.array_equal(rec, ref_vertex_records(verts, faces, cam, 48, RC.TWO_HAND, 150))
    assert np.array_equal(img, ri) and np.array_equal(fid, rf)
    for f in (292, 293, 294, 295):                                             # the zero-area faces and the face behind the near distance draw nothing
        assert not (rf == f).any(), f
    assert 0.05 < (rf >= 0).mean() < 0.98 and np.array_equal(ri[rf < 0], bg[rf < 0])


@needs_gxx
def test_host_build_matches_the_restatement_on_the_synthetic_hands(driver):
    f = RC.faces()
    sc = RC.scene("s64")
    want_img, want_ids = RC.reference("s64")
    for b in range(3):
        rec, img, fid = driver(sc["verts"][b], f, sc["cam"][b], 64, sc["albedo"][b], RC.SPLIT, sc["present"][b], sc["bg"][b])
        assert np.array_equal(rec, ref_vertex_records(sc["verts"][b], f, sc["cam"][b], 64, sc["albedo"][b], RC.SPLIT)), b
        assert np.array_equal(img, want_img[b]) and np.array_equal(fid, want_ids[b]), b


@needs_gxx
def test_host_keypoints_match_the_restatement(driver):
    S, K = 40, 9
    rng = np.random.RandomState(3)
    kps = rng.uniform(-1.1, 1.1, (K, 2)).astype(f32)
    kps[0], kps[1], kps[2] = (-1.0, -1.0), (0.999, 0.2), (0.1, 0.1)
    kps[3] = kps[2] + f32(2.0 / S)                                            # overlaps the one before: the later one wins
    w = np.ones(K, f32)
    w[4], w[5] = 0.0, -1.0
    img = RC.background(1, S, 8)[0]
    raw = driver.raw("keypoints", b"".join([np.array([S, K], np.int32).tobytes(), bytes([7, 200, 90, 0]), kps.tobytes(), w.tobytes(), img.tobytes()]))
    got = np.frombuffer(raw, np.uint8).reshape(S, S, 3)
    assert np.array_equal(got, R.draw_keypoints(img.copy(), kps, w, (7, 200, 90)))


# ------------------------------------------------------------------------------------------------------------------ known answers
def grid_verts(cols, rows, z, S=64):
    """Model-space vertices that project exactly onto (col, row) (in pixels, multiples of 1/256) at model depth z, under CAM_KA."""
    cols, rows, z = np.broadcast_arrays(np.asarray(cols, np.float64), np.asarray(rows, np.float64), np.asarray(z, np.float64))
    F, half = 0.5 * S * 5.0, 0.5 * S
    return np.stack([(cols - half) / F * (z + 1.0), (rows - half) / F * (z + 1.0), z], -1).astype(f32)


CAM_KA = np.array([5.0, 0.0, 0.0], f32)                                         # t_z = 1


def draw(verts, faces, S=64, split=None, light=None, albedo=GREY, present=(1, 1)):
    return R.render_sample(verts, np.asarray(faces, np.int64), CAM_KA, S, albedo, len(faces) if split is None else split, present, None, None, light)


def test_projection_lands_on_the_grid():
    v = grid_verts([10, 20.5, 63.99609375], [12, 0.00390625, 31], [0.0, 0.5, -0.25])
    X, Y, iz, ok = R.project(R.translate(v, CAM_KA), 64)
    assert ok.all() and X.tolist() == [2560, 5248, 16383] and Y.tolist() == [3072, 1, 7936]
    assert np.array_equal(iz, f32(1) / np.array([1.0, 1.5, 0.75], f32))
    # the snap is numpy's rint: exact ties go to the even neighbour
    assert np.rint(np.array([0.5, 1.5, 2.5], f32)).tolist() == [0.0, 2.0, 2.0]


@pytest.mark.parametrize("order", [((0, 1, 2), (0, 2, 3)), ((0, 2, 1), (0, 3, 2)), ((1, 2, 3), (1, 3, 0)), ((0, 1, 2), (3, 2, 0))])
def test_square_on_pixel_centres_covers_what_the_top_left_rule_gives(order):
    """Corners (10,12), (20,12), (20,25), (10,25): the top row and the left column belong to the square, the bottom row and the right
    column do not -- whichever diagonal splits it and whichever way the triangles wind."""
    v = grid_verts([10, 20, 20, 10], [12, 12, 25, 25], 0.0)
    _, ids = draw(v, order)
    want = np.zeros((64, 64), bool)
    want[12:25, 10:20] = True
    assert np.array_equal(ids >= 0, want)


def test_two_triangles_of_a_quad_cover_every_pixel_once():
    """200 random convex quads with corners on the 1/256 grid, split along a diagonal: no pixel of the interior is missed, none is
    covered by both triangles (the pixels ON the shared diagonal are the ones at stake)."""
    rng = np.random.RandomState(7)
    S, doubles, holes, on_diagonal, n = 48, 0, 0, 0, 0
    ones = np.ones(4, f32)
    col = np.zeros((4, 3), f32)
    py, px = np.mgrid[0:S, 0:S].astype(np.int64) * 256
    while n < 200:
        if n % 2:                    # corners on whole pixels: the diagonal passes through many pixel centres
            q = rng.randint(2, S - 2, (4, 2)).astype(np.int64) * 256
        else:
            q = rng.randint(2 * 256, (S - 2) * 256, (4, 2)).astype(np.int64)
        c = q.mean(0)
        q = q[np.argsort(np.arctan2(q[:, 1] - c[1], q[:, 0] - c[0]))]
        e = np.roll(q, -1, 0) - q
        cr = e[:, 0] * np.roll(e, -1, 0)[:, 1] - e[:, 1] * np.roll(e, -1, 0)[:, 0]
        if not ((cr > 0).all() or (cr < 0).all()):
            continue
        n += 1
        X, Y = q[:, 0].astype(np.int32), q[:, 1].astype(np.int32)
        if n % 4 < 2:
            X, Y = X[::-1].copy(), Y[::-1].copy()                                 # the other winding
        _, a = R.rasterise(X, Y, ones, col, np.array([[0, 1, 2]]), S)
        _, b = R.rasterise(X, Y, ones, col, np.array([[0, 2, 3]]), S)
        _, both = R.rasterise(X, Y, ones, col, np.array([[0, 1, 2], [0, 2, 3]]), S)
        cnt = (a >= 0).astype(int) + (b >= 0)
        inside = np.ones((S, S), bool)
        s = 1 if cr[0] > 0 else -1
        for k in range(4):
            x0, y0, x1, y1 = int(q[k, 0]), int(q[k, 1]), int(q[(k + 1) % 4, 0]), int(q[(k + 1) % 4, 1])
            inside &= s * ((x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)) > 0
        doubles += int((cnt == 2).sum())
        holes += int((inside & (cnt == 0)).sum())
        on_diagonal += int((inside & ((int(X[2]) - int(X[0])) * (py - int(Y[0])) == (int(Y[2]) - int(Y[0])) * (px - int(X[0])))).sum())
        assert np.array_equal(both >= 0, cnt > 0)
    assert on_diagonal >= 100, on_diagonal            # the tie rule was really asked: one pixel per whole-pixel quad on average
    assert doubles == 0 and holes == 0, (doubles, holes)


def test_nearer_triangle_hides_the_farther_one_in_either_order():
    near = grid_verts([10, 40, 20], [10, 15, 40], 0.0)
    far = grid_verts([12, 45, 15], [8, 30, 45], 0.5)
    for v, f_near in ((np.concatenate([near, far]), 0), (np.concatenate([far, near]), 1)):
        _, ids = draw(v, [[0, 1, 2], [3, 4, 5]])
        _, only_near = draw(v, [[0, 1, 2], [3, 4, 5]][f_near:f_near + 1])
        _, only_far = draw(v, [[0, 1, 2], [3, 4, 5]][1 - f_near:2 - f_near])
        overlap = (only_near >= 0) & (only_far >= 0)
        assert overlap.sum() > 100 and (ids[overlap] == f_near).all()
        assert (ids[(only_far >= 0) & ~overlap] == 1 - f_near).all()


def test_identical_triangles_the_lower_index_wins():
    v = grid_verts([10, 40, 20], [10, 15, 40], [0.0, 0.3, -0.2])
    _, ids = draw(v, [[0, 1, 2], [0, 1, 2], [0, 1, 2]])
    assert (ids >= 0).sum() > 100 and set(np.unique(ids)) == {-1, 0}
    _, ids = draw(v, [[2, 0, 1], [0, 1, 2]], split=1, present=(0, 1))            # with face 0's hand not drawn, face 1 shows
    assert set(np.unique(ids)) == {-1, 1}


def test_one_lit_face_has_the_hand_computed_colour():
    """A fronto-parallel face whose normal points at the camera, one white light far away on that normal, the two others dark: n . l is 1
    to within a float32 rounding at every vertex, so the colour is the albedo: (0.5, 0.25, 0.75) * 255 = 127.5, 63.75, 191.25 -> 127, 63, 191
    (the bytes keep a distance of 0.25 or more from the next integer: 1e-6 of rounding cannot move them)."""
    v = grid_verts([10, 20, 40], [10, 40, 15], 0.0)                              # (v1 - v0) x (v2 - v0) points to -z, towards the camera
    n = R.vertex_normals(v, np.array([[0, 1, 2]]))
    assert np.array_equal(n, np.tile(np.array([0, 0, -1], f32), (3, 1)))
    light = (np.array([[0, 0, -1.0e6], [0, 0, 0], [0, 0, 0]], f32), np.array([[1, 1, 1], [0, 0, 0], [0, 0, 0]], f32))
    albedo = np.array([[0.5, 0.25, 0.75], [0, 0, 0]], f32)
    img, ids = draw(v, [[0, 1, 2]], light=light, albedo=albedo)
    assert (ids == 0).sum() > 100
    assert {tuple(c) for c in img[ids == 0].tolist()} == {(127, 63, 191)}
    assert (img[ids < 0] == 255).all()                                          # no background: white
    # the same face seen from behind (no back-face culling): the normal points away from the light, the face is drawn black
    img, ids = draw(v, [[0, 2, 1]], light=light, albedo=albedo)
    assert {tuple(c) for c in img[ids == 0].tolist()} == {(0, 0, 0)}


def test_keypoint_disc_is_the_3_3_2_1_table_and_is_clipped_at_a_corner():
    S = 32
    img = np.zeros((S, S, 3), np.uint8)
    kp = np.array([[0.0, 0.0]], f32)                                             # centre (16, 16)
    R.draw_keypoints(img, kp, np.ones(1, f32), (1, 2, 3))
    want = np.zeros((S, S), bool)
    for dy, hw in ((-3, 1), (-2, 2), (-1, 3), (0, 3), (1, 3), (2, 2), (3, 1)):
        want[16 + dy, 16 - hw:16 + hw + 1] = True
    assert np.array_equal(img[..., 0] == 1, want) and np.array_equal(img[..., 2] == 3, want) and want.sum() == 37
    img = np.zeros((S, S, 3), np.uint8)
    R.draw_keypoints(img, np.array([[-1.0, -1.0], [0.97, 1.0], [0.5, 0.5]], f32), np.array([1, 1, 0], f32), (9, 9, 9))
    corner = np.zeros((S, S), bool)
    for dy, hw in ((0, 3), (1, 3), (2, 2), (3, 1)):
        corner[dy, 0:hw + 1] = True
    assert np.array_equal(img[:8, :8, 0] == 9, corner[:8, :8])
    low = img[:, :, 0] == 9
    assert low[S - 3:, 28:].any() and low.sum() == corner.sum() + low[S - 3:, :].sum()   # centre row 32 lies below the image: only its rows dy = -3..-1 are inside
    assert not low[12:28, 12:28].any()                                           # the keypoint of weight 0 is not drawn


# ------------------------------------------------------------------------------------------------------------------ fixture replay
def test_host_scene_setup_reproduces_what_the_reference_handed_to_opendr():
    """tests/golden/render.npz: the reference's own render_together / render_mesh_to_image ran on four seeded cases with recording
    stand-ins for OpenDR's classes.  This build's host half gives the same camera, translated vertices, faces, albedo, lights and
    background: floats to float64 rounding (4 ulp of the largest magnitude), integers and shapes exactly."""
    from ihmr_amd import render
    g = np.load(os.path.join(ROOT, "tests", "golden", "render.npz"))
    fr, fl = g["faces_right"].astype(np.int64), g["faces_left"].astype(np.int64)

    def close(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        assert np.all(np.abs(a.astype(np.float64) - b) <= 4 * np.finfo(np.float64).eps * max(1.0, float(np.abs(b).max()))), what

    for k in range(4):
        cam = g[f"c{k}_in_cam"]
        if k < 2:
            img = g["c0_in_img"] if k == 0 else None
            sc = render.scene_together([g[f"c{k}_in_verts_right"], g[f"c{k}_in_verts_left"]], [fr, fl], [g[f"c{k}_in_color0"], g[f"c{k}_in_color1"]], cam, 64, img)
        else:
            sc = render.scene_single(64, g[f"c{k}_in_image"], cam, g[f"c{k}_in_vert"], fr if k == 2 else fl)
        F, c, cam_t, (lpos, lcol) = render.scene_setup(cam, 64)
        close(F, g[f"c{k}_f"], "f"), close(c, g[f"c{k}_c"], "c")
        close(sc["f"], g[f"c{k}_f"], "f"), close(sc["c"], g[f"c{k}_c"], "c")
        assert sc["width"] == int(g[f"c{k}_width"]) == 64 and sc["height"] == int(g[f"c{k}_height"]) == 64
        close(sc["v"], g[f"c{k}_v"], "v")
        assert np.array_equal(np.asarray(sc["faces"], np.int64), g[f"c{k}_faces"].astype(np.int64))
        close(sc["vc"], g[f"c{k}_vc"], "vc")
        close(sc["light_pos"], g[f"c{k}_light_pos"], "light_pos"), close(lpos, g[f"c{k}_light_pos"], "light_pos")
        close(sc["light_color"], g[f"c{k}_light_color"], "light_color")
        close(sc["background"], g[f"c{k}_background"], "background")
        assert not g[f"c{k}_rt"].any() and not g[f"c{k}_t"].any() and (g[f"c{k}_bgcolor"] == 1).all()
        # the cast this build makes: the lights as float32 are the restatement's table; the merged face table is the renderer's
        pos32, col32 = R.lights()
        assert np.array_equal(pos32, g[f"c{k}_light_pos"].astype(f32)) and np.array_equal(col32, g[f"c{k}_light_color"].astype(f32))
    r = render.MeshRenderer(fr, fl)
    assert np.array_equal(r.faces, g["c0_faces"]) and r.face_split == 1538 and r.n_verts == 1556
    off, ids = R.build_csr(g["c0_faces"], 1556)
    assert np.array_equal(r.csr_offsets, off) and np.array_equal(r.csr_ids, ids)
    assert np.allclose(np.asarray(render.COLORS["light_green"]), g["c0_in_color0"][0]) and np.allclose(render.SINGLE_HAND_COLOR, g["c2_vc"])
    assert np.array_equal(RC.TWO_HAND, np.concatenate([g["c0_in_color0"], g["c0_in_color1"]]).astype(f32))


def test_recover_img_follows_the_reference():
    from ihmr_amd import render
    import torch
    g = np.load(os.path.join(ROOT, "tests", "golden", "render.npz"))
    chw = g["c2_in_image"]
    got = render.recover_img(torch.from_numpy(chw))
    assert got.shape == (64, 64, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ((chw + 1) * 0.5 * 255).transpose(1, 2, 0).astype(np.uint8))
    assert np.array_equal(render.recover_img(g["c3_in_image"]), g["c3_in_image"])


def test_product_renderer_raises_without_a_gpu(monkeypatch):
    import torch
    from ihmr_amd import render
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    fr, fl = RC.hand_faces()
    r = render.MeshRenderer(fr, fl)
    with pytest.raises(RuntimeError):
        r.render(torch.zeros(1, 778, 3), torch.zeros(1, 778, 3), torch.ones(1, 3), size=64)
    with pytest.raises(RuntimeError):
        render.draw_keypoints(np.zeros((64, 64, 3), np.uint8), np.zeros((2, 2), f32), np.ones((2, 1), f32), "red", 64)


# ------------------------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("name", RC.TWO_HAND_SCENES)
def test_two_hand_scenes_cover_the_image_and_overlap(name):
    """Asserted on the restatement, not on the kernel: in every two-hand sample the meshes cover 5-60 % of the pixels and at least 1 %
    of the covered pixels lie where both hands project -- there the depth test decides."""
    sc = RC.scene(name)
    _, ids = RC.reference(name)
    seen = 0
    for b in range(ids.shape[0]):
        cov = (ids[b] >= 0).mean()
        assert 0.05 <= cov <= 0.60, (name, b, cov)
        if sc["present"][b].all():
            right, left = RC.hand_masks(name, b)
            both = (right & left).sum() / (ids[b] >= 0).sum()
            print(f"[scene] {name}[{b}]: {cov:.3f} covered, {both:.3f} of it under both hands")
            assert both >= 0.01, (name, b, both)
            assert (ids[b][right & left] < RC.SPLIT).any() and (ids[b][right & left] >= RC.SPLIT).any()   # each hand wins somewhere
            seen += 1
    assert seen >= 1


def test_extreme_scenes_reach_what_they_are_for():
    # one tile: every usable vertex of both hands inside tile 0 of the 96-pixel image, so each of the 13 chunks keeps all its faces
    sc = RC.scene("one_tile")
    for b in range(2):
        X, Y, _, ok = R.project(R.translate(sc["verts"][b], sc["cam"][b]), 96)
        assert ok.all() and X.min() >= 0 and X.max() <= 31 * 256 and Y.min() >= 0 and Y.max() <= 31 * 256
    assert (RC.reference("one_tile")[1] >= 0).any()
    # oversize: sample 0 fills most of the image and loses part of its vertices to the near distance; sample 1 loses all of them;
    # sample 2 has projections on both sides of 16384 pixels
    sc = RC.scene("oversize")
    _, ids = RC.reference("oversize")
    p = [R.translate(sc["verts"][b], sc["cam"][b]) for b in range(3)]
    assert (ids[0] >= 0).mean() > 0.9 and 0 < (p[0][:, 2] < 0.1).sum() < 1556
    assert (p[1][:, 2] < 0.1).all() and (ids[1] < 0).all()
    ok2 = R.project(p[2], 64)[3]
    assert (p[2][:, 2] >= 0.1).all() and 0 < ok2.sum() < 1556 and (ids[2] < 0).all()
    for name in ("bad_cam0", "bad_cam_neg", "bad_cam_nan"):
        img, ids = RC.reference(name)
        assert (ids[1] < 0).all() and np.array_equal(img[1], RC.scene(name)["bg"][1]) and (ids[0] >= 0).any() and (ids[2] >= 0).any()

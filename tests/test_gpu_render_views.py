"""Rotated views, per-vertex colours and the penetration heat map of the mesh renderer on the GPU (``ihmr_view_vertices``,
``ihmr_heat_colours``, ``ihmr_paint_meshes``; ``MeshRenderer.render(view=, pivot=, vertex_colors=, return_alpha=)``, ``render_views``,
``penetration_colors``, ``rotated``, ``Evaluator.visualize_result(views=, collision_map=)``) against the numpy restatement
``tests/render_views_ref.py``: vertices, colours, image bytes and face ids bit for bit.  tests/test_render_views_cpu.py checks on the CPU
that the scenes and depths used here exercise what they are meant to."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_cases as RC  # noqa: E402
import render_ref as R  # noqa: E402
import render_views_ref as V  # noqa: E402
from guarded import Guarded, assert_guards  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
LO, HI = f32(0.0), f32(0.005)
HOT = np.array([0, 0, 1], f32)
PRESENT = ((1, 1), (1, 0), (0, 1), (0, 0))


@pytest.fixture(scope="module")
def renderer():
    from ihmr_amd import render
    fr, fl = RC.hand_faces()
    return render.MeshRenderer(fr, fl)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gptr(g):
    return C.c_void_p(g.data_ptr)


def guarded_copy(a):
    t = up(a)
    g = Guarded(t.numel() * t.element_size())
    g.copy_in(t)
    return g


def edge_depths(lo=LO, hi=HI):
    up_, down = lambda x: np.nextafter(f32(x), f32(np.inf)), lambda x: np.nextafter(f32(x), f32(-np.inf))
    return np.array([-1.0, -1e-3, -0.0, 0.0, lo, up_(lo), down(lo), hi, up_(hi), down(hi), 0.5 * (lo + hi), 0.001, 0.0049, 0.01, 1.0, 3e38,
                     np.nan, np.inf, -np.inf, 1e-45, -1e-45], f32)


# ------------------------------------------------------------------------------------------------------------------ ihmr_view_vertices
def view_vertices(verts, present, n_split, rot, pivot):
    """The entry point on guarded buffers: verts (B,nV,3), present (B,2) or None, rot (3,3) or (B,3,3), pivot (B,3) or None."""
    from ihmr_amd import hip
    B, nV = verts.shape[:2]
    g = dict(verts=guarded_copy(verts), rot=guarded_copy(rot), out=Guarded(B * nV * 12, fill=0xFF))
    if present is not None:
        g["present"] = guarded_copy(np.asarray(present, np.uint8))
    if pivot is not None:
        g["pivot"] = guarded_copy(pivot)
    hip.check(hip.lib().ihmr_view_vertices(gptr(g["verts"]), gptr(g["present"]) if present is not None else None, nV, n_split, gptr(g["rot"]),
                                           int(rot.ndim == 3), gptr(g["pivot"]) if pivot is not None else None, gptr(g["out"]), B,
                                           hip.stream_ptr()), "ihmr_view_vertices")
    torch.cuda.synchronize()
    assert_guards(g, "ihmr_view_vertices")
    assert np.array_equal(g["verts"].view(torch.float32, verts.shape).cpu().numpy().view(np.uint32), verts.view(np.uint32))   # the input is only read
    return g["out"].view(torch.float32, (B, nV, 3)).cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_verts", [1, 63, 64, 65, 257, 1556])
def test_view_vertices_match_the_restatement_bit_for_bit(n_verts, B):
    """One vertex, one short of a wave, a wave, one more, one more than the workgroup, the two hands: every pattern of drawn hands, the
    matrix shared and per sample, the pivot given and taken from the bounding box (with NaN / Inf vertices that must not count)."""
    rng = np.random.RandomState(100 * n_verts + B)
    n_split = (n_verts + 1) // 2
    verts = (rng.normal(0, 0.1, (B, n_verts, 3)) + rng.uniform(-0.5, 0.5, (B, 1, 3))).astype(f32)
    if n_verts >= 63:
        for b in range(B):
            verts[b, rng.choice(n_verts, 9, replace=False), rng.randint(0, 3, 9)] = np.array([np.nan, np.inf, -np.inf] * 3, f32)
            verts[b, np.argmax(np.where(np.isfinite(verts[b, :, 0]), verts[b, :, 0], -9)), 2] = np.inf    # the vertex of the x maximum does not count
    views = [V.VIEWS[(b + n_verts) % 5] for b in range(B)]
    rots = np.stack([V.view_rotation(*v) for v in views]).astype(f32)
    given = rng.uniform(-0.3, 0.3, (B, 3)).astype(f32)
    for k in range(4):
        present = np.array([PRESENT[(k + b) % 4] for b in range(B)], np.uint8)
        for per_sample in (0, 1):
            for pivot in (None, given):
                got = view_vertices(verts, None if (k == 0 and B == 1) else present, n_split, rots if per_sample else rots[0], pivot)
                pres = np.ones((B, 2), np.uint8) if (k == 0 and B == 1) else present
                for b in range(B):
                    c = V.bbox_mid(verts[b], n_split, pres[b]) if pivot is None else pivot[b]
                    want = V.view_points(verts[b], c, rots[b if per_sample else 0])
                    assert same_bits(got[b], want), (n_verts, B, k, per_sample, pivot is None, b)
    if B == 3:                                                                   # a permuted batch gives the permuted result
        present = np.array(PRESENT[:3], np.uint8)
        a = view_vertices(verts, present, n_split, rots, None)
        perm = [2, 0, 1]
        b_ = view_vertices(verts[perm], present[perm], n_split, rots[perm], None)
        assert same_bits(b_, a[perm])


def test_view_vertices_refuses_in_place_and_overlapping_output():
    from ihmr_amd import hip
    v = torch.zeros(2, 100, 3, device="cuda")
    rot = torch.eye(3, device="cuda")
    L = hip.lib()
    assert L.ihmr_view_vertices(hip.ptr(v), None, 100, 50, hip.ptr(rot), 0, None, hip.ptr(v), 2, hip.stream_ptr()) == -1
    assert L.ihmr_view_vertices(hip.ptr(v), None, 100, 50, hip.ptr(rot), 0, None, C.c_void_p(v.data_ptr() + 1200), 1, hip.stream_ptr()) == 0
    assert L.ihmr_view_vertices(hip.ptr(v), None, 100, 50, hip.ptr(rot), 0, None, C.c_void_p(v.data_ptr() + 1196), 1, hip.stream_ptr()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ views
def run(renderer, sc, **kw):
    v = up(sc["verts"])
    out = renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]), kw.pop("background", None), present=up(sc["present"]),
                          colors=up(sc["albedo"]), return_face_ids=True, size=sc["S"], **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def check_view(name, view, got_img, got_ids):
    want_img, want_ids = V.view_reference(name, view)
    bad_ids, bad_px = int((got_ids != want_ids).sum()), int((got_img != want_img).any(-1).sum())
    print(f"[views] {name} {view}: {want_ids.size} pixels, {int((want_ids >= 0).sum())} covered, {bad_ids} ids differ, {bad_px} pixels differ")
    assert bad_ids == 0 and bad_px == 0, (name, view, bad_ids, bad_px)


@pytest.mark.parametrize("view", V.VIEWS)
@pytest.mark.parametrize("name", ["s64", "s50", "deep"])
def test_rotated_views_match_the_restatement_bit_for_bit(renderer, name, view):
    """s64 / s50 (S no multiple of the tile): both hands, right only, left only -- the pivot follows the hands that are drawn; deep:
    four interpenetrating pairs.  The view is given as an (axis, degrees) pair, drawn on white."""
    check_view(name, view, *run(renderer, RC.scene(name), view=view))


def test_rotated_view_at_the_evaluators_size_and_over_a_background(renderer):
    sc = RC.scene("s448")
    img, ids = run(renderer, sc, view=("y", 90))
    check_view("s448", ("y", 90), img, ids)
    # the same view as a matrix, per sample, over the scene's background: the same faces, the background where there is none
    rot = np.repeat(V.view_rotation("y", 90)[None], 1, 0).astype(f32)
    img2, ids2 = run(renderer, sc, view=up(rot), background=up(sc["bg"]))
    assert np.array_equal(ids2, ids) and np.array_equal(img2[ids >= 0], img[ids >= 0]) and np.array_equal(img2[ids < 0], sc["bg"][ids < 0])


def test_no_view_is_the_call_without_the_argument_and_a_given_pivot_is_used(renderer):
    sc = RC.scene("s64")
    a = run(renderer, sc, background=up(sc["bg"]))
    b = run(renderer, sc, background=up(sc["bg"]), view=None, pivot=None, vertex_colors=None, return_alpha=False)
    assert len(b) == 2 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], RC.reference("s64")[0]) and np.array_equal(a[1], RC.reference("s64")[1])
    pivot = np.array([[0.05, 0.0, 0.0], [0.1, 0.02, -0.01], [0.08, -0.02, 0.01]], f32)
    rot = V.view_rotation("y", 90)
    img, ids = run(renderer, sc, view=rot, pivot=up(pivot))
    f = RC.faces()
    for k in range(3):
        wi, wd = V.render_sample_view(sc["verts"][k], f, sc["cam"][k], 64, sc["albedo"][k], RC.SPLIT, 778, rot, pivot[k], sc["present"][k])
        assert np.array_equal(img[k], wi) and np.array_equal(ids[k], wd), k
    assert not np.array_equal(ids, V.view_reference("s64", ("y", 90))[1])
    with pytest.raises(ValueError):
        run(renderer, sc, pivot=up(pivot))
    with pytest.raises(ValueError):
        run(renderer, sc, view=np.eye(4))
    with pytest.raises(TypeError):
        v = up(sc["verts"])
        renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]), None, None, None, False, 64, ("y", 90))       # keyword only


def test_render_views_stacks_the_camera_view_over_the_background_and_the_others_on_white(renderer):
    sc = RC.scene("s64")
    v = up(sc["verts"])
    views = [None, ("y", 90), ("x", 90)]
    out = renderer.render_views(v[:, :778], v[:, 778:], up(sc["cam"]), views, up(sc["bg"]), present=up(sc["present"]), colors=up(sc["albedo"]))
    assert out.shape == (3, 3, 64, 64, 3) and out.dtype == torch.uint8
    out = out.cpu().numpy()
    assert np.array_equal(out[:, 0], RC.reference("s64")[0])
    for k in (1, 2):
        assert np.array_equal(out[:, k], V.view_reference("s64", views[k])[0]), k


# ------------------------------------------------------------------------------------------------------------------ ihmr_paint_meshes
@pytest.mark.parametrize("name", RC.TWO_HAND_SCENES)
def test_hand_colours_expanded_per_vertex_give_the_bytes_of_the_plain_render(renderer, name):
    sc = RC.scene(name)
    vc = np.repeat(sc["albedo"], 778, axis=1)
    assert vc.shape == (sc["verts"].shape[0], 1556, 3)
    img, ids = run(renderer, sc, background=None if sc["bg"] is None else up(sc["bg"]), vertex_colors=up(vc))
    want_img, want_ids = RC.reference(name)
    assert np.array_equal(img, want_img) and np.array_equal(ids, want_ids)


@pytest.mark.parametrize("name", ["s50", "deep"])
def test_random_vertex_colours_match_the_restatement_inside_guards(renderer, name):
    from ihmr_amd import hip
    from ihmr_amd.render import _lights_struct
    sc = RC.scene(name)
    B, S = sc["verts"].shape[0], sc["S"]
    vc = np.random.RandomState(31).uniform(0, 1, (B, 1556, 3)).astype(f32)
    g = dict(verts=guarded_copy(sc["verts"]), vc=guarded_copy(vc), cam=guarded_copy(sc["cam"]), present=guarded_copy(sc["present"]),
             bg=guarded_copy(sc["bg"]), img=Guarded(B * S * S * 3, fill=0x5A), ids=Guarded(B * S * S * 4, fill=0x5A))
    L = hip.lib()
    g["ws"] = Guarded(L.ihmr_render_workspace_bytes(B, 1556), fill=0xFF)
    faces, off, ids = renderer._tables(torch.device("cuda", torch.cuda.current_device()))
    lights = _lights_struct()
    hip.check(L.ihmr_paint_meshes(gptr(g["verts"]), hip.ptr(faces), hip.ptr(off), hip.ptr(ids), 1556, 3076, 1538, gptr(g["present"]), gptr(g["vc"]),
                                  gptr(g["cam"]), C.byref(lights), gptr(g["bg"]), S, gptr(g["img"]), gptr(g["ids"]), gptr(g["ws"]), B,
                                  hip.stream_ptr()), "ihmr_paint_meshes")
    torch.cuda.synchronize()
    assert_guards(g, "ihmr_paint_meshes")
    img = g["img"].view(torch.uint8, (B, S, S, 3)).cpu().numpy()
    fid = g["ids"].view(torch.int32, (B, S, S)).cpu().numpy()
    f = RC.faces()
    for b in range(B):
        wi, wd = V.render_sample_painted(sc["verts"][b], f, sc["cam"][b], S, vc[b], RC.SPLIT, sc["present"][b], sc["bg"][b])
        assert np.array_equal(fid[b], wd) and np.array_equal(img[b], wi), (name, b)
    assert np.array_equal(fid, RC.reference(name)[1]) and not np.array_equal(img, RC.reference(name)[0])


# ------------------------------------------------------------------------------------------------------------------ ihmr_heat_colours
@pytest.mark.parametrize("layout", [0, 1])
def test_heat_colours_at_the_edge_depths_inside_guards(layout):
    """Depths below, at and next to lo and hi, NaN and the infinities at both ends of both halves of a (3,1556) table, three ranges."""
    from ihmr_amd import hip
    rng = np.random.RandomState(41)
    albedo = np.stack([RC.TWO_HAND, RC.TWO_HAND[::-1], rng.uniform(0, 1, (2, 3)).astype(f32)])
    for lo, hi in ((LO, HI), (f32(0.001), f32(0.0035)), (f32(-0.002), f32(1e-3))):
        e = edge_depths(lo, hi)
        half = np.concatenate([e, rng.uniform(-0.002, 0.008, 778 - 2 * len(e)).astype(f32), e[::-1]])
        depth = np.stack([np.concatenate([half, half[::-1]]), np.concatenate([half[::-1], half]), rng.permutation(np.concatenate([half, half]))])
        g = dict(depth=guarded_copy(depth), albedo=guarded_copy(albedo), out=Guarded(3 * 1556 * 12, fill=0xFF))
        hot = (C.c_float * 3)(*HOT)
        hip.check(hip.lib().ihmr_heat_colours(gptr(g["depth"]), gptr(g["albedo"]), hot, float(lo), float(hi), 1556, 778, layout, gptr(g["out"]), 3,
                                              hip.stream_ptr()), "ihmr_heat_colours")
        torch.cuda.synchronize()
        assert_guards(g, "ihmr_heat_colours")
        got = g["out"].view(torch.float32, (3, 1556, 3)).cpu().numpy()
        for b in range(3):
            assert same_bits(got[b], V.heat_colours(depth[b], albedo[b], HOT, lo, hi, 778, layout)), (layout, lo, hi, b)


def test_penetration_colors_binding_and_refusals():
    from ihmr_amd import render
    depth = np.zeros((2, 1556), f32)
    depth[0, 5], depth[1, 778 + 7] = 0.01, 0.0025
    c = render.penetration_colors(up(depth)).cpu().numpy()
    want = np.repeat(RC.TWO_HAND, 778, 0)
    assert same_bits(c[0, 778 + 5], HOT) and same_bits(np.delete(c[0], 778 + 5, 0), np.delete(want, 778 + 5, 0))      # the OTHER hand's vertex 5
    assert same_bits(c[1], V.heat_colours(depth[1], RC.TWO_HAND, HOT, LO, HI, 778, 1)) and not same_bits(c[1, 7], want[7])
    c = render.penetration_colors(up(depth), colors=up(RC.TWO_HAND[::-1].copy()), hot=(1, 0, 0), lo=0.001, hi=0.02, layout="vertex").cpu().numpy()
    assert same_bits(c[0], V.heat_colours(depth[0], RC.TWO_HAND[::-1], (1, 0, 0), 0.001, 0.02, 778, 0))
    for kw in (dict(lo=0.005, hi=0.005), dict(lo=0.01), dict(hi=float("nan")), dict(hi=float("inf")), dict(layout="other")):
        with pytest.raises(ValueError):
            render.penetration_colors(up(depth), **kw)
    with pytest.raises(ValueError):
        render.penetration_colors(up(depth[:, :1555]))                            # the collision layout needs two equal halves


def test_collision_depths_painted_front_and_turned_match_the_restatement(renderer):
    """The (4,1556) origin_scale table of SDFLoss on the deep-overlap hands -> penetration_colors -> rendered in the camera's view over
    the background and turned by 90 degrees about y on white, against the restatement fed the same depths."""
    from ihmr_amd import render
    from ihmr_amd.assets import synthetic_mano
    from ihmr_amd.sdf import SDFLoss
    sc, f = RC.scene("deep"), RC.faces()
    right, left = synthetic_mano(True), synthetic_mano(False)
    hv = up(sc["verts"]).reshape(4, 2, 778, 3)
    _, _, osc = SDFLoss(right["faces"], left["faces"]).cuda()(hv, return_per_vert_loss=True, return_origin_scale_loss=True)
    assert osc.shape == (4, 1556)
    depth = osc.detach().cpu().numpy()
    paint = render.penetration_colors(osc.detach(), up(sc["albedo"]))
    got = paint.cpu().numpy()
    v = up(sc["verts"])
    args = (v[:, :778], v[:, 778:], up(sc["cam"]))
    front, fid = renderer.render(*args, up(sc["bg"]), colors=up(sc["albedo"]), vertex_colors=paint, return_face_ids=True)
    side, sid = renderer.render(*args, None, colors=up(sc["albedo"]), vertex_colors=paint, return_face_ids=True, size=64, view=("y", 90))
    front, fid, side, sid = (t.cpu().numpy() for t in (front, fid, side, sid))
    rot = V.view_rotation("y", 90)
    for b in range(4):
        vc = V.heat_colours(depth[b], sc["albedo"][b], HOT, LO, HI, 778, 1)
        assert same_bits(got[b], vc), b
        assert ((depth[b] > 0) & (depth[b] < HI)).sum() >= 200 and (depth[b] >= HI).sum() >= 20       # ramp and saturation are reached
        wi, wd = V.render_sample_painted(sc["verts"][b], f, sc["cam"][b], 64, vc, RC.SPLIT, (1, 1), sc["bg"][b])
        assert np.array_equal(fid[b], wd) and np.array_equal(front[b], wi), b
        wi, wd = V.render_sample_view(sc["verts"][b], f, sc["cam"][b], 64, None, RC.SPLIT, 778, rot, vertex_albedo=vc)
        assert np.array_equal(sid[b], wd) and np.array_equal(side[b], wi), b
        flat = (front[b] != RC.reference("deep")[0][b]).any(-1).sum()
        flat_side = (side[b] != V.view_reference("deep", ("y", 90))[0][b]).any(-1).sum()
        print(f"[heat] deep[{b}]: {flat} pixels of the front view and {flat_side} of the turned view differ from the flat colours")
        assert flat >= 1 and flat_side >= 1, b
    assert np.array_equal(fid, RC.reference("deep")[1])


# ------------------------------------------------------------------------------------------------------------------ alpha
def test_alpha_is_where_a_face_is_visible(renderer):
    sc = RC.scene("s50")
    for kw in (dict(), dict(view=("x", 90))):
        img, ids, alpha = run(renderer, sc, return_alpha=True, **kw)
        assert alpha.dtype == np.uint8 and alpha.shape == ids.shape and np.array_equal(alpha, np.where(ids >= 0, 255, 0))
        assert 0 < (alpha == 255).mean() < 1
    v = up(sc["verts"])
    img2, alpha2 = renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]), present=up(sc["present"]), colors=up(sc["albedo"]), size=50,
                                   view=("x", 90), return_alpha=True)
    assert np.array_equal(alpha2.cpu().numpy(), alpha) and np.array_equal(img2.cpu().numpy(), img)


def test_rotated_follows_the_two_alpha_rules():
    """The single-sample numpy form: without an image alpha is 255 exactly where a face is visible (a white pixel of the hand stays
    opaque); with an image it is 255 everywhere."""
    from ihmr_amd import render
    sc = RC.scene("s64")
    fr, _ = RC.hand_faces()
    verts, cam, bg = sc["verts"][0, :778].astype(np.float64), sc["cam"][0].astype(np.float64), sc["bg"][0]
    one = np.array([render.SINGLE_HAND_COLOR] * 2, f32)
    for axis, deg in (("y", 90), ("x", -60), ("anything", 30)):
        rot = V.view_rotation(axis, deg)
        wi, wd = V.render_sample_view(verts.astype(f32), fr, cam.astype(f32), 64, one, fr.shape[0], 778, rot)
        got = render.rotated(verts, fr, deg, cam, 64, axis)
        assert got.shape == (64, 64, 4) and got.dtype == np.uint8
        assert np.array_equal(got[..., :3], wi) and np.array_equal(got[..., 3], np.where(wd >= 0, 255, 0))
        assert 0 < (wd >= 0).mean() < 1
        wi, _ = V.render_sample_view(verts.astype(f32), fr, cam.astype(f32), 64, one, fr.shape[0], 778, rot, background=bg)
        got = render.rotated(verts, fr, deg, cam, 64, axis, img=bg)
        assert np.array_equal(got[..., :3], wi) and (got[..., 3] == 255).all()
        assert np.array_equal(render.rotated(verts, fr, deg, cam, 64, axis, img=bg, do_alpha=False), wi)


# ------------------------------------------------------------------------------------------------------------------ visualize_result
def _evaluator(tmp_path, monkeypatch):
    from ihmr_amd import evaluator as E
    fr, fl = RC.hand_faces()
    ev = E.Evaluator(dict(right=types.SimpleNamespace(faces=fr), left=types.SimpleNamespace(faces=fl)))
    verts16 = RC.hand_verts().astype(np.float16)
    rng = np.random.RandomState(51)
    kinds = ("interacting", "right", "interacting", "left")
    cams = ([6.0, -0.0875, 0.0], [5.0, -0.07, 0.02], [5.5, -0.08, 0.01], [5.5, -0.09, -0.01])
    images = {}
    for k, ht in enumerate(kinds):
        path = f"/data/set{k}/cap/seq/cam/img{k}.png"
        images[path] = rng.randint(0, 256, ((200, 240), (224, 224), (256, 128), (224, 224))[k] + (3,)).astype(np.uint8)
        ev.pred_results.append(dict(img_path=path, hand_type=ht, pred_cam_params=np.array(cams[k], f32),
                                    pred_right_hand_verts=verts16[k, :778], pred_left_hand_verts=verts16[k, 778:],
                                    collision_loss_origin_scale=rng.uniform(-0.002, 0.008, 1556).astype(f32)))
    written = {}
    monkeypatch.setattr(E, "write_image_bgr", lambda path, img: written.__setitem__(path, np.array(img)))
    return ev, images, written


def test_visualize_result_stacks_views_and_the_collision_map(tmp_path, monkeypatch, renderer):
    """Four records (two interacting ones among them) in batches of three, at S = 224: image, the camera's view and the view turned by
    90 degrees about y stacked; the interacting samples painted from their own depth table, the others in their plain colour."""
    from ihmr_amd import render
    from ihmr_amd.preprocess import DataProcessor
    ev, images, written = _evaluator(tmp_path, monkeypatch)
    ev.visualize_result(str(tmp_path / "images"), str(tmp_path / "objs"), size_type="normalized", batch_size=3, image_loader=lambda p: images[p],
                        views=(("y", 90),), collision_map=True)
    assert len(written) == 4
    one = np.array([render.SINGLE_HAND_COLOR] * 2, f32)
    for k, r in enumerate(ev.pred_results):
        res = written[str(tmp_path / "images" / f"cap/seq/cam_img{k}.jpg")]
        assert res.shape == (3 * 224, 224, 3) and res.dtype == np.uint8
        img = DataProcessor(final_size=224)([images[r["img_path"]]], return_uint8=True)["img_uint8"]
        ht = r["hand_type"]
        inter = ht == "interacting"
        present = up(np.array([[1, 1] if inter else [ht == "right", ht == "left"]], np.uint8))
        colors = up(RC.TWO_HAND if inter else one)
        paint = render.penetration_colors(up(r["collision_loss_origin_scale"][None]), colors) if inter else None
        vr, vl = up(r["pred_right_hand_verts"].astype(f32))[None], up(r["pred_left_hand_verts"].astype(f32))[None]
        panels = renderer.render_views(vr, vl, up(r["pred_cam_params"])[None], [None, ("y", 90)], img, present=present, colors=colors,
                                       vertex_colors=paint)
        want = torch.cat([img[0], panels[0, 0], panels[0, 1]], dim=0).cpu().numpy()
        assert np.array_equal(res, want), (k, ht)
        flat = renderer.render_views(vr, vl, up(r["pred_cam_params"])[None], [None, ("y", 90)], img, present=present, colors=colors).cpu().numpy()[0]
        assert (res[224:448] != res[:224]).any() and (res[448:] != 255).any()
        assert ((res[224:448] != flat[0]).any() and (res[448:] != flat[1]).any()) == inter, (k, ht)


def test_visualize_result_with_the_defaults_is_the_call_without_the_new_arguments(tmp_path, monkeypatch):
    ev, images, written = _evaluator(tmp_path, monkeypatch)
    ev.visualize_result(str(tmp_path / "a"), str(tmp_path / "objs_a"), size_type="normalized", batch_size=3, image_loader=lambda p: images[p])
    first = {os.path.basename(k): v for k, v in written.items()}
    written.clear()
    ev.visualize_result(str(tmp_path / "b"), str(tmp_path / "objs_b"), size_type="normalized", batch_size=3, image_loader=lambda p: images[p],
                        views=(), collision_map=False, collision_range=(0.0, 0.005))
    second = {os.path.basename(k): v for k, v in written.items()}
    assert len(first) == 4 and sorted(first) == sorted(second)
    for k in first:
        assert first[k].shape == (448, 224, 3) and np.array_equal(first[k], second[k]), k
    # only the collision map: two panels, the interacting samples differ from the plain render, the others do not
    written.clear()
    ev.visualize_result(str(tmp_path / "c"), str(tmp_path / "objs_c"), size_type="normalized", batch_size=3, image_loader=lambda p: images[p],
                        collision_map=True)
    third = {os.path.basename(k): v for k, v in written.items()}
    for k, r in enumerate(ev.pred_results):
        name = f"cam_img{k}.jpg"
        assert third[name].shape == (448, 224, 3)
        assert np.array_equal(third[name], first[name]) == (r["hand_type"] != "interacting"), name

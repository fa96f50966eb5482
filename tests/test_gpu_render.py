"""The mesh renderer on the GPU (``ihmr_render_meshes``, ``ihmr_draw_keypoints``; ``ihmr_amd/render.py``, ``Evaluator.visualize_result``,
``get_current_visuals``) against the numpy restatement ``tests/render_ref.py``: image bytes and face ids bit for bit.  The scenes and
their references are those of ``tests/render_cases.py`` (computed once per process; tests/test_render_cpu.py checks on the CPU that
each scene exercises what it is meant to)."""
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

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def renderer():
    from ihmr_amd import render
    fr, fl = RC.hand_faces()
    return render.MeshRenderer(fr, fl)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(renderer, sc, verts=None, **kw):
    v = up(sc["verts"] if verts is None else verts)
    out, fid = renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]), None if sc["bg"] is None else up(sc["bg"]), present=up(sc["present"]),
                               colors=up(sc["albedo"]), return_face_ids=True, size=sc["S"], **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), fid.cpu().numpy()


def check(name, got_img, got_ids):
    want_img, want_ids = RC.reference(name)
    bad_ids, bad_px = int((got_ids != want_ids).sum()), int((got_img != want_img).any(-1).sum())
    print(f"[render] {name}: {want_ids.size} pixels, {int((want_ids >= 0).sum())} covered, {bad_ids} ids differ, {bad_px} pixels differ")
    assert bad_ids == 0 and bad_px == 0, (name, bad_ids, bad_px)


@pytest.mark.parametrize("name", ["s64", "s80", "s50", "s448", "deep", "one_tile", "oversize"])
def test_image_and_face_ids_match_the_restatement_bit_for_bit(renderer, name):
    """s64 / s80 / s50: both hands, right only, left only (s80 has partial tiles, s50 rows that are no multiple of the 12-byte run);
    s448 the evaluator's size; deep: interpenetrating hands; one_tile: all 3076 faces inside one tile, every chunk list full;
    oversize: hands larger than the image, vertices in front of the near distance and beyond +-16384 pixels."""
    check(name, *run(renderer, RC.scene(name)))


@pytest.mark.parametrize("name", ["bad_cam0", "bad_cam_neg", "bad_cam_nan"])
def test_a_sample_without_a_usable_camera_shows_its_background(renderer, name):
    sc = RC.scene(name)
    img, ids = run(renderer, sc)
    assert (ids[1] == -1).all() and np.array_equal(img[1], sc["bg"][1])
    check(name, img, ids)                                                        # the neighbours are what they are without it
    good = RC.reference("s64")
    assert np.array_equal(ids[0], good[1][0])                                    # sample 0 is sample 0 of s64 (another background)


def test_permuted_batch_gives_permuted_output_and_runs_repeat(renderer):
    sc = RC.scene("deep")
    a = run(renderer, sc)
    b = run(renderer, sc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    perm = [2, 0, 3, 1]
    scp = dict(sc, **{k: sc[k][perm] for k in ("verts", "cam", "present", "albedo", "bg")})
    c = run(renderer, scp)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm])


@pytest.mark.parametrize("guard", [64, 61])
def test_guard_bytes_around_the_outputs_stay_untouched(renderer, guard):
    """The entry point writes the (B,S,S,3) image and the (B,S,S) ids and nothing else; with the odd guard the image starts at an
    address that is no multiple of 4, which takes the byte-wise form of the output run."""
    from ihmr_amd import hip
    sc = RC.scene("s80")
    B, S = sc["verts"].shape[0], sc["S"]
    n_img, n_ids = B * S * S * 3, B * S * S * 4
    img_buf = torch.full((guard + n_img + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ids_buf = torch.full((64 + n_ids + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    L = hip.lib()
    v, cam, pres, alb, bg = up(sc["verts"]), up(sc["cam"]), up(sc["present"]), up(sc["albedo"]), up(sc["bg"])
    faces, off, ids = renderer._tables(v.device)
    ws = torch.empty(L.ihmr_render_workspace_bytes(B, 1556), dtype=torch.uint8, device="cuda")
    from ihmr_amd.render import _lights_struct
    lights = _lights_struct()
    hip.check(L.ihmr_render_meshes(hip.ptr(v), hip.ptr(faces), hip.ptr(off), hip.ptr(ids), 1556, 3076, 1538, hip.ptr(pres), hip.ptr(alb),
                                   hip.ptr(cam), C.byref(lights), hip.ptr(bg), S, C.c_void_p(img_buf.data_ptr() + guard),
                                   C.c_void_p(ids_buf.data_ptr() + 64), hip.ptr(ws), B, hip.stream_ptr()), "ihmr_render_meshes")
    torch.cuda.synchronize()
    ib, db = img_buf.cpu().numpy(), ids_buf.cpu().numpy()
    assert (ib[:guard] == 0xA5).all() and (ib[guard + n_img:] == 0xA5).all()
    assert (db[:64] == 0x5A).all() and (db[64 + n_ids:] == 0x5A).all()
    check("s80", ib[guard:guard + n_img].reshape(B, S, S, 3), db[64:64 + n_ids].copy().view(np.int32).reshape(B, S, S))


def test_background_is_kept_where_nothing_is_drawn(renderer):
    sc = RC.scene("white")
    img, ids = run(renderer, sc)
    check("white", img, ids)
    assert (img[ids < 0] == 255).all() and (ids >= 0).any()
    sc = RC.scene("s64")
    img, ids = run(renderer, sc)
    assert np.array_equal(img[ids < 0], sc["bg"][ids < 0])
    # a face id says which hand: the right-only sample shows no left face and the other way round
    assert (ids[1] < RC.SPLIT).all() and ((ids[2] >= RC.SPLIT) | (ids[2] < 0)).all()


def test_fp16_vertices_give_the_bytes_of_their_fp32_upcast(renderer):
    sc = RC.scene("s64")
    h = torch.from_numpy(sc["verts"]).half()
    a = run(renderer, sc, verts=h.float().numpy())
    v = h.cuda()
    out, fid = renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]), up(sc["bg"]), present=up(sc["present"]), colors=up(sc["albedo"]),
                               return_face_ids=True)
    assert np.array_equal(out.cpu().numpy(), a[0]) and np.array_equal(fid.cpu().numpy(), a[1])
    assert (a[1] >= 0).any()


def test_entry_point_refuses_bad_shapes(renderer):
    sc = RC.scene("s64")
    v = up(sc["verts"])
    with pytest.raises(ValueError):
        renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]), size=8)
    with pytest.raises(ValueError):
        renderer.render(v[:, :700], v[:, 778:], up(sc["cam"]), size=64)
    with pytest.raises(ValueError):
        renderer.render(v[:, :778], v[:, 778:], up(sc["cam"]))


def test_keypoints_match_the_restatement():
    """B = 2, K = 42 on a 64-pixel image: keypoints on the border and in the corner (clipped), outside the image, overlapping ones
    (the later one wins), weights of zero and below (not drawn)."""
    from ihmr_amd import render
    S, K = 64, 42
    rng = np.random.RandomState(9)
    kps = rng.uniform(-1.05, 1.05, (2, K, 2)).astype(f32)
    kps[0, 0], kps[0, 1], kps[0, 2], kps[0, 3] = (-1.0, -1.0), (0.999, 0.0), (0.0, 0.97), (1.2, 0.3)
    kps[0, 5] = kps[0, 4] + f32(2.0 / S)
    kps[1, 7] = kps[1, 6]
    w = np.ones((2, K), f32)
    w[0, 8], w[0, 9], w[1, 0] = 0.0, -1.0, 0.0
    img = RC.background(2, S, 21)
    want = np.stack([R.draw_keypoints(img[b].copy(), kps[b], w[b], (0, 255, 0)) for b in range(2)])
    dev = up(img)
    render.draw_keypoints_device(dev, up(kps), up(w), (0, 255, 0))
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), want)
    assert (want != img).any()
    # the reference-shaped function: recovered image, discs in BGR red, channels reversed on return (vis_util.py:53-71)
    chw = (img[0].transpose(2, 0, 1).astype(f32) / 127.5 - 1).astype(f32)
    got = render.draw_keypoints(chw, kps[0], w[0][:, None], "red", S)
    base = ((chw + 1) * 0.5 * 255).transpose(1, 2, 0).astype(np.uint8)
    assert np.array_equal(got, R.draw_keypoints(base.copy(), kps[0], w[0], (0, 0, 255))[:, :, ::-1])


def test_reference_shaped_functions_render_what_the_batched_renderer_renders():
    """render_together / render_mesh_to_image (numpy in, numpy out, BGR) on sample 0 of s64: the bytes of the restatement."""
    from ihmr_amd import render
    sc = RC.scene("s64")
    fr, fl = RC.hand_faces()
    v, cam, bg = sc["verts"][0].astype(np.float64), sc["cam"][0].astype(np.float64), sc["bg"][0]
    c0, c1 = np.array(render.COLORS["light_green"]).reshape(1, 3), np.array(render.COLORS["light_blue"]).reshape(1, 3)
    got = render.render_together([v[:778], v[778:]], [fr, fl], [c0, c1], cam, 64, bg)
    assert got.dtype == np.uint8 and np.array_equal(got, RC.reference("s64")[0][0])
    got = render.render_together([v[:778], v[778:]], [fr, fl], [c0, c1], cam, 64)
    assert np.array_equal(got, RC.reference("white")[0][0])
    one = np.array([render.SINGLE_HAND_COLOR] * 2, f32)
    for verts, faces in ((v[:778], fr), (v[778:], fl)):
        got = render.render(verts, faces, cam, 64, bg)
        want, _ = R.render_sample(verts.astype(f32), faces, cam.astype(f32), 64, one, faces.shape[0], (1, 1), bg)
        assert np.array_equal(got, want)


def test_visualize_result_writes_image_over_render_and_the_mesh(tmp_path, monkeypatch):
    """Three records (interacting, right, left) whose images have three different sizes: 896 x 448 .jpg files whose top half is the
    padded and resized image and whose bottom half is the render over it, and .obj files of the recorded vertices and faces."""
    from ihmr_amd import evaluator as E
    from ihmr_amd import render, ry_utils
    from oracle import preprocess_ref as P
    from PIL import Image
    fr, fl = RC.hand_faces()
    models = dict(right=types.SimpleNamespace(faces=fr), left=types.SimpleNamespace(faces=fl))
    ev = E.Evaluator(models)
    verts16 = RC.hand_verts().astype(np.float16)
    shapes = {"interacting": (300, 400), "right": (512, 256), "left": (224, 224)}
    cams = {"interacting": [6.0, -0.0875, 0.0], "right": [5.0, -0.07, 0.02], "left": [5.5, -0.09, -0.01]}
    images = {}
    for k, (ht, (h, w)) in enumerate(shapes.items()):
        path = f"/data/set{k}/cap/seq/cam/img{k}.png"
        images[path] = np.random.RandomState(40 + k).randint(0, 256, (h, w, 3)).astype(np.uint8)
        ev.pred_results.append(dict(img_path=path, hand_type=ht, pred_cam_params=np.array(cams[ht], f32),
                                    pred_right_hand_verts=verts16[k, :778], pred_left_hand_verts=verts16[k, 778:]))
    written = {}
    real_write = E.write_image_bgr

    def hook(path, img):
        written[path] = np.array(img)
        real_write(path, img)
    monkeypatch.setattr(E, "write_image_bgr", hook)
    vis, obj = tmp_path / "images", tmp_path / "objs"
    ev.visualize_result(str(vis), str(obj), batch_size=2, image_loader=lambda p: images[p])
    assert len(written) == 3
    two = RC.TWO_HAND
    one = np.array([render.SINGLE_HAND_COLOR] * 2, f32)
    for k, r in enumerate(ev.pred_results):
        name = f"cap/seq/cam_img{k}"
        jpg = vis / (name + ".jpg")
        assert jpg.is_file() and Image.open(jpg).size == (448, 896)
        res = written[str(jpg)]
        assert res.shape == (896, 448, 3) and res.dtype == np.uint8
        top, _ = P.padding_and_resize(images[r["img_path"]], np.zeros((1, 3), f32), 448)
        assert np.array_equal(res[:448], top)
        ht = r["hand_type"]
        present = (1, 1) if ht == "interacting" else (ht == "right", ht == "left")
        want, _ = R.render_sample(verts16[k].astype(f32), RC.faces(), r["pred_cam_params"], 448, two if ht == "interacting" else one, RC.SPLIT, present, top)
        assert np.array_equal(res[448:], want), ht
        assert (want != top).any()
        if ht == "interacting":
            ev_verts, ev_faces = verts16[k], np.concatenate([fr.astype(np.int64), fl.astype(np.int64) + 778])
        else:
            ev_verts, ev_faces = (verts16[k, :778], fr) if ht == "right" else (verts16[k, 778:], fl)
        ry_utils.save_mesh_to_obj(str(tmp_path / "want.obj"), ev_verts, ev_faces)
        assert (obj / (name + ".obj")).read_text() == (tmp_path / "want.obj").read_text()


def _opt(B, **kw):
    d = dict(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, input_nc=3, num_joints=42,
             total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20, trans_params_dim=3,
             model_root="", mean_param_file="mean_mano_params.pkl", checkpoints_dir="./checkpoints", strategy="mlp_default")
    d.update(kw)
    return types.SimpleNamespace(**d)


def _check_visuals(vis, img_chw):
    from ihmr_amd import render
    assert list(vis) == ["img", "gt_render_img (separate)", "pred_render_img (separate)", "render together (gt / pred)", "keypoint (gt / pred)"]
    for k, v in vis.items():
        assert v.shape == (224, 448, 3) and v.dtype == np.uint8, k
    show = render.recover_img(img_chw)[:, :, ::-1]
    assert np.array_equal(vis["img"], np.concatenate((show, show), axis=1))
    for k in list(vis)[1:]:
        assert (vis[k] != vis["img"]).any(), k                                   # something was drawn


def test_baseline_get_current_visuals_has_the_reference_layout(mano_arrays):
    from helpers import seeded_state_dict
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    B = 2
    m = InterHandModel(_opt(B, use_test_graph=False))
    sd = seeded_state_dict(m.encoder, 100)
    sd["regressor_ih.0.weight"] *= 0.05; sd["regressor_ih.0.bias"] *= 0.05      # the predicted pose stays hand-like
    m.encoder.load_state_dict(sd)
    m.eval()
    fwd = lambda p, s, t: two_hand.forward_from_packed(m.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    batch = synthetic_opt_batch(B, fwd, seed=77, with_image=True)
    m.set_input(batch)
    m.test()
    torch.cuda.synchronize()
    # the seeded encoder's camera is arbitrary: look at the hands with the camera of the test scenes
    m.pred_cam_params = torch.tensor([[6.0, -0.0875, 0.0]] * B, device="cuda")
    _check_visuals(m.get_current_visuals(1), batch["img"][1].numpy())


def test_mlp_get_current_visuals_has_the_reference_layout(mano_arrays):
    import helpers as H
    from ihmr_amd.mlp_model import MLPModel
    from ihmr_amd.strategies import make_mlp_strategy
    B = 2
    batch = H.synthetic_mlp_batch(mano_arrays, B, 31)
    batch["img"] = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (B, 3, 224, 224)).astype(f32))
    strategy = make_mlp_strategy()
    model = MLPModel(_opt(B))
    model.set_update_info(strategy, 10)
    for sid in range(len(strategy)):
        model.add_new_network(sid)
        model.sub_network_list[sid].load_state_dict(H.seeded_state_dict(model.sub_network_list[sid], 900 + sid, last_scale=0.02))
    model.eval()
    model.set_input(batch)
    model.test()
    torch.cuda.synchronize()
    _check_visuals(model.get_current_visuals(0), batch["img"][0].numpy())

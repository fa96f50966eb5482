"""Predicted hand meshes rendered over the image on the GPU -- the visualisation half of the reference
(``src/utils/render_color_utils.py``, ``src/utils/vis_util.py``; callers ``src/utils/evaluator.py:206-275`` and ``get_current_visuals``
of the training loops, ``baseline_model.py:412-488``, ``mlp_model.py:755-831``).

The reference builds an OpenDR scene per image (``ColoredRenderer`` + three ``LambertianPointLight``, an OpenGL / Mesa CPU path spread
over 16 processes).  Here a batch is two launches of ``ihmr_render_meshes`` (``csrc/render.h``): per-vertex Lambertian shading, an exact
integer-coverage triangle rasteriser with a z-buffer in registers, Gouraud interpolation, composite over the image.  What the
reference's own code computes before it calls OpenDR -- camera, translated vertices, merged faces, per-vertex albedo, lights,
background -- is :func:`scene_setup` / :func:`scene_together` / :func:`scene_single` and is pinned by ``tests/golden/render.npz``.  The
pixel arithmetic (``csrc/render_pure.h``) is this build's own: PARITY UNPINNED against OpenDR; no silhouette
anti-aliasing, no back-face culling.

:class:`MeshRenderer` is the batched device interface; :func:`render_together`, :func:`render_mesh_to_image`, :func:`render`,
:func:`draw_keypoints` and :func:`recover_img` keep the reference's single-sample numpy signatures and BGR conventions.  No CPU
fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import hip

FOCAL_LENGTH = 5.0                      # render_color_utils.py:46, vis_util.py:80

# render_color_utils.py:16-24 (BGR): what render_together is called with by the evaluator and the training loops
COLORS = {
    "light_blue": [1.0, 128 / 255, 0],
    "light_pink": [.9, .7, .7],
    "light_green": [166 / 255.0, 178 / 255.0, 30 / 255.0],
    "light_purple_han": [0.8, 0.53, 0.53],
    "light_purple_rongyu": [255.0 / 255.0, 102 / 255, 102 / 255],
    "light_gray": [192 / 255, 192 / 255, 192 / 255],
}
# vis_util.py:91-97 (BGR): render_mesh_to_image takes color_id = 2 of this table's values
VIS_COLORS = {
    "light_blue": [0.65098039, 0.74117647, 0.85882353],
    "light_pink": [.9, .7, .7],
    "light_green": [166 / 255.0, 178 / 255.0, 30 / 255.0],
}
SINGLE_HAND_COLOR = list(VIS_COLORS.values())[2 % len(VIS_COLORS)]

LIGHT_POSITIONS = ([-200, -100, -100], [800, 10, 300], [-500, 500, 1000])       # simple_renderer: back, left, right light
LIGHT_COLORS = ([1, 1, 1], [1, 1, 1], [.7, .7, .7])
MIN_SIZE, MAX_SIZE = 16, 2048


def _rotate_y(points, angle):
    """render_color_utils.py:155-159."""
    ry = np.array([[np.cos(angle), 0., np.sin(angle)], [0., 1., 0.], [-np.sin(angle), 0., np.cos(angle)]])
    return np.dot(points, ry)


def light_table(yrot=np.radians(120)):
    """(3,3) positions after ``_rotateY`` and (3,3) colours of simple_renderer's three lights, float64."""
    pos = np.stack([_rotate_y(np.array(p), yrot) for p in LIGHT_POSITIONS]).astype(np.float64)
    col = np.stack([np.array(c, np.float64) for c in LIGHT_COLORS])
    return pos, col


def scene_setup(cam, inputSize):
    """The host arithmetic of ``render`` (render_color_utils.py:46-56) / ``render_mesh_to_image`` (vis_util.py:78-83) in float64:
    focal length in pixels ``F`` (2,), principal point ``c`` (2,), the translation ``cam_t`` added to the vertices, and the lights."""
    cam = np.asarray(cam)
    f = FOCAL_LENGTH
    tz = f / cam[0]
    cam_for_render = 0.5 * inputSize * np.array([f, 1, 1])
    cam_t = np.array([cam[1], cam[2], tz])
    return cam_for_render[0] * np.ones(2), cam_for_render[1:3], cam_t, light_table()


def _scene(verts, faces, color, cam, inputSize, background):
    F, c, cam_t, (lpos, lcol) = scene_setup(cam, inputSize)
    h, w = background.shape[:2]
    return OrderedDict(f=F, c=c, width=w, height=h, v=verts + cam_t, faces=faces, vc=color, light_pos=lpos, light_color=lcol,
                       background=background)


def scene_together(verts_list, faces_list, color_list, cam, inputSize, img=None):
    """Everything ``render_together`` hands to OpenDR (render_color_utils.py:27-66,103-127,232-242): merged vertices (translated) and
    faces, per-vertex albedo, camera, frustum size, lights, and the background scaled to [0,1] when its maximum exceeds 1."""
    assert len(verts_list) == 2, "Current version only support 2 sets of mesh"
    assert len(verts_list) == len(faces_list) and len(faces_list) == len(color_list)
    verts0, verts1 = verts_list
    faces0, faces1 = faces_list
    color0, color1 = color_list
    assert color0.shape == (1, 3) and color1.shape == (1, 3)
    verts = np.concatenate((verts0, verts1), axis=0)
    faces = np.concatenate((faces0, faces1 + verts0.shape[0]), axis=0)
    color = np.concatenate((np.repeat(color0, verts0.shape[0], axis=0), np.repeat(color1, verts1.shape[0], axis=0)), axis=0)
    if img is None:
        img = np.ones((inputSize, inputSize, 3), dtype=np.float32)
    return _scene(verts, faces, color, cam, inputSize, img / 255. if img.max() > 1 else img)


def scene_single(inputSize, image, cam, vert, face):
    """Everything ``render_mesh_to_image`` hands to OpenDR (vis_util.py:78-88,121-155,278-301)."""
    image = recover_img(image)
    color = np.array(SINGLE_HAND_COLOR)
    return _scene(vert, face, color, cam, inputSize, image / 255. if image.max() > 1.1 else image)


def recover_img(image):
    """vis_util.py:13-30: a normalised (max < 1.1) image goes back to [0,255], CHW becomes HWC, uint8."""
    if isinstance(image, torch.Tensor):
        image = image.detach().cpu().numpy()
    else:
        assert isinstance(image, np.ndarray)
    if np.max(image) < 1.1:
        image = (image + 1) * 0.5 * 255
    if image.shape[2] != 3:
        image = np.transpose(image, (1, 2, 0))
    image = image.copy()
    return image.astype(np.uint8)


def build_csr(faces, n_verts):
    """Per vertex its incident faces in ascending face index: int32 offsets (n_verts+1) and ids (3 n_faces)."""
    faces = np.asarray(faces, np.int64)
    flat_v = faces.reshape(-1)
    flat_f = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    order = np.lexsort((flat_f, flat_v))
    counts = np.bincount(flat_v, minlength=n_verts)
    off = np.zeros(n_verts + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return off.astype(np.int32), flat_f[order].astype(np.int32)


def _lights_struct():
    pos, col = light_table()
    L = hip.RenderLights()
    for l in range(3):
        for k in range(3):
            L.pos[l][k] = float(np.float32(pos[l, k]))
            L.color[l][k] = float(np.float32(col[l, k]))
    return L


class MeshRenderer:
    """Batched renderer of a right / left hand pair.  ``faces_right`` (nF0,3), ``faces_left`` (nF1,3) or None; the merged table is
    ``concat(faces_right, faces_left + n_verts_right)`` (evaluator.py:212-213), built once with its incident-face CSR."""

    def __init__(self, faces_right, faces_left=None, n_verts_right=hip.NUM_VERTS, n_verts_left=None):
        fr = np.asarray(faces_right, np.int64).reshape(-1, 3)
        fl = np.zeros((0, 3), np.int64) if faces_left is None else np.asarray(faces_left, np.int64).reshape(-1, 3)
        self.n_verts_right = int(n_verts_right)
        self.n_verts_left = 0 if faces_left is None else int(n_verts_left if n_verts_left is not None else n_verts_right)
        self.n_verts = self.n_verts_right + self.n_verts_left
        if fr.size and (fr.min() < 0 or fr.max() >= self.n_verts_right) or fl.size and (fl.min() < 0 or fl.max() >= self.n_verts_left):
            raise ValueError("a face names a vertex outside its hand")
        self.faces = np.concatenate((fr, fl + self.n_verts_right), axis=0).astype(np.int32)
        if self.faces.shape[0] == 0:
            raise ValueError("no faces to render")
        self.face_split = fr.shape[0]
        self.csr_offsets, self.csr_ids = build_csr(self.faces, self.n_verts)
        self._dev = None

    def _tables(self, device):
        if self._dev is None or self._dev[0] != device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev = (device, up(self.faces), up(self.csr_offsets), up(self.csr_ids))
        return self._dev[1:]

    def render(self, verts_right, verts_left, cam, background=None, present=None, colors=None, return_face_ids=False, size=None):
        """Device tensors: ``verts_right`` (B,nV0,3), ``verts_left`` (B,nV1,3) or None, fp32 or fp16; ``cam`` (B,3) = [s, tx, ty];
        ``background`` (B,S,S,3) uint8 or None (white; then ``size`` = S); ``present`` (B,2) marks the hands to draw (default: those
        given); ``colors`` (B,2,3) or (2,3) albedo per hand in the image's channel order (default right ``light_green``, left
        ``light_blue`` of render_color_utils.colors, BGR).  Returns the (B,S,S,3) uint8 image, with ``return_face_ids`` also the
        (B,S,S) int32 visible face per pixel (-1 = none).  Asynchronous on the current stream."""
        hip.require_gpu()
        dev = verts_right.device
        B = verts_right.shape[0]
        f32 = lambda t: t.detach().to(dev, torch.float32)
        if verts_left is None:
            if self.n_verts_left:
                verts_left = torch.zeros(B, self.n_verts_left, 3, device=dev)
                if present is None:
                    present = torch.tensor([[1, 0]], dtype=torch.uint8).repeat(B, 1)
        verts = f32(verts_right) if verts_left is None else torch.cat([f32(verts_right), f32(verts_left)], dim=1)
        verts = verts.contiguous()
        if verts.shape != (B, self.n_verts, 3):
            raise ValueError(f"vertices {tuple(verts.shape)} do not match the face tables ({B}, {self.n_verts}, 3)")
        if background is not None:
            if background.dtype != torch.uint8 or background.dim() != 4 or background.shape[0] != B or background.shape[3] != 3 or \
                    background.shape[1] != background.shape[2]:
                raise ValueError("background must be a (B,S,S,3) uint8 tensor")
            S = background.shape[1]
            background = background.to(dev).contiguous()
        else:
            if size is None:
                raise ValueError("without a background the image size must be given")
            S = int(size)
        if not MIN_SIZE <= S <= MAX_SIZE:
            raise ValueError(f"image size {S} outside [{MIN_SIZE}, {MAX_SIZE}]")
        cam = f32(cam).reshape(B, 3).contiguous()
        if colors is None:
            colors = torch.tensor([COLORS["light_green"], COLORS["light_blue"]], dtype=torch.float32)
        colors = torch.as_tensor(colors, dtype=torch.float32).to(dev)
        albedo = (colors.reshape(1, 2, 3).expand(B, 2, 3) if colors.dim() == 2 else colors.reshape(B, 2, 3)).contiguous()
        pres = None if present is None else torch.as_tensor(present).to(dev, torch.uint8).reshape(B, 2).contiguous()
        faces, off, ids = self._tables(dev)
        L = hip.lib()
        ws = torch.empty(L.ihmr_render_workspace_bytes(B, self.n_verts), dtype=torch.uint8, device=dev)
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
        fid = torch.empty(B, S, S, dtype=torch.int32, device=dev) if return_face_ids else None
        lights = _lights_struct()
        hip.check(L.ihmr_render_meshes(hip.ptr(verts), hip.ptr(faces), hip.ptr(off), hip.ptr(ids), self.n_verts, self.faces.shape[0],
                                       self.face_split, hip.ptr(pres), hip.ptr(albedo), hip.ptr(cam), C.byref(lights),
                                       hip.ptr(background), S, hip.ptr(out), hip.ptr(fid), hip.ptr(ws), B, hip.stream_ptr()),
                  "ihmr_render_meshes")
        return (out, fid) if return_face_ids else out


def draw_keypoints_device(img, kps, weight, color):
    """In place on a (B,S,S,3) uint8 device tensor: ``kps`` (B,K,2) in [-1,1], ``weight`` (B,K), ``color`` three bytes in the image's
    channel order (``ihmr_draw_keypoints``)."""
    hip.require_gpu()
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3 or img.shape[1] != img.shape[2] or not img.is_contiguous():
        raise ValueError("img must be a contiguous (B,S,S,3) uint8 tensor")
    B, S = img.shape[0], img.shape[1]
    kps = kps.detach().to(img.device, torch.float32).reshape(B, -1, 2).contiguous()
    K = kps.shape[1]
    weight = weight.detach().to(img.device, torch.float32).reshape(B, K).contiguous()
    hip.check(hip.lib().ihmr_draw_keypoints(hip.ptr(img), hip.ptr(kps), hip.ptr(weight), bytes(int(c) & 255 for c in color), B, S, K,
                                            hip.stream_ptr()), "ihmr_draw_keypoints")
    return img


# ------------------------------------------------------------------------------- the reference's single-sample functions (numpy)
def _background_bytes(img, inputSize):
    if img is None:
        return None
    img = np.asarray(img)
    if img.shape[:2] != (inputSize, inputSize):
        raise ValueError(f"the image {img.shape[:2]} is not {inputSize} x {inputSize}")
    return torch.from_numpy(np.ascontiguousarray(img.astype(np.uint8)))[None].cuda()


def render_together(verts_list, faces_list, color_list, cam, inputSize, img=None):
    """render_color_utils.py:27-43: two meshes with one colour each over ``img`` (uint8 HWC, BGR) or white -> (S,S,3) uint8."""
    hip.require_gpu()
    scene = scene_together(verts_list, faces_list, color_list, cam, inputSize, img)          # the reference's checks and merged tables
    r = MeshRenderer(faces_list[0], faces_list[1], verts_list[0].shape[0], verts_list[1].shape[0])
    assert np.array_equal(r.faces, scene["faces"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()
    colors = np.concatenate((color_list[0], color_list[1]), axis=0)
    out = r.render(dev(verts_list[0])[None], dev(verts_list[1])[None], dev(np.asarray(cam)[:3])[None], _background_bytes(img, inputSize),
                   colors=dev(colors), size=inputSize)
    return out[0].cpu().numpy()


def render_mesh_to_image(inputSize, image, cam, vert, face):
    """vis_util.py:78-88: one hand in ``light_green`` over ``image`` (any form :func:`recover_img` takes) -> (S,S,3) uint8."""
    hip.require_gpu()
    image = recover_img(image)
    r = MeshRenderer(face, None, vert.shape[0])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()
    colors = np.array([SINGLE_HAND_COLOR, SINGLE_HAND_COLOR])
    out = r.render(dev(vert)[None], None, dev(np.asarray(cam)[:3])[None], _background_bytes(image, inputSize), colors=dev(colors))
    return out[0].cpu().numpy()


def render(verts, faces, cam, inputSize, image):
    """vis_util.py:74-75."""
    return render_mesh_to_image(inputSize, image, cam, verts, faces)


def draw_keypoints(image, kps, kps_weight, color=(0, 0, 255), img_size=224):
    """vis_util.py:53-71: filled radius-3 discs at ``(kps + 1) * 0.5 * img_size`` where the weight is positive, drawn on the recovered
    image; the result has its channels reversed, as the reference returns it."""
    hip.require_gpu()
    image = recover_img(image)
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    kps, kps_weight = to_np(kps), to_np(kps_weight)
    if color == "red":
        color = (0, 0, 255)
    elif color == "green":
        color = (0, 255, 0)
    elif color == "blue":
        color = (255, 0, 0)
    else:
        assert isinstance(color, tuple) and len(color) == 3
    if image.shape[0] != img_size or image.shape[1] != img_size:
        raise ValueError(f"the image {image.shape[:2]} is not {img_size} x {img_size}")
    K = kps.shape[0]
    img = torch.from_numpy(np.ascontiguousarray(image))[None].cuda()
    draw_keypoints_device(img, torch.from_numpy(np.ascontiguousarray(kps[:, :2], np.float32))[None].cuda(),
                          torch.from_numpy(np.ascontiguousarray(np.asarray(kps_weight, np.float32).reshape(K, -1)[:, 0]))[None].cuda(), color)
    return img[0].cpu().numpy()[:, :, ::-1].astype(np.uint8)


def current_visuals(model, idx=0):
    """``get_current_visuals`` of the training loops (baseline_model.py:412-488, mlp_model.py:755-831): the ordered dict of five images
    -- the input twice, ground-truth and predicted hands rendered separately (right | left), both rendered together (gt | pred), and
    the ground-truth / predicted keypoints."""
    size = model.opt.inputSize
    img = model.input_img[idx].cpu().detach().numpy()
    show_img = recover_img(img)[:, :, ::-1]
    visual_dict = OrderedDict([("img", np.concatenate((show_img, show_img), axis=1))])
    kp = model.joints_2d[idx][:, :2].cpu().detach().numpy()
    pred_kp = model.pred_joints_2d[idx][:, :2].cpu().detach().numpy()
    kp_weight = model.joints_2d[idx][:, 2:].cpu().detach().numpy()
    kp_img = np.concatenate((draw_keypoints(img, kp, kp_weight, "red", size), draw_keypoints(img, pred_kp, kp_weight, "green", size)), axis=1)
    cam = model.pred_cam_params[idx].cpu().detach().numpy()
    faces = {h: np.asarray(model.mano_models[h].faces) for h in ("right", "left")}
    color_list = [np.array(COLORS["light_green"]).reshape(1, 3), np.array(COLORS["light_blue"]).reshape(1, 3)]
    separate, together = {}, {}
    for mode in ("gt", "pred"):
        v = {h: getattr(model, f"{mode}_{h}_hand_verts")[idx].cpu().detach().numpy() for h in ("right", "left")}
        one = {h: render_mesh_to_image(size, img, cam, v[h], faces[h])[:, :, ::-1] for h in ("left", "right")}
        separate[mode] = np.concatenate((one["right"], one["left"]), axis=1)
        together[mode] = render_together([v["right"], v["left"]], [faces["right"], faces["left"]], color_list, cam, size, show_img)
    visual_dict["gt_render_img (separate)"] = separate["gt"]
    visual_dict["pred_render_img (separate)"] = separate["pred"]
    visual_dict["render together (gt / pred)"] = np.concatenate([together["gt"], together["pred"]], axis=1)[:, :, ::-1]
    visual_dict["keypoint (gt / pred)"] = kp_img
    return visual_dict

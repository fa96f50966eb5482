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

:meth:`MeshRenderer.render` also turns the hands before it draws them (``view``: ``SMPLRenderer.rotated``, vis_util.py:159-188, about the
middle of the drawn hands' bounding box), paints them per vertex (``vertex_colors``; :func:`penetration_colors` makes the colours from
the collision module's per-vertex penetration depth) and returns the coverage mask (``return_alpha``); :meth:`MeshRenderer.render_views`
stacks several views, :func:`rotated` is the single-sample numpy form.

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


def view_rotation(axis, deg):
    """The (3,3) float64 matrix ``cv2.Rodrigues`` gives ``SMPLRenderer.rotated`` (vis_util.py:171-176) for a turn of ``deg`` degrees
    about 'y', 'x' or -- any other value -- z, written out for a coordinate axis (cos, +-sin, 0 and 1, nothing summed).  The renderer
    multiplies a row vector with it: ``(p - c) R + c``."""
    t = np.radians(float(deg))
    c, s = np.cos(t), np.sin(t)
    if axis == "y":
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    if axis == "x":
        return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _view_matrix(view):
    """``view`` as a float32 array (3,3) or (B,3,3): a matrix, or an ``(axis, deg)`` pair."""
    if isinstance(view, (tuple, list)) and len(view) == 2 and isinstance(view[0], str):
        return view_rotation(view[0], view[1]).astype(np.float32)
    if isinstance(view, torch.Tensor):
        return view.detach().to(torch.float32)
    return np.asarray(view, np.float32)


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
        self._views = {}

    def _view_on_device(self, view, device):
        """The float32 matrix of ``view`` on ``device``; that of an ``(axis, deg)`` pair is uploaded once and kept (an upload per call
        would make the host wait for the stream)."""
        pair = isinstance(view, (tuple, list)) and len(view) == 2 and isinstance(view[0], str)
        key = (view[0], float(view[1]), device) if pair else None
        if key in self._views:
            return self._views[key]
        rot = _view_matrix(view)
        rot = (rot if isinstance(rot, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rot))).to(device).contiguous()
        if pair:
            self._views[key] = rot
        return rot

    def _tables(self, device):
        if self._dev is None or self._dev[0] != device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev = (device, up(self.faces), up(self.csr_offsets), up(self.csr_ids))
        return self._dev[1:]

    def render(self, verts_right, verts_left, cam, background=None, present=None, colors=None, return_face_ids=False, size=None, *,
               view=None, pivot=None, vertex_colors=None, return_alpha=False):
        """Device tensors: ``verts_right`` (B,nV0,3), ``verts_left`` (B,nV1,3) or None, fp32 or fp16; ``cam`` (B,3) = [s, tx, ty];
        ``background`` (B,S,S,3) uint8 or None (white; then ``size`` = S); ``present`` (B,2) marks the hands to draw (default: those
        given); ``colors`` (B,2,3) or (2,3) albedo per hand in the image's channel order (default right ``light_green``, left
        ``light_blue`` of render_color_utils.colors, BGR).  Returns the (B,S,S,3) uint8 image, with ``return_face_ids`` also the
        (B,S,S) int32 visible face per pixel (-1 = none).  Asynchronous on the current stream.

        Keyword only: ``view`` a (3,3) or (B,3,3) matrix R or an ``(axis, deg)`` pair (:func:`view_rotation`): the hands are drawn at
        ``(v - c) R + c`` (``ihmr_view_vertices``), c = ``pivot`` (B,3) or (3,), by default the middle of the bounding box of the hands
        that are drawn; None draws them where they are (no transform: an identity matrix would round).  ``vertex_colors`` (B,nV,3)
        float32: one albedo per vertex of the merged mesh instead of ``colors`` (``ihmr_paint_meshes``).  ``return_alpha`` appends a
        (B,S,S) uint8 mask, 255 where a face is visible, to what is returned."""
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
        if view is not None:
            rot = self._view_on_device(view, dev)
            if tuple(rot.shape) not in ((3, 3), (B, 3, 3)):
                raise ValueError(f"view must be a (3,3) or ({B},3,3) matrix or an (axis, deg) pair, not {tuple(rot.shape)}")
            if pivot is not None:
                pivot = torch.as_tensor(pivot, dtype=torch.float32).to(dev)
                pivot = (pivot.reshape(1, 3).expand(B, 3) if pivot.dim() == 1 else pivot.reshape(B, 3)).contiguous()
            turned = torch.empty_like(verts)
            hip.check(L.ihmr_view_vertices(hip.ptr(verts), hip.ptr(pres), self.n_verts, self.n_verts_right, hip.ptr(rot), int(rot.dim() == 3),
                                           hip.ptr(pivot), hip.ptr(turned), B, hip.stream_ptr()), "ihmr_view_vertices")
            verts = turned
        elif pivot is not None:
            raise ValueError("a pivot without a view")
        ws = torch.empty(L.ihmr_render_workspace_bytes(B, self.n_verts), dtype=torch.uint8, device=dev)
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
        fid = torch.empty(B, S, S, dtype=torch.int32, device=dev) if return_face_ids or return_alpha else None
        lights = _lights_struct()
        if vertex_colors is not None:
            vc = f32(vertex_colors).contiguous()
            if vc.shape != (B, self.n_verts, 3):
                raise ValueError(f"vertex_colors {tuple(vc.shape)} is not ({B}, {self.n_verts}, 3)")
            draw, name, albedo = L.ihmr_paint_meshes, "ihmr_paint_meshes", vc
        else:
            draw, name = L.ihmr_render_meshes, "ihmr_render_meshes"
        hip.check(draw(hip.ptr(verts), hip.ptr(faces), hip.ptr(off), hip.ptr(ids), self.n_verts, self.faces.shape[0],
                       self.face_split, hip.ptr(pres), hip.ptr(albedo), hip.ptr(cam), C.byref(lights),
                       hip.ptr(background), S, hip.ptr(out), hip.ptr(fid), hip.ptr(ws), B, hip.stream_ptr()), name)
        ret = (out,) + ((fid,) if return_face_ids else ()) + (((fid >= 0).to(torch.uint8) * 255,) if return_alpha else ())
        return ret if len(ret) > 1 else out

    def render_views(self, verts_right, verts_left, cam, views, background=None, present=None, colors=None, size=None, *, pivot=None,
                     vertex_colors=None):
        """(B,V,S,S,3) uint8: one render per entry of ``views``.  An entry None is the camera's own view, drawn over ``background``
        (white without one); any other entry (what :meth:`render` takes as ``view``) is drawn on white, as ``SMPLRenderer.rotated`` is
        called without an image.  The other arguments are those of :meth:`render`."""
        views = list(views)
        if not views:
            raise ValueError("no views")
        if background is None and size is None:
            raise ValueError("without a background the image size must be given")
        S = int(size) if background is None else background.shape[1]
        out = [self.render(verts_right, verts_left, cam, background if v is None else None, present=present, colors=colors, size=S,
                           view=v, pivot=None if v is None else pivot, vertex_colors=vertex_colors) for v in views]
        B, V, row = out[0].shape[0], len(out), S * S * 3
        if row % 4:
            return torch.stack(out, dim=1)
        # whole dwords: the images are put side by side as 32-bit words (a byte-wise device copy is several times slower)
        words = torch.stack([o.reshape(B, row).view(torch.int32) for o in out], dim=1)
        return words.view(torch.uint8).reshape(B, V, S, S, 3)


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


def penetration_colors(depth, colors=None, hot=(0, 0, 1), lo=0.0, hi=0.005, layout="collision", n_split=None):
    """Per-vertex albedo (B,nV,3) float32 for ``vertex_colors`` from a per-vertex penetration depth (``ihmr_heat_colours``): the hand's
    colour of ``colors`` ((2,3) or (B,2,3), default ``light_green`` / ``light_blue``) where the depth is ``lo`` or less (or NaN), ``hot``
    (image channel order: the default is red in BGR) from ``hi`` on, a linear blend between.  ``depth`` (B,nV) device tensor in metres;
    ``layout`` "collision" is the order of ``collision_loss_origin_scale`` / ``SDFLoss``'s ``origin_scale`` (entry h*778 + v was sampled
    at vertex v of hand 1 - h), "vertex" means entry k belongs to vertex k of the merged mesh.  Vertices below ``n_split`` (default
    half of them) belong to the right hand."""
    hip.require_gpu()
    if layout not in ("collision", "vertex"):
        raise ValueError(f"layout {layout!r} is neither 'collision' nor 'vertex'")
    if depth.dim() != 2:
        raise ValueError("depth must be (B, n_verts)")
    dev = depth.device
    depth = depth.detach().to(torch.float32).contiguous()
    B, nV = depth.shape
    n_split = nV // 2 if n_split is None else int(n_split)
    if colors is None:
        colors = torch.tensor([COLORS["light_green"], COLORS["light_blue"]], dtype=torch.float32)
    colors = torch.as_tensor(colors, dtype=torch.float32).to(dev)
    albedo = (colors.reshape(1, 2, 3).expand(B, 2, 3) if colors.dim() == 2 else colors.reshape(B, 2, 3)).contiguous()
    out = torch.empty(B, nV, 3, dtype=torch.float32, device=dev)
    hot3 = (C.c_float * 3)(*[float(h) for h in hot])
    rc = hip.lib().ihmr_heat_colours(hip.ptr(depth), hip.ptr(albedo), hot3, float(lo), float(hi), nV, n_split, int(layout == "collision"),
                                     hip.ptr(out), B, hip.stream_ptr())
    if rc == -1:
        raise ValueError(f"ihmr_heat_colours refused lo = {lo}, hi = {hi}, n_verts = {nV}, n_split = {n_split}, layout = {layout!r}")
    hip.check(rc, "ihmr_heat_colours")
    return out


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


def rotated(verts, faces, deg, cam, inputSize, axis='y', img=None, do_alpha=True):
    """``SMPLRenderer.rotated`` (vis_util.py:159-188) for one hand: ``verts`` turned by ``deg`` degrees about ``axis`` around the middle
    of their bounding box (the reference: their mean), drawn in ``light_green`` with the camera ``cam`` = [s, tx, ty] over ``img``
    (uint8 HWC) or white -> (S,S,3) uint8, with ``do_alpha`` (S,S,4).  The fourth channel is 255 everywhere with ``img``
    (``append_alpha``); without it 255 exactly where a face is visible (``get_alpha`` keys on the pixel being white instead)."""
    hip.require_gpu()
    r = MeshRenderer(faces, None, verts.shape[0])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()
    colors = np.array([SINGLE_HAND_COLOR, SINGLE_HAND_COLOR])
    out, alpha = r.render(dev(verts)[None], None, dev(np.asarray(cam)[:3])[None], _background_bytes(img, inputSize), colors=dev(colors),
                          size=inputSize, view=(axis, deg), return_alpha=True)
    out = out[0].cpu().numpy()
    if not do_alpha:
        return out
    a = np.full(out.shape[:2], 255, np.uint8) if img is not None else alpha[0].cpu().numpy()
    return np.concatenate((out, a[:, :, None]), axis=2)


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

#!/usr/bin/env python3
"""Writes ``tests/golden/render.npz``: what the reference's visualisation code hands to OpenDR, recorded IN THE BUILD CONTAINER
(``/root/reference/src`` imported with CPU stubs, ``_ref_import.py``).

What runs: the reference's own ``utils/render_color_utils.render_together`` (-> ``render`` -> ``SMPLRenderer`` -> ``render_model`` ->
``simple_renderer``) and ``utils/vis_util.render_mesh_to_image`` on four seeded cases at S = 64.  OpenDR is absent, so its three
classes ``ProjectPoints``, ``ColoredRenderer`` and ``LambertianPointLight`` are replaced by recorders: they keep every attribute set on
them and every ``set(...)``, support ``+=`` of lights, and return a zero image for ``.r``.  Stored per case ``k`` (``c<k>_*``): the
inputs (``in_*``) and what reached OpenDR -- the camera's ``f`` and ``c``, the frustum's width and height, the translated vertices,
the faces, the albedo as set, the three lights' positions and colours, the background image.  No pixel of OpenDR is recorded: the
pixel arithmetic of this build is its own (tests/render_ref.py, PARITY UNPINNED)."""
import importlib
import os.path as osp
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import import_reference  # noqa: E402

S = 64


class Recorder:
    """Keeps attribute sets; ``set(**kw)`` sets several at once."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def set(self, **kw):
        self.__dict__.update(kw)


class Camera(Recorder):
    pass


class Light(Recorder):
    """One LambertianPointLight; a sum of lights is the list of them."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.terms = [self]

    def __add__(self, other):
        out = Light()
        out.terms = self.terms + other.terms
        return out


class Renderer(Recorder):
    last = None

    def __init__(self):
        super().__init__()
        Renderer.last = self

    @property
    def r(self):
        return np.zeros((self.frustum["height"], self.frustum["width"], 3))


def captured():
    rn = Renderer.last
    lights = rn.vc.terms
    assert len(lights) == 3 and all(l.vc is lights[0].vc for l in lights)          # the albedo rn.set(vc=...) took
    return dict(f=np.asarray(rn.camera.f, np.float64), c=np.asarray(rn.camera.c, np.float64), rt=np.asarray(rn.camera.rt, np.float64),
                t=np.asarray(rn.camera.t, np.float64), width=np.int64(rn.frustum["width"]), height=np.int64(rn.frustum["height"]),
                v=np.asarray(rn.v, np.float64), faces=np.asarray(rn.f, np.int32), vc=np.asarray(lights[0].vc, np.float64),
                light_pos=np.stack([np.asarray(l.light_pos, np.float64) for l in lights]),
                light_color=np.stack([np.asarray(l.light_color, np.float64) for l in lights]),
                background=np.asarray(rn.background_image, np.float64), bgcolor=np.asarray(rn.bgcolor, np.float64))


def main():
    import torch
    from ihmr_amd.assets import synthetic_mano
    import_reference()
    rcu = importlib.import_module("utils.render_color_utils")
    vu = importlib.import_module("utils.vis_util")
    for mod in (rcu, vu):
        mod.ProjectPoints, mod.ColoredRenderer, mod.LambertianPointLight = Camera, Renderer, Light
    rng = np.random.RandomState(20260)
    right, left = synthetic_mano(True), synthetic_mano(False)
    fr, fl = np.asarray(right["faces"], np.int64), np.asarray(left["faces"], np.int64)
    # every input is a short binary fraction (noise on a 2^-14 grid, dyadic cameras with 5 / s exact): the float64 sums the reference
    # forms are then exact and the file compresses to a fraction of what full-entropy mantissas would take
    noise = lambda: np.round(rng.normal(0, 0.002, (778, 3)) * 2.0 ** 14) / 2.0 ** 14
    hands = lambda: (np.asarray(right["v_template"], np.float64) + noise(),
                     np.asarray(left["v_template"], np.float64) + noise() + np.array([0.0078125, 0.00390625, 0.015625]))
    cams = [np.array([5.0, -0.078125, 0.0078125]), np.array([4.0, -0.046875, -0.015625]), np.array([8.0, -0.09375, 0.0], np.float32),
            np.array([5.0, 0.078125, 0.015625])]
    c0, c1 = np.array(rcu.colors["light_green"]).reshape(1, 3), np.array(rcu.colors["light_blue"]).reshape(1, 3)
    blocks = lambda: np.kron(rng.randint(0, 256, (S // 8, S // 8, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8)   # 8 x 8 colour blocks
    out = {}

    def keep(k, inputs, got):
        for n, v in inputs.items():
            out[f"c{k}_in_{n}"] = v
        for n, v in got.items():
            out[f"c{k}_{n}"] = v

    # 0: two hands over an image; 1: two hands, no image
    for k, img in ((0, blocks()), (1, None)):
        vr, vl = hands()
        res = rcu.render_together([vr, vl], [fr, fl], [c0, c1], cams[k], S, img)
        assert res.shape == (S, S, 3) and res.dtype == np.uint8
        inputs = dict(verts_right=vr, verts_left=vl, cam=cams[k], color0=c0, color1=c1)
        if img is not None:
            inputs["img"] = img
        keep(k, inputs, captured())
    # 2: right hand only, the image a normalised CHW float tensor; 3: left hand only, uint8 HWC image
    vr, vl = hands()
    chw = torch.from_numpy((blocks().transpose(2, 0, 1) / 127.5 - 1).astype(np.float32))
    res = vu.render_mesh_to_image(S, chw, cams[2], vr, fr)
    assert res.shape == (S, S, 3) and res.dtype == np.uint8
    keep(2, dict(vert=vr, cam=cams[2], image=chw.numpy()), captured())
    hwc = blocks()
    res = vu.render_mesh_to_image(S, hwc, cams[3], vl, fl)
    keep(3, dict(vert=vl, cam=cams[3], image=hwc), captured())
    out["faces_right"], out["faces_left"] = fr.astype(np.int32), fl.astype(np.int32)
    path = osp.join(HERE, "render.npz")
    np.savez_compressed(path, **out)
    print(path, osp.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()

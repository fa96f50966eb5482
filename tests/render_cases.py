"""The scenes of the renderer tests, shared by tests/test_render_cpu.py (which checks on the restatement that they exercise what they
are meant to) and tests/test_gpu_render.py (which compares the kernels with the restatement on them).  A scene is a dict of numpy
arrays: ``verts`` (B,1556,3) float32, ``cam`` (B,3), ``present`` (B,2) uint8, ``albedo`` (B,2,3) float32, ``bg`` (B,S,S,3) uint8 or
None, ``S``.  The restatement's result per scene is computed once per process (``reference``) and never modified.

Geometry: the deep-overlap pairs of the collision tests (``synthetic_opt_batch(overlap="deep")``: the half-turned left hand lies almost
on the right one, so the two hands project onto the same pixels and the depth test decides).  The synthetic hand spans x in [0, 0.175] m;
weak perspective puts a point at 0.5 S (1 + s (x + t)), so s = 6 with t_x = -0.0875 fills about half the image width."""
import functools

import numpy as np

import helpers as H
import render_ref as R

TWO_HAND = np.array([[166 / 255.0, 178 / 255.0, 30 / 255.0], [1.0, 128 / 255, 0]], np.float32)      # light_green, light_blue (BGR)
SPLIT = 1538


@functools.lru_cache(maxsize=None)
def _assets():
    from ihmr_amd.assets import synthetic_mano
    right, left = synthetic_mano(True), synthetic_mano(False)
    hv, _ = H.oracle_two_hand_verts((right, left), 4, H.DEEP_SEED, overlap="deep")
    verts = np.ascontiguousarray(hv.numpy().reshape(4, 1556, 3), np.float32)
    fr, fl = np.asarray(right["faces"], np.int64), np.asarray(left["faces"], np.int64)
    faces = np.concatenate([fr, fl + 778]).astype(np.int32)
    return verts, faces, fr.astype(np.int32), fl.astype(np.int32)


def hand_verts():
    return _assets()[0]


def faces():
    return _assets()[1]


def hand_faces():
    return _assets()[2], _assets()[3]


def background(B, S, seed):
    return np.random.RandomState(seed).randint(0, 256, (B, S, S, 3)).astype(np.uint8)


def _scene(name, S, rows, cams, present, bg_seed):
    v = hand_verts()[list(rows)]
    B = len(rows)
    return dict(name=name, S=S, verts=v, cam=np.asarray(cams, np.float32).reshape(B, 3), present=np.asarray(present, np.uint8).reshape(B, 2),
                albedo=np.repeat(TWO_HAND[None], B, 0), bg=None if bg_seed is None else background(B, S, bg_seed))


# name -> builder; TWO_HAND_SCENES below names the scenes the input condition (5-60 % coverage, >= 1 % of it under both hands) applies to
SCENES = {
    "s64": lambda: _scene("s64", 64, (0, 1, 2), [[6.0, -0.0875, 0.0], [5.0, -0.07, 0.02], [6.5, -0.09, -0.01]], [[1, 1], [1, 0], [0, 1]], 11),
    "s80": lambda: _scene("s80", 80, (1, 2, 3), [[6.0, -0.0875, 0.0], [5.5, -0.1, 0.015], [4.5, -0.06, -0.02]], [[1, 1], [1, 0], [0, 1]], 12),
    "s50": lambda: _scene("s50", 50, (2, 3, 0), [[6.0, -0.0875, 0.0], [5.0, -0.08, 0.02], [6.0, -0.09, 0.01]], [[1, 1], [1, 0], [0, 1]], 18),
    "s448": lambda: _scene("s448", 448, (0,), [[6.0, -0.0875, 0.0]], [[1, 1]], 13),
    "deep": lambda: _scene("deep", 64, (0, 1, 2, 3), [[6.0, -0.0875, 0.0], [5.0, -0.0875, 0.0], [5.5, -0.08, 0.01], [7.0, -0.09, 0.0]], [[1, 1]] * 4, 14),
    "white": lambda: _scene("white", 64, (0, 3), [[6.0, -0.0875, 0.0], [5.0, -0.07, 0.02]], [[1, 1]] * 2, None),
    # every face inside one 32 x 32 tile of a 96-pixel image: s = 1.0 makes the 0.175 m hand 8 pixels wide; every chunk list is full
    "one_tile": lambda: _scene("one_tile", 96, (0, 1), [[1.0, -0.55, -0.55], [0.9, -0.6, -0.5]], [[1, 1]] * 2, 15),
    # hands larger than the image (s = 40: 224 pixels wide, bounding boxes clipped to tiles, and with t_z = 0.125 part of the mesh lies
    # in front of the near distance); s = 200: every vertex in front of it; t_x = 17: projections on both sides of +-16384 pixels
    "oversize": lambda: _scene("oversize", 64, (0, 1, 2), [[40.0, -0.0875, 0.0], [200.0, -0.05, 0.0], [30.0, 17.0, 0.0]], [[1, 1]] * 3, 16),
    # cam[0] of 0, negative and NaN in the middle sample
    "bad_cam0": lambda: _scene("bad_cam0", 64, (0, 1, 2), [[6.0, -0.0875, 0.0], [0.0, 0.0, 0.0], [5.0, -0.07, 0.02]], [[1, 1]] * 3, 17),
    "bad_cam_neg": lambda: _scene("bad_cam_neg", 64, (0, 1, 2), [[6.0, -0.0875, 0.0], [-3.0, 0.0, 0.0], [5.0, -0.07, 0.02]], [[1, 1]] * 3, 17),
    "bad_cam_nan": lambda: _scene("bad_cam_nan", 64, (0, 1, 2), [[6.0, -0.0875, 0.0], [np.nan, 0.0, 0.0], [5.0, -0.07, 0.02]], [[1, 1]] * 3, 17),
}
TWO_HAND_SCENES = ("s64", "s80", "s50", "s448", "deep", "white")


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(B,S,S,3) uint8 images and (B,S,S) int32 face ids of the restatement; read-only."""
    sc = scene(name)
    f = faces()
    csr = R.build_csr(f, 1556)
    out = [R.render_sample(sc["verts"][b], f, sc["cam"][b], sc["S"], sc["albedo"][b], SPLIT, sc["present"][b],
                           None if sc["bg"] is None else sc["bg"][b], csr) for b in range(sc["verts"].shape[0])]
    img, ids = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    img.setflags(write=False)
    ids.setflags(write=False)
    return img, ids


def hand_masks(name, b):
    """Pixels each hand covers when drawn alone (sample b of a scene): two (S,S) bool arrays."""
    sc = scene(name)
    f = faces()
    out = []
    for present in ((1, 0), (0, 1)):
        _, ids = R.render_sample(sc["verts"][b], f, sc["cam"][b], sc["S"], sc["albedo"][b], SPLIT, present, None)
        out.append(ids >= 0)
    return out

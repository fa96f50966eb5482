#!/usr/bin/env python3
"""Writes ``tests/golden/augment.npz``: the training-time augmentation chain of the reference run IN THE BUILD CONTAINER
(``/root/reference/src`` imported with CPU stubs, ``_ref_import.py``) on seeded samples with recorded random draws.

What runs: the reference's own ``BaselineDataset.preprocess_data`` (data/baseline_dataset.py:67-108) with its own
``DataProcessor.padding_and_resize / random_flip / random_rescale / random_rotate / color_jitter / add_motion_blur /
normalize_joints_2d`` (data/data_preprocess.py) and ``utils/rotate_utils.py`` -- so the order of the steps, the flip, every label
formula and the float types numpy / torch give them are the reference's.  ``random`` / ``np.random.random`` are patched to the
recorded draws.  The third-party seams are filled as follows:

* ``cv2.resize`` -> ``oracle/preprocess_ref.resize_linear_u8``; ``cv2.getRotationMatrix2D``, ``cv2.warpAffine``, ``cv2.filter2D`` ->
  the restatements of ``tests/augment_ref.py`` (PARITY UNPINNED, see there);
* ``transforms.ColorJitter`` (torchvision is absent) -> a stand-in that applies torchvision 0.7's four functions written out with the
  REAL Pillow (``ImageEnhance``, ``convert('HSV')``; ``augment_ref.pil_color_jitter``) in the recorded order with the recorded factors.

For every float label three things are stored: the reference's result as run here (``ref_*``), the float64 result of
``augment_ref.labels_f64`` (``f64_*``) and ``tol_* = max(2 max|ref - f64|, 8 ulp of float32 at the array's largest magnitude)``.
The factor 2 is there because the device's ``sinf`` / ``cosf`` / ``atan2f`` differ from torch's by a few ulp.  numpy >= 2 runs
``rotate_joints_2d`` in float64 where the reference's numpy 1.18 may have used float32: the bound covers both.  Inputs are chosen so
that every composed orientation has a rotation angle in [0.3, 2.8] rad (asserted): at the angle-axis branch points the reference's
own float32 formulas are ill-conditioned.
"""
import importlib
import os
import os.path as osp
import sys
import types

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, osp.dirname(HERE))

import augment_ref as A  # noqa: E402
from _ref_import import import_reference  # noqa: E402
from oracle import preprocess_ref as P  # noqa: E402


class Draws:
    """Stands in for the ``random`` module inside data_preprocess.py: hands out the recorded draws in call order."""

    def __init__(self, randoms, randints, choice):
        self.randoms, self.randints, self.choice_index = list(randoms), list(randints), choice

    def random(self):
        return self.randoms.pop(0)

    def randint(self, a, b):
        v = self.randints.pop(0)
        assert a <= v <= b, (a, v, b)
        return v

    def choice(self, seq):
        return seq[self.choice_index]


def smooth_image(rng, h, w):
    """Flat rectangles, one smooth band and sparse noise: compresses well (the golden stays small) and still has the edges, ramps and
    single pixels at which an interpolation weight, a border or a rounding can go wrong."""
    img = np.empty((h, w, 3), np.uint8)
    img[:] = rng.randint(0, 256, size=3)
    for _ in range(10):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + rng.randint(1, max(2, h // 2)), x0:x0 + rng.randint(1, max(2, w // 2))] = rng.randint(0, 256, size=3)
    y0 = rng.randint(0, max(1, h - h // 6))
    ramp = np.linspace(0, 255, w)[None, :, None] * np.array([1.0, 0.5, 0.25])
    img[y0:y0 + max(1, h // 6)] = np.clip(np.rint(ramp + rng.randint(0, 60)), 0, 255).astype(np.uint8)
    m = rng.uniform(size=(h, w)) < 0.006
    img[m] = rng.randint(0, 256, size=(int(m.sum()), 3))
    return img


def scale_draw_for(S, new_size):
    """random.random() value whose ``int(S * (r * 0.4 + 0.6))`` is new_size."""
    r = ((new_size + 0.5) / S - 0.6) / 0.4
    assert 0 <= r < 1 and int(S * (r * (1.0 - 0.6) + 0.6)) == new_size
    return r


def cases():
    # (S, (H, W), hand type, np.random draw for the flip, use_flip, rescale: None | (random draw, position?, x, y), angle slice | None,
    #  colour: None | (order, b, c, s, hue), blur: None | (prob draw, kernel index), image kind)
    S = 64
    r06, rS1 = 0.0, scale_draw_for(S, S - 1)
    c = [
        (S, (80, 64), [1, 1], 0.7, True, (0.35, True, 3, 7), 9, ((0, 1, 2, 3), 1.1, 1.2, 0.7, 0.05), (0.1, 1), "smooth"),
        (S, (64, 64), [1, 0], 0.9, True, None, None, None, None, "smooth"),                           # every switch off
        (S, (50, 90), [0, 1], 0.1, False, None, None, None, None, "smooth"),                          # left-only: always mirrored
        (S, (64, 100), [1, 1], 0.3, True, (r06, True, 0, 0), 0, None, None, "smooth"),                # int(0.6 S), position 0, -90
        (S, (64, 64), [1, 1], 0.6, True, (r06, True, S - int(0.6 * S) - 1, S - int(0.6 * S) - 1), 5, None, None, "smooth"),  # end, 0 deg
        (S, (128, 128), [1, 0], 0.5, False, (rS1, True, 0, 0), 2, ((3, 2, 1, 0), 0.9, 0.8, 0.4, -0.1), (0.9, 0), "smooth"),  # S - 1; no blur
        (S, (33, 64), [0, 1], 0.5, True, (0.8, False, 0, 0), 7, ((1, 0, 3, 2), 1.3, 1.3, 1.6, 0.1), (0.2, 0), "smooth"),
        (S, (64, 64), [1, 1], 0.2, True, None, 4, ((2, 3, 0, 1), 1.0, 1.0, 1.0, 0.0), None, "constant"),                      # contrast on a constant image
        (S, (64, 64), [1, 1], 0.8, True, None, None, ((2, 1, 3, 0), 1.2, 0.9, 1.5, -0.05), (0.3, 2), "grey"),                 # saturation on a grey image
        (S, (70, 64), [1, 0], 0.5, True, (0.5, True, 5, 0), None, None, (0.0, 3), "smooth"),
        (S, (64, 64), [0, 1], 0.5, True, None, 3, None, (0.1, 2), "smooth"),
        (S, (20, 30), [1, 1], 0.55, True, (0.99, True, 0, 0), 6, ((1, 3, 2, 0), 0.95, 1.25, 0.5, 0.08), (0.4, 1), "smooth"),
    ]
    S = 224
    c += [
        (S, (240, 200), [1, 1], 0.7, True, (0.45, True, 11, 23), 8, ((3, 0, 2, 1), 1.25, 0.85, 1.4, 0.07), (0.1, 1), "smooth"),
        (S, (224, 224), [0, 1], 0.5, True, (0.1, False, 0, 0), 1, ((0, 2, 1, 3), 0.92, 1.28, 0.45, -0.09), None, "smooth"),
    ]
    return c


def main():
    import_reference()
    cv2 = sys.modules["cv2"]
    cv2.INTER_LINEAR = 1
    cv2.resize = lambda img, dsize: P.resize_linear_u8(img, dsize[0], dsize[1])
    cv2.getRotationMatrix2D = A.get_rotation_matrix_2d
    cv2.warpAffine = lambda img, M, dsize, flags=None: A.warp_affine(img, M, dsize, flags)
    cv2.filter2D = lambda img, ddepth, k: A.filter2d(img, k)
    dp = importlib.import_module("data.data_preprocess")
    ru = importlib.import_module("utils.rotate_utils")
    bd = importlib.import_module("data.baseline_dataset")
    dp.cv2 = ru.cv2 = cv2
    from PIL import Image

    rng = np.random.RandomState(11)
    bank = [np.ones((1, 1), np.float32) * 0.75,
            (rng.uniform(0, 1, (4, 6)) / 12).astype(np.float32),             # even sides: off-centre anchor
            np.eye(9, dtype=np.float32) / 9,
            np.zeros((3, 5), np.float32)]
    out = {f"bank{i}": k for i, k in enumerate(bank)}
    out["n_bank"] = np.array(len(bank))
    real_np_random = np.random.random
    cs = cases()
    for i, (S, (H, W), ht, flip_draw, use_flip, resc, slice_id, col, blur, kind) in enumerate(cs):
        img = smooth_image(rng, H, W)
        if kind == "constant":
            img[:] = np.array([90, 140, 30], np.uint8)
        elif kind == "grey":
            img[..., 1] = img[..., 0]; img[..., 2] = img[..., 0]
        hta = np.array(ht, np.float32)
        j2 = np.concatenate([rng.uniform(0, [W, H], size=(42, 2)), rng.randint(0, 2, size=(42, 1))], 1).astype(np.float32)
        j3 = np.concatenate([rng.normal(0, 0.08, size=(42, 3)), rng.randint(0, 2, size=(42, 1))], 1).astype(np.float32)
        if i % 3 != 2:
            j3[0, 3] = j3[21, 3] = 1.0                                       # hand_trans valid for most samples
        pose = rng.normal(0, 0.3, size=96).astype(np.float32)
        angle = None if slice_id is None else (90 - -90) / 10 * slice_id + -90
        for _ in range(200):                                                 # orientations away from the angle-axis branch points
            pose[0:3] = rng.normal(0, 0.9, size=3); pose[48:51] = rng.normal(0, 0.9, size=3)
            angs = [A.composed_rotation_angle(pose[s:s + 3] * f, angle or 0.0) for s in (0, 48) for f in (np.ones(3), np.array([1, -1, -1]))]
            angs += [float(np.linalg.norm(pose[s:s + 3])) for s in (0, 48)]
            if all(0.3 <= a <= 2.8 for a in angs):
                break
        else:
            raise AssertionError("no well-conditioned orientation found")
        betas = rng.normal(0, 0.5, size=20).astype(np.float32)
        weight = np.array([1, rng.randint(0, 2)], np.float32)

        proc = object.__new__(dp.DataProcessor)
        proc.opt = types.SimpleNamespace(inputSize=S)
        proc.rescale_range, proc.angle_scale, proc.num_slice = [0.6, 1.0], [-90, 90], 10
        proc.blur_kernels, proc.motion_blur_prob = bank, 0.5
        stages = {}

        def record(name, fn, which=0):
            def wrapped(*a, **k):
                res = fn(*a, **k)
                stages[name] = np.array(res[which] if isinstance(res, tuple) else res, copy=True)
                return res
            return wrapped
        proc.padding_and_resize = record("pad", proc.padding_and_resize)
        proc.random_flip = record("flip", proc.random_flip)
        proc.random_rescale = record("rescale", proc.random_rescale)
        proc.random_rotate = record("rotate", proc.random_rotate)
        proc.color_jitter = record("color", proc.color_jitter)
        proc.add_motion_blur = record("blur", proc.add_motion_blur)
        if col is not None:
            order, cb, cc, csat, chue = col
            proc.color_transfomer = lambda pil: Image.fromarray(A.pil_color_jitter(np.asarray(pil), order, cb, cc, csat, chue))
        randoms, randints = [], []
        if resc is not None:
            randoms.append(resc[0])
            if resc[1]:
                randints += [resc[2], resc[3]]
        if slice_id is not None:
            randints.append(slice_id)
        if blur is not None:
            randoms.append(blur[0])
        dp.random = Draws(randoms, randints, blur[1] if blur is not None else 0)
        ds = types.SimpleNamespace(data_processor=proc, isTrain=True, use_random_flip=use_flip, use_random_rescale=resc is not None,
                                   use_random_position=bool(resc and resc[1]), use_random_rotation=slice_id is not None,
                                   use_color_jittering=col is not None, use_motion_blur=blur is not None)
        np.random.random = lambda: flip_draw
        try:
            r_img, r_hta, r_j2, r_j3, (r_pose, r_betas, r_w), r_flip = bd.BaselineDataset.preprocess_data(
                ds, img.copy(), hta.copy(), j2.copy(), j3.copy(), (pose.copy(), betas.copy(), weight.copy()))
        finally:
            np.random.random = real_np_random
        assert not dp.random.randoms and not dp.random.randints, "a recorded draw was not consumed"
        r_j3 = np.asarray(r_j3)
        if r_j3[0, -1] > 0.0 and r_j3[21, -1] > 0.0:                         # baseline_dataset.py:192-199
            r_trans = np.concatenate((-r_j3[0, :3] + r_j3[21, :3], np.ones((1,), np.float32))).reshape(1, 4)
        else:
            r_trans = np.concatenate((np.zeros((3,), np.float32), np.zeros((1,), np.float32))).reshape(1, 4)
        import torch
        ref = dict(joints_2d=torch.from_numpy(np.asarray(r_j2)).float().numpy(), joints_3d=torch.from_numpy(r_j3).float().numpy(),
                   mano_pose=torch.from_numpy(np.asarray(r_pose)).float().numpy(), hand_trans=torch.from_numpy(r_trans).float().numpy())

        scale = None if resc is None else resc[0] * (1.0 - 0.6) + 0.6
        blurred = blur is not None and blur[0] < proc.motion_blur_prob
        ratio = S / H if H > W else S / W
        f64 = A.labels_f64(S, ratio, j2, j3, pose, betas, weight, hta, bool(r_flip), resc is not None, scale or 1.0,
                           resc[2] if resc and resc[1] else 0, resc[3] if resc and resc[1] else 0, slice_id is not None, angle or 0.0)
        for k, v in ref.items():
            err = float(np.abs(v.astype(np.float64) - f64[k]).max())
            ulp = float(np.spacing(np.float32(np.abs(v).max())))
            out[f"ref_{k}{i}"], out[f"f64_{k}{i}"] = v, f64[k]
            out[f"tol_{k}{i}"] = np.array(max(2 * err, 8 * ulp))
        assert np.array_equal(np.asarray(r_betas, np.float64), f64["mano_betas"]) and np.array_equal(np.asarray(r_w, np.float64), f64["mano_params_weight"])
        assert np.array_equal(np.asarray(r_hta, np.float64), f64["hand_type_array"])
        out[f"ref_mano_betas{i}"], out[f"ref_mano_params_weight{i}"] = np.asarray(r_betas, np.float32), np.asarray(r_w, np.float32)
        out[f"ref_hand_type_array{i}"], out[f"ref_do_flip{i}"] = np.asarray(r_hta, np.float32), np.array(float(r_flip), np.float32)

        # the uint8 image after every step that ran (a step that did not run leaves the previous bytes)
        cur = stages["flip"] if "flip" in stages else stages["pad"]
        out[f"u8_flip{i}"] = cur
        for name in ("rescale", "rotate", "color", "blur"):
            ran = name in stages and not (name == "blur" and not blurred)
            if ran:
                cur = stages[name]
                out[f"u8_{name}{i}"] = cur
            elif name in stages:
                assert np.array_equal(stages[name], cur)
        assert np.array_equal(cur, r_img)
        out[f"img{i}"], out[f"in_joints_2d{i}"], out[f"in_joints_3d{i}"] = img, j2, j3
        out[f"in_mano_pose{i}"], out[f"in_mano_betas{i}"], out[f"in_mano_params_weight{i}"], out[f"in_hand_type_array{i}"] = pose, betas, weight, hta
        c = col if col is not None else ((0, 1, 2, 3), 1.0, 1.0, 1.0, 0.0)
        out[f"draw{i}"] = np.array([S, int(bool(r_flip)), resc is not None, scale or 1.0, resc[2] if resc and resc[1] else 0,
                                    resc[3] if resc and resc[1] else 0, slice_id is not None, angle or 0.0, col is not None, c[1], c[2], c[3], c[4],
                                    blur[1] if blurred else -1], np.float64)
        out[f"order{i}"] = np.array(c[0], np.int32)
    out["n"] = np.array(len(cs))
    path = osp.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print("augment.npz", len(cs), "cases", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == "__main__":
    main()

"""Test helper (like ``bf16_emulation.py``): numpy restatement of every step of the training-time augmentation chain of
``BaselineDataset.preprocess_data`` (data/baseline_dataset.py:67-108), against which ``ihmr_amd/csrc/augment_pure.h`` (host build)
and the kernels of ``csrc/augment.h`` are compared byte for byte, plus a float64 version of the label formulas.

What is pinned and what is not:

* colour: ``brightness`` / ``contrast`` / ``saturation`` / ``hue`` restate Pillow (``ImageEnhance`` = ``Image.blend`` against a
  degenerate image, ``convert("L")``, ``convert("HSV")``, HSV -> RGB) as torchvision 0.7's ``ColorJitter`` drives it on the BGR array
  taken as RGB.  PINNED: tests/test_augment_cpu.py compares them with the installed Pillow (every HSV triple both ways, the golden's
  colour cases), and tests/golden/make_golden_augment.py runs the real Pillow.
* rescale: ``oracle/preprocess_ref.resize_linear_u8`` (PARITY UNPINNED there).
* rotation image: PARITY UNPINNED.  ``cv2.getRotationMatrix2D`` / ``cv2.warpAffine(..., INTER_LINEAR)`` are third-party
  (``opencv-python==4.2.0.32``), absent here.  ``warp_affine`` restates the published algorithm of OpenCV 4.2.0
  ``modules/imgproc/src/imgwarp.cpp`` for CV_8UC3 as this build understands it: the 2x3 matrix is inverted in double;
  per column ``adelta = cvRound(M0 x 1024)``, ``bdelta = cvRound(M3 x 1024)``; per row ``X0 = cvRound((M1 y + M2) 1024) + 16``
  (Y0 alike); ``X = (X0 + adelta) >> 5``, source column ``X >> 5``, fraction ``X & 31``; remap's bilinear table
  ``(32-fx)(32-fy) 32, fx(32-fy) 32, (32-fx)fy 32, fx fy 32`` (always summing to 32768, so the table's sum correction never fires);
  ``out = (sum w p + 16384) >> 15`` with taps outside the image counted as 0 (constant zero border).
* blur: PARITY UNPINNED.  ``cv2.filter2D(img, -1, k)``: correlation, anchor ``(kw // 2, kh // 2)``, BORDER_REFLECT_101, float32 sum over
  the NON-ZERO taps in row-major order without contraction, rounded half to even, clamped.  OpenCV takes a DFT route for kernels of
  130 taps or more that is not reproducible to the bit: the direct sum is this project's definition for every size.
* labels: the reference's own lines (data_preprocess.py:63-143, utils/rotate_utils.py, utils/geometry_utils.py), here in float64
  (``labels_f64``); the golden holds the reference's own result next to it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import preprocess_ref as P  # noqa: E402

OPS = ("brightness", "contrast", "saturation", "hue")      # ColorJitter's list order = operation ids 0..3


# ------------------------------------------------------------------------------------------------------------------ colour
def gray(img):
    """Pillow ``convert("L")`` of an (...,3) uint8 array (channel 0 plays R)."""
    c = img.astype(np.int64)
    return (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16


def blend(a, d, alpha):
    """``Image.blend(degenerate d, image a, alpha)``: float32 ``d + alpha * (a - d)``; truncated for 0 <= alpha <= 1, else clipped."""
    al = np.float32(alpha)
    a = np.asarray(a, np.int64)
    d = np.asarray(d, np.int64)
    t = (d.astype(np.float32) + (al * (a - d).astype(np.float32)).astype(np.float32)).astype(np.float32)
    if 0.0 <= float(al) <= 1.0:
        return t.astype(np.int64)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.int64)


def brightness(img, f):
    return blend(img, np.zeros_like(img, dtype=np.int64), f).astype(np.uint8)


def contrast_degenerate(img):
    g = gray(img)
    return int(float(g.sum()) / float(g.size) + 0.5)


def contrast(img, f):
    return blend(img, np.full(img.shape, contrast_degenerate(img), np.int64), f).astype(np.uint8)


def saturation(img, f):
    return blend(img, np.repeat(gray(img)[..., None], 3, axis=-1), f).astype(np.uint8)


def rgb2hsv(img):
    """Pillow ``convert("HSV")`` of an (...,3) uint8 array."""
    c = img.astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = c.max(-1), c.min(-1)
    grey = maxc == minc
    f32 = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = (maxc - r).astype(f32) / cr, (maxc - g).astype(f32) / cr, (maxc - b).astype(f32) / cr
        rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
        h = np.where(r == maxc, (bc - gc).astype(np.float64), np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(f32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
        uh = np.clip((h.astype(np.float64) * 255.0), 0, 255)
        us = np.clip((s.astype(np.float64) * 255.0), 0, 255)
    uh = np.where(grey, 0, np.nan_to_num(uh)).astype(np.int64)
    us = np.where(grey, 0, np.nan_to_num(us)).astype(np.int64)
    return np.stack([uh, us, maxc], -1).astype(np.uint8)


def hsv2rgb(hsv):
    """Pillow HSV -> ``convert("RGB")`` of an (...,3) uint8 array."""
    c = hsv.astype(np.int64)
    h, s, v = c[..., 0], c[..., 1], c[..., 2]
    h6 = h.astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = h6 - i
    fs = s.astype(np.float64) / 255.0
    vd = v.astype(np.float64)
    p = np.floor(vd * (1.0 - fs) + 0.5).astype(np.int64)
    q = np.floor(vd * (1.0 - fs * f) + 0.5).astype(np.int64)
    t = np.floor(vd * (1.0 - fs * (1.0 - f)) + 0.5).astype(np.int64)
    k = i % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    out = np.stack([r, g, b], -1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def hue_shift_byte(hue):
    """torchvision's ``np_h += np.uint8(hue_factor * 255)``: the shift as a byte."""
    return int(hue * 255) & 0xFF


def hue(img, shift_byte):
    hsv = rgb2hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(shift_byte)) & 0xFF).astype(np.uint8)
    return hsv2rgb(hsv)


def color_jitter(img, order, b, c, s, shift_byte):
    """The four operations in ``order`` (ids into OPS); every one quantises to uint8."""
    for op in order:
        op = int(op)
        if op == 0:
            img = brightness(img, b)
        elif op == 1:
            img = contrast(img, c)
        elif op == 2:
            img = saturation(img, s)
        else:
            img = hue(img, shift_byte)
    return img


# ------------------------------------------------------------------------------------------------------- rescale + position
def rescale(img, new_size, x_pos, y_pos):
    """``random_rescale``'s image half (data_preprocess.py:102-113)."""
    S = img.shape[0]
    res = np.zeros((S, S, 3), np.uint8)
    res[y_pos:new_size + y_pos, x_pos:new_size + x_pos, :] = P.resize_linear_u8(img, new_size, new_size)
    return res


# ---------------------------------------------------------------------------------------------------------------- rotation
def get_rotation_matrix_2d(center, angle, scale=1.0):
    """``cv2.getRotationMatrix2D``."""
    a = angle * np.pi / 180.0
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], np.float64)


def invert_affine(M):
    """``cv::warpAffine``'s inversion of the 2x3 matrix (double) -> 6 values, destination -> source."""
    m = np.asarray(M, np.float64).reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1; m[5] = b2
    return m


def warp_matrix(angle, S):
    """The inverted matrix of ``rotate_utils.rotate_image`` for an S x S image."""
    return invert_affine(get_rotation_matrix_2d((S / 2, S / 2), angle, 1.0))


def warp_coords(m, S):
    """Source column / row and 1/32 fractions of every destination pixel: (sx, sy, fx, fy), each (S,S) int64."""
    x = np.arange(S, dtype=np.float64)
    y = np.arange(S, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024.0).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024.0).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def warp_weights(fx, fy):
    return np.stack([(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32], -1)


def warp_inverse(img, m):
    """The remap half of ``cv2.warpAffine`` with the already inverted matrix."""
    S = img.shape[0]
    sx, sy, fx, fy = warp_coords(m, S)
    w = warp_weights(fx, fy)
    src = img.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
        return np.where(ok[..., None], src[np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)], 0)
    acc = (w[..., 0:1] * tap(sy, sx) + w[..., 1:2] * tap(sy, sx + 1) + w[..., 2:3] * tap(sy + 1, sx) + w[..., 3:4] * tap(sy + 1, sx + 1))
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_affine(img, M, dsize=None, flags=None):
    """``cv2.warpAffine(img, M, dsize, flags=cv2.INTER_LINEAR)`` for a square uint8 image and dsize = its own size."""
    assert img.shape[0] == img.shape[1] and (dsize is None or tuple(dsize) == (img.shape[1], img.shape[0]))
    return warp_inverse(img, invert_affine(M))


def rotate(img, angle):
    return warp_inverse(img, warp_matrix(angle, img.shape[0]))


# -------------------------------------------------------------------------------------------------------------------- blur
def reflect101(p, n):
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def filter2d(img, k):
    """``cv2.filter2D(img, -1, k)`` (see the module docstring)."""
    k = np.asarray(k, np.float32)
    if k.ndim == 1:
        k = k[None, :]
    kh, kw = k.shape
    ay, ax = kh // 2, kw // 2
    H, W = img.shape[:2]
    src = img.astype(np.float32)
    acc = np.zeros(img.shape, np.float32)
    for ky in range(kh):
        rows = reflect101(np.arange(H) - ay + ky, H)
        for kx in range(kw):
            w = k[ky, kx]
            if w == 0:
                continue
            cols = reflect101(np.arange(W) - ax + kx, W)
            acc = (acc + (w * src[rows][:, cols]).astype(np.float32)).astype(np.float32)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ labels
def _aa_to_rotmat64(r):
    r = np.asarray(r, np.float64)
    theta2 = float(r @ r)
    if theta2 > 1e-6:
        theta = np.sqrt(theta2)
        wx, wy, wz = r / (theta + 1e-6)
        c, s = np.cos(theta), np.sin(theta)
        k = 1.0 - c
        return np.array([[c + wx * wx * k, wx * wy * k - wz * s, wy * s + wx * wz * k],
                         [wz * s + wx * wy * k, c + wy * wy * k, -wx * s + wy * wz * k],
                         [-wy * s + wx * wz * k, wx * s + wy * wz * k, c + wz * wz * k]])
    return np.array([[1.0, -r[2], r[1]], [r[2], 1.0, -r[0]], [-r[1], r[0], 1.0]])


def _rotmat_to_aa64(R):
    m = R.T                                                   # rmat_t
    d2, d0_d1, d0_nd1 = m[2, 2] < 1e-6, m[0, 0] > m[1, 1], m[0, 0] < -m[1, 1]
    if d2 and d0_d1:
        t = 1 + m[0, 0] - m[1, 1] - m[2, 2]
        q = [m[1, 2] - m[2, 1], t, m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]]
    elif d2:
        t = 1 - m[0, 0] + m[1, 1] - m[2, 2]
        q = [m[2, 0] - m[0, 2], m[0, 1] + m[1, 0], t, m[1, 2] + m[2, 1]]
    elif d0_nd1:
        t = 1 - m[0, 0] - m[1, 1] + m[2, 2]
        q = [m[0, 1] - m[1, 0], m[2, 0] + m[0, 2], m[1, 2] + m[2, 1], t]
    else:
        t = 1 + m[0, 0] + m[1, 1] + m[2, 2]
        q = [t, m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]]
    q = np.array(q, np.float64) / np.sqrt(t) * 0.5
    sin2 = q[1] ** 2 + q[2] ** 2 + q[3] ** 2
    sin_t, cos_t = np.sqrt(sin2), q[0]
    two_theta = 2.0 * (np.arctan2(-sin_t, -cos_t) if cos_t < 0 else np.arctan2(sin_t, cos_t))
    k = two_theta / sin_t if sin2 > 0 else 2.0
    return q[1:] * k


def rot_z_f32(angle):
    """``torch.Tensor((0, 0, -np.pi*angle/180))``: the z rotation as the float32 the reference feeds its formulas."""
    return np.float32(-np.pi * angle / 180)


def composed_rotation_angle(orient, angle):
    """Rotation angle (rad) of R_z . R(orient): the generator keeps it away from the angle-axis branch points."""
    R = _aa_to_rotmat64(np.array([0, 0, float(rot_z_f32(angle))])) @ _aa_to_rotmat64(orient)
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def labels_f64(S, ratio, joints_2d, joints_3d, mano_pose, mano_betas, weight, hand_type, flip, rescale_on, scale, x_pos, y_pos,
               rotate_on, angle):
    """The label chain in float64 on float32 inputs.  -> dict of float64 arrays with the batch-dict shapes of one sample."""
    j2 = np.asarray(joints_2d, np.float64).copy()
    j3 = np.asarray(joints_3d, np.float64).copy()
    pose = np.asarray(mano_pose, np.float64).copy()
    betas = np.asarray(mano_betas, np.float64).copy()
    w = np.asarray(weight, np.float64).copy()
    ht = np.asarray(hand_type, np.float64).copy()
    j2[:, :2] *= float(np.float32(ratio))
    if flip:
        j2 = np.concatenate([j2[21:], j2[:21]])
        j2[:, 0] = S - j2[:, 0]
        j3 = np.concatenate([j3[21:], j3[:21]])
        j3[:, 0] = -j3[:, 0]
        pose = np.concatenate([pose[48:], pose[:48]]).reshape(-1, 3) * np.array([1.0, -1.0, -1.0])
        pose = pose.reshape(-1)
        betas = np.zeros(20)
        w, ht = w[::-1].copy(), ht[::-1].copy()
    if rescale_on:
        j2[:, :2] *= float(np.float32(scale))
        j2[:, 0] += x_pos
        j2[:, 1] += y_pos
    if rotate_on:
        rz = float(rot_z_f32(angle))
        pose[:3] = _rotmat_to_aa64(_aa_to_rotmat64(np.array([0, 0, rz])) @ _aa_to_rotmat64(pose[:3]))
        a = -angle / 180 * np.pi
        o = S / 2
        dx, dy = j2[:, 0] - o, j2[:, 1] - o
        j2[:, 0], j2[:, 1] = o + np.cos(a) * dx - np.sin(a) * dy, o + np.sin(a) * dx + np.cos(a) * dy
        j3[:, :3] = (_aa_to_rotmat64(np.array([0, 0, rz])) @ j3[:, :3].T).T
    j2[:, 0] = (j2[:, 0] / S) * 2.0 - 1.0
    j2[:, 1] = (j2[:, 1] / S) * 2.0 - 1.0
    if j3[0, 3] > 0 and j3[21, 3] > 0:
        trans = np.concatenate([-j3[0, :3] + j3[21, :3], [1.0]])
    else:
        trans = np.zeros(4)
    return dict(joints_2d=j2, joints_3d=j3, mano_pose=pose, mano_betas=betas, mano_params_weight=w, hand_type_array=ht,
                do_flip=np.float64(1.0 if flip else 0.0), hand_trans=trans.reshape(1, 4))


# --------------------------------------------------------------------------------------------- the real Pillow (CPU tests only)
def pil_color_jitter(img, order, b, c, s, hue_factor):
    """torchvision 0.7's ``ColorJitter`` transform list on a PIL image, written out with the real Pillow (imported here, so that
    nothing on the GPU path needs it): ``adjust_brightness / contrast / saturation`` = ``ImageEnhance.*(img).enhance(f)``,
    ``adjust_hue`` = ``convert('HSV')``, ``np_h += np.uint8(hue_factor * 255)`` with wrap-around, ``convert('RGB')``."""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(np.ascontiguousarray(img))
    for op in order:
        op = int(op)
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(b)
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(c)
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(s)
        else:
            h, sat, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.uint8(int(hue_factor * 255) & 0xFF)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), sat, v)).convert("RGB")
    return np.asarray(im).copy()

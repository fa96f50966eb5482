"""Training-time augmentation of IHMR-Baseline on the GPU: the training-time half of the reference's
``BaselineDataset.preprocess_data`` (src/data/baseline_dataset.py:67-108), which ``bash/train_baseline.sh:35-41`` switches on with
``--use_random_flip --use_random_rescale --use_random_position --use_random_rotation --use_color_jittering --use_motion_blur``
and which the reference runs per image in its DataLoader workers --

    DataProcessor.padding_and_resize / random_flip   src/data/data_preprocess.py:45-93
    DataProcessor.random_rescale                     src/data/data_preprocess.py:96-119
    DataProcessor.random_rotate                      src/data/data_preprocess.py:122-143, src/utils/rotate_utils.py
    DataProcessor.color_jitter                       src/data/data_preprocess.py:146-152 (torchvision 0.7 ColorJitter, Pillow)
    DataProcessor.add_motion_blur                    src/data/data_preprocess.py:155-159 (cv2.filter2D)
    ToTensor + Normalize, hand_trans                 src/data/baseline_dataset.py:41-44,192-202

for a whole batch at once, device-resident, without a host synchronisation between the steps (``ihmr_augment_images``: one kernel
per step over two uint8 ping-pong buffers, every step quantising to uint8 as the reference does; ``ihmr_augment_labels``: one
workgroup per sample).  The random draws are made on the host (``draw``) and travel as one struct array in one copy; they can always
be given explicitly.  No CPU fallback: without the library or a GPU the calls raise.

Motion blur: ``cv2.filter2D`` is restated as the direct float32 sum over the non-zero taps (correlation, anchor ``(kw // 2, kh // 2)``,
reflect-101 border, round half to even).  OpenCV itself takes a DFT route for kernels of 130 taps or more whose result is not
reproducible to the bit; the direct sum is this project's definition for every size up to 33 x 33.  The reference loads its kernels
from ``.mat`` files (``data_utils.load_blur_kernel``); here they are given as float arrays.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hip
from .preprocess import DataProcessor

RESCALE, ROTATE, COLOR, BLUR = 1, 2, 4, 8            # IHMR_AUG_* (include/ihmr_hip.h)
BLUR_MAX = 33
# ihmr_aug_params (include/ihmr_hip.h)
PARAMS_DTYPE = np.dtype([("warp", "f8", (6,)), ("rot_cos", "f8"), ("rot_sin", "f8"), ("rot_z", "f4"), ("scale", "f4"),
                         ("brightness", "f4"), ("contrast", "f4"), ("saturation", "f4"), ("flip", "i4"), ("flags", "i4"),
                         ("new_size", "i4"), ("x_pos", "i4"), ("y_pos", "i4"), ("hue_shift", "i4"), ("blur_kernel", "i4"),
                         ("order", "i4", (4,)), ("angle", "f4"), ("reserved", "i4")], align=True)
assert PARAMS_DTYPE.itemsize == 136
LABEL_KEYS = ("joints_2d", "joints_3d", "mano_pose", "mano_betas", "mano_params_weight", "hand_type_array")
LABEL_SHAPES = dict(joints_2d=(42, 3), joints_3d=(42, 4), mano_pose=(96,), mano_betas=(20,), mano_params_weight=(2,), hand_type_array=(2,))


def warp_matrix(angle: float, S: int) -> np.ndarray:
    """``cv2.getRotationMatrix2D((S/2, S/2), angle, 1)`` inverted as ``cv::warpAffine`` inverts it (double): destination -> source."""
    a = angle * np.pi / 180.0
    alpha, beta = np.cos(a), np.sin(a)
    cx = cy = S / 2
    m = np.array([alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy], np.float64)
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1; m[5] = b2
    return m


def empty_params(n: int) -> np.ndarray:
    """A table of n samples with every switch off."""
    p = np.zeros((n,), PARAMS_DTYPE)
    p["blur_kernel"] = -1
    p["scale"] = 1.0
    p["brightness"] = p["contrast"] = p["saturation"] = 1.0
    p["order"] = np.arange(4)
    p["warp"] = np.array([1, 0, 0, 0, 1, 0], np.float64)
    p["rot_cos"] = 1.0
    return p


def set_flip(p: np.ndarray, i: int, flip: bool):
    p["flip"][i] = int(bool(flip))


def set_rescale(p: np.ndarray, i: int, S: int, scale: float, x_pos: int = 0, y_pos: int = 0, new_size: Optional[int] = None):
    """``random_rescale`` (data_preprocess.py:96-119): new_size = int(S * scale) unless given."""
    p["flags"][i] |= RESCALE
    p["scale"][i] = scale
    p["new_size"][i] = int(S * scale) if new_size is None else new_size
    p["x_pos"][i], p["y_pos"][i] = x_pos, y_pos


def set_rotation(p: np.ndarray, i: int, S: int, angle: float):
    """``random_rotate`` (data_preprocess.py:122-143): the image's inverted warp matrix and the label rotations' constants."""
    p["flags"][i] |= ROTATE
    p["angle"][i] = angle
    p["warp"][i] = warp_matrix(angle, S)
    a = -angle / 180 * np.pi                                   # rotate_joints_2d
    p["rot_cos"][i], p["rot_sin"][i] = np.cos(a), np.sin(a)
    p["rot_z"][i] = np.float32(-np.pi * angle / 180)           # rotate_orient / rotate_joints_3d: torch.Tensor((0, 0, ...))


def set_color(p: np.ndarray, i: int, brightness: float, contrast: float, saturation: float, hue: float, order=(0, 1, 2, 3),
              hue_shift: Optional[int] = None):
    """torchvision 0.7 ``ColorJitter``: the four factors and the order of brightness (0), contrast (1), saturation (2), hue (3)."""
    p["flags"][i] |= COLOR
    p["brightness"][i], p["contrast"][i], p["saturation"][i] = brightness, contrast, saturation
    p["hue_shift"][i] = (int(hue * 255) & 0xFF) if hue_shift is None else (int(hue_shift) & 0xFF)   # np_h += np.uint8(hue * 255)
    p["order"][i] = order


def set_blur(p: np.ndarray, i: int, kernel_index: int):
    p["blur_kernel"][i] = kernel_index


def line_blur_kernels(lengths=(5, 9, 13), angles=(0.0, 45.0, 90.0, 135.0)):
    """A small built-in bank of motion-blur kernels: normalised lines through the centre of an n x n kernel."""
    bank = []
    for n in lengths:
        for a in angles:
            k = np.zeros((n, n), np.float32)
            c = n // 2
            t = np.linspace(-c, c, 4 * n)
            ys = np.rint(c - t * np.sin(np.deg2rad(a))).astype(int)
            xs = np.rint(c + t * np.cos(np.deg2rad(a))).astype(int)
            k[ys, xs] = 1.0
            bank.append(k / k.sum())
    return bank


class TrainDataProcessor:
    """Training-time half of the reference's ``DataProcessor`` (``data_preprocess.py:17``) with ``BaselineDataset.preprocess_data``'s
    order of steps, batched on the device.  ``opt`` carries the reference's option names (``use_random_flip``, ``use_random_rescale``,
    ``use_random_position``, ``use_random_rotation``, ``use_color_jittering``, ``use_motion_blur``, ``motion_blur_prob``, ``inputSize``);
    ``blur_kernels``: float arrays of any shape up to 33 x 33 (larger ones raise ``ValueError``)."""

    rescale_range = (0.6, 1.0)
    angle_scale = (-90, 90)
    num_slice = 10

    def __init__(self, opt=None, blur_kernels: Optional[Sequence[np.ndarray]] = None, seed: Optional[int] = None):
        g = lambda k, d=False: getattr(opt, k, d)
        self.final_size = int(g("inputSize", 224))
        if self.final_size % 4:
            raise ValueError("inputSize must be a multiple of 4")
        self.use_random_flip, self.use_random_rescale = bool(g("use_random_flip")), bool(g("use_random_rescale"))
        self.use_random_position, self.use_random_rotation = bool(g("use_random_position")), bool(g("use_random_rotation"))
        self.use_color_jittering, self.use_motion_blur = bool(g("use_color_jittering")), bool(g("use_motion_blur"))
        self.motion_blur_prob = float(g("motion_blur_prob", 0.5))
        self.blur_kernels = []
        for k in (blur_kernels or []):
            k = np.asarray(k, np.float32)
            k = k.reshape(1, -1) if k.ndim == 1 else k
            if k.ndim != 2 or k.size == 0:
                raise ValueError("a blur kernel is a non-empty 2-D float array")
            if k.shape[0] > BLUR_MAX or k.shape[1] > BLUR_MAX:
                raise ValueError(f"blur kernel of shape {k.shape} is larger than {BLUR_MAX} x {BLUR_MAX}")
            self.blur_kernels.append(np.ascontiguousarray(k))
        if self.use_motion_blur and not self.blur_kernels:
            raise ValueError("use_motion_blur needs blur_kernels")
        self.rng = np.random.default_rng(seed)
        self._pre = DataProcessor(final_size=self.final_size)
        self._bank = None

    # ------------------------------------------------------------------------------------------------------------ draws
    def draw(self, hand_type_array, generator: Optional[np.random.Generator] = None) -> np.ndarray:
        """The reference's draws for a batch (data_preprocess.py:22-28,63-64,96-126,155-157, baseline_dataset.py:71-80) -> the
        parameter table (numpy, ``PARAMS_DTYPE``)."""
        rng = generator if generator is not None else self.rng
        S = self.final_size
        h = np.asarray(hand_type_array, np.float32).reshape(-1, 2)
        p = empty_params(h.shape[0])
        for i in range(h.shape[0]):
            if h[i, 0] < 0.5 and h[i, 1] > 0.5:                   # left-only: always mirrored
                set_flip(p, i, True)
            elif self.use_random_flip and h[i].sum() > 1.5:       # interacting: np.random.random() > 0.5
                set_flip(p, i, rng.random() > 0.5)
            if self.use_random_rescale:
                lo, hi = self.rescale_range
                scale = rng.random() * (hi - lo) + lo
                new_size = int(S * scale)
                x = y = 0
                if self.use_random_position:
                    end = S - new_size - 1                        # random.randint(0, end), both ends included
                    x, y = int(rng.integers(0, end + 1)), int(rng.integers(0, end + 1))
                set_rescale(p, i, S, scale, x, y)
            if self.use_random_rotation:
                lo, hi = self.angle_scale
                set_rotation(p, i, S, (hi - lo) / self.num_slice * int(rng.integers(0, self.num_slice)) + lo)
            if self.use_color_jittering:
                set_color(p, i, rng.uniform(0.9, 1.3), rng.uniform(0.8, 1.3), rng.uniform(0.4, 1.6), rng.uniform(-0.1, 0.1),
                          rng.permutation(4))
            if self.use_motion_blur and rng.random() < self.motion_blur_prob:
                set_blur(p, i, int(rng.integers(0, len(self.blur_kernels))))
        return p

    def check_params(self, params: np.ndarray, B: int):
        S = self.final_size
        if params.dtype != PARAMS_DTYPE or params.shape != (B,):
            raise ValueError(f"params must be a ({B},) array of augment.PARAMS_DTYPE")
        r = params[(params["flags"] & RESCALE) != 0]
        if ((r["new_size"] < 1) | (r["x_pos"] < 0) | (r["y_pos"] < 0) | (r["x_pos"] + r["new_size"] > S) | (r["y_pos"] + r["new_size"] > S)).any():
            raise ValueError("rescaled image does not fit the canvas")
        c = params[(params["flags"] & COLOR) != 0]
        if c.size and not (np.sort(c["order"], axis=1) == np.arange(4)).all():
            raise ValueError("order must be a permutation of 0..3")
        if (params["blur_kernel"] >= len(self.blur_kernels)).any():
            raise ValueError("blur_kernel index outside the bank")

    def _blur_bank(self):
        if self._bank is None and self.blur_kernels:
            bank = np.zeros((len(self.blur_kernels), BLUR_MAX * BLUR_MAX), np.float32)
            dims = np.zeros((len(self.blur_kernels), 2), np.int32)
            for i, k in enumerate(self.blur_kernels):
                bank[i, :k.size] = k.reshape(-1)
                dims[i] = k.shape
            self._bank = (torch.from_numpy(bank).cuda(), torch.from_numpy(dims).cuda())
        return self._bank if self._bank is not None else (None, None)

    # ------------------------------------------------------------------------------------------------------------ chain
    def apply_packed(self, pixels: torch.Tensor, offsets: torch.Tensor, sizes: torch.Tensor, labels: Optional[Dict[str, torch.Tensor]],
                     params: np.ndarray) -> Dict[str, torch.Tensor]:
        """Device-resident inputs (bytes, offsets int64, sizes int32 (B,2) as ``DataProcessor.pack`` lays them out; labels: float32
        tensors ``joints_2d`` (B,42,3) in source pixels, ``joints_3d`` (B,42,4), ``mano_pose`` (B,96), ``mano_betas`` (B,20),
        ``mano_params_weight`` (B,2), ``hand_type_array`` (B,2)) through the chain.  A kernel runs iff some sample takes its step."""
        hip.require_gpu()
        B, S = sizes.shape[0], self.final_size
        self.check_params(params, B)
        steps = int(np.bitwise_or.reduce(params["flags"])) & (RESCALE | ROTATE | COLOR)
        if (params["blur_kernel"] >= 0).any():
            steps |= BLUR
        bank, dims = self._blur_bank() if steps & BLUR else (None, None)
        dparams = torch.from_numpy(np.ascontiguousarray(params).view(np.uint8).copy()).cuda(non_blocking=True)
        img = torch.empty((B, 3, S, S), dtype=torch.float32, device="cuda")
        bufs = [torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        sums = torch.empty((B,), dtype=torch.int32, device="cuda") if steps & COLOR else None
        final = C.c_int(-1)
        st = hip.stream_ptr()
        hip.check(hip.lib().ihmr_augment_images(hip.ptr(pixels), hip.ptr(offsets), hip.ptr(sizes), hip.ptr(dparams), B, S, steps,
                                                hip.ptr(bank), hip.ptr(dims), len(self.blur_kernels), hip.ptr(bufs[0]), hip.ptr(bufs[1]),
                                                hip.ptr(sums), hip.ptr(img), C.byref(final), st), "ihmr_augment_images")
        out = dict(img=img, img_uint8=bufs[final.value])
        if labels is not None:
            lin = {}
            for k in LABEL_KEYS:
                t = labels[k]
                if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape[1:]) == LABEL_SHAPES[k] and t.shape[0] == B):
                    raise ValueError(f"labels[{k!r}] must be a float32 device tensor of shape {(B,) + LABEL_SHAPES[k]}")
                lin[k] = t.contiguous()
            lout = {k: torch.empty_like(lin[k]) for k in LABEL_KEYS}
            lout["do_flip"] = torch.empty((B,), dtype=torch.float32, device="cuda")
            lout["hand_trans"] = torch.empty((B, 1, 4), dtype=torch.float32, device="cuda")
            hip.check(hip.lib().ihmr_augment_labels(hip.ptr(sizes), hip.ptr(dparams), B, S, *[hip.ptr(lin[k]) for k in LABEL_KEYS],
                                                    *[hip.ptr(lout[k]) for k in LABEL_KEYS], hip.ptr(lout["do_flip"]),
                                                    hip.ptr(lout["hand_trans"]), st), "ihmr_augment_labels")
            out.update(lout)
            if "hand_type_valid" in labels:
                out["hand_type_valid"] = labels["hand_type_valid"]
        else:
            out["do_flip"] = torch.from_numpy(params["flip"].astype(np.float32)).cuda(non_blocking=True)
        return out

    def apply(self, images: Sequence[np.ndarray], labels: Optional[dict], params: np.ndarray) -> Dict[str, torch.Tensor]:
        """Host images ((H,W,3) uint8, BGR as ``cv2.imread`` returns them) and labels (arrays or tensors) -> the batch-dict fields
        ``InterHandModel.set_input`` reads, all on the device (plus ``img_uint8``, the final bytes, and ``ori_img_size``)."""
        hip.require_gpu()
        buf, offsets, sizes = self._pre.pack(images)
        self._pre.check_sizes(sizes.numpy())
        dl = None
        if labels is not None:
            dl = {k: torch.as_tensor(np.asarray(labels[k].cpu() if torch.is_tensor(labels[k]) else labels[k], np.float32))
                  .reshape((len(images),) + LABEL_SHAPES[k]).contiguous().cuda(non_blocking=True) for k in LABEL_KEYS}
            if "hand_type_valid" in labels:
                dl["hand_type_valid"] = torch.as_tensor(labels["hand_type_valid"]).float().cuda(non_blocking=True)
        out = self.apply_packed(buf.cuda(non_blocking=True), offsets.cuda(non_blocking=True), sizes.cuda(non_blocking=True), dl, params)
        out["ori_img_size"] = sizes.max(dim=1)[0]
        return out

    def __call__(self, images: Sequence[np.ndarray], labels: dict, generator: Optional[np.random.Generator] = None):
        return self.apply(images, labels, self.draw(np.asarray(torch.as_tensor(labels["hand_type_array"]).cpu()), generator))

"""Every launch of the BACKWARD pass of one IHMR-Baseline training step at a batch size B, derived from ``encoder_shapes.trunk_layers``
(which is pinned to the module's own containers): per conv + BatchNorm unit the weight-gradient launch (``ihmr_conv_wgrad``) and the
input-gradient launch or launches (``ihmr_conv_igemm`` with the roles turned), with the case split of
``EncoderTrainer._unit_backward`` / ``conv_dgrad`` / ``conv_dgrad_s2_3x3`` (ihmr_amd/encoder_train.py) restated.  Also a host
restatement of ``ihmr_conv_wgrad``'s selection (tile form, pixel split, last slice, reduce kernel, workspace prefix), a numpy float32
restatement of the kernel's reciprocal pixel division, and the operand draws.  A test oracle for WHICH FORM RUNS and for the draws'
exactness, never for values.  Shared by tests/test_encoder_train_shapes_cpu.py and tests/test_gpu_encoder_train_shapes.py."""
import collections
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_shapes as E  # noqa: E402

WGRAD_WORKSPACE_BYTES = 64 * 1024 * 1024 * 4     # encoder_train.conv_wgrad: torch.empty(64 * 1024 * 1024) floats of pixel-range partials
WGRAD_MAX_PIXELS = 1 << 23                       # ihmr_conv_wgrad refuses N * Ho * Wo >= 2^23 (the reciprocal division's range)
CONV_BK = 16                                     # pixels per reduction step (csrc/encoder.h)


# ---------------------------------------------------------------------------------------------------------------- the table
def wgrad_units(B, size=224):
    """The 53 weight-gradient launches, one per unit, in forward order: the unit's forward Shape (x [N*H*W][Cin], dy [N*Ho*Wo][Cout],
    ldx = Cin, lddy = Cout, dw [ceil16(K)][packed_ldw(Cout)])."""
    return E.trunk_layers(B, size)


def wgrad_table(B, size=224):
    """``wgrad_units`` de-duplicated by geometry: the same 23 entries as ``encoder_shapes.trunk_table``."""
    return E.trunk_table(B, size)


def dgrad_route(u):
    """Which input-gradient path ``_unit_backward`` takes for the unit: 'none' (the stem: no gradient w.r.t. the image), 'phase' (3 x 3 /
    stride 2 / pad 1: four parity-phase convolutions + interleave2), 'ds' (1 x 1 / stride 2: GEMM on Ho x Wo + dilate2), 's1' (stride 1:
    one turned convolution with pad k - 1 - pad)."""
    if u.name == "stem":
        return "none"
    if u.k == 3 and u.stride == 2 and u.pad == 1:
        return "phase"
    if u.stride == 2:
        assert u.k == 1 and u.pad == 0, u
        return "ds"
    assert u.stride == 1, u
    return "s1"


DLaunch = collections.namedtuple("DLaunch", "kind unit shapes also")
# kind: dgrad_route; unit: the unit's forward Shape; shapes: the ihmr_conv_igemm launches as forward Shapes with the roles turned
# (Cin = the unit's Cout, Cout = the unit's Cin, x = dY, residual = the skip gradient); also: later units of the same geometry.


def _turned(u, name, H, W, kh, kw, pad, residual, Ho=None, Wo=None):
    return E.Shape(name, u.N, H, W, u.Cout, u.Cin, max(kh, kw), 1, pad, u.Cout, u.Cin, u.Cin if residual else 0, residual, 0, (),
                   kh, kw, Ho, Wo)


def dgrad_units(B, size=224):
    """Per unit behind the stem, in forward order, the launches its input gradient makes."""
    out = []
    for u in E.trunk_layers(B, size):
        route = dgrad_route(u)
        Ho, Wo = E.out_hw(u)
        if route == "none":
            continue
        if route == "s1":
            assert (Ho, Wo) == (u.H, u.W)
            res = u.name.endswith(".c1")             # _block_backward: the skip gradient rides in c1's epilogue
            shapes = (_turned(u, u.name + ".dx", u.H, u.W, u.k, u.k, u.k - 1 - u.pad, res),)
        elif route == "ds":
            assert (u.H, u.W) == (2 * Ho, 2 * Wo)
            shapes = (_turned(u, u.name + ".dx", Ho, Wo, 1, 1, 0, False),)
        else:
            assert (u.H, u.W) == (2 * Ho, 2 * Wo)
            # phase (pi, pj): filter (1 + pi) x (1 + pj), stride 1, pad 0, output map = input map Ho x Wo: the second tap of an odd
            # phase reads dY row / column io + 1, which runs off the bottom / right edge at io = Ho - 1
            shapes = tuple(_turned(u, f"{u.name}.dx.p{pi}{pj}", Ho, Wo, 1 + pi, 1 + pj, 0, False, Ho, Wo) for pi in (0, 1) for pj in (0, 1))
        out.append(DLaunch(route, u, shapes, ()))
    return out


def dgrad_table(B, size=224):
    """``dgrad_units`` de-duplicated by (kind, geometry, residual); the first unit names the geometry."""
    seen = collections.OrderedDict()
    for d in dgrad_units(B, size):
        u = d.unit
        g = (d.kind, u.N, u.H, u.W, u.Cin, u.Cout, u.k, u.stride, u.pad, d.shapes[0].residual)
        if g in seen:
            seen[g] = seen[g]._replace(also=seen[g].also + (u.name,))
        else:
            seen[g] = d
    return list(seen.values())


def zero_insertion_shape(u):
    """The launch of ``conv_dgrad`` for a 3 x 3 / stride-2 unit (the route the trainer does NOT take): dY dilated to H x W, then a
    stride-1 convolution with the flipped filter."""
    return _turned(u, u.name + ".dx.zins", u.H, u.W, u.k, u.k, u.k - 1 - u.pad, False)


def unit_rows(B, size=224):
    """(name, cin, cout, k, stride, pad, route) per unit in forward order: what ``EncoderTrainer.units`` must be."""
    return [(u.name, u.Cin, u.Cout, u.k, u.stride, u.pad, dgrad_route(u)) for u in E.trunk_layers(B, size)]


# ---------------------------------------------------------------------------------------------------------------- ihmr_conv_wgrad's selection
def plan_wgrad(u, workspace_bytes=WGRAD_WORKSPACE_BYTES):
    """dict(tile=(BM over K, BN over Cout), msplit, chunks_per, last (chunks of the last slice), nchunks, reduce='wgrad_reduce' |
    'splitk_reduce4' | 'splitk_reduce1', prefix (floats of the workspace written), form).  None: the launcher refuses the shape."""
    M, K = E.gemm_dims(u)
    ldw = E.packed_ldw(u.Cout)
    cap = workspace_bytes // (K * u.Cout * 4)
    if M >= WGRAD_MAX_PIXELS or u.Cin % 4 or u.ldx % 4 or u.Cout % 4 or cap < 1:
        return None
    BM, BN = (128 if K > 64 else 64), (128 if u.Cout > 64 else 64)
    tiles = ((K + BM - 1) // BM) * ((u.Cout + BN - 1) // BN)
    nchunks = (M + CONV_BK - 1) // CONV_BK
    msplit = max(1, min(cap, 256, (1024 + tiles - 1) // tiles, max(1, nchunks // 8)))
    chunks_per = (nchunks + msplit - 1) // msplit
    msplit = (nchunks + chunks_per - 1) // chunks_per                  # the re-division: no empty slice
    last = nchunks - (msplit - 1) * chunks_per
    assert 1 <= last <= chunks_per
    reduce = "wgrad_reduce" if (u.Cout % 4 == 0 and ldw % 4 == 0 and msplit >= 32) else "splitk_reduce4" if u.Cout % 4 == 0 else "splitk_reduce1"
    return dict(tile=(BM, BN), tiles=tiles, msplit=msplit, chunks_per=chunks_per, last=last, nchunks=nchunks, reduce=reduce,
                prefix=msplit * K * u.Cout, form=f"{BM}x{BN}_msplit{msplit}x{chunks_per}_last{last}_{reduce}")


# ---------------------------------------------------------------------------------------------------------------- the pixel division
def sdiv_f32(v, d, rd, correct=True):
    """conv_wgrad_kernel's ``sdiv`` in numpy float32: q = (int)((float)v * rd), then the +-1 correction from the remainder.  v: int32
    array, 0 <= v < 2^23 (exact as float); rd: a float32 near 1 / d."""
    q = (v.astype(np.float32) * np.float32(rd)).astype(np.int32)      # one rounded fp32 product, truncated
    if correct:
        r = v - q * np.int32(d)
        q = q + (r >= d).astype(np.int32) - (r < 0).astype(np.int32)
    return q


def sdiv_divisors(B, size=224):
    """Every divisor the kernel's loaders use at batch B: Ho * Wo and Wo of every unit."""
    out = set()
    for u in E.trunk_layers(B, size):
        Ho, Wo = E.out_hw(u)
        out |= {Ho * Wo, Wo}
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- operand draws
def _gen(u, salt):
    return torch.Generator().manual_seed(zlib.crc32(f"train-{salt}:{u.name}:{u.N}:{u.H}:{u.Cin}:{u.Cout}:{u.k}".encode()))


def wgrad_ranges(u):
    """Integer ranges (x, dy) with M * max|x| * max|dy| < 2^24: every product, every partial sum of ANY summation order and the result
    are exact fp32 integers.  x in [-8, 8] and dy in [-7, 9] where M allows it (M <= 233 016), otherwise x in [-4, 4] and dy as wide as
    the bound allows: [-3, 5] for the stem's 802 816 pixels (802 816 * 20 = 16 056 320 < 16 777 216).  dy is asymmetric on purpose: a
    swapped or negated operand pair changes the sum."""
    M, _ = E.gemm_dims(u)
    xmax = 8 if M * 8 * 9 < 2 ** 24 else 4
    dmax = min(9, (2 ** 24 - 1) // (M * xmax))
    assert dmax >= 3, (u.name, M)
    return (-xmax, xmax), (-(dmax - 2), dmax)


def wgrad_integer_bound(u):
    M, _ = E.gemm_dims(u)
    xr, dr = wgrad_ranges(u)
    return M * max(map(abs, xr)) * max(map(abs, dr))


def draw_wgrad_integers(u, images=None):
    """(x [N][H][W][Cin], dy [N][Ho][Wo][Cout]) as fp32 tensors of small integers; every input channel is filled (the stem's fourth,
    which the network pads with zeros, too: its gradient rows are computed like any other)."""
    g = _gen(u, "wg-int")
    N = u.N if images is None else images
    Ho, Wo = E.out_hw(u)
    xr, dr = wgrad_ranges(u)
    ri = lambda lo_hi, shape: torch.randint(lo_hi[0], lo_hi[1] + 1, shape, generator=g, dtype=torch.int8).float()
    return ri(xr, (N, u.H, u.W, u.Cin)), ri(dr, (N, Ho, Wo, u.Cout))


def draw_wgrad_random(u):
    """randn operands at unit output scale: x ~ N(0, 1), dy ~ N(0, 1 / M), so dW ~ N(0, 1) (less at the border taps)."""
    g = _gen(u, "wg-rnd")
    M, _ = E.gemm_dims(u)
    Ho, Wo = E.out_hw(u)
    return torch.randn(u.N, u.H, u.W, u.Cin, generator=g), torch.randn(u.N, Ho, Wo, u.Cout, generator=g) / M ** 0.5


def wgrad_reference(u, x, dy, dtype=torch.float64):
    """dW in the forward packed order [K = (fh, fw, cin)][Cout], `dtype` on the CPU: torch.nn.grad.conv2d_weight of the same operands."""
    w = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).to(dtype), (u.Cout, u.Cin, u.k, u.k), dy.permute(0, 3, 1, 2).to(dtype),
                                    stride=u.stride, padding=u.pad)
    return w.permute(2, 3, 1, 0).reshape(u.k * u.k * u.Cin, u.Cout)


def draw_dgrad(d, kind):
    """Operands of a unit's input gradient in the unit's own terms: (dy [N][Ho][Wo][Cout], w (Cout, Cin, k, k), r [N*H*W][Cin] or None).
    'int': the forward draw of encoder_shapes (dy in [-8, 8], w in [-5, 7], r in [-9, 9]); the reduction runs over k * k * Cout <= 4608
    values, so |dx| <= 4608 * 56 + 9 < 2^18.  'rnd': dy ~ N(0, 1), w ~ N(0, 1 / (k * k * Cout)), r ~ N(0, 1): unit output scale."""
    u = d.unit
    g = _gen(u, "dg-" + kind)
    Ho, Wo = E.out_hw(u)
    res = d.shapes[0].residual
    if kind == "int":
        ri = lambda lo_hi, shape: torch.randint(lo_hi[0], lo_hi[1] + 1, shape, generator=g, dtype=torch.int8).float()
        return (ri(E.FP32_X, (u.N, Ho, Wo, u.Cout)), ri(E.FP32_W, (u.Cout, u.Cin, u.k, u.k)),
                ri(E.FP32_R, (u.N * u.H * u.W, u.Cin)) if res else None)
    return (torch.randn(u.N, Ho, Wo, u.Cout, generator=g), torch.randn(u.Cout, u.Cin, u.k, u.k, generator=g) / (u.k * u.k * u.Cout) ** 0.5,
            torch.randn(u.N * u.H * u.W, u.Cin, generator=g) if res else None)


def dgrad_integer_bound(u):
    return u.k * u.k * u.Cout * max(map(abs, E.FP32_X)) * max(map(abs, E.FP32_W)) + max(map(abs, E.FP32_R))


def dgrad_reference(u, dy, w, r, dtype=torch.float64):
    """dx [N*H*W][Cin] in `dtype` on the CPU: torch.nn.grad.conv2d_input of the same operands (+ the skip gradient)."""
    dx = torch.nn.grad.conv2d_input((u.N, u.Cin, u.H, u.W), w.to(dtype), dy.permute(0, 3, 1, 2).to(dtype), stride=u.stride, padding=u.pad)
    dx = dx.permute(0, 2, 3, 1).reshape(-1, u.Cin)
    return dx if r is None else dx + r.to(dtype)

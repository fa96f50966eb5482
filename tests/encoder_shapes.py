"""Every convolution / Linear launch of ``InterHandEncoder.forward`` at a batch size B, derived from the module's own parameter
containers, and a host restatement of which kernel form ``ihmr_conv_igemm`` / ``ihmr_conv_igemm_bf16`` (csrc/ihmr_hip.hip) select
for it.  The restatement is a test oracle for WHICH FORM RUNS (tile, gather mode, split-K depth, Stream-K, reduce width), never for
values; ``tests/test_streamk_partition.py`` restates the Stream-K partition the same way and is reused here for the slots a
Stream-K layer writes.  Also the operand draws shared by tests/test_encoder_shapes_cpu.py (which proves on the CPU that the integer
draws stay exact) and tests/test_gpu_encoder_shapes.py (which uses them on the device)."""
import collections
import functools
import os
import sys
import types
import zlib

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_streamk_partition import worker_pieces  # noqa: E402

WORKSPACE_BYTES = 128 * 1024 * 1024          # networks._splitk_workspace
SLOT_FLOATS = 128 * 128                      # one Stream-K tile slot (64 KB)

Shape = collections.namedtuple("Shape", "name N H W Cin Cout k stride pad ldx ldy ldr residual act also kh kw Ho Wo", defaults=(None,) * 4)
# ldx / ldy / ldr: the strides networks.py passes; residual: the network adds one; act: the network's activation (0 none, 1 ReLU,
# 2 sigmoid); also: the later layers of the same geometry.  Heads: y (and the residual) of `reg` start at column HEAD_COL of the
# ldy-wide buffer.  kh, kw (default k, k) and Ho, Wo (default: the convolution formula) describe the launches of the training backward
# pass (tests/encoder_train_shapes.py): non-square phase filters with the output map given by the caller.
HEAD_COL = 1024


def filter_hw(s):
    return (s.k, s.k) if s.kh is None else (s.kh, s.kw)


def out_hw(s):
    if s.Ho is not None:
        return s.Ho, s.Wo
    return (s.H + 2 * s.pad - s.k) // s.stride + 1, (s.W + 2 * s.pad - s.k) // s.stride + 1


def gemm_dims(s):
    Ho, Wo = out_hw(s)
    kh, kw = filter_hw(s)
    return s.N * Ho * Wo, kh * kw * s.Cin


@functools.lru_cache(maxsize=None)
def _encoder():
    from ihmr_amd.networks import InterHandEncoder
    return InterHandEncoder(types.SimpleNamespace(total_params_dim=122), torch.zeros(1, 122))


def _ceil(x, m):
    return (x + m - 1) // m * m


def trunk_layers(B, size=224):
    """Every conv of the trunk in ``_trunk_layers()`` order behind the stem, with the spatial bookkeeping of ``forward``: (name, conv
    geometry, residual?, act), NOT de-duplicated."""
    enc = _encoder()
    c = enc.main_encoder.conv1
    k_extra = 1                                             # forward pads the image to 4 channels (_pack: k_extra = 1)
    cin = c.in_channels + k_extra
    out = [Shape("stem", B, size, size, cin, c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0], cin, c.out_channels, 0, False, 1, ())]
    H = W = (size + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
    H, W = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1      # MaxPool2d(3, 2, 1)
    Hin = Win = H2 = W2 = None
    for key, conv, _bn, st, pd in enc._trunk_layers():
        role = key.rsplit(".", 1)[1]
        k = conv.kernel_size[0]
        assert conv.kernel_size == (k, k) and conv.bias is None
        if role == "c1":
            Hin, Win = H, W                                 # the block's input map: c1 and the downsample read it
            h, w, res, act = H, W, False, 1
        elif role == "c2":
            h, w, res, act = Hin, Win, False, 1
            H2, W2 = (Hin + 2 * pd - k) // st + 1, (Win + 2 * pd - k) // st + 1
        elif role == "c3":
            h, w, res, act = H2, W2, True, 1
            H, W = H2, W2                                   # the block's output map
        else:
            assert role == "ds"
            h, w, res, act = Hin, Win, False, 0
        out.append(Shape(key, B, h, w, conv.in_channels, conv.out_channels, k, st, pd, conv.in_channels, conv.out_channels,
                         conv.out_channels if res else 0, res, act, ()))
    assert (H, W) == (7, 7) or size != 224
    return out


def trunk_table(B, size=224):
    """``trunk_layers`` de-duplicated by geometry (N, H, W, Cin, Cout, k, stride, pad); the first layer of a geometry names it and
    carries its residual / activation, the others are listed in ``also``."""
    seen = collections.OrderedDict()
    for s in trunk_layers(B, size):
        g = (s.N, s.H, s.W, s.Cin, s.Cout, s.k, s.stride, s.pad)
        if g in seen:
            seen[g] = seen[g]._replace(also=seen[g].also + (s.name,))
        else:
            seen[g] = s
    return list(seen.values())


def head_table(B):
    """fc1, feat_encoder, regressor_ih and hand_classifier as ``forward`` launches them: 1 x 1 'images', K padded to a multiple of 16
    for the regressor (its input buffer is [feat 1024 | params 122 | 6 zeros])."""
    enc = _encoder()
    fc1, feat, reg, cls = enc.main_encoder.fc1, enc.feat_encoder[1], enc.regressor_ih[0], enc.hand_classifier[0]
    Kp = _ceil(reg.in_features, 16)
    assert reg.in_features == HEAD_COL + enc.total_params_dim and reg.out_features == enc.total_params_dim
    lin = lambda name, cin, m, ldx, ldy, ldr, res, act: Shape(name, B, 1, 1, cin, m.out_features, 1, 1, 0, ldx, ldy, ldr, res, act, ())
    return [lin("fc1", fc1.in_features, fc1, fc1.in_features, fc1.out_features, 0, False, 1),
            lin("feat", feat.in_features, feat, feat.in_features, Kp, 0, False, 1),
            lin("reg", Kp, reg, Kp, Kp, Kp, True, 0),
            lin("cls", cls.in_features, cls, Kp, cls.out_features, 0, False, 2)]


def packed_ldw(cout):
    return _ceil(cout, 128) if cout > 64 else 64          # networks._Packed / _PackedBF16


# ---------------------------------------------------------------------------------------------------------------- launcher restatements
def plan_fp32(s, cus, workspace_bytes=WORKSPACE_BYTES, y_aligned16=True):
    """ihmr_conv_igemm's selection.  Returns dict(tile=(BM, BN), mode='fast'|'c4'|'generic', ksplit, streamk, workers, tiles, nk,
    reduce=None|4|1, form=<one word for the tables>)."""
    M, K = gemm_dims(s)
    nk = (K + 15) // 16
    ldw = packed_ldw(s.Cout)
    wide_ok = s.Cout > 64 and ldw % 128 == 0
    tiles = [(128, 128), (64, 128), (128, 64), (64, 64)]
    blocks = lambda t: ((M + tiles[t][0] - 1) // tiles[t][0]) * ((s.Cout + tiles[t][1] - 1) // tiles[t][1])
    cap = workspace_bytes // (M * s.Cout * 4) if workspace_bytes else 1
    pick, ksplit = (0 if wide_ok else 2), 1
    if M <= 64:
        pick = 1 if wide_ok else 3
        ksplit = max(1, min(32, cap, nk // 4))
    elif blocks(pick) < 64:
        ksplit = max(1, min(32, cap, nk // 4))
    elif blocks(pick) < 384 and nk >= 64 and cap >= 2:
        ksplit = 2
    elif wide_ok and 768 < blocks(0) < 896:
        pick = 1
    fast = s.Cin % 16 == 0 and s.ldx % 4 == 0 and s.Cin <= 2048
    workers = max(8, min(512, 2 * cus // 8 * 8))
    sk_tiles = blocks(0)
    if (fast and pick == 0 and M > 64 and s.Cout % 128 == 0 and s.ldy % 4 == 0 and y_aligned16 and 64 <= sk_tiles <= 768 and nk >= 64
            and sk_tiles * nk >= 4 * workers and workspace_bytes >= workers * 2 * SLOT_FLOATS * 4):
        return dict(tile=(128, 128), mode="fast", ksplit=1, streamk=True, workers=workers, tiles=sk_tiles, nk=nk, reduce=None, form="streamk")
    mode = "fast" if fast else "c4" if (s.Cin == 4 and s.ldx % 4 == 0 and filter_hw(s)[1] >= 4 and not wide_ok) else "generic"
    if mode == "c4" and pick != 2:
        tile = (64, 64)
    else:
        tile = tiles[pick]
    reduce = None if ksplit == 1 else 4 if s.Cout % 4 == 0 else 1
    form = f"{tile[0]}x{tile[1]}_{mode}" + ("" if ksplit == 1 else f"_splitk_reduce{reduce}")
    return dict(tile=tile, mode=mode, ksplit=ksplit, streamk=False, workers=0, tiles=blocks(tiles.index(tile)), nk=nk, reduce=reduce, form=form)


def plan_bf16(s, cus, workspace_bytes=WORKSPACE_BYTES):
    """ihmr_conv_igemm_bf16's selection: dict(tile=(128, BN), mode, ksplit, tiles, nk)."""
    M, K = gemm_dims(s)
    nk = (K + 31) // 32
    ldw = packed_ldw(s.Cout)
    BN = 128 if (s.Cout > 64 and ldw % 128 == 0) else 64
    tiles = ((M + 127) // 128) * ((s.Cout + BN - 1) // BN)
    ksplit = 1
    if workspace_bytes and tiles < 2 * cus and nk >= 8:
        cap = workspace_bytes // (M * s.Cout * 4)
        ksplit = max(1, min(8, cap, nk // 4, (2 * cus + tiles - 1) // tiles))
    mode = "fast" if (s.Cin % 32 == 0 and s.ldx % 8 == 0 and s.Cin <= 4096) else "c4" if (s.Cin == 4 and s.ldx == 4) else "generic"
    return dict(tile=(128, BN), mode=mode, ksplit=ksplit, tiles=tiles, nk=nk)


def streamk_slots(plan):
    """The (worker, slot) pairs a Stream-K layer writes, and whether any worker finishes a whole tile itself."""
    slots, whole = set(), False
    for w in range(plan["workers"]):
        for p in worker_pieces(w, plan["workers"], plan["tiles"], plan["nk"]):
            if p["whole"]:
                whole = True
            else:
                assert (w, p["slot"]) not in slots
                slots.add((w, p["slot"]))
    return slots, whole


def workspace_footprint(s, plan):
    """What a launch writes into the workspace, as ('none',), ('prefix', n_floats) or ('slots', {slot indices of SLOT_FLOATS floats})."""
    M, _ = gemm_dims(s)
    if plan.get("streamk"):
        return ("slots", {2 * w + sl for w, sl in streamk_slots(plan)[0]})
    if plan["ksplit"] > 1:
        return ("prefix", plan["ksplit"] * M * s.Cout)
    return ("none",)


# ---------------------------------------------------------------------------------------------------------------- operand draws
def _gen(s, salt):
    return torch.Generator().manual_seed(zlib.crc32(f"{salt}:{s.name}:{s.N}:{s.H}:{s.Cin}:{s.Cout}:{s.k}".encode()))


# fp32 integer draw: x in [-8, 8], w in [-5, 7] (asymmetric on purpose: a swapped or negated operand pair changes the sum), bias in
# [-7, 7], residual in [-9, 9].  |y| <= K * 8 * 7 + 16 <= 4608 * 56 + 16 < 2^18: every product, partial sum and the result are exact
# fp32 integers in any summation order.
FP32_X, FP32_W, FP32_B, FP32_R = (-8, 8), (-5, 7), (-7, 7), (-9, 9)


def fp32_integer_bound(s):
    _, K = gemm_dims(s)
    return K * max(map(abs, FP32_X)) * max(map(abs, FP32_W)) + max(map(abs, FP32_B)) + max(map(abs, FP32_R))


def draw_integers(s, precision, images=None):
    """(x [N][H][W][Cin], w [Cout][Cin][k][k], b [Cout], r [M][Cout] or None) as fp32 tensors of small integers.  bf16: the thinned
    draw of test_conv_bf16_layers_exact_on_integers (x in [-2, 2] kept with probability min(1, 500 / K), w in {-1, 0, 1}, bias and
    residual in [-3, 3]): Var(sum) <= 667, so |y| <= 256 (every output a bf16-exact integer) is ten standard deviations away."""
    g = _gen(s, "int-" + precision)
    N = s.N if images is None else images
    M, K = gemm_dims(s._replace(N=N))
    ri = lambda lo_hi, shape: torch.randint(lo_hi[0], lo_hi[1] + 1, shape, generator=g, dtype=torch.int8).float()
    if precision == "fp32":
        x, w, b = ri(FP32_X, (N, s.H, s.W, s.Cin)), ri(FP32_W, (s.Cout, s.Cin, s.k, s.k)), ri(FP32_B, (s.Cout,))
        r = ri(FP32_R, (M, s.Cout)) if s.residual else None
    else:
        px = min(1.0, 500.0 / K)
        x = ri((-2, 2), (N, s.H, s.W, s.Cin))
        if px < 1.0:
            x = x * (torch.rand(x.shape, generator=g) < px)
        w, b = ri((-1, 1), (s.Cout, s.Cin, s.k, s.k)), ri((-3, 3), (s.Cout,))
        r = ri((-3, 3), (M, s.Cout)) if s.residual else None
    return x, w, b, r


def draw_random(s, precision):
    """randn operands at unit output scale (w ~ N(0, 1 / K)) as in test_conv_streamk_matches_torch; bf16: x, w, r rounded to bf16 first."""
    g = _gen(s, "rnd-" + precision)
    M, K = gemm_dims(s)
    x = torch.randn(s.N, s.H, s.W, s.Cin, generator=g)
    w = torch.randn(s.Cout, s.Cin, s.k, s.k, generator=g) / K ** 0.5
    b = torch.randn(s.Cout, generator=g)
    r = torch.randn(M, s.Cout, generator=g) if s.residual else None
    if precision == "bf16":
        x, w = x.bfloat16().float(), w.bfloat16().float()
        r = None if r is None else r.bfloat16().float()
    return x, w, b, r


def reference(s, x, w, b, r, dtype=torch.float64):
    """Pre-activation reference [M][Cout] in `dtype` on the CPU: F.conv2d of the same operands (+ residual)."""
    y = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), b.to(dtype), stride=s.stride, padding=s.pad)
    y = y.permute(0, 2, 3, 1).reshape(-1, s.Cout)
    return y if r is None else y + r.to(dtype)


def activate(y, act):
    return torch.relu(y) if act == 1 else torch.sigmoid(y) if act == 2 else y


def reg_chain(B):
    """The three IEF iterations on integers: (feat [B][1024], params [B][122], W [122][1146], bias [122], [float64 params after
    iteration 1, 2, 3]) with params += [feat | params] W^T + bias.  The draw is narrow (feat in [-2, 2], W in [-1, 2]) because the
    iterations feed on their own output: the values grow about 13-fold per iteration."""
    g = torch.Generator().manual_seed(977)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    feat, params = ri(-2, 2, (B, HEAD_COL)), ri(-3, 3, (B, 122))
    W, bias = ri(-1, 2, (122, HEAD_COL + 122)), ri(-3, 3, (122,))
    refs, p = [], params.double()
    for _ in range(3):
        p = p + torch.cat([feat.double(), p], 1) @ W.double().t() + bias.double()
        refs.append(p)
    return feat, params, W, bias, refs


def reg_chain_partial_bound(feat, params, W, bias, refs):
    """max over the chain of sum_k |x_k| |w_k| + |bias| + |residual|: no partial sum of any summation order exceeds it."""
    top = 0.0
    for pin in [params.double()] + refs[:-1]:
        rowsum = torch.cat([feat.double().abs(), pin.abs()], 1) @ W.double().abs().t() + bias.double().abs() + pin.abs()
        top = max(top, float(rowsum.max()))
    return top

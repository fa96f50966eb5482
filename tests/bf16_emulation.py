"""CPU restatement of the numerics contract of ``encoder_precision = "bf16"`` ("bf16 encoder path"): the checker of
tests/test_encoder_bf16_cpu.py and tests/test_gpu_encoder_bf16.py.  Plain torch on the CPU, no project kernel involved.

Every trunk conv reads bf16 activations and bf16 weights (BatchNorm folded in fp32 first, then ONE round-to-nearest-even), sums in
fp32 (a bf16 x bf16 product is exact in fp32, so ``F.conv2d`` on the widened values is the same sum up to its order), adds the fp32
bias and the widened bf16 residual, applies ReLU and rounds ONCE to bf16.  Max-pool is exact on bf16 values; AvgPool2d(7) + ReLU
reads bf16 and writes fp32; fc1, feat_encoder, the three IEF iterations and the hand classifier are fp32 as in the default path.
"""
import torch
import torch.nn.functional as F


def r(t):
    """Round to bf16 (nearest even) and widen back."""
    return t.bfloat16().float()


def cv(x, conv, bn, stride, pad, res=None, relu=True, conv_dtype=torch.float32):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    w, b = conv.weight * s[:, None, None, None], bn.bias - bn.running_mean * s
    if conv_dtype == torch.float32:
        y = F.conv2d(x, r(w), b, stride=stride, padding=pad)          # bf16 x bf16 products are exact in fp32
    else:
        y = F.conv2d(x.to(conv_dtype), r(w).to(conv_dtype), None, stride=stride, padding=pad).float() + b[None, :, None, None]
    if res is not None:
        y = y + res
    return r(torch.relu(y) if relu else y)


@torch.no_grad()
def trunk(me, img, conv_dtype=torch.float32):
    """``me``: a ResNet-50 container with the reference's attribute names (conv1, bn1, layer1..4 of bottlenecks with conv1..3, bn1..3,
    downsample); returns the fp32 feature after AvgPool2d(7) + ReLU, [B][2048].  ``conv_dtype=torch.float64`` takes the conv sums in
    float64 (a proxy for what another fp32 summation order changes)."""
    x = r(img)
    x = cv(x, me.conv1, me.bn1, 2, 3, conv_dtype=conv_dtype)
    x = F.max_pool2d(x, 3, 2, 1)
    for li in range(1, 5):
        for blk in getattr(me, f"layer{li}"):
            stride = blk.conv2.stride[0]
            y = cv(x, blk.conv1, blk.bn1, 1, 0, conv_dtype=conv_dtype)
            y = cv(y, blk.conv2, blk.bn2, stride, 1, conv_dtype=conv_dtype)
            res = x if blk.downsample is None else cv(x, blk.downsample[0], blk.downsample[1], stride, 0, relu=False, conv_dtype=conv_dtype)
            x = cv(y, blk.conv3, blk.bn3, 1, 0, res=res, conv_dtype=conv_dtype)
    return torch.relu(F.avg_pool2d(x, 7).flatten(1))


@torch.no_grad()
def encoder(enc, img, conv_dtype=torch.float32):
    """``enc``: an InterHandEncoder container (main_encoder, feat_encoder, regressor_ih, hand_classifier, mean_params).
    Returns (main_feat, params, hand_class), all fp32."""
    me = enc.main_encoder
    main_feat = torch.relu(me.fc1(trunk(me, img, conv_dtype)))
    feat = torch.relu(enc.feat_encoder[1](torch.relu(main_feat)))
    params = enc.mean_params
    if params.shape[0] != img.shape[0]:
        params = params[:1].expand(img.shape[0], -1)
    for _ in range(3):
        params = params + enc.regressor_ih[0](torch.cat([feat, params], dim=1))
    return main_feat, params, torch.sigmoid(enc.hand_classifier[0](feat))

"""The IHMR-MLP stage head (``ihmr_mlp_stage_head``: four Linear layers as 16 x 16 output tiles, at most MLPI_MAX_WG = 256
workgroups per layer, the residual added to the stage's columns and scattered into the fused kernels' parameter buffers)
driven directly through the C ABI and compared with float64, layer by layer, up to batches where every layer's
workgroups walk more than one tile."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MLPI_MAX_WG = 256                           # csrc/mlp_infer.h
U = 2.0 ** -24                              # unit roundoff of fp32


def _gamma(n):
    return n * U / (1 - n * U)


def _tiles(B, k_out):
    """Tiles per layer as ihmr_mlp_stage_head launches them: ceil(B / 16) row tiles x (32, 16, 8, ceil(k_out / 16)) column tiles."""
    tr = (B + 15) // 16
    return [tr * 32, tr * 16, tr * 8, tr * ((k_out + 15) // 16)]


def _stages():
    """The distinct widths of make_mlp_strategy's stages (3, 20, 90) with their real column maps (mlp_model.py's order)."""
    from ihmr_amd.mlp_model import COLS
    from ihmr_amd.strategies import make_mlp_strategy
    out = {}
    for st in make_mlp_strategy():
        cols = [c for n in st["update_params"] for c in range(COLS[n].start, COLS[n].stop)]
        out.setdefault(len(cols), cols)
    assert sorted(out) == [3, 20, 90]
    return [(k, out[k]) for k in sorted(out)]


def _check_layer(name, got, a, w, b, relu, extra=None):
    """got (B, N) fp32 vs float64 act(a @ w + b [+ extra]).  Per element the bar is gamma_{K+1} sum_k |a_k w_k| + u |b|
    (+ gamma_2 |extra| for the residual the last layer adds): the forward error bound of ANY summation order of an fp32 dot
    product, fmaf chains and MFMA included.  Dropping or duplicating one 16-wide K chunk moves an element by about
    sqrt(16 / K) of its own scale, ~50 x the bar at K = 128 and ~300 x at K = 1146; a tile stored at the wrong place or
    read from the wrong rows is off by the element itself.  The self-check below shows that a chunk drop fails the bar."""
    K = a.shape[1]
    ref = a @ w + b
    if extra is not None:
        ref = ref + extra
    bar = _gamma(K + 1) * (a.abs() @ w.abs()) + U * b.abs()
    if extra is not None:
        bar = bar + _gamma(2) * (extra.abs() + ref.abs())
    if relu:
        ref = ref.clamp_min(0)
    err = (got.double() - ref).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    print(f"[parity] {name}: max|err|={float(err.max()):.3e} max|ref|={float(ref.abs().max()):.3e} max err / bar = {ratio:.3f}")
    assert bool((err <= bar).all()), f"{name}: {int((err > bar).sum())} elements beyond the bar, worst err / bar {ratio:.2f}"
    # the bar's power: the same layer with one 16-wide K chunk left out is beyond it almost everywhere
    j = (K // 16) // 2 * 16
    drop = a[:, j:j + 16] @ w[j:j + 16]
    beyond = float((drop.abs() > 2 * bar).double().mean()) if drop.numel() else 1.0
    assert beyond > 0.5, (name, beyond)


@pytest.mark.parametrize("B", [1, 17, 128, 129, 513, 1000, 4100])
def test_mlp_stage_head_matches_float64(B):
    from helpers import seeded_state_dict
    from ihmr_amd import hip
    from ihmr_amd.networks import InterHandSubNetwork
    L, dev = hip.lib(), torch.device("cuda")
    tiles = _tiles(B, 90)
    loops = [t > MLPI_MAX_WG for t in tiles]
    print(f"[parity] MLP head B={B}: tiles per layer (k_out = 90) {tiles}, workgroups {[min(t, MLPI_MAX_WG) for t in tiles]}")
    # the path: up to B = 128 no workgroup runs a second tile (what every earlier test reached); from 129 layer 0 loops, from 513
    # layers 0-2, from 673 also layer 3 at k_out = 90, and at 4100 every layer at every width
    assert loops == [B > 128, B > 256, B > 512, B > 672]
    if B == 4100:
        assert all(t > MLPI_MAX_WG for k in (3, 20, 90) for t in _tiles(B, k))
    g = torch.Generator().manual_seed(B)
    feat = torch.randn(B, 1024, generator=g).to(dev)
    prev = (torch.randn(B, 122, generator=g) * 0.5).to(dev)
    for sid, (k_out, cols) in enumerate(_stages()):
        net = InterHandSubNetwork(None, 1146, k_out)
        net.load_state_dict(seeded_state_dict(net, 900 + sid, last_scale=0.02))
        pk = net.packed(dev)
        cn = hip.MlpNet()
        for l in range(4):
            cn.w[l], cn.b[l], cn.ldw[l] = pk[l].w.data_ptr(), pk[l].b.data_ptr(), pk[l].ldw
        cn.k_out = k_out
        for j, c in enumerate(cols):
            cn.col[j] = c
        new = torch.full((B, 122), float("nan"), device=dev)
        tab = hip.MlpTables(img_feat=feat.data_ptr(), final_params=prev.data_ptr(), new_params=new.data_ptr())
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        bufs = dict(cam=nan(B, 3), trans=nan(B, 3), orient=nan(2, B, 3), pose=nan(2, B, 45), shape=nan(2, B, 10))
        io = hip.OptIO()
        for k, v in bufs.items():
            setattr(io, k, v.data_ptr())
        nbytes = L.ihmr_mlp_workspace_bytes(B)
        assert nbytes >= 256 + B * (512 + 256 + 128) * 4
        ws = torch.full((nbytes // 4,), float("nan"), device=dev)
        hip.check(L.ihmr_mlp_stage_head(C.byref(cn), C.byref(tab), C.byref(io), B, ws.data_ptr(), hip.stream_ptr()), "ihmr_mlp_stage_head")
        torch.cuda.synchronize()
        h = ws[64:64 + B * (512 + 256 + 128)]                    # h[0..2] at byte offset 256 of the workspace
        h0, h1, h2 = h[:B * 512].view(B, 512), h[B * 512:B * 768].view(B, 256), h[B * 768:].view(B, 128)
        W = [p.w.double() for p in pk]
        bias = [p.b.double() for p in pk]
        a0 = torch.cat([feat, prev], 1).double()
        tag = f"B={B} k_out={k_out}"
        _check_layer(f"head layer 0 {tag}", h0, a0, W[0][:1146, :512], bias[0], True)
        _check_layer(f"head layer 1 {tag}", h1, h0.double(), W[1][:512, :256], bias[1], True)
        _check_layer(f"head layer 2 {tag}", h2, h1.double(), W[2][:256, :128], bias[2], True)
        _check_layer(f"head layer 3 + residual {tag}", new[:, cols], h2.double(), W[3][:128, :k_out], bias[3], False,
                     extra=prev[:, cols].double())
        others = [c for c in range(122) if c not in cols]
        assert torch.equal(new[:, others], prev[:, others]), f"{tag}: a column the stage does not update changed"
        # the scattered parameter buffers = new_params, bit for bit (opt_unpack_params_kernel's layout)
        assert torch.equal(bufs["cam"], new[:, 0:3]) and torch.equal(bufs["trans"], new[:, 119:122]), tag
        assert torch.equal(bufs["orient"][0], new[:, 3:6]) and torch.equal(bufs["orient"][1], new[:, 51:54]), tag
        assert torch.equal(bufs["pose"][0], new[:, 6:51]) and torch.equal(bufs["pose"][1], new[:, 54:99]), tag
        assert torch.equal(bufs["shape"][0], new[:, 99:109]) and torch.equal(bufs["shape"][1], new[:, 109:119]), tag

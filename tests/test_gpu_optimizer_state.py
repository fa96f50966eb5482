"""The optimizer of the two trainers at trainer level: the layout of the flat buffers, the step counter and the interchange of
the Adam state with ``torch.optim.Adam`` in torch's own format -- HeadTrainer (IHMR-MLP; ``InterHandSubNetwork(None, 1146, 90)``
at B = 20: 32 padded rows, kpad 1152 > 1146, ldw 128 > 90) and EncoderTrainer (IHMR-Baseline; the whole encoder at B = 2).

Gradients are injected, not computed: per parameter (named as the reference's state_dict) and per step a seeded tensor of the
`steady` class, +-U[0.1, 1] -- nothing is symmetric under transposition, no entry is near zero (no ill-conditioned update), every
parameter and every step has its own seed, so a swapped index, a K-major weight where torch expects [out][in] or a mis-read step
shows as an error of the size of the quantity itself.  They are written with the trainer's own ``_from_named`` and applied with
``optimizer_step()``; the float64 reference is ``torch.optim.Adam`` on a float64 copy of the module fed the same tensors, the
yardstick the same on an fp32 copy.  The rule, per parameter and per quantity, is that of tests/test_gpu_adam.py:

    max |HIP - float64| <= 3 x max |torch-fp32 - float64| + 2**-23 x max |float64|

with HIP measured from the float64 run that has the float-rounded lr, betas and eps the entry point receives, and torch-fp32
from the float64 run with the decimal constants it was given itself (the two float64 runs differ by the beta rounding that
DESIGN.md and tests/adam_ref.py derive: 1.29e-5 of exp_avg_sq, 2.4e-7 of exp_avg -- 50 and 5 times the bar here).
"""
import copy
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 4                                # steps before the state changes hands; step K + 1 is taken on both sides
KINDS = ("head", "encoder")


def _gradient(index, shape, step):
    rng = np.random.RandomState(40000 + 1000 * step + index)
    mag = rng.uniform(0.1, 1.0, shape)
    return torch.tensor(np.where(rng.randint(0, 2, shape) > 0, mag, -mag), dtype=torch.float32)


def _make(kind):
    """(module with seeded weights on the CPU, lr, factory of the trainer for a module on the GPU)."""
    from helpers import seeded_state_dict
    dev = torch.device("cuda")
    if kind == "head":
        from ihmr_amd.mlp_train import HeadTrainer
        from ihmr_amd.networks import InterHandSubNetwork
        mod = InterHandSubNetwork(None, 1146, 90)
        mod.load_state_dict(seeded_state_dict(mod, 4100))
        return mod, 1e-3, lambda m: HeadTrainer(m, 20, 1e-3, dev)
    from ihmr_amd.encoder_train import EncoderTrainer
    from ihmr_amd.networks import InterHandEncoder
    mean = torch.tensor(np.random.RandomState(3).normal(0, 0.2, (1, 122)), dtype=torch.float32)
    mod = InterHandEncoder(types.SimpleNamespace(total_params_dim=122), mean.repeat(2, 1))
    mod.load_state_dict(seeded_state_dict(mod, 4200))
    return mod, 1e-4, lambda m: EncoderTrainer(m, 2, 1e-4, dev)


def _flat(tr):
    """The trainer's flat (params, grads, exp_avg, exp_avg_sq)."""
    f = getattr(tr, "flat", tr)
    return f.params, f.grads, f.exp_avg, f.exp_avg_sq


def _named_mask(kind, tr):
    """bool per element of the flat buffers: True where a named parameter entry lives -- worked out from the layout alone
    (offsets, kpad / ldw, filter geometry), not with the trainer's own _to_named / _from_named."""
    n = _flat(tr)[0].numel()
    mask = np.zeros(n, bool)
    if kind == "head":
        for l, (i, o) in enumerate(tr.dims):
            w = mask[tr.offsets[2 * l]:tr.offsets[2 * l + 1]].reshape(tr.kpad[l], tr.ldw[l])
            w[:i, :o] = True                                          # rows in_f..kpad and columns out_f..ldw are padding
            mask[tr.offsets[2 * l + 1]:tr.offsets[2 * l + 1] + o] = True    # the bias; its tail up to ldw is padding
        assert tr.kpad[0] > tr.dims[0][0] and tr.ldw[3] > tr.dims[3][1]
        return mask
    spec = {name: (shape, off) for name, shape, off, _ in tr.flat.specs}
    for u in tr.units:
        (rows, ld), off = spec[u["name"] + ".w"]
        w = mask[off:off + rows * ld].reshape(rows, ld)
        k, cin, cout = u["k"], u["cin"], u["cout"]
        real_cin = 3 if u is tr.stem else cin                         # the stem's fourth input channel is padding
        r = np.arange(rows)
        w[np.ix_((r < k * k * cin) & (r % cin < real_cin), np.arange(ld) < cout)] = True
        for s in (".gamma", ".beta"):
            (c,), off = spec[u["name"] + s]
            mask[off:off + c] = True
    for l in (tr.fc1, tr.feat, tr.reg, tr.cls):
        (rows, ld), off = spec[l.name + ".weight"]
        mask[off:off + rows * ld].reshape(rows, ld)[:l.in_f, :l.out_f] = True
        mask[spec[l.name + ".bias"][1]:spec[l.name + ".bias"][1] + l.out_f] = True
    return mask


def _params(mod):
    return {k: v.detach().cpu().clone() for k, v in mod.named_parameters()}


def _state(opt, names):
    sd = opt.state_dict()["state"]
    return {q: {k: sd[i][q].clone() for i, k in enumerate(names)} for q in ("exp_avg", "exp_avg_sq")}, [float(sd[i]["step"]) for i in range(len(names))]


@functools.lru_cache(maxsize=None)
def _scenario(kind):
    """Runs everything once per trainer and returns what the tests compare (CPU tensors keyed by parameter name)."""
    mod, lr, make = _make(kind)
    names = [k for k, _ in mod.named_parameters()]
    shapes = [tuple(v.shape) for _, v in mod.named_parameters()]
    grads = lambda step: {k: _gradient(i, s, step) for i, (k, s) in enumerate(zip(names, shapes))}
    ref32, ref64, ref64r = copy.deepcopy(mod), copy.deepcopy(mod).double(), copy.deepcopy(mod).double()
    opt32 = torch.optim.Adam(ref32.parameters(), lr=lr, foreach=False)
    opt64 = torch.optim.Adam(ref64.parameters(), lr=lr, foreach=False)
    f = lambda x: float(np.float32(x))                            # the constants as ihmr_adam_step receives them
    opt64r = torch.optim.Adam(ref64r.parameters(), lr=f(lr), betas=(f(0.9), f(0.999)), eps=f(1e-8), foreach=False)

    def torch_step(m, opt, g):
        for k, p in m.named_parameters():
            p.grad = g[k].to(p.dtype)
        opt.step()

    gpu_mod = copy.deepcopy(mod).cuda()
    tr = make(gpu_mod)
    out = dict(names=names, lr=lr, shapes=shapes)
    for step in range(1, K + 1):
        g = grads(step)
        tr._from_named(_flat(tr)[1], g)
        tr.optimizer_step()
        torch_step(ref32, opt32, g)
        torch_step(ref64, opt64, g)
        torch_step(ref64r, opt64r, g)
    torch.cuda.synchronize()
    # ---- after K steps: weights, torch-format state, padding
    tr.sync_to_module()
    out["hip_K"], out["t32_K"], out["f64_K"], out["f64r_K"] = _params(gpu_mod), _params(ref32), _params(ref64), _params(ref64r)
    osd = tr.optimizer_state_dict()
    out["hip_osd"] = osd
    out["t32_state_K"], _ = _state(opt32, names)
    out["f64_state_K"], _ = _state(opt64, names)
    out["f64r_state_K"], _ = _state(opt64r, names)
    mask = _named_mask(kind, tr)
    out["n_named"], out["n_flat"] = int(mask.sum()), mask.size
    out["padding_K"] = {q: int(np.count_nonzero(b.cpu().numpy()[~mask])) for q, b in zip(("params", "grads", "exp_avg", "exp_avg_sq"), _flat(tr))}
    out["step_K"] = tr.step
    sd32_K, osd32_K = copy.deepcopy(ref32.state_dict()), copy.deepcopy(opt32.state_dict())
    # ---- HIP -> torch: a torch optimizer over the synced weights loads the trainer's state; step K + 1 on every side
    mod_t = copy.deepcopy(gpu_mod).cpu()
    opt_t = torch.optim.Adam(mod_t.parameters(), lr=lr, foreach=False)
    opt_t.load_state_dict(copy.deepcopy(osd))          # (torch adopts the tensors it is given and steps them in place)
    g = grads(K + 1)
    torch_step(mod_t, opt_t, g)
    torch_step(ref32, opt32, g)
    torch_step(ref64, opt64, g)
    torch_step(ref64r, opt64r, g)
    tr._from_named(_flat(tr)[1], g)
    tr.optimizer_step()
    tr.sync_to_module()
    out["hip_K1"], out["hip_to_torch_K1"], out["t32_K1"], out["f64_K1"] = _params(gpu_mod), _params(mod_t), _params(ref32), _params(ref64)
    out["f64r_K1"] = _params(ref64r)
    out["hip_to_torch_steps"] = _state(opt_t, names)[1]
    # ---- torch -> HIP: the trainer loads torch's fp32 weights and state after K steps and takes step K + 1
    gpu_mod.load_state_dict(sd32_K)
    tr.load_from_module()
    tr.load_optimizer_state_dict(osd32_K)
    out["torch_to_hip_step_loaded"] = tr.step
    tr._from_named(_flat(tr)[1], g)
    tr.optimizer_step()
    tr.sync_to_module()
    torch.cuda.synchronize()
    out["torch_to_hip_K1"], out["torch_to_hip_step"] = _params(gpu_mod), tr.step
    out["padding_end"] = {q: int(np.count_nonzero(b.cpu().numpy()[~mask])) for q, b in zip(("params", "grads", "exp_avg", "exp_avg_sq"), _flat(tr))}
    return out


def _rule(tag, got, ref64r, t32, ref64):
    """got against ref64r (float64, float-rounded constants); the yardstick t32 against ref64 (float64, decimal constants)."""
    assert list(got) == list(ref64r) == list(t32) == list(ref64), f"{tag}: parameter names / order differ"
    for k in ref64r:
        assert tuple(got[k].shape) == tuple(ref64r[k].shape), f"{tag} {k}: shape {tuple(got[k].shape)} != {tuple(ref64r[k].shape)}"
        r = ref64r[k].double()
        e_hip = float((got[k].double() - r).abs().max())
        e_t32 = float((t32[k].double() - ref64[k].double()).abs().max())
        bar = 3.0 * e_t32 + 2.0 ** -23 * float(r.abs().max())
        print(f"[parity] {tag} {k} vs float64: HIP {e_hip:.3e} torch-fp32 {e_t32:.3e} bar {bar:.3e}")
        assert e_hip <= bar, f"{tag} {k}: HIP vs float64 {e_hip:.3e} > {bar:.3e}"


@pytest.mark.parametrize("kind", KINDS)
def test_injected_gradients_weights_and_torch_format_state(kind):
    """K = 4 steps on injected gradients: the weights after ``sync_to_module()`` and ``optimizer_state_dict()``'s exp_avg,
    exp_avg_sq (under torch's parameter indices, torch layouts) and step of every parameter against float64."""
    s = _scenario(kind)
    names = s["names"]
    _rule(f"{kind} weights after {K} steps", s["hip_K"], s["f64r_K"], s["t32_K"], s["f64_K"])
    osd = s["hip_osd"]
    assert sorted(osd["state"]) == list(range(len(names))) and osd["param_groups"][0]["params"] == list(range(len(names)))
    assert osd["param_groups"][0]["lr"] == s["lr"] and tuple(osd["param_groups"][0]["betas"]) == (0.9, 0.999)
    for q in ("exp_avg", "exp_avg_sq"):
        got = {k: osd["state"][i][q] for i, k in enumerate(names)}
        _rule(f"{kind} state {q} after {K} steps", got, s["f64r_state_K"][q], s["t32_state_K"][q], s["f64_state_K"][q])
    assert all(float(osd["state"][i]["step"]) == K for i in range(len(names))) and s["step_K"] == K


@pytest.mark.parametrize("kind", KINDS)
def test_padding_of_the_flat_buffers_stays_zero(kind):
    """Adam runs over the whole flat buffer and the forward GEMMs read its padding (kpad rows, ldw columns): after the K steps,
    and again after the state has been loaded from torch and stepped, every entry of params, exp_avg and exp_avg_sq outside the
    named views is exactly 0 -- rows in_f..kpad and columns out_f..ldw of each weight, the bias tails, the stem's fourth input
    channel, the 16-byte alignment filler of _Flat."""
    s = _scenario(kind)
    n_params = sum(int(np.prod(sh)) for sh in s["shapes"])
    assert s["n_named"] == n_params and s["n_flat"] > n_params, (s["n_named"], n_params, s["n_flat"])
    print(f"[parity] {kind}: {s['n_flat'] - s['n_named']} padding entries of {s['n_flat']}; non-zero after {K} steps {s['padding_K']}, "
          f"at the end {s['padding_end']}")
    assert not any(s["padding_K"].values()), s["padding_K"]
    assert not any(s["padding_end"].values()), s["padding_end"]


@pytest.mark.parametrize("kind", KINDS)
def test_state_hip_to_torch(kind):
    """``torch.optim.Adam(module.parameters()).load_state_dict(trainer.optimizer_state_dict())`` on a torch copy with the synced
    weights; both sides take step K + 1 on the same injected gradient: the trainer's weights and the torch continuation's both
    meet the rule against the float64 run (a state that torch reads differently -- index, layout, step -- moves the weights by
    a good part of lr)."""
    s = _scenario(kind)
    assert s["hip_to_torch_steps"] == [float(K + 1)] * len(s["names"])
    _rule(f"{kind} weights after step {K + 1}", s["hip_K1"], s["f64r_K1"], s["t32_K1"], s["f64_K1"])
    _rule(f"{kind} weights after step {K + 1}, torch continuing from the trainer's state", s["hip_to_torch_K1"], s["f64r_K1"], s["t32_K1"], s["f64_K1"])


@pytest.mark.parametrize("kind", KINDS)
def test_state_torch_to_hip(kind):
    """torch runs K fp32 steps; the trainer loads those weights and ``load_optimizer_state_dict(opt.state_dict())``; both take
    step K + 1: the weights meet the rule, the trainer's step is K, then K + 1."""
    s = _scenario(kind)
    assert s["torch_to_hip_step_loaded"] == K and s["torch_to_hip_step"] == K + 1
    _rule(f"{kind} weights after step {K + 1}, the trainer continuing from torch's state", s["torch_to_hip_K1"], s["f64r_K1"], s["t32_K1"], s["f64_K1"])

"""``ihmr_adam_step`` (adam_flat_kernel, csrc/train.h) through the C ABI, past step one: against the float64 reference of
tests/adam_ref.py (pinned to torch's float64 Adam by tests/test_adam_ref_cpu.py) on the same seeded gradients, with
``torch.optim.Adam`` in fp32 on the CPU as the yardstick of what fp32 can do.

The rule (the suite's own, per quantity and per case):

    max |HIP - float64| <= 3 x max |torch-fp32 - torch-float64| + 2**-23 x max |float64|

HIP is measured from the float64 reference with the float-rounded constants the entry point receives; torch-fp32 from torch's
float64 Adam with the decimal betas it was given.  The floor of one fp32 ulp of the quantity's scale covers the cases where
torch-fp32 happens to be exact.  Every comparison prints a ``[parity]`` line before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                          # floats on each side of every buffer
SENTINEL = 0x4B1D5EA7               # their bit pattern (a finite float, 1.03e7)
CASES = [(k, "zero") for k in R.KINDS] + [("steady", "normal")]


class _Guarded:
    """n floats inside a larger device allocation, 64 sentinel words on each side."""

    def __init__(self, host):
        host = np.ascontiguousarray(host, np.float32)
        self.n = host.size
        self.full = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.full[GUARD:GUARD + self.n].view(torch.float32)
        self.t.copy_(torch.from_numpy(host))

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def host(self):
        return self.t.cpu().numpy()

    def bits(self):
        return self.full.cpu().numpy().copy()

    def guards_intact(self):
        f = self.full.cpu().numpy()
        return bool((f[:GUARD] == SENTINEL).all() and (f[GUARD + self.n:] == SENTINEL).all())


def _adam(p, g, m, v, n, grad_scale, step, lr=R.LR):
    from ihmr_amd import hip
    return hip.lib().ihmr_adam_step(p, g, m, v, n, grad_scale, lr, R.BETA1, R.BETA2, R.EPS, step, hip.stream_ptr())


def _run_hip(p0, grads, grad_scale=1.0, first_step=1, m0=None, v0=None):
    """The entry point over `grads`, one launch per gradient; checks the guards of all four buffers and that `grads` comes back
    unchanged; returns fp32 (p, exp_avg, exp_avg_sq)."""
    z = np.zeros(len(p0), np.float32)
    p, m, v = _Guarded(p0), _Guarded(z if m0 is None else m0), _Guarded(z if v0 is None else v0)
    for i, g in enumerate(grads):
        gb = _Guarded(g)
        assert _adam(p.ptr(), gb.ptr(), m.ptr(), v.ptr(), len(p0), grad_scale, first_step + i) == 0
        assert np.array_equal(gb.host().view(np.int32), np.asarray(g, np.float32).view(np.int32)), "the gradient was written"
        assert gb.guards_intact(), "guard of grads"
    torch.cuda.synchronize()
    for name, b in (("params", p), ("exp_avg", m), ("exp_avg_sq", v)):
        assert b.guards_intact(), f"guard of {name}"
    return p.host(), m.host(), v.host()


def _torch_adam(p0, grads, dtype, grad_scale, first_step=1, m0=None, v0=None):
    """torch.optim.Adam(lr, (0.9, 0.999), 1e-8, foreach=False) on the CPU in `dtype`, fed the same fp32 gradients times the
    float grad_scale (the product formed in `dtype`), optionally from a given state."""
    p = torch.nn.Parameter(torch.tensor(np.asarray(p0, np.float32)).to(dtype))
    opt = torch.optim.Adam([p], lr=R.LR, betas=(R.BETA1, R.BETA2), eps=R.EPS, foreach=False)
    if first_step > 1:
        opt.state[p] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=torch.tensor(m0).to(dtype), exp_avg_sq=torch.tensor(v0).to(dtype))
    gs = torch.tensor(np.float32(grad_scale)).to(dtype)
    for g in grads:
        p.grad = torch.tensor(g).to(dtype) * gs
        opt.step()
    st = opt.state[p]
    assert int(st["step"]) == first_step - 1 + len(grads)
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _rule(name, got, ref64, t32, t64):
    ref64 = np.asarray(ref64, np.float64)
    e_hip = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    e_t32 = float(np.abs(np.asarray(t32, np.float64) - np.asarray(t64, np.float64)).max())
    bar = 3.0 * e_t32 + 2.0 ** -23 * float(np.abs(ref64).max())
    print(f"[parity] {name} vs float64: HIP {e_hip:.3e} torch-fp32 {e_t32:.3e} bar {bar:.3e}")
    assert np.all(np.isfinite(got)), name
    assert e_hip <= bar, f"{name}: HIP vs float64 {e_hip:.3e} > {bar:.3e}"
    return bar


@pytest.mark.parametrize("grad_scale", R.GRAD_SCALES, ids=["scale1", "scale1_8", "scale1_3"])
@pytest.mark.parametrize("T", R.MANY_STEPS_T)
@pytest.mark.parametrize("kind,init", CASES, ids=[f"{k}-from-{i}" for k, i in CASES])
def test_many_steps_from_zero_state(kind, init, T, grad_scale):
    """T steps from zero moments at n = 4100 (17 blocks, the last one partial): p, exp_avg and exp_avg_sq after the last step
    under the rule above.  A wrong beta, bias correction, moment update or grad_scale is 1e-3 relative or more from T = 2 on.

    Separately, the distance of the final moments from the float64 reference with the DECIMAL betas: the kernel forms
    1.0f - beta from the float betas, so a gradient enters exp_avg_sq with the weight 1 - float32(0.999), 1.29e-5 relative from
    0.001, and exp_avg with 1 - float32(0.9), 2.4e-7 from 0.1 (adam_ref.beta_rounding()).  The distance must be within that
    constant (times max exp_avg_sq; for exp_avg, whose terms carry signs, times max |exp_avg|) plus the rounding bar of the
    rule.  Where the gradients have stopped (`decay`) the moment is a pure power of the beta, and d steps of decay add
    d x |float32(beta) / beta - 1| (1.29e-8 and 2.65e-8 per step): the float64 references alone are 10.6 x 2.4e-7 apart in exp_avg
    after 100 such steps, so the constant of that class is the derived sum of the two."""
    n = R.MANY_STEPS_N
    p0 = R.initial_params(init, n)
    grads = list(R.gradients(kind, n, T, seed=11))
    ref = R.run(p0, grads, grad_scale=grad_scale)
    got = _run_hip(p0, grads, grad_scale)
    t32 = _torch_adam(p0, grads, torch.float32, grad_scale)
    t64 = _torch_adam(p0, grads, torch.float64, grad_scale)
    tag = f"adam {kind} from {init} T={T} grad_scale={grad_scale:.4g}"
    bars = [_rule(f"{tag} {q}", got[i], ref[i], t32[i], t64[i]) for i, q in enumerate(("p", "exp_avg", "exp_avg_sq"))]
    exact = R.run(p0, grads, grad_scale=float(np.float32(grad_scale)), exact=True)
    c1, c2 = R.beta_rounding()
    d = T - T // 2 if kind == "decay" else 0                      # steps of pure decay at the end
    c1 += d * abs(float(np.float32(R.BETA1)) / R.BETA1 - 1.0)
    c2 += d * abs(float(np.float32(R.BETA2)) / R.BETA2 - 1.0)
    for i, q, c in ((1, "exp_avg", c1), (2, "exp_avg_sq", c2)):
        dist, scale = float(np.abs(got[i].astype(np.float64) - exact[i]).max()), float(np.abs(exact[i]).max())
        print(f"[parity] {tag} {q} vs float64 with decimal betas: HIP {dist:.3e} = {dist / scale if scale else 0.0:.3e} relative; "
              f"constant {c:.3e} x {scale:.3e} + rounding bar {bars[i]:.3e}")
        assert dist <= c * scale + bars[i], (q, dist, c * scale + bars[i])
    if kind == "zero":                                             # exactly: nothing moves
        assert np.array_equal(got[0].view(np.int32), p0.view(np.int32)) and not got[1].any() and not got[2].any()


@pytest.mark.parametrize("step", R.FROM_STATE_STEPS)
def test_one_step_from_a_given_state(step):
    """The float64 reference runs step - 1 steady steps; its p, exp_avg, exp_avg_sq rounded to fp32 are uploaded and the entry is
    called once with that step number: bias corrections far from 1 (step 1, 2, 10), near it (1000) and at their limit (1e5:
    bc1 = 1, bc2 = 1 - 4e-44) without a thousand launches.  The comparators take the same single step from the same fp32 state.
    step - 1 passed for step, a dropped or squared bias correction: 5e-4 .. 0.5 of the update at step 2, 1e-2 of it at step 10."""
    p0, m0, v0, g = R.state_before(step)
    assert p0.shape == (R.FROM_STATE_N,)
    ref = R.run(p0, [g], first_step=step, m0=m0, v0=v0)
    got = _run_hip(p0, [g], 1.0, step, m0, v0)
    t32 = _torch_adam(p0, [g], torch.float32, 1.0, step, m0, v0)
    t64 = _torch_adam(p0, [g], torch.float64, 1.0, step, m0, v0)
    for i, q in enumerate(("p", "exp_avg", "exp_avg_sq")):
        _rule(f"adam one step at step={step} {q}", got[i], ref[i], t32[i], t64[i])


@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_guards_and_untouched_gradients(n):
    """3 steps at sizes around the block of 256 and at 2**20 + 3: every entry under the rule (an entry left out or done twice is
    off by lr or more), the 64 sentinel floats on each side of params, grads, exp_avg and exp_avg_sq unchanged, grads unchanged."""
    p0 = R.initial_params("normal", n, seed=n % 1000)
    grads = list(R.gradients("steady", n, 3, seed=n % 1000))
    ref = R.run(p0, grads, grad_scale=0.5)
    got = _run_hip(p0, grads, 0.5)
    t32 = _torch_adam(p0, grads, torch.float32, 0.5)
    t64 = _torch_adam(p0, grads, torch.float64, 0.5)
    for i, q in enumerate(("p", "exp_avg", "exp_avg_sq")):
        _rule(f"adam n={n} {q}", got[i], ref[i], t32[i], t64[i])


def test_exact_properties():
    """Zero-gradient entries keep their parameter bit for bit and m = v = 0; permuting the entries permutes the three outputs
    bit for bit (no entry sees another, no dependence on the position in the block or wave); two runs give the same bits; all
    finite in the `wide` class (gradients 1e-7 .. 1e3) and after `decay`."""
    n, T = 4100, 6
    rng = np.random.RandomState(8)
    p0 = R.initial_params("normal", n)
    p0[::7] = -0.0
    grads = [g.copy() for g in R.gradients("wide", n, T, seed=2)]
    dead = rng.rand(n) < 0.25
    for g in grads:
        g[dead] = 0.0
    a = _run_hip(p0, grads, 1.0 / 3.0)
    b = _run_hip(p0, grads, 1.0 / 3.0)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), "two runs differ"
        assert np.all(np.isfinite(x))
    assert np.array_equal(a[0][dead].view(np.int32), p0[dead].view(np.int32)), "a parameter with zero gradient moved"
    assert not a[1][dead].any() and not a[2][dead].any()
    assert np.all(a[2][~dead] > 0)
    perm = rng.permutation(n)
    c = _run_hip(p0[perm], [g[perm] for g in grads], 1.0 / 3.0)
    for x, y in zip(a, c):
        assert np.array_equal(x[perm].view(np.int32), y.view(np.int32)), "not a per-entry map"
    for kind in ("wide", "decay"):
        out = _run_hip(R.initial_params("zero", n), list(R.gradients(kind, n, 40, seed=4)), 1.0)
        assert all(np.all(np.isfinite(x)) for x in out), kind


def test_refusals_write_nothing():
    """step = 0, n = 0 or a null pointer: non-zero return and no byte written.  Every other argument of each call is one a
    launch could use (live buffers of n floats), so a missing check would show as a write, not as a fault."""
    n = 300
    rng = np.random.RandomState(1)
    bufs = [_Guarded(rng.uniform(0.5, 1.0, n).astype(np.float32)) for _ in range(4)]      # p, g, m, v (v > 0)
    before = [b.bits() for b in bufs]
    ptrs = [b.ptr() for b in bufs]
    assert _adam(*ptrs, n, 1.0, 0) != 0
    assert _adam(*ptrs, n, 1.0, -3) != 0
    assert _adam(*ptrs, 0, 1.0, 1) != 0
    for k in range(4):
        args = list(ptrs)
        args[k] = None
        assert _adam(*args, n, 1.0, 1) != 0, f"null pointer {k}"
    torch.cuda.synchronize()
    for b, was in zip(bufs, before):
        assert np.array_equal(b.bits(), was)
    assert _adam(*ptrs, n, 1.0, 1) == 0                           # the same arguments with a valid step are taken
    torch.cuda.synchronize()
    assert not np.array_equal(bufs[0].bits(), before[0]) and np.array_equal(bufs[1].bits(), before[1])

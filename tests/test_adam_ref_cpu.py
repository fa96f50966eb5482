"""The float64 Adam reference of the GPU optimizer tests (tests/adam_ref.py) against ``torch.optim.Adam`` in float64, and the
properties of the shared gradient cases that those tests rely on."""
import numpy as np
import pytest
import torch

import adam_ref as R

ULP64 = 2.0 ** -52


def _torch_adam(p0, grads, dtype, lr, betas, eps):
    """torch.optim.Adam(foreach=False) on one tensor, fed `grads` (already scaled) one per step; returns (p, exp_avg, exp_avg_sq)."""
    p = torch.nn.Parameter(torch.tensor(np.asarray(p0), dtype=dtype))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    for g in grads:
        p.grad = torch.as_tensor(np.asarray(g)).to(dtype)
        opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("T", [1, 2, 10, 200])
@pytest.mark.parametrize("kind,init,grad_scale", [("steady", "zero", 1.0), ("wide", "zero", 1.0 / 3.0), ("decay", "normal", 0.125),
                                                  ("flip", "zero", 1.0), ("zero", "normal", 1.0)])
def test_reference_equals_torch_float64(kind, init, grad_scale, T, exact):
    """Same gradients, same betas (float-rounded or decimal): p, exp_avg and exp_avg_sq of the numpy statement equal torch's
    float64 Adam.  The statement performs torch's operations in torch's order, so the only room is a fused multiply-add where
    torch's vectorised kernels contract one (lerp, addcmul, addcdiv): one rounding per operation, at most one ulp (2**-52) of
    the quantity each, two such operations per quantity and step.  A moment that only decays (gradient 0) carries these on
    multiplicatively, so after T steps the rigorous bar is 2 + 2 T ulps of the quantity's scale -- max |exp_avg|,
    max |exp_avg_sq|, and for the parameter max |p| + T * max |update| with |update| <= lr / (1 - beta1).  (Measured: 0 to 11
    ulps; a wrong beta, bias correction or scale is 1e-3 relative or more, 1e13 ulps.)"""
    n = 257
    lr, b1, b2, eps, gs = R.constants(grad_scale=grad_scale, exact=exact)
    p0 = R.initial_params(init, n)
    grads = list(R.gradients(kind, n, T, seed=3))
    p, m, v = R.run(p0, grads, grad_scale=grad_scale, exact=exact)
    tp, tm, tv = _torch_adam(p0, [g.astype(np.float64) * gs for g in grads], torch.float64, lr, (b1, b2), eps)
    for name, got, ref, scale in (("p", p, tp, np.abs(tp).max() + T * lr / (1.0 - b1)), ("exp_avg", m, tm, np.abs(tm).max()),
                                  ("exp_avg_sq", v, tv, np.abs(tv).max())):
        err = float(np.abs(got - ref).max())
        print(f"[parity] adam_ref {name} {kind} T={T} exact={exact}: max|err| {err:.3e} = {err / (ULP64 * scale) if scale else 0.0:.2f} ulp of {scale:.3e}")
        assert err <= (2 + 2 * T) * ULP64 * scale, (name, err, scale)


def test_constants_are_the_floats_the_entry_point_receives():
    lr, b1, b2, eps, gs = R.constants(grad_scale=1.0 / 3.0)
    assert (lr, b1, b2, eps, gs) == tuple(float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8, 1.0 / 3.0))
    assert R.constants(grad_scale=1.0 / 3.0, exact=True) == (1e-3, 0.9, 0.999, 1e-8, 1.0 / 3.0)
    c1, c2 = R.beta_rounding()
    assert abs(c2 - 1.29e-5) < 1e-7 and abs(c1 - 2.4e-7) < 1e-8
    # the difference between the two references is that constant: one step from zero moments, v = (1 - beta2) g^2
    g = np.array([0.5], np.float32)
    v_f = R.adam_step([0.0], g, [0.0], [0.0], 1)[2]
    v_e = R.adam_step([0.0], g, [0.0], [0.0], 1, exact=True)[2]
    assert abs(abs(v_f[0] / v_e[0] - 1.0) - c2) < 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
def test_cases_are_deterministic_and_of_their_class(kind):
    n, T = 4100, 20
    a, b = list(R.gradients(kind, n, T, seed=1)), list(R.gradients(kind, n, T, seed=1))
    assert len(a) == T and all(x.dtype == np.float32 and x.shape == (n,) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    if kind != "zero":
        assert not np.array_equal(a[0], next(R.gradients(kind, n, T, seed=2)))
    live = a[:T // 2] if kind == "decay" else a
    if kind == "zero":
        assert all(not x.any() for x in a)
        return
    floor = np.float32(R.NONZERO_FLOOR.get(kind, 0.1))
    for x in live:
        assert np.abs(x).min() >= floor, (kind, float(np.abs(x).min()))
        assert np.abs(x).max() <= (1e3 if kind == "wide" else 1.0)
    if kind == "decay":
        assert all(not x.any() for x in a[T // 2:])
    if kind == "flip":
        for x, y in zip(a, a[1:]):
            assert np.array_equal(np.sign(x), -np.sign(y))
    if kind == "wide":                                          # the per-entry scale spans the nine decades
        s = np.abs(a[0])
        assert s.min() < 1e-5 and s.max() > 1e2
    if kind == "steady":                                        # both signs, fresh every step
        assert 0.4 < np.mean(a[0] > 0) < 0.6 and not np.array_equal(np.sign(a[0]), np.sign(a[1]))


def test_initial_params_and_states_are_deterministic():
    assert not R.initial_params("zero", 50).any()
    assert np.array_equal(R.initial_params("normal", 50), R.initial_params("normal", 50))
    p, m, v, g = R.state_before(1)
    assert not p.any() and not m.any() and not v.any() and np.abs(g).min() >= np.float32(0.1)
    p, m, v, g = R.state_before(10)
    ref = R.run(np.zeros(R.FROM_STATE_N), list(R.gradients("steady", R.FROM_STATE_N, 10, seed=5))[:9])
    for got, want in zip((p, m, v), ref):
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))

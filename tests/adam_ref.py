"""float64 numpy statement of one ``torch.optim.Adam`` step (no weight decay, no amsgrad) as ``ihmr_adam_step`` takes it, a driver
that runs a sequence of gradients through it, and the seeded gradient cases shared by tests/test_adam_ref_cpu.py (which pins this
file to torch's own float64 Adam) and the GPU tests of the optimizer.

Constants.  The C ABI takes lr, beta1, beta2, eps and grad_scale as ``float``; the kernel forms ``1.0f - beta`` and the host the
bias corrections from those floats.  ``constants(...)`` therefore returns ``float(np.float32(x))`` of each -- the values the
entry point receives -- and everything here (the bias corrections included) is computed from them in float64.
``exact=True`` gives the decimal constants as written (0.9, 0.999, ...): what torch's float64 Adam uses.  The two references
differ by a derived, bounded amount, ``beta_rounding()``:

    exp_avg_sq:  |(1 - float32(0.999)) / 0.001 - 1| = 1.29e-5 relative
    exp_avg:     |(1 - float32(0.9))   / 0.1   - 1| = 2.4e-7  relative
"""
import numpy as np

LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8
KINDS = ("steady", "wide", "decay", "zero", "flip")
NONZERO_FLOOR = {"steady": 0.1, "flip": 0.1, "wide": 0.1 * 10.0 ** -6}      # "bounded away from zero": min |g| of these classes


def constants(lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS, grad_scale=1.0, exact=False):
    c = (lr, beta1, beta2, eps, grad_scale)
    return tuple(float(x) for x in c) if exact else tuple(float(np.float32(x)) for x in c)


def beta_rounding(beta1=BETA1, beta2=BETA2):
    """Relative weight of a new gradient (1 - beta) as the kernel forms it from the float betas, against the decimal one."""
    rel = lambda b: abs((1.0 - float(np.float32(b))) / (1.0 - b) - 1.0)
    return rel(beta1), rel(beta2)


def _step(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale):
    g = g * grad_scale
    m = m + (1.0 - beta1) * (g - m)                         # exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + ((1.0 - beta2) * g) * g                 # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v) / (bc2 ** 0.5) + eps
    p = p + (-(lr / bc1)) * m / denom                       # param.addcdiv_(exp_avg, denom, value=-step_size)
    return p, m, v


def adam_step(p, g, m, v, step, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS, grad_scale=1.0, exact=False):
    """One step, number ``step`` (1-based), in float64; returns new (p, m, v).  Operation order as torch's single-tensor Adam."""
    assert step >= 1
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    return _step(p, g, m, v, step, *constants(lr, beta1, beta2, eps, grad_scale, exact))


def run(p0, grads, first_step=1, m0=None, v0=None, snapshots=(), **kw):
    """Drive ``adam_step`` over an iterable of gradients, the first one taken as step ``first_step``.  Returns (p, m, v) after
    the last; with ``snapshots`` (step numbers) a dict {step: (p, m, v)} of the state AFTER each of those steps (0 = the start)."""
    p = np.array(p0, np.float64)
    m = np.zeros_like(p) if m0 is None else np.array(m0, np.float64)
    v = np.zeros_like(p) if v0 is None else np.array(v0, np.float64)
    keep = {}
    if 0 in snapshots:
        keep[0] = (p.copy(), m.copy(), v.copy())
    step = first_step - 1
    for g in grads:
        step += 1
        p, m, v = adam_step(p, g, m, v, step, **kw)
        if step in snapshots:
            keep[step] = (p, m, v)
    return keep if snapshots else (p, m, v)


# --------------------------------------------------------------------------------------------------------- the cases
def gradients(kind, n, T, seed=0):
    """Generator of T float32 gradients (n,), class ``kind``, per entry, fixed seed:

      steady  +-U[0.1, 1], sign and magnitude fresh every step
      wide    the same times a per-entry scale 10**U[-6, 3] that stays for the whole sequence
      decay   steady for the first T // 2 steps, exactly 0 afterwards
      zero    always zero
      flip    magnitude U[0.1, 1] fresh every step, the sign of an entry alternates every step
    """
    assert kind in KINDS, kind
    rng = np.random.RandomState(1000003 * KINDS.index(kind) + seed)
    scale = (10.0 ** rng.uniform(-6.0, 3.0, n)) if kind == "wide" else None
    sign0 = np.where(rng.randint(0, 2, n) > 0, 1.0, -1.0)
    for t in range(T):
        if kind == "zero" or (kind == "decay" and t >= T // 2):
            yield np.zeros(n, np.float32)
            continue
        mag = rng.uniform(0.1, 1.0, n)
        sign = sign0 * (1.0 if t % 2 == 0 else -1.0) if kind == "flip" else np.where(rng.randint(0, 2, n) > 0, 1.0, -1.0)
        g = mag * sign
        if scale is not None:
            g = g * scale
        yield g.astype(np.float32)                          # (rounding is monotone: |g| >= float32(the class's floor) still holds)


def initial_params(kind, n, seed=0):
    """'zero': the accuracy cases (the error of the update is not hidden under the rounding of a parameter of size 1);
    'normal': N(0, 1)."""
    if kind == "zero":
        return np.zeros(n, np.float32)
    assert kind == "normal"
    return np.random.RandomState(77 + seed).normal(0.0, 1.0, n).astype(np.float32)


MANY_STEPS_N = 4100
MANY_STEPS_T = (1, 2, 3, 20, 200)
GRAD_SCALES = (1.0, 0.125, 1.0 / 3.0)
FROM_STATE_N = 260                                           # more than one block, and one that is not full
FROM_STATE_STEPS = (1, 2, 10, 1000, 100000)
SIZES = (1, 3, 255, 256, 257, 4100, 2 ** 20 + 3)


class _SteadyRun:
    """The float64 reference (float-rounded constants) on steady gradients from zero state and zero parameters at
    n = FROM_STATE_N, advanced on demand; remembers the state before each of FROM_STATE_STEPS."""

    def __init__(self):
        self.grads = gradients("steady", FROM_STATE_N, max(FROM_STATE_STEPS), seed=5)
        self.c = constants()
        self.p = np.zeros(FROM_STATE_N)
        self.m, self.v = self.p.copy(), self.p.copy()
        self.done, self.kept = 0, {}

    def before(self, step):
        assert step in FROM_STATE_STEPS
        while step not in self.kept:
            g = next(self.grads)                             # the gradient of step done + 1
            if self.done + 1 in FROM_STATE_STEPS:
                self.kept[self.done + 1] = (self.p.astype(np.float32), self.m.astype(np.float32), self.v.astype(np.float32), g)
            self.p, self.m, self.v = _step(self.p, g.astype(np.float64), self.m, self.v, self.done + 1, *self.c)
            self.done += 1
        return self.kept[step]


_RUN = []


def state_before(step):
    """fp32-rounded (p, m, v) of the float64 reference after ``step - 1`` steady steps, and the float32 gradient of step
    ``step``.  One run, shared by every caller in the process, serves every step asked."""
    if not _RUN:
        _RUN.append(_SteadyRun())
    return _RUN[0].before(step)

"""One refinement stage at every parameter subset that changes a launch: one representative mask per plan class of
tests/stage_cases.py (95; 48 when the camera bit is ignored), three iterations, B = 3, on the ragged default batch and -- the 48 --
on the deep-overlap batch.  Every run is a fresh `OptimizeModel` with the one stage as its strategy, two passes (capture, replay).

a. Bit for bit (`STATE_KEYS` of test_gpu_stage_tails.py, every array of `get_pred_result()`, the selection): the default run against
   the generic tail forms and against the separate launches; with the translated reuse off, the exact accelerations on against static
   reuse and candidate lists off; iterations 0 and 1 of a three-iteration stage (STEP tails) against the two-iteration stage (whose
   iteration 1 is the last-iteration form).
b. The whole-loss gradient of the LAST iteration against the float64 oracle at the product's own state.  Adam's first moment is
   m_n = 0.9 m_(n-1) + 0.1 g_(n-1), so g_2 = (m_3 - 0.9 m_2) / 0.1 from the three- and the two-iteration run (replays are
   deterministic); it was evaluated at `snap_params[2]` inside the stage's blocks and at the batch's values outside.  Iteration 0 the
   same way from the one-iteration run (g_0 = m_1 / 0.1), against one oracle gradient per batch.  Per block of the mask,
   max|g_hip - g_64| <= max(1.5 x max|g_32 - g_64|, 3e-4 x max|g_64|), maxima over the block and the batch: the rule of
   test_gpu_mano_layer.py and the floor of the single-step gradient tests; tests/test_stage_cases_cpu.py shows what the floor can
   see.  These runs have the translated reuse off (the kept grid of a translated hand is rounding-level by design and has its own
   tests); where the moving box applies the default run is compared too, against the floor alone.
c. Nothing outside the mask moves: parameters, optimizer state (zero), snapshots (`snap_params` is filled with NaN before each pass:
   `init_optimize` leaves it alone, and only the slots of the mask may be written).
d. `opt_select_kernel` replayed in numpy float32 from the device's own `snap_loss`; the parameters after the stage are
   `snap_params[selected]` inside the mask.
e. SGD (momentum buffer m_n = 0.9 m_(n-1) + g_(n-1)) with one mask per tail form: the bit-for-bit trio and the gradient bar.

Every distance is printed, tagged `[parity]`: the product's and the float32 oracle's distance from float64, max|g_64| and the ratio.

Worst observed |g_hip - g_64| / max|g_64| per block family on an MI355X -- 95 masks, both batches, iterations 0 and 2, Adam and SGD, 844
comparisons; the floor is 3e-4:

    camera       6.1e-7   (mask 1, deep, iteration 0)
    translation  3.1e-6   (mask 22, deep, iteration 2)
    orientation  1.6e-5   (mask 76, default, iteration 2)      2.6e-4 in mask 84, deep, iteration 2 (*)
    finger pose  2.3e-6   (mask 43, default, iteration 2)      5.1e-5 (*)
    shape        2.5e-6   (mask 112, deep, iteration 2)        1.4e-4 (*)

The float32 oracle's own distance is 3e-8 .. 1.5e-5 x max|g_64|, the product's 0.2 .. 5.3 times that (median 1.2; the camera gradient of
mask 1 on the deep batch 18 times, at 6e-7): the 1.5 x rule alone would hold in two comparisons out of three, the floor decides the
rest -- in 90 of the 95 classes at least once -- and is twenty times the worst case off (*).

(*) One state, one sample: two Adam iterations into mask 84 (right orientation + right finger pose + right shape) on the deep batch,
vertex 608 of sample 1's right hand sits 1.0e-6 cells below the face x = 9 of the left hand's grid (one float32 ulp of 9 is 9.5e-7).
Trilinear sampling is continuous across a cell face, its derivative is not: the product's float32 coordinate evidently lands on the other side of
the face than both oracles', the collision VALUES agree to 3e-8, and the whole gradient difference is 0.0104 x d(that vertex's x) /
d(parameters) (cosine 0.99998 over the 58 slots; zero with the collision weight at zero; the same from a fresh one-iteration stage
started at that state).  A kink of the loss, not an error of either side -- and the reason the floor stays where it is."""
import types

import numpy as np
import pytest
import torch

import stage_cases as sc

pytestmark = pytest.mark.gpu

B = 3
EXACT = dict(sdf_no_translated_reuse=True)                                   # the rounding-level acceleration off: what is left is exact
SCRATCH = dict(EXACT, sdf_no_static_reuse=True, sdf_no_candidate_lists=True)     # ... and the exact ones off as well


def _make_opt(epoch, optimizer, **extra):
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root="", strategy="opt_default", save_mid_freq=1,
                                 optimizer=optimizer, opt_epoch=epoch, **extra)


def _packed(buf):
    """The parameter buffers as (B, 122) in slot order (refine.h: opt_slot_ptr)."""
    return torch.cat([buf["cam"], buf["trans"], buf["orient"][0], buf["orient"][1], buf["pose"][0], buf["pose"][1], buf["shape"][0],
                      buf["shape"][1]], dim=1).cpu().numpy()


def _run(data, mask, n, generic=False, optimizer="adam", **extra):
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import OptimizeModel
    from test_gpu_stage_tails import STATE_KEYS
    prev = hip.lib().ihmr_debug_force_generic_tail(1 if generic else 0)
    try:
        m = OptimizeModel(_make_opt(n - 1, optimizer, **extra))
        m.strategy = [sc.stage_for(mask, n)]
        assert m.buf["snap_params"].shape[0] == n
        for rep in range(2):
            m.set_input(data); m.init_optimize()
            m.buf["snap_params"].fill_(float("nan"))
            before = _packed(m.buf)
            m.optimize()
            torch.cuda.synchronize()
    finally:
        hip.lib().ihmr_debug_force_generic_tail(prev)
    out = {f"export/{k}": np.ascontiguousarray(v) for k, v in m.get_pred_result().items() if isinstance(v, np.ndarray)}
    out.update({f"state/{k}": m.buf[k].cpu().numpy() for k in STATE_KEYS})
    out["selected_history"] = torch.stack(m.selected_history).cpu().numpy()
    out["before"], out["after"] = before, _packed(m.buf)
    return out


def _differing(a, b):
    from test_gpu_stage_tails import _bits
    assert a.keys() == b.keys()
    return [k for k in a if a[k].shape != b[k].shape or not np.array_equal(_bits(a[k]), _bits(b[k]))]


class _Case:
    """The runs of one (mask, batch, optimizer), made on demand; failures are collected so that one case reports everything it finds."""

    def __init__(self, mano_arrays, mask, kind, optimizer="adam"):
        self.mano_arrays, self.mask, self.kind, self.optimizer = mano_arrays, mask, kind, optimizer
        self.data = sc.batch(mano_arrays, kind)
        self.tag = f"mask {mask} {kind} {optimizer}"
        self.failures = []
        self.inside = np.zeros(122, bool)
        for sl in sc.block_slices(mask).values():
            self.inside[sl] = True

    def run(self, n, generic=False, **extra):
        return _run(self.data, self.mask, n, generic, self.optimizer, **extra)

    def fail(self, what):
        self.failures.append(f"{self.tag}: {what}")

    def same(self, a, b, what):
        diff = _differing(a, b)
        if diff:
            self.fail(f"{what}: {', '.join(diff)} differ")

    def same_head(self, longer, shorter, what):
        """Iterations 0 .. n-2 of the longer stage against the stage one iteration shorter: snapshots of parameters and losses."""
        from test_gpu_stage_tails import _bits
        k = shorter["state/snap_params"].shape[0]
        for key in ("state/snap_params", "state/snap_loss"):
            if not np.array_equal(_bits(longer[key][:k]), _bits(shorter[key])):
                self.fail(f"{what}: {key}[0:{k}] differs")

    # ------------------------------------------------------------------------------------------------------------------- b / e
    def gradient(self, longer, shorter):
        """The product's gradient of the longer run's last iteration: (m_n - 0.9 m_(n-1)) / 0.1 (SGD: m_n - 0.9 m_(n-1)), in float64 on
        the float32 optimizer states and with the float32 constants of the update (ihmr_pure.h: m + 0.1f (g - m); m 0.9f + g)."""
        m_n = longer["state/adam_m"].astype(np.float64)
        m_p = shorter["state/adam_m"].astype(np.float64) if shorter is not None else np.zeros_like(m_n)
        if self.optimizer == "sgd":
            return m_n - float(np.float32(0.9)) * m_p
        return m_p + (m_n - m_p) / float(np.float32(0.1))

    def oracle_at(self, run):
        """(g_64, g_32) at the state the run's last iteration was evaluated at."""
        x = run["state/snap_params"][-1]
        state = {name: x[:, sl] for name, sl in sc.block_slices(self.mask).items()}
        w = sc.stage_for(self.mask, 1)["loss_weights"]
        return tuple(sc.oracle_gradients(self.mano_arrays, self.data, w, dt, state) for dt in (torch.float64, torch.float32))

    def grad_check(self, what, g_hip, g64, g32, floor_only=False):
        for name, sl in sc.block_slices(self.mask).items():
            scale = float(np.abs(g64[:, sl]).max())
            d_hip = float(np.abs(g_hip[:, sl] - g64[:, sl]).max())
            d32 = float(np.abs(g32[:, sl] - g64[:, sl]).max())
            bar, which = sc.gradient_bar(g32, g64, sl)
            if floor_only:
                bar, which = sc.GRAD_FLOOR * scale, "floor"
            print(f"[parity] {self.tag} {what} dL/d{name}: hip {d_hip:.3e} f32-oracle {d32:.3e} max|g64| {scale:.3e} "
                  f"ratio {d_hip / scale if scale else float('nan'):.3e} hip/f32 {d_hip / d32 if d32 else float('inf'):.2f} bar {which}"
                  f"{'' if d_hip <= sc.GRAD_RULE * d32 else ' NEEDS-FLOOR'}")
            if not scale > 0:
                self.fail(f"{what} dL/d{name}: the oracle's gradient is zero, nothing is compared")
            if not d_hip <= bar:
                self.fail(f"{what} dL/d{name}: |g_hip - g_64| = {d_hip:.3e} > {bar:.3e} ({which}; float32 oracle {d32:.3e}, max|g_64| {scale:.3e})")

    # ----------------------------------------------------------------------------------------------------------------------- c
    def only_the_mask_moves(self, run, what):
        from test_gpu_stage_tails import _bits
        out = ~self.inside
        if not np.array_equal(_bits(run["after"][:, out]), _bits(run["before"][:, out])):
            self.fail(f"{what}: a parameter outside the mask moved")
        for k in ("adam_m", "adam_v"):
            if np.any(_bits(run[f"state/{k}"][:, out]) != 0):
                self.fail(f"{what}: {k} outside the mask is not zero")
        if self.optimizer == "sgd" and np.any(_bits(run["state/adam_v"]) != 0):
            self.fail(f"{what}: SGD wrote a second moment")
        snap = run["state/snap_params"]
        if not np.isnan(snap[:, :, out]).all():
            self.fail(f"{what}: snap_params written outside the mask")
        if np.isnan(snap[:, :, self.inside]).any():
            self.fail(f"{what}: snap_params not written (or NaN) inside the mask")
        if not np.array_equal(_bits(snap[0][:, self.inside]), _bits(run["before"][:, self.inside])):
            self.fail(f"{what}: snapshot 0 is not the stage's starting point")

    # ----------------------------------------------------------------------------------------------------------------------- d
    def selection(self, run, n, what):
        from ihmr_amd.optimize_model import stage_to_args
        from test_gpu_stage_tails import _bits
        sg = stage_to_args(sc.stage_for(self.mask, n), self.optimizer, 1)
        loss = run["state/snap_loss"]                                                        # (S, 3, B) float32
        assert loss.dtype == np.float32 and loss.shape == (n, 3, B)
        valid = np.ones((n, B), bool)
        for l in range(3):
            if sg.use_filter[l]:
                valid &= loss[:, l] <= loss[0, l] * np.float32(sg.filter_factor[l])
        key = np.where(valid, loss[:, sg.select_loss], np.float32(100000000000.0))
        key[0] = loss[0, sg.select_loss]
        want = np.argmin(key, axis=0)                                                        # (the first minimum)
        got = run["state/selected"]
        if not (np.array_equal(got, want) and np.array_equal(run["selected_history"][0], want)):
            self.fail(f"{what}: selected {got.tolist()}, the host replay of opt_select_kernel gives {want.tolist()}")
            return
        chosen = run["state/snap_params"][want, np.arange(B)]
        if not np.array_equal(_bits(run["after"][:, self.inside]), _bits(chosen[:, self.inside])):
            self.fail(f"{what}: the parameters after the stage are not snap_params[selected]")


_INITIAL = {}


def _initial_oracle(mano_arrays, kind):
    """(g_64, g_32) over all eight blocks at the batch's initial state: every mask's iteration 0."""
    if kind not in _INITIAL:
        w = sc.stage_for(255, 1)["loss_weights"]
        data = sc.batch(mano_arrays, kind)
        _INITIAL[kind] = tuple(sc.oracle_gradients(mano_arrays, data, w, dt) for dt in (torch.float64, torch.float32))
    return _INITIAL[kind]


def _stage_case(mano_arrays, mask, kind):
    c = _Case(mano_arrays, mask, kind)
    # a
    new = c.run(3)
    c.same(new, c.run(3, generic=True), "default vs generic tail forms")
    c.same(new, c.run(3, no_fused_tail=True), "default vs separate launches")
    exact = c.run(3, **EXACT)
    c.same(exact, c.run(3, **SCRATCH), "static reuse and candidate lists on vs off (translated reuse off in both)")
    new2, exact2 = c.run(2), c.run(2, **EXACT)
    c.same_head(new, new2, "3 iterations vs 2")
    c.same_head(exact, exact2, "3 iterations vs 2 (translated reuse off)")
    if not sc.moving_box(mask):
        c.same(new, exact, "the translated-reuse switch in a stage without a moving box")
    # b
    exact1 = c.run(1, **EXACT)
    c.same_head(exact2, exact1, "2 iterations vs 1 (translated reuse off)")
    c.grad_check("iteration 0", c.gradient(exact1, None), *_initial_oracle(mano_arrays, kind))
    g64, g32 = c.oracle_at(exact)
    c.grad_check("iteration 2", c.gradient(exact, exact2), g64, g32)
    if sc.moving_box(mask):
        if np.array_equal(new["state/snap_params"][2][:, c.inside], exact["state/snap_params"][2][:, c.inside]):
            d64, d32 = g64, g32
        else:
            d64, d32 = c.oracle_at(new)
        c.grad_check("iteration 2, moving box", c.gradient(new, new2), d64, d32, floor_only=True)
    # c, d
    for what, run, n in (("default", new, 3), ("translated reuse off", exact, 3), ("2 iterations", new2, 2), ("1 iteration", exact1, 1)):
        c.only_the_mask_moves(run, what)
        c.selection(run, n, what)
    return c.failures


@pytest.mark.parametrize("mask", sc.REPRESENTATIVES)
def test_stage_mask(mano_arrays, mask):
    """a - d of the module docstring for one plan class: on the default batch, and -- the representatives of the classes that differ in
    more than the camera bit -- on the deep batch."""
    print(f"[parity] mask {mask}: {', '.join(sc.block_names(mask))}; {sc.plan(mask)}")
    failures = _stage_case(mano_arrays, mask, "default")
    if mask in sc.REPRESENTATIVES_NO_CAM:
        failures += _stage_case(mano_arrays, mask, "deep")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["default", "deep"])
@pytest.mark.parametrize("mask", [1, 2, 12, 48, 192])
def test_stage_mask_sgd(mano_arrays, mask, kind):
    """e: the SGD step under every tail form -- separate launches (1), opt_tail_kernel_trans (2), <true, true> (12), <false> with the
    stand-alone head (48), <true> (192)."""
    c = _Case(mano_arrays, mask, kind, optimizer="sgd")
    new = c.run(3)
    c.same(new, c.run(3, generic=True), "default vs generic tail forms")
    c.same(new, c.run(3, no_fused_tail=True), "default vs separate launches")
    exact, exact2, exact1 = c.run(3, **EXACT), c.run(2, **EXACT), c.run(1, **EXACT)
    c.same_head(exact, exact2, "3 iterations vs 2")
    c.same_head(exact2, exact1, "2 iterations vs 1")
    c.grad_check("iteration 0", c.gradient(exact1, None), *_initial_oracle(mano_arrays, kind))
    c.grad_check("iteration 2", c.gradient(exact, exact2), *c.oracle_at(exact))
    for what, run, n in (("default", new, 3), ("translated reuse off", exact, 3), ("1 iteration", exact1, 1)):
        c.only_the_mask_moves(run, what)
        c.selection(run, n, what)
    assert not c.failures, "\n".join(c.failures)

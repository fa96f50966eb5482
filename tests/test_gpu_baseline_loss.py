"""GPU parity of the IHMR-Baseline training objective: ``InterHandModel.compute_loss_gradients()`` (ihmr_opt_set_params +
ihmr_mlp_train_grad with the Baseline's wiring + the handedness term) against the float64 statement of tests/baseline_train_ref.py,
which tests/test_baseline_loss_cpu.py pins to the reference's own loss functions and whose bars it shows to be sharp.  The encoder
never runs here except in the composed step: ``final_params`` and ``pred_hand_type`` are assigned."""
import types

import numpy as np
import pytest
import torch

import baseline_train_ref as R

pytestmark = pytest.mark.gpu
B = 8                                                      # the smallest size the ragged batch exists at
SINGLE = ("joints_2d", "joints_3d", "mano_pose", "mano_shape", "hand_trans", "shape_reg", "collision")
# blocks of final_params a term CAN touch (every other column of _grad122 must be exactly 0 when the term stands alone)
CAM, ORIENT, POSE, SHAPE, TRANS = ("pred_cam_params",), ("pred_right_orient", "pred_left_orient"), \
    ("pred_right_pose_params", "pred_left_pose_params"), ("pred_right_shape_params", "pred_left_shape_params"), ("pred_hand_trans",)
TOUCHES = dict(joints_2d=CAM + ORIENT + POSE + SHAPE + TRANS, joints_3d=ORIENT + POSE + SHAPE + TRANS, mano_pose=POSE, mano_shape=SHAPE,
               hand_trans=TRANS, shape_reg=SHAPE, collision=ORIENT + POSE + SHAPE + TRANS)


def _opt(B, **kw):
    d = dict(isTrain=True, dist=False, process_rank=-1, batchSize=B, inputSize=224, input_nc=3, num_joints=42, total_params_dim=122,
             cam_params_dim=3, pose_params_dim=96, shape_params_dim=20, trans_params_dim=3, model_root="", mean_param_file="mean_mano_params.pkl",
             checkpoints_dir="./checkpoints", lr=1e-4, lr_decay_type="none", total_epoch=3)
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.fixture(scope="module")
def inputs(mano_arrays):
    """Regular and ragged batch at B = 8 with the seeded predictions (the inputs whose preconditions the CPU test asserts)."""
    torch.set_num_threads(8)
    out = {}
    for name in ("regular", "ragged"):
        batch = R.baseline_batch(mano_arrays, B)
        if name == "ragged":
            batch = R.ragged_baseline_batch(batch)
        final, hand = R.seeded_predictions(batch)
        out[name] = types.SimpleNamespace(batch=batch, final=final, hand=hand)
    return out


@pytest.fixture(scope="module")
def models():
    """One training model per collision setting; the cases change ``loss_weights`` in place."""
    from ihmr_amd.baseline_model import InterHandModel
    torch.manual_seed(11)
    return {False: InterHandModel(_opt(B)), True: InterHandModel(_opt(B, use_collision_loss=True, collision_loss_weight=1.0))}


def _run(model, case, weights):
    model.loss_weights.update(weights)
    model.set_input(case.batch)
    model.final_params, model.pred_hand_type = case.final.cuda().contiguous(), case.hand.cuda().contiguous()
    model.compute_loss_gradients()
    torch.cuda.synchronize()
    return model.get_current_errors(), model._grad122.cpu(), model._d_hand.cpu()


def _check(tag, mano_arrays, got, case, weights, gate=None):
    """Terms within 2e-6 + 2e-5 |ref| of the float64 statement; every block of the gradient, per sample, within 3 x (float32 statement vs
    float64) + 1e-6 of the block's scale (``gate``: within that fraction instead, samples beyond the tight rule counted).  Returns the
    float64 gradient and the samples beyond the tight rule."""
    err, g, h = got
    t64, g64, h64 = R.baseline_loss_statement(mano_arrays, case.batch, case.final, case.hand, weights, torch.float64)
    _, g32, h32 = R.baseline_loss_statement(mano_arrays, case.batch, case.final, case.hand, weights, torch.float32)
    names = [n for n in R.TERMS if n != "collision_loss" or weights["collision"]] + ["total_loss"]
    assert list(err) == names, (list(err), names)
    for n in names:
        d, bar = abs(err[n] - t64[n]), R.term_bar(t64[n])
        print(f"[parity] {tag} {n}: HIP {err[n]:.8e} float64 {t64[n]:.8e} |diff| {d:.3e} bar {bar:.3e}")
    for n in names:
        assert abs(err[n] - t64[n]) <= R.term_bar(t64[n]), (tag, n, err[n], t64[n])
    beyond, worst = set(), []
    blocks = [(n, sl, g, g32, g64) for n, sl in R.gradient_blocks().items()] + [("pred_hand_type", slice(0, 2), h, h32, h64)]
    for n, sl, a, a32, a64 in blocks:
        e_hip, bar = R.block_distance(a, a64, sl), R.block_bar(a32, a64, sl)
        off = [int(b) for b in torch.nonzero(e_hip > bar).flatten()]
        beyond.update(off)
        print(f"[parity] {tag} d loss / d {n} (scale {float(a64[:, sl].abs().max()):.3e}): HIP vs float64 {float(e_hip.max()):.3e}, float32 statement "
              f"vs float64 {(bar - 1e-6) / 3.0:.3e}, bar {bar:.3e}; samples beyond {off}")
        worst.append((n, float(e_hip.max()), bar))
    for n, e, bar in worst:
        assert e <= (bar if gate is None else gate), (tag, n, e, bar)
    return g64, sorted(beyond)


def test_default_weights_match_the_float64_statement(mano_arrays, inputs, models):
    """(a) Default weights, collision off, regular and ragged batch: every term, total_loss, d loss / d final_params per COLS block and
    per sample, and d loss / d pred_hand_type."""
    for name, case in inputs.items():
        w = dict(R.DEFAULT_WEIGHTS)
        assert models[False].loss_weights == w                         # the defaults of both sides agree
        _check(name, mano_arrays, _run(models[False], case, w), case, w)


@pytest.mark.parametrize("term", SINGLE)
def test_one_term_at_a_time(mano_arrays, inputs, models, term):
    """(b) Every weight 0 but one (the handedness term has no weight: present and checked in each run), ragged batch, the same bars; the
    columns the term cannot touch are exactly 0 in _grad122."""
    case = inputs["ragged"]
    w = {k: 0.0 for k in R.DEFAULT_WEIGHTS}
    w[term] = 1.0 if term == "collision" else (R.DEFAULT_WEIGHTS[term] or 1.0)
    model = models[term == "collision"]
    keep = dict(model.loss_weights)
    try:
        got = _run(model, case, w)
    finally:
        model.loss_weights.update(keep)
    _check(term, mano_arrays, got, case, w)                # (the collision term alone too: the tight rule, not the 1e-3 of case (c))
    g = got[1]
    for n, sl in R.gradient_blocks().items():
        if n not in TOUCHES[term]:
            assert float(g[:, sl].abs().max()) == 0.0, (term, n, float(g[:, sl].abs().max()))
        else:
            assert float(g[:, sl].abs().max()) > 0.0, (term, n)


def test_collision_on_matches_the_float64_statement(mano_arrays, inputs, models):
    """(c) Collision on (use_collision_loss, weight 1.0), regular batch: the collision term within the terms' bar, every block within
    1e-3 of its scale (ray parity is discontinuous: the MLP test's number); the samples beyond the tight rule are printed, not gated."""
    case, model = inputs["regular"], models[True]
    w = dict(R.DEFAULT_WEIGHTS, collision=1.0)
    assert model.loss_weights == w
    got = _run(model, case, w)
    assert got[0]["collision_loss"] > 0.0
    _, beyond = _check("collision on", mano_arrays, got, case, w, gate=1e-3)
    print(f"[parity] collision on: samples beyond the 3 x float32 rule: {beyond}")


def test_target_pointers_return_and_a_second_call_gives_the_same_bits(inputs, models):
    """(d) The try/finally swap: io.init_joints_2d / io.init_joints_3d hold their former addresses afterwards, and differ from the
    annotation's (so the swap does swap); a second call gives the same bits."""
    model, case = models[False], inputs["ragged"]
    io = model._core.io
    before = (io.init_joints_2d, io.init_joints_3d)
    assert before[0] != io.gt_joints_2d and before[1] != io.gt_joints_3d
    err1, g1, h1 = _run(model, case, dict(R.DEFAULT_WEIGHTS))
    assert (io.init_joints_2d, io.init_joints_3d) == before
    t1 = model._terms5.clone()
    err2, g2, h2 = _run(model, case, dict(R.DEFAULT_WEIGHTS))
    assert (io.init_joints_2d, io.init_joints_3d) == before
    assert torch.equal(g1, g2) and torch.equal(h1, h2) and torch.equal(t1, model._terms5) and err1 == err2


def test_composed_step_equals_optimize_parameters(tmp_path):
    """(e) B = 4, two models built as the resume test builds them, the same batch: forward_train + optimize_parameters on one,
    forward_train + compute_loss_gradients + trainer.backward(the first model's gradients) + optimizer_step on the other -- the same bits
    in the flat gradient, the weights, both Adam moments, the stem's running variance and the step count."""
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    Bs = 4

    def make():
        torch.manual_seed(11)
        return InterHandModel(_opt(Bs, checkpoints_dir=str(tmp_path)))
    a, b = make(), make()
    fwd = lambda p, s, t: two_hand.forward_from_packed(a.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    batch = {k: v.cuda() for k, v in synthetic_opt_batch(Bs, fwd, seed=77, with_image=True).items()}
    a.set_input(batch); a.forward_train(); a.optimize_parameters()
    b.set_input(batch); b.forward_train(); b.compute_loss_gradients()
    assert torch.equal(a._grad122, b._grad122) and torch.equal(a._d_hand, b._d_hand)
    b.trainer.backward(a._grad122.clone(), a._d_hand.clone())
    b.trainer.optimizer_step(1)
    torch.cuda.synchronize()
    for name in ("grads", "params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a.trainer.flat, name), getattr(b.trainer.flat, name)), name
    assert float(a.trainer.flat.grads.abs().max()) > 0.0
    assert torch.equal(a.trainer.stem["run_var"], b.trainer.stem["run_var"])
    assert a.trainer.step == b.trainer.step == 1

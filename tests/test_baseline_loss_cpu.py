"""The float64 statement of the IHMR-Baseline training objective (tests/baseline_train_ref.py), checked without a GPU: against the
reference's own loss functions (tests/golden/baseline_loss.npz), for the POWER of the bars the GPU test applies (a flipped or
mis-normalised term would fail them tenfold), and for the preconditions under which those bars are fair."""
import contextlib
import os
import os.path as osp
import types

import numpy as np
import pytest
import torch

import baseline_train_ref as R
from oracle import losses_ref as L

GOLD = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
B = 8
# The tolerances tests/test_oracle_golden.py applies to the `losses` fixture, term by term: (value atol, gradient atol).  The terms that
# test does not differentiate take the 2-D term's pair.  The gradients here reach final_params THROUGH the MANO layer, whose matrix
# products round differently with the host's thread count: they also get that test's relative part for gradients (1e-5, finger term).
TOL = dict(hand_type_loss=(1e-7, 1e-9), joints_2d_loss=(1e-7, 1e-9), joints_3d_loss=(1e-9, 1e-10), mano_pose_loss=(1e-7, 1e-9),
           mano_shape_loss=(1e-7, 1e-9), shape_reg_loss=(1e-7, 1e-8))
GRAD_RTOL = 1e-5
INPUT_ATOL = 1e-6     # test_oracle_golden.py: "same ops on the same machine class: round-off only"


def close(a, b, atol, rtol=0.0, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    print(f"[golden] {what}: max|err|={err.max():.3e} max|ref|={np.abs(b).max():.3e}")
    assert np.all(err <= atol + rtol * np.abs(b)), f"{what}: max err {err.max():.3e}"


@pytest.fixture(scope="module")
def cases(mano_arrays):
    """The inputs of the GPU test (B = 8: regular and ragged batch, seeded predictions) with the float64 and the float32 statement."""
    torch.set_num_threads(8)
    out = {}
    for name in ("regular", "ragged"):
        batch = R.baseline_batch(mano_arrays, B)
        if name == "ragged":
            batch = R.ragged_baseline_batch(batch)
        final, hand = R.seeded_predictions(batch)
        c = types.SimpleNamespace(batch=batch, final=final, hand=hand)
        c.s64 = R.baseline_loss_statement(mano_arrays, batch, final, hand, R.DEFAULT_WEIGHTS, torch.float64)
        c.s32 = R.baseline_loss_statement(mano_arrays, batch, final, hand, R.DEFAULT_WEIGHTS, torch.float32)
        out[name] = c
    return out


# ---------------------------------------------------------------------------------------------------------- statement vs the reference
def _statement_vs(g, mano_arrays):
    batch = {k: torch.tensor(g["in_" + k]) for k in R.BATCH_KEYS}
    two = R.separate_two_hand_forward(mano_arrays)
    for n in TOL:
        fp, ph = torch.tensor(g["in_final_params"]).requires_grad_(True), torch.tensor(g["in_pred_hand_type"]).requires_grad_(True)
        t = R.baseline_loss_terms(two, batch, fp, ph)[n]
        t.backward()
        close(t.detach(), g["term_" + n], TOL[n][0], what=n)
        if n == "hand_type_loss":
            assert fp.grad is None
            close(ph.grad, g["dht_" + n], TOL[n][1], GRAD_RTOL, what=f"d {n} / d pred_hand_type")
        else:
            assert ph.grad is None
            close(fp.grad, g["dfp_" + n], TOL[n][1], GRAD_RTOL, what=f"d {n} / d final_params")
            assert np.abs(g["dfp_" + n]).max() > 1e-4, n        # a fixture of zeros would pin nothing


def test_statement_reproduces_the_reference_terms(mano_arrays, cases):
    """The float32 statement gives every term the reference's own LossUtil gives, and autograd's gradient of it; the fixture's inputs are
    the ragged batch and the seeded predictions the GPU test uses."""
    torch.set_num_threads(8)
    g = dict(np.load(osp.join(GOLD, "baseline_loss.npz")))
    assert set(g) == ({"in_" + k for k in R.BATCH_KEYS} | {"in_final_params", "in_pred_hand_type"} | {"term_" + n for n in TOL}
                      | {"dfp_" + n for n in TOL if n != "hand_type_loss"} | {"dht_hand_type_loss"})
    assert set(TOL) == set(R.TERMS) - {"hand_trans_loss", "collision_loss"}
    _statement_vs(g, mano_arrays)
    c = cases["ragged"]
    for k in R.BATCH_KEYS:
        close(c.batch[k], g["in_" + k], INPUT_ATOL, what=f"input {k}")
    close(c.final, g["in_final_params"], INPUT_ATOL, what="input final_params")
    close(c.hand, g["in_pred_hand_type"], INPUT_ATOL, what="input pred_hand_type")


def test_fixture_regenerates_from_the_reference(tmp_path):
    """Where the reference tree is present: the generator, run again, gives the committed fixture.  In a process of its own: importing
    the reference on a CPU patches torch (``.cuda()`` becomes the identity) and registers stand-in modules, which must not reach the
    other tests."""
    import subprocess
    import sys
    sys.path.insert(0, GOLD)
    from _ref_import import reference_available
    if not reference_available():
        pytest.skip("the reference tree is not on this machine")
    path = str(tmp_path / "baseline_loss.npz")
    subprocess.run([sys.executable, osp.join(GOLD, "make_golden_baseline_loss.py"), path], check=True, timeout=300,
                   env=dict(os.environ, OMP_NUM_THREADS="8"))
    new, g = dict(np.load(path)), dict(np.load(osp.join(GOLD, "baseline_loss.npz")))
    assert set(new) == set(g)
    for k in sorted(g):
        n = k.split("_", 1)[1]
        atol, rtol = (INPUT_ATOL, 0.0) if k.startswith("in_") else ((TOL[n][0], 0.0) if k.startswith("term_") else (TOL[n][1], GRAD_RTOL))
        close(new[k], g[k], atol, rtol, what=f"regenerated {k}")


# ------------------------------------------------------------------------------------------------------------------ power of the bar
@contextlib.contextmanager
def patched(module, name, make):
    orig = getattr(module, name)
    setattr(module, name, make(orig))
    try:
        yield
    finally:
        setattr(module, name, orig)


def _scaled(k, pair=True):
    """orig -> k * orig (the loss functions that return (scalar, per sample) keep their second value)."""
    def make(orig):
        def f(*a):
            r = orig(*a)
            return (k * r[0],) + tuple(r[1:]) if pair else k * r
        return f
    return make


def _other_hand(orig):
    """Two calls per statement, right then left, each with ITS hand's column of mano_params_weight: hand them the other hand's."""
    calls = []

    def swapped(gt, pred, w):
        base, col = w._base, len(calls) % 2          # the statement slices both columns from one (B,2) tensor
        calls.append(col)
        assert base is not None and base.shape[1] == 2 and torch.equal(base[:, col:col + 1], w)
        return orig(gt, pred, base[:, 1 - col:2 - col])
    return swapped


ALL = ("pred_cam_params", "pred_right_orient", "pred_right_pose_params", "pred_left_orient", "pred_left_pose_params", "pred_right_shape_params",
       "pred_left_shape_params", "pred_hand_trans")
HANDS = ALL[1:]
POSE, SHAPE, TRANS, HAND_TYPE = ("pred_right_pose_params", "pred_left_pose_params"), ("pred_right_shape_params", "pred_left_shape_params"), \
    ("pred_hand_trans",), ("pred_hand_type",)
# (term, what a plausible bug does to it, module, function, mutation, blocks of the gradient the term touches)
MUTANTS = [
    ("hand_type_loss", "sign", R, "hand_type_loss", _scaled(-1.0, False), HAND_TYPE),
    ("hand_type_loss", "1/B for 1/(2B)", R, "hand_type_loss", _scaled(2.0, False), HAND_TYPE),
    ("hand_type_loss", "hand_type_valid ignored", R, "hand_type_loss", lambda o: (lambda gt, pr, v: o(gt, pr, torch.ones_like(v))), HAND_TYPE),
    ("joints_2d_loss", "sign", L, "joints_2d_loss", _scaled(-1.0), ALL),
    ("joints_2d_loss", "mean over (B,42) for (B,42,2)", L, "joints_2d_loss", _scaled(2.0), ALL),
    ("joints_3d_loss", "sign", L, "joints_3d_loss_", _scaled(-1.0), HANDS),
    ("joints_3d_loss", "mean over (B,42) for (B,42,3)", L, "joints_3d_loss_", _scaled(3.0), HANDS),
    ("mano_pose_loss", "sign", L, "mano_pose_loss", _scaled(-1.0, False), POSE),
    ("mano_pose_loss", "48/3 joints for 15 in the normaliser", L, "mano_pose_loss", _scaled(15.0 / 16.0, False), POSE),
    ("mano_pose_loss", "the other hand's weights", L, "mano_pose_loss", _other_hand, POSE),
    ("mano_shape_loss", "sign", L, "mano_shape_loss", _scaled(-1.0, False), SHAPE),
    ("mano_shape_loss", "mean over (B,20) for (B,10)", L, "mano_shape_loss", _scaled(0.5, False), SHAPE),
    ("mano_shape_loss", "the other hand's weights", L, "mano_shape_loss", _other_hand, SHAPE),
    ("hand_trans_loss", "sign", R, "hand_trans_loss_documented", _scaled(-1.0, False), TRANS),
    ("hand_trans_loss", "target from the next column of hand_trans", R, "hand_trans_loss_documented",
     lambda o: (lambda gt, pr, w: o(gt.roll(-1, 1), pr, w)), TRANS),
    ("hand_trans_loss", "per-sample weight for the batch mean", R, "hand_trans_loss_documented",
     lambda o: (lambda gt, pr, w: (w[:, None] * (gt - pr) ** 2).mean()), TRANS),
    ("shape_reg_loss", "sign", L, "shape_reg_loss", _scaled(-1.0, False), SHAPE),
    ("shape_reg_loss", "mean over (B,20) for (B,10)", L, "shape_reg_loss", _scaled(0.5, False), SHAPE),
    ("collision_loss", "sign", L, "collision_loss", _scaled(-1.0), HANDS),
    ("collision_loss", "divisor 1 for 4", L, "collision_loss", _scaled(4.0), HANDS),
]


def test_every_term_has_a_mutant():
    assert {m[0] for m in MUTANTS} == set(R.TERMS)
    for term in R.TERMS:
        assert any(m[0] == term and m[1] == "sign" for m in MUTANTS), term


@pytest.fixture(scope="module")
def collision_case(mano_arrays, cases):
    c = cases["regular"]
    w = dict(R.DEFAULT_WEIGHTS, collision=1.0)
    return types.SimpleNamespace(batch=c.batch, final=c.final, hand=c.hand, weights=w,
                                 s64=R.baseline_loss_statement(mano_arrays, c.batch, c.final, c.hand, w, torch.float64),
                                 s32=R.baseline_loss_statement(mano_arrays, c.batch, c.final, c.hand, w, torch.float32))


@pytest.mark.parametrize("mutant", MUTANTS, ids=[f"{m[0]}-{m[1]}".replace(" ", "_") for m in MUTANTS])
def test_a_mutated_term_misses_the_gpu_bars_tenfold(mano_arrays, cases, collision_case, mutant):
    """Every other term on at its default weight (shape_reg at 0.1 beside four terms at 10): the mutated float64 statement differs from the
    true one by more than 10 x the bar the GPU test applies -- in the term, in total_loss, and in EVERY block of the gradient the term
    touches.  Collision mutants on the regular batch with the collision term on (the tight rule, stricter than the 1e-3 gate applied
    there, and the term's own bar); all others on the ragged batch."""
    term, _, module, fn, make, blocks = mutant
    torch.set_num_threads(8)
    c = collision_case if term == "collision_loss" else cases["ragged"]
    w = getattr(c, "weights", R.DEFAULT_WEIGHTS)
    with patched(module, fn, make):
        m_terms, m_g, m_h = R.baseline_loss_statement(mano_arrays, c.batch, c.final, c.hand, w, torch.float64)
    t64, g64, h64 = c.s64
    _, g32, h32 = c.s32
    for n in (term, "total_loss"):
        d, bar = abs(m_terms[n] - t64[n]), R.term_bar(t64[n])
        print(f"[power] {n}: mutant {m_terms[n]:.6e} true {t64[n]:.6e} |diff| {d:.3e} = {d / bar:.1f} x bar")
        assert d > 10.0 * bar, (n, d, bar)
    for n in R.TERMS:
        if n != term:
            assert m_terms[n] == t64[n], n                   # the mutation reached one term only
    cols = R.gradient_blocks()
    for blk in blocks:
        if blk == "pred_hand_type":
            d, bar = float(R.block_distance(m_h, h64, slice(0, 2)).max()), R.block_bar(h32, h64, slice(0, 2))
        else:
            d, bar = float(R.block_distance(m_g, g64, cols[blk]).max()), R.block_bar(g32, g64, cols[blk])
        print(f"[power] block {blk}: mutant - true {d:.3e} = {d / bar:.1f} x bar ({bar:.3e})")
        assert d > 10.0 * bar, (blk, d, bar)


# ------------------------------------------------------------------------------------------------- preconditions of the GPU test
def test_preconditions_of_the_gpu_test(mano_arrays, cases):
    """(1) every weighted L1 residual (2-D joints, shape) of the float64 statement is at least 100 x the largest float32-vs-float64
    difference of any joint or shape entry, so no sign() differs between precisions; (2) no root weight lies in (1e-7, 0.5] except in
    the two samples ragged_opt_batch puts there; (3) the regular batch penetrates."""
    from oracle.sdf_ref import SDFLossRef
    torch.set_num_threads(8)
    two64, two32 = R.separate_two_hand_forward(mano_arrays, torch.float64), R.separate_two_hand_forward(mano_arrays)
    for name, c in cases.items():
        f, f64, b = c.final, c.final.double(), c.batch
        o64, o32 = two64(f64[:, 3:99], f64[:, 99:119], f64[:, 119:]), two32(f[:, 3:99], f[:, 99:119], f[:, 119:])
        p64, p32 = L.batch_orthogonal_project(o64[2], f64[:, :3]), L.batch_orthogonal_project(o32[2], f[:, :3])
        diff = max(float((p32.double() - p64).abs().max()), float((o32[2].double() - o64[2]).abs().max()),
                   float((f[:, 99:119].double() - f64[:, 99:119]).abs().max()))
        g2, mw = b["joints_2d"].double(), b["mano_params_weight"].double()
        r2 = (g2[:, :, :2] - p64).abs() * g2[:, :, 2:3]
        rs = (b["mano_betas"].double() - f64[:, 99:119]).abs() * mw.repeat_interleave(10, 1)
        lo2, los = float(r2[g2[:, :, 2:3].expand_as(r2) > 0].min()), float(rs[mw.repeat_interleave(10, 1) > 0].min())
        print(f"[pre] {name}: float32 vs float64 entries {diff:.3e}; smallest weighted residual 2-D {lo2:.3e}, shape {los:.3e}")
        assert min(lo2, los) >= 100.0 * diff, (name, lo2, los, diff)
        for key, on_purpose in (("joints_3d", {5}), ("init_joints_3d", {4})):          # helpers.ragged_opt_batch: samples 4 / 5
            rw = b[key][:, 0, 3]
            between = set(torch.nonzero((rw > 1e-7) & (rw <= 0.5)).flatten().tolist())
            assert between == (on_purpose if name == "ragged" else set()), (name, key, between)
    c = cases["regular"]
    rv, lv, _ = two32(c.final[:, 3:99], c.final[:, 99:119], c.final[:, 119:])
    _, pv, _ = SDFLossRef(mano_arrays[0]["faces"], mano_arrays[1]["faces"])(torch.stack([rv, lv], 1), return_per_vert_loss=True,
                                                                            return_origin_scale_loss=True)
    print(f"[pre] positive per-vertex collision values per sample: {(pv > 0).sum(1).tolist()}")
    assert int((pv > 0).sum()) > 50
    # the ragged batch is what its docstring says: translation weights average to 6/8, valid handedness targets cover all three kinds
    b = cases["ragged"].batch
    assert float(b["hand_trans"][:, 0, 3].mean()) == 0.75
    valid = b["hand_type_valid"][:, 0] > 0
    assert int((~valid).sum()) == 2
    assert {tuple(r) for r in b["hand_type_array"][valid].tolist()} == {(1.0, 1.0), (1.0, 0.0), (0.0, 1.0)}
    assert b["mano_params_weight"].tolist() == [[1, 1], [1, 0], [0, 1], [1, 1], [0, 1], [1, 1], [1, 1], [1, 1]]


def test_training_refuses_a_robustifier():
    """The training launches evaluate the collision term with the robustifier off: an option that asks for one is refused, not ignored."""
    from ihmr_amd.sdf import refuse_training_robustifier
    ns = types.SimpleNamespace
    refuse_training_robustifier(ns(isTrain=True))
    refuse_training_robustifier(ns(isTrain=True, sdf_robustifier=None))
    refuse_training_robustifier(ns(isTrain=False, sdf_robustifier=0.05))
    with pytest.raises(ValueError, match="sdf_robustifier"):
        refuse_training_robustifier(ns(isTrain=True, sdf_robustifier=0.05))

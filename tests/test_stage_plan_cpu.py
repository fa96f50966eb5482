"""The launch plan of the refinement loop (ihmr_amd/csrc/stage_plan.h: stage_ok, plan_stage, plan_iter, plan_step, plan_sdf_flags and
the size-dependent launch forms -- the very functions ihmr_opt_run_stage and run_iteration dispatch on) compiled for the HOST by g++
with -fsanitize=address,undefined and compared field for field with the Python restatement the stage tests choose their cases from
(tests/stage_cases.py: plan, tail_form) at every mask, switch combination and iteration -- and checked against invariants of the
launch sequence that do not rest on that restatement.  An expression edited on either side fails here, without a GPU."""
import itertools
import math
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_cases as sc  # noqa: E402
import hostbuild  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# the enums of stage_plan.h
SKIN = {"FULL": 0, "REUSE": 1, "KEEP_P": 2, "FULL_STORE_P": 3}
SKIN_NONE = 4
LISTS = {"OFF": 0, "REUSE": 1, "REBUILD": 2, "KEEP": 3}
TAIL_NONE = 0
TAIL = {sc.TAIL_SEPARATE: 1, sc.TAIL_PLAIN: 2, sc.TAIL_STEP: 3, sc.TAIL_STEP_SKIN: 4, sc.TAIL_TRANS: 5}
STEPPING = (TAIL[sc.TAIL_STEP], TAIL[sc.TAIL_STEP_SKIN], TAIL[sc.TAIL_TRANS])
AFTER_NONE, AFTER_LBS_BWD, AFTER_BWD23 = 0, 1, 2
STAGE_FIELDS = "need_mask need_cam vposed_fixed pose_fixed pose_stage first_skin later_skin static_mask fused_tail trans_tail keep_rot lists_first".split()
ITER_FIELDS = "head skin lists tail after first need_cam need_mask static_mask keep_rot".split()

SWITCH_NAMES = ("no_fused_tail", "tail_fits", "sdf_no_static_reuse", "force_generic_tail", "keep_lists")
SWITCHES = tuple(itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1)))
ITERS = tuple((it, n) for n in range(1, 5) for it in range(n))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_plan")
    exe = hostbuild.build("stage_plan_driver.cpp", d, hostbuild.X86_V3)

    def run(op, records):
        records = np.ascontiguousarray(records, np.float64)
        assert records.ndim == 2 and len(records)
        fin, fout = str(d / f"{op}.in"), str(d / f"{op}.out")
        with open(fin, "wb") as fh:
            fh.write(np.int64(records.shape[0]).tobytes())
            fh.write(records.tobytes())
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, np.float64).reshape(records.shape[0], -1)
    return run


@pytest.fixture(scope="module")
def stage_plans(driver):
    """(mask, switches) -> the C++ StagePlan as a dict, for all 255 x 48 inputs."""
    cases = [(m,) + s for m in sc.ALL_MASKS for s in SWITCHES]
    got = driver("stage", cases)
    assert got.shape == (len(cases), len(STAGE_FIELDS)) and (got == np.round(got)).all()
    return {c: dict(zip(STAGE_FIELDS, map(int, row))) for c, row in zip(cases, got)}


@pytest.fixture(scope="module")
def iter_plans(driver):
    """(mask, switches, it, n) -> the C++ IterPlan as a dict."""
    cases = [(m,) + s + itn for m in sc.ALL_MASKS for s in SWITCHES for itn in ITERS]
    got = driver("iter", cases)
    assert got.shape == (len(cases), len(ITER_FIELDS)) and (got == np.round(got)).all()
    return {c: dict(zip(ITER_FIELDS, map(int, row))) for c, row in zip(cases, got)}


def test_the_restated_classes_are_the_default_switches():
    assert SWITCHES.index((0, 1, 0, 0, 0)) >= 0 and len(SWITCHES) == 48
    assert all(sc.plan(m) == sc.plan(m, **dict(zip(SWITCH_NAMES, (0, 1, 0, 0, 0)))) for m in sc.ALL_MASKS)


def test_plan_stage_is_the_restatement(stage_plans):
    assert len(stage_plans) == 255 * 48
    for (m, *sw), got in stage_plans.items():
        p = sc.plan(m, **dict(zip(SWITCH_NAMES, sw)))
        want = dict(need_mask=p.need_mask, need_cam=p.need_cam, vposed_fixed=int(p.vposed_fixed), pose_fixed=int(p.pose_fixed),
                    pose_stage=int(p.pose_stage), first_skin=SKIN[p.first_skin], later_skin=SKIN[p.later_skin], static_mask=p.static_mask,
                    fused_tail=int(p.fused_tail), trans_tail=int(p.trans_tail), keep_rot=p.keep_rot, lists_first=LISTS[p.lists_first])
        assert got == want, (m, sw)


def test_plan_iter_is_the_restatement(iter_plans):
    assert len(iter_plans) == 255 * 48 * len(ITERS)
    for (m, *rest), q in iter_plans.items():
        sw, (it, n) = dict(zip(SWITCH_NAMES, rest[:5])), rest[5:]
        p = sc.plan(m, **sw)
        assert q["tail"] == TAIL[sc.tail_form(m, it, n, **sw)], (m, rest)
        assert (q["need_cam"], q["need_mask"], q["static_mask"], q["keep_rot"]) == (p.need_cam, p.need_mask, p.static_mask, p.keep_rot)
        # the rules of the loop, written out: fused -- head in the first iteration and in the finger-pose stage, no skin launch after the
        # first iteration of a stage that keeps v_posed, bwd2 + bwd3 after the tail of a finger-pose stage; separate -- every launch
        if p.fused_tail:
            want = (int(it == 0 or p.pose_stage), SKIN[p.first_skin] if it == 0 else (SKIN_NONE if p.vposed_fixed else SKIN[p.later_skin]),
                    AFTER_BWD23 if p.pose_stage else AFTER_NONE)
        else:
            want = (1, SKIN[p.first_skin if it == 0 else p.later_skin], AFTER_LBS_BWD if p.need_mask else AFTER_NONE)
        assert (q["head"], q["skin"], q["after"]) == want, (m, rest)


def test_the_launch_sequence_holds_together(stage_plans, iter_plans):
    """Invariants of consecutive iterations, from the C++ plans alone: a launch is left out exactly when the previous tail did its work."""
    for m in sc.ALL_MASKS:
        for sw in SWITCHES:
            p = stage_plans[(m,) + sw]
            force_generic = sw[3]
            if force_generic:
                assert p["trans_tail"] == 0 and p["keep_rot"] == 0
            for n in range(1, 5):
                qs = [iter_plans[(m,) + sw + (it, n)] for it in range(n)]
                assert qs[-1]["tail"] in (TAIL[sc.TAIL_PLAIN], TAIL[sc.TAIL_SEPARATE])
                assert qs[0]["head"] == 1 and qs[0]["skin"] != SKIN_NONE      # (nothing precedes the first iteration)
                for it, q in enumerate(qs):
                    assert q["tail"] != TAIL_NONE
                    if it > 0:
                        prev = qs[it - 1]["tail"]
                        assert q["head"] == int(prev not in STEPPING), (m, sw, it, n)
                        assert (q["skin"] == SKIN_NONE) == (prev in (TAIL[sc.TAIL_STEP_SKIN], TAIL[sc.TAIL_TRANS])), (m, sw, it, n)
                    if force_generic:
                        assert q["tail"] != TAIL[sc.TAIL_TRANS] and q["keep_rot"] == 0
                    if not p["fused_tail"]:
                        assert q["tail"] == TAIL[sc.TAIL_SEPARATE]
                    assert q["lists"] == (p["lists_first"] if it == 0 else LISTS["REUSE"]) and q["first"] == int(it == 0)
                    assert (q["after"] == AFTER_BWD23) == bool(q["tail"] != TAIL[sc.TAIL_SEPARATE] and p["pose_stage"])
                    assert (q["after"] == AFTER_LBS_BWD) == bool(q["tail"] == TAIL[sc.TAIL_SEPARATE] and p["need_mask"])


def test_single_shot_plans(driver):
    """The constant plans of the entry points that run one forward pass: head + skin always, no step, nothing static, no camera."""
    which = [0, 1, 2, 10, 11, 12, 13]
    got = {w: dict(zip(ITER_FIELDS, map(int, row))) for w, row in zip(which, driver("single", [[w] for w in which]))}
    base = dict(head=1, skin=SKIN["FULL"], lists=LISTS["OFF"], tail=TAIL[sc.TAIL_SEPARATE], after=AFTER_NONE, first=0, need_cam=0, need_mask=0,
                static_mask=0, keep_rot=0)
    assert got[0] == base                                                           # ihmr_opt_forward_losses, ihmr_opt_sdf_stats
    assert got[1] == dict(base, after=AFTER_LBS_BWD, need_mask=15)                  # ihmr_mlp_train_grad
    assert got[2] == dict(base, tail=TAIL_NONE)                                     # ihmr_opt_forward_verts
    assert got[10] == got[12] == dict(base, lists=LISTS["REUSE"])                   # ihmr_mlp_forward_select: modes 0 and 2
    assert got[11] == dict(base, lists=LISTS["REBUILD"])                            # mode 1 opens the batch
    assert got[13] == dict(base, lists=LISTS["REUSE"], skin=SKIN["REUSE"])          # mode 3: v_posed kept


def test_plan_step_constants(driver):
    """Adam's bias corrections, bit for bit as float32, against Python's `**` on float64 (the host `pow` of this toolchain agrees with
    it at every t checked; `math.pow` is asserted to give the same values, so either names the reference).  `lr` is the float32 that
    ihmr_opt_stage::lr carries, widened: that is what the product divides."""
    ts = range(1, 201)
    for lr in (1e-2, 1e-4):
        lr32 = float(np.float32(lr))
        got = driver("step", [(lr32, 0, t - 1, 1) for t in ts])
        want_step = np.array([np.float32(lr32 / (1 - 0.9 ** t)) for t in ts], np.float32)
        want_bc2 = np.array([np.float32(math.sqrt(1 - 0.999 ** t)) for t in ts], np.float32)
        assert [math.pow(0.9, t) for t in ts] == [0.9 ** t for t in ts] and [math.pow(0.999, t) for t in ts] == [0.999 ** t for t in ts]
        assert got[:, 0].astype(np.float32).tobytes() == want_step.tobytes() and (got[:, 0] == got[:, 0].astype(np.float32)).all()
        assert got[:, 1].astype(np.float32).tobytes() == want_bc2.tobytes() and (got[:, 1] == got[:, 1].astype(np.float32)).all()
        sgd = driver("step", [(lr32, 1, t - 1, 1) for t in ts])
        assert (sgd[:, 0].astype(np.float32) == np.float32(lr)).all() and (sgd[:, 1] == got[:, 1]).all()     # SGD passes lr through


def test_plan_step_snapshots(driver):
    for n, f in itertools.product((1, 2, 3, 50, 200), (1, 3, 10)):
        snap = driver("step", [(1e-2, 0, it, f) for it in range(n)])[:, 2].astype(int)
        assert [(it, s) for it, s in enumerate(snap) if s >= 0] == [(k * f, k) for k in range(-(-n // f))], (n, f)
        assert set(snap[snap < 0]) <= {-1}
        assert int(driver("snaps", [(n, f)])[0, 0]) == int((snap >= 0).sum()) == -(-n // f)


def test_plan_sdf_flags(driver):
    cases = list(itertools.product(range(4), range(16), (0, 1), (0, 1, 2)))
    assert len(cases) == 4 * 16 * 2 * 3
    got = driver("sdf", cases).astype(int)
    for (lists, static_mask, no_lists, no_static), row in zip(cases, got):
        list_mode = int(lists != 0 and not no_lists)
        static_stage = (static_mask & 3) if (list_mode and no_static != 1) else 0
        want = (list_mode, int(lists == 2), static_stage, 0 if lists >= 2 else static_stage, (static_mask >> 2) & static_stage)
        assert tuple(row) == want, (lists, static_mask, no_lists, no_static)


def test_stage_ok(driver):
    good = (2, 0, 5, 1, 2)                                     # param_mask optimizer n_iters save_freq select_loss
    bad = [(0,) + good[1:], (256,) + good[1:], (-1,) + good[1:],                   # what test_plan_rejects_what_the_product_rejects lists
           (2, 2, 5, 1, 2), (2, -1, 5, 1, 2), (2, 0, 0, 1, 2), (2, 0, -3, 1, 2), (2, 0, 5, 0, 2), (2, 0, 5, -1, 2), (2, 0, 5, 1, 3), (2, 0, 5, 1, -1)]
    for b in bad[:3]:
        with pytest.raises(ValueError):
            sc.plan(b[0])
    ok = [good, (1, 1, 1, 1, 0), (255, 0, 200, 10, 1), (2, 0, 1, 7, 2)]
    assert driver("ok", ok)[:, 0].tolist() == [1.0] * len(ok)
    assert driver("ok", bad)[:, 0].tolist() == [0.0] * len(bad)
    assert driver("ok", [(m, o, 3, 1, s) for m in sc.ALL_MASKS for o in (0, 1) for s in (0, 1, 2)]).all()


def test_size_forms(driver):
    """One record on each side of each threshold: LBS_SMALL_MAX_HANDS = 256 (csrc/mano_lbs.h), SDF_PREP_SMALL_MAX_HANDS = 128
    (csrc/sdf_collision.h), LBS_B2_MIN_HANDS = 256 and the streaming switch.  ihmr_hip.hip asserts the thresholds against the headers."""
    PREP_LARGE, PREP_SMALL, PREP_DENSE = 0, 1, 2
    cases = [(256, 0, 0), (257, 0, 0), (128, 0, 0), (129, 0, 0), (128, 1, 0), (129, 1, 0), (255, 0, 0), (256, 0, 1), (255, 0, 1), (2, 0, 0)]
    got = driver("forms", cases).astype(int)
    skin_small, prep, bwd2_lds = got[:, 0].tolist(), got[:, 1].tolist(), got[:, 2].tolist()
    assert skin_small == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert prep == [PREP_LARGE, PREP_LARGE, PREP_SMALL, PREP_LARGE, PREP_DENSE, PREP_DENSE, PREP_LARGE, PREP_LARGE, PREP_LARGE, PREP_SMALL]
    assert bwd2_lds == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]

"""One non-finite sample leaves the rest of its batch untouched.

A production batch is 512 samples for 4 x 301 iterations; a NaN in an annotation, an inf out of an untrained head or a parameter that
diverges mid-stage is an ordinary event there.  Every test here runs a CONTROL batch and the same batch with ONE sample (the victim)
poisoned in one place (tests/nonfinite_cases.py), every buffer inside guards (tests/guarded.py), and asserts -- exactly, on bit
patterns, no tolerance anywhere:

  (i)   every call returns 0 and the stream synchronises;
  (ii)  no guard is damaged, with the workspace pre-filled with 0x00, 0xFF and 0xA5 in turn;
  (iii) every output and state word of the OTHER samples is the control's;
  (iv)  the poisoned runs (one per fill) agree with each other everywhere, the victim's rows included;
  (v)   the victim's rows are the same bytes at every batch position the case is run at (seam B: 0, 1 and 2; the loop: 1, and 0 -- the
        sample whose workgroup zeroes the shared inside-voxel counters -- for the translation and orientation stages).

The inputs are those the audit of DESIGN.md ("Non-finite input") shows to be bounded; none is chosen to make a kernel fault.  What the
victim's rows hold is printed per case ([nonfinite] lines) and recorded in DESIGN.md.  `InterHandModel.test()` allocates its buffers
itself (torch): nothing of it can be moved between guards, its cases assert (i), (iii) and (iv); the encoder's ReLU is fmaxf, which
removes the NaN at the first layer (the rule for such a ReLU), so that case compares a sample whose values differ."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import nonfinite_cases as nc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
VICTIM = nc.VICTIM  # the control sample that is poisoned, wherever the case places it

# where the batch axis of a state buffer is (tests/test_gpu_stage_tails.py: STATE_KEYS); exports and everything else: axis 0
AXIS = {"state/orient": 1, "state/pose": 1, "state/shape": 1, "state/snap_loss": 2, "state/snap_params": 1, "state/verts": 1,
        "state/loss_batch": 1, "selected_history": 1, "kept": 1}


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _rows(res, b):
    """The victim's rows of every array."""
    return {k: np.take(v, [b], axis=AXIS.get(k, 0)) for k, v in res.items()}


def _assert_neighbours(got, ctrl, b, what):
    assert got.keys() == ctrl.keys(), what
    for k in got:
        x, y = np.delete(got[k], b, axis=AXIS.get(k, 0)), np.delete(ctrl[k], b, axis=AXIS.get(k, 0))
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), f"{what}: {k} of a sample other than {b} differs from the control's"


def _nonfinite(a):
    a = np.asarray(a)
    return int((~np.isfinite(a)).sum()) if a.dtype.kind == "f" else 0


# ================================================================================================ seam B: ihmr_sdf_collision_ex
def _faces(mano_arrays):
    right, left = mano_arrays
    return (torch.tensor(right["faces"].astype(np.int32)).cuda(), torch.tensor(left["faces"].astype(np.int32)).cuda())


def _collision(mano_arrays, hv, fill):
    from guarded import WORKSPACE_GUARD, Guarded, assert_guards
    from ihmr_amd import hip
    L, B = hip.lib(), hv.shape[0]
    fr, fl = _faces(mano_arrays)
    g = dict(hand_verts=Guarded(B * 2 * 778 * 3 * 4), loss=Guarded(B * 4), per_vert=Guarded(B * 1556 * 4), origin_scale=Guarded(B * 1556 * 4),
             dval=Guarded(B * 1556 * 3 * 4), workspace=Guarded(L.ihmr_sdf_workspace_bytes(B), guard=WORKSPACE_GUARD, fill=fill))
    g["hand_verts"].copy_in(hv.cuda())
    p = lambda k: C.c_void_p(g[k].data_ptr)
    hip.check(L.ihmr_sdf_collision_ex(hip.ptr(fr), hip.ptr(fl), p("hand_verts"), B, 0.0, None, p("loss"), p("per_vert"), p("origin_scale"),
                                      p("dval"), p("workspace"), hip.stream_ptr()), "ihmr_sdf_collision_ex")
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_sdf_collision_ex, B = {B}, fill = {fill:#04x}")
    assert np.array_equal(_bits(g["hand_verts"].view(torch.float32, tuple(hv.shape))), _bits(hv)), "the input vertices were written"
    return dict(loss=g["loss"].view(torch.float32, (B,)).cpu().numpy(), per_vert=g["per_vert"].view(torch.float32, (B, 1556)).cpu().numpy(),
                origin_scale=g["origin_scale"].view(torch.float32, (B, 1556)).cpu().numpy(),
                dval=g["dval"].view(torch.float32, (B, 1556, 3)).cpu().numpy())


_SEAM_CONTROL = {}


def _placed_pairs(mano_arrays, control, position):
    """(hand pairs with the victim at `position`, the control's outputs for them) -- computed once per control batch and position."""
    key = (control, position)
    if key not in _SEAM_CONTROL:
        hv, _ = nc.control(mano_arrays, control)
        order = list(range(nc.B))
        order[VICTIM], order[position] = order[position], order[VICTIM]
        placed = hv[torch.tensor(order)].contiguous()
        out = _collision(mano_arrays, placed, 0xA5)
        assert all(int((out["per_vert"][b] > 0).sum()) > 0 for b in range(nc.B)), "every control sample must penetrate"
        _SEAM_CONTROL[key] = (placed, out)
    return _SEAM_CONTROL[key]


@pytest.mark.parametrize("control", nc.CONTROL_KINDS)
@pytest.mark.parametrize("hands", list(nc.HANDS))
@pytest.mark.parametrize("kind", nc.VERTEX_KINDS)
def test_collision_entry_point_confines_a_poisoned_pair(mano_arrays, kind, hands, control):
    from guarded import FILLS
    victims, vertex = [], nc.deepest_vertices(mano_arrays, control)
    for position in range(nc.B):
        placed, ctrl = _placed_pairs(mano_arrays, control, position)
        poisoned = nc.poison_vertices(placed, position, kind, nc.HANDS[hands], vertex)
        runs = [_collision(mano_arrays, poisoned, fill) for fill in FILLS]
        for fill, r in zip(FILLS[1:], runs[1:]):
            _same(r, runs[0], f"{kind} / {hands}: workspace pre-filled with {fill:#04x} vs {FILLS[0]:#04x}")
        _assert_neighbours(runs[0], ctrl, position, f"{kind} / {hands} hand at position {position}")
        assert not all(np.array_equal(_bits(_rows(runs[0], position)[k]), _bits(_rows(ctrl, position)[k])) for k in ctrl), "the poison changed nothing"
        victims.append(_rows(runs[0], position))
    for position in (1, 2):
        _same(victims[position], victims[0], f"{kind} / {hands}: the victim's rows at position {position} vs position 0")
    v = victims[0]
    halves = lambda a: [a[0, :778], a[0, 778:]]        # entries 0..777 sample the RIGHT hand's grid at the left hand's vertices, 778.. the left hand's
    print(f"[nonfinite] seam B {control} {kind} / {hands}: loss {v['loss'][0]!r}; per grid (right, left): per_vert > 0 "
          f"{[int((h > 0).sum()) for h in halves(v['per_vert'])]}, non-finite per_vert {[_nonfinite(h) for h in halves(v['per_vert'])]}, "
          f"origin_scale {[_nonfinite(h) for h in halves(v['origin_scale'])]}, dval {[_nonfinite(h) for h in halves(v['dval'])]}")


# ================================================================================================ the refinement loop
def _make_opt(B, n_iters, **extra):
    return types.SimpleNamespace(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, num_joints=42,
                                 total_params_dim=122, cam_params_dim=3, pose_params_dim=96, shape_params_dim=20,
                                 trans_params_dim=3, model_root="", strategy="opt_default", save_mid_freq=1,
                                 optimizer="adam", opt_epoch=n_iters - 1, **extra)


def _loop_run(batch, stages, graphs, fill):
    """A fresh instance on guarded buffers: optimize() as the driver runs it (the stages, `keep_lists` on after the first, the closing
    forward).  Every C call is checked (`hip.check` raises on a non-zero return)."""
    from guarded import assert_guards, guard_model
    from ihmr_amd.optimize_model import OptimizeModel
    from test_gpu_stage_tails import STATE_KEYS
    B, n_iters = batch["init_cam"].shape[0], stages[0]["epoch"] + 1
    m = OptimizeModel(_make_opt(B, n_iters, use_graphs=graphs))
    m.strategy = stages
    guards = guard_model(m, fill)
    m.set_input(batch); m.init_optimize()
    m.optimize()
    torch.cuda.synchronize()
    assert_guards(guards, f"optimize(), B = {B}, graphs = {graphs}, fill = {fill:#04x}")
    out = {f"export/{k}": np.ascontiguousarray(v) for k, v in m.get_pred_result().items() if isinstance(v, np.ndarray)}
    out.update({f"state/{k}": m.buf[k].cpu().numpy() for k in STATE_KEYS})
    out["selected_history"] = torch.stack(m.selected_history).cpu().numpy()
    return out


def _param_vector(res):
    """(B,122): the parameter buffers in the slot order of snap_params (include/ihmr_hip.h: IHMR_PB_*)."""
    s = lambda k: res[f"state/{k}"]
    return np.concatenate([s("cam"), s("trans"), s("orient")[0], s("orient")[1], s("pose")[0], s("pose")[1], s("shape")[0], s("shape")[1]], axis=1)


def _initial_vector(batch):
    p, sh = batch["init_pose_params"].numpy(), batch["init_shape_params"].numpy()
    B = p.shape[0]
    return np.concatenate([batch["init_cam"].numpy(), batch["init_hand_trans"].numpy().reshape(B, -1)[:, :3], p[:, 0:3], p[:, 48:51], p[:, 3:48], p[:, 51:96],
                           sh[:, :10], sh[:, 10:]], axis=1).astype(np.float32)


def _check_selection(res, stage, victim, initial=None):
    """`selected` is the numpy replay of the product's select rule on the device's own snapshots; the stage's blocks hold
    snap_params[selected]; a select loss that is NaN from iteration 0 selects snapshot 0.  Returns (selected, the victim's select losses)."""
    from ihmr_amd import hip
    from ihmr_amd.optimize_model import stage_to_args
    sg = stage_to_args(stage, "adam", 1)
    S = stage["epoch"] + 1
    snap, sel = res["state/snap_loss"][:S], res["state/selected"]
    want = nc.select_replay(snap, list(sg.use_filter), list(sg.filter_factor), sg.select_loss)
    assert np.array_equal(sel, want), (sel.tolist(), want.tolist())
    vec, sp = _param_vector(res), res["state/snap_params"]
    for name, (bit, lo, size) in hip.PARAM_BLOCKS.items():
        if sg.param_mask & bit:
            for b in range(vec.shape[0]):
                assert np.array_equal(_bits(vec[b, lo:lo + size]), _bits(sp[sel[b], b, lo:lo + size])), f"{name} of sample {b} is not snapshot {sel[b]}"
                if initial is not None:
                    assert np.array_equal(_bits(sp[0, b, lo:lo + size]), _bits(initial[b, lo:lo + size])), f"snapshot 0 of {name}, sample {b}: not the entry value"
    key = snap[:, sg.select_loss, victim]
    if np.isnan(key[0]):
        assert sel[victim] == 0, "a select loss that is NaN from iteration 0 must leave the sample with the parameters it entered with"
    return sel, key


_LOOP_CONTROL = {}


def _loop_control(mano_arrays, control, tag, stages, graphs, position):
    key = (control, tag, graphs, position)
    if key not in _LOOP_CONTROL:
        _, batch = nc.control(mano_arrays, control)
        res = _loop_run(nc.place(batch, VICTIM, position), stages, graphs, 0xA5)
        assert all(np.isfinite(v).all() for v in res.values() if v.dtype.kind == "f"), "the control run is not finite"
        assert (res["state/loss_batch"][2] > 0).all(), "every control sample must collide"
        _LOOP_CONTROL[key] = res
    return _LOOP_CONTROL[key]


def _loop_case(mano_arrays, control, tag, stages, graphs, kind, positions):
    from guarded import FILLS
    _, batch = nc.control(mano_arrays, control)
    victims = {}
    for position in positions:
        placed = nc.place(batch, VICTIM, position)
        ctrl = _loop_control(mano_arrays, control, tag, stages, graphs, position)
        poisoned = nc.poison_batch(placed, position, kind)
        runs = [_loop_run(poisoned, stages, graphs, fill) for fill in FILLS]
        for fill, r in zip(FILLS[1:], runs[1:]):
            _same(r, runs[0], f"{kind}, {tag}: workspace pre-filled with {fill:#04x} vs {FILLS[0]:#04x}")
        _assert_neighbours(runs[0], ctrl, position, f"{kind}, {tag}, victim at position {position}")
        sel, key = _check_selection(runs[0], stages[-1], position, _initial_vector(poisoned) if len(stages) == 1 else None)
        _check_selection(ctrl, stages[-1], position)
        victims[position] = _rows(runs[0], position)
        v = victims[position]
        print(f"[nonfinite] loop {control} {kind} {tag} graphs={graphs} position {position}: select losses {key.tolist()} -> selected "
              f"{v['selected_history'][:, 0].tolist()}; non-finite words: parameters {_nonfinite(_param_vector(runs[0])[position])}, "
              f"adam_m {_nonfinite(v['state/adam_m'])}, verts {_nonfinite(v['state/verts'])}, loss_batch {_nonfinite(v['state/loss_batch'])}, "
              f"collision {v['state/loss_batch'][2, 0]!r}")
    first = positions[0]
    for position in positions[1:]:
        _same(victims[position], victims[first], f"{kind}, {tag}: the victim's rows at position {position} vs position {first}")
    return victims[first]


LOOP_CASES = [(kind, mask) for kind in nc.LOOP_KINDS for mask in nc.LOOP_MASKS]


@pytest.mark.parametrize("control,graphs", [("deep", True), ("deep", False), ("default", True), ("default", False)],
                         ids=["deep-graphs", "deep-eager", "default-graphs", "default-eager"])
@pytest.mark.parametrize("kind,mask", LOOP_CASES, ids=[f"{k}-mask{m}" for k, m in LOOP_CASES])
def test_one_stage_confines_a_poisoned_sample(mano_arrays, kind, mask, control, graphs):
    """One stage per tail form (masks 2, 3, 12, 48, 192, 255 of stage_cases.stage_for), three iterations, a snapshot each."""
    import stage_cases as sc
    assert len({sc.plan(m).step_tail for m in nc.LOOP_MASKS}) >= 4
    positions = (1, 0) if mask in nc.SAMPLE0_MASKS else (1,)
    _loop_case(mano_arrays, control, f"mask{mask}", [sc.stage_for(mask, nc.N_ITERS)], graphs, kind, positions)


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_a_nan_that_passes_the_filter_is_never_selected(mano_arrays, graphs):
    """The one difference from the reference's selection (include/ihmr_hip.h): a stage whose select loss carries no filter
    criterion (stage 1 of helpers.variant_strategy: filter on the collision loss, select on the 2-D joint loss).  The victim's 3-D target
    is +inf: its 2-D loss is finite at iteration 0 and NaN from iteration 1 on (the parameters are NaN by then), while its collision loss
    falls to 0 -- NaN vertices touch no voxel -- and passes the filter.  torch.argmin would select snapshot 1; the product keeps 0."""
    from helpers import variant_strategy
    from ihmr_amd.optimize_model import stage_to_args
    stage = variant_strategy(nc.N_ITERS - 1)[1]
    v = _loop_case(mano_arrays, "deep", "variant-stage1", [stage], graphs, "joints3d-inf", (1,))
    sg = stage_to_args(stage, "adam", 1)
    assert sg.use_filter[sg.select_loss] == 0, "the select loss must carry no filter criterion"
    snap = v["state/snap_loss"]                                          # (S,3,1): the victim's
    key, coll = snap[:, sg.select_loss, 0], snap[:, 2, 0]
    assert np.isfinite(key[0]) and np.isnan(key[1:]).all(), key.tolist()
    assert coll[0] > 0 and (coll[1:] == 0).all(), coll.tolist()
    assert int(v["state/selected"][0]) == 0
    assert int(nc.reference_select(snap, list(sg.use_filter), list(sg.filter_factor), sg.select_loss)[0]) == 1


@pytest.mark.parametrize("kind", ["joints2d-nan", "joints3d-inf", "trans-target-nan"])
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_default_stages_in_sequence_confine_a_poisoned_sample(mano_arrays, graphs, kind):
    """opt_default's four stages on one instance, `keep_lists` on after the first, the victim poisoned through a target.
    joints2d-nan: the 2-D loss is an L1 distance and the kernel's sign(NaN) is 0, so the NaN target contributes a zero gradient -- the
    victim's 2-D loss row is NaN in every iteration while its parameters stay finite (the reference's autograd would hand on a NaN).
    joints3d-inf: the gradient is infinite, the translation is NaN from the first stage's second iteration on -- while the candidate
    lists built in its first iteration exist -- and stage 0 hands the NaN on (snapshot 0's key is +inf: a rejected snapshot's 1e11 beats
    it, in the reference too), so stages 1 - 3 run on a NaN sample from their first iteration and their lists are kept, never read.
    trans-target-nan: the hand that comes BACK.  The translation's own gradient is NaN, so in the translation stage the victim is NaN
    in iterations 1 and 2 while the lists of iteration 0 exist; the stage selects snapshot 0 and the orientation stage starts -- with
    `keep_lists` -- on the finite entry pose again: its first iteration measures the displacement from the reference pose the lists
    were built at (never overwritten while the hand was NaN) and reuses them.  The later stages do not move the translation: finite."""
    from ihmr_amd.strategies import make_opt_strategy
    v = _loop_case(mano_arrays, "deep", "four-stages", make_opt_strategy(nc.N_ITERS - 1), graphs, kind, (1,))
    assert v["selected_history"].shape == (4, 1) and _nonfinite(v["state/loss_batch"]) > 0
    if kind == "joints2d-nan":
        assert np.isnan(v["state/loss_batch"][0, 0]) and _nonfinite(v["state/verts"]) == 0 and _nonfinite(v["state/adam_m"]) == 0
    elif kind == "trans-target-nan":
        # back to finite: the translation is the entry value's bits (snapshot 0 of stage 0), vertices and parameters finite at the end
        assert int(v["selected_history"][0, 0]) == 0 and _nonfinite(v["state/verts"]) == 0 and _nonfinite(v["state/trans"]) == 0
        entry = nc.control(mano_arrays, "deep")[1]["init_hand_trans"][VICTIM, 0, :3].numpy()
        assert np.array_equal(_bits(v["state/trans"][0]), _bits(entry)), "the victim's translation is not the value it entered with"
        assert np.isnan(v["state/loss_batch"][6, 0]), "the translation loss of a NaN target is NaN"
    else:
        assert v["selected_history"][:, 0].tolist() == [1, 0, 0, 0] and _nonfinite(v["state/verts"]) > 0 and _nonfinite(v["state/trans"]) > 0


@pytest.mark.parametrize("kind", ["joints2d-nan", "joints3d-inf"])
def test_four_stages_at_65_samples_confine_the_last_one(mano_arrays, kind):
    """B = 65 is 130 hands, more than SDF_PREP_SMALL_MAX_HANDS = 128: the 512-thread form of the prep kernel; the last sample is the
    victim, two iterations per stage."""
    import stage_cases as sc
    from guarded import FILLS
    from ihmr_amd.strategies import make_opt_strategy
    B, stages = 65, make_opt_strategy(1)
    batch = sc.batch(mano_arrays, "deep", B)
    key = ("deep65", "four-stages-2", True, B - 1)
    if key not in _LOOP_CONTROL:
        _LOOP_CONTROL[key] = _loop_run(batch, stages, True, 0xA5)
    ctrl = _LOOP_CONTROL[key]
    assert all(np.isfinite(v).all() for v in ctrl.values() if v.dtype.kind == "f")
    poisoned = nc.poison_batch(batch, B - 1, kind)
    runs = [_loop_run(poisoned, stages, True, fill) for fill in FILLS]
    for r in runs[1:]:
        _same(r, runs[0], "B = 65: two fills")
    _assert_neighbours(runs[0], ctrl, B - 1, "B = 65, victim 64")
    _check_selection(runs[0], stages[-1], B - 1)
    victim = _rows(runs[0], B - 1)
    if kind == "joints2d-nan":
        assert np.isnan(victim["state/loss_batch"][0, 0]) and _nonfinite(victim["state/verts"]) == 0
    else:
        assert _nonfinite(victim["state/verts"]) > 0 and _nonfinite(victim["state/adam_m"]) > 0, "the victim never turned NaN"


# ================================================================================================ MLPModel.test()
def _mlp_run(batch, fill, graph):
    """MLPModel.test() on the golden batch, the core's buffers, the four "prev" tables and both workspaces guarded (as
    tests/test_gpu_guarded_refinement.py does)."""
    from guarded import WORKSPACE_GUARD, Guarded, assert_guards, guard_model
    from helpers import seeded_state_dict
    from ihmr_amd import hip
    from ihmr_amd.mlp_model import MLPModel
    from ihmr_amd.strategies import make_mlp_strategy
    from test_gpu_guarded_refinement import TABLES, _mlp_opt
    B, num_data, strategy = batch["init_cam"].shape[0], 10, make_mlp_strategy()
    m = MLPModel(_mlp_opt(B, use_test_graph=graph))
    guards = guard_model(m._core, fill)
    m.set_update_info(strategy, num_data)
    for sid in range(len(strategy)):
        m.add_new_network(sid)
        m.sub_network_list[sid].load_state_dict(seeded_state_dict(m.sub_network_list[sid], 900 + sid, last_scale=0.02))
    m.eval()
    gen = torch.Generator().manual_seed(17)
    for k in TABLES:
        t = getattr(m, k)
        if k != "data_idxs_all":
            t.copy_(torch.rand(t.shape, generator=gen).to(m.device))      # rows no batch touches carry a pattern
        guards[k] = Guarded(t.numel() * t.element_size())
        setattr(m, k, guards[k].copy_in(t))
    m.set_input(batch)
    g = m._glue()
    guards["mlp_workspace"] = Guarded(hip.lib().ihmr_mlp_workspace_bytes(B), guard=WORKSPACE_GUARD, fill=fill)
    assert g["ws"].numel() == guards["mlp_workspace"].nbytes
    g["ws"] = guards["mlp_workspace"].payload_bytes()
    m.set_input(batch); m.test()
    torch.cuda.synchronize()
    assert_guards(guards, f"MLPModel.test(), fill = {fill:#04x}, graph = {graph}")
    res = {f"export/{k}": np.asarray(v) for k, v in m.get_pred_result().items()}
    res["kept"] = torch.stack(m.kept_history).cpu().numpy().astype(np.uint8)
    tables = {k: getattr(m, k).cpu().numpy().astype(np.uint8 if k == "data_idxs_all" else np.float32) for k in TABLES}
    return res, tables, m._init_packed.cpu().numpy()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("poison", [("img_feat", (100,), nc.NAN), ("init_pose_params", (10,), nc.NAN)], ids=["img-feat-nan", "pose-nan"])
def test_mlp_evaluation_confines_a_poisoned_sample(mano_arrays, poison, graph):
    from guarded import FILLS
    g = dict(np.load(os.path.join(GOLD, "mlp_test.npz")))
    batch = {k[3:]: torch.tensor(v) for k, v in g.items() if k.startswith("in_")}
    b = 2                       # (the golden batch's sample 2 keeps two stages' updates in the control run; sample 1 keeps none)
    row = int(batch["index"][b])
    ctrl, ctrl_tables, _ = _mlp_run(batch, 0xA5, graph)
    assert ctrl["kept"][:, b].any(), "the control's victim keeps no update: `kept == 0` would say nothing"
    poisoned = nc.poison_batch(batch, b, poison)
    runs = [_mlp_run(poisoned, fill, graph) for fill in FILLS]
    for res, tables, _ in runs[1:]:
        _same(res, runs[0][0], "MLPModel.test(): two fills")
        _same(tables, runs[0][1], "MLPModel.test(): the tables of two fills")
    res, tables, first = runs[0]
    _assert_neighbours(res, ctrl, b, f"MLPModel.test(), {poison[0]}")
    for k in tables:
        assert np.array_equal(_bits(np.delete(tables[k], row, axis=0)), _bits(np.delete(ctrl_tables[k], row, axis=0))), f"{k}: a row of another sample differs"
    assert not res["kept"][:, b].any(), f"the victim kept an update: {res['kept'][:, b].tolist()}"
    assert np.array_equal(_bits(tables["prev_final"][row]), _bits(first[b])), "the victim's prev_final row is not its first evaluation's"
    assert tables["data_idxs_all"][row] == 1
    print(f"[nonfinite] MLP {poison[0]} graph={graph}: kept (control) {ctrl['kept'].sum(axis=0).tolist()} (poisoned) {res['kept'].sum(axis=0).tolist()}; "
          f"victim prev_loss {tables['prev_loss'][row].tolist()}, non-finite prev_final {_nonfinite(tables['prev_final'][row])}, "
          f"verts {_nonfinite(res['export/pred_right_hand_verts'][b]) + _nonfinite(res['export/pred_left_hand_verts'][b])}")


# ================================================================================================ InterHandModel.test()
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_baseline_inference_confines_a_nan_pixel(mano_arrays, precision, graph):
    from helpers import seeded_state_dict
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    from test_gpu_models import _opt
    B, b = 4, VICTIM
    m = InterHandModel(_opt(B, use_test_graph=graph, encoder_precision=precision))
    sd = seeded_state_dict(m.encoder, 40)
    sd["regressor_ih.0.weight"] *= 0.05; sd["regressor_ih.0.bias"] *= 0.05
    m.encoder.load_state_dict(sd)
    m.eval()
    fwd = lambda p, s, t: two_hand.forward_from_packed(m.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    batch = synthetic_opt_batch(B, fwd, seed=5, with_image=True)
    poisoned = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    poisoned["img"][b, 1, 17, 23] = nc.NAN

    def run(data):
        m.set_input(data); m.test()
        torch.cuda.synchronize()
        out = {k: np.asarray(v) for k, v in m.get_pred_result().items()}
        out["final_params"] = m.final_params.cpu().numpy()
        return out
    ctrl, first, second, again = run(batch), run(poisoned), run(poisoned), run(batch)
    assert all(np.isfinite(v).all() for v in ctrl.values() if v.dtype.kind == "f")
    _same(second, first, "two poisoned calls")
    _same(again, ctrl, "the control after the poisoned calls")
    _assert_neighbours(first, ctrl, b, f"InterHandModel.test(), {precision}")
    for k in ("final_params", "pred_right_hand_verts", "pred_left_hand_verts"):
        assert k in first
    changed = not np.array_equal(_bits(first["final_params"][b]), _bits(ctrl["final_params"][b]))
    print(f"[nonfinite] baseline {precision} graph={graph}: victim's final_params non-finite {_nonfinite(first['final_params'][b])} of 122 "
          f"(changed: {changed}), vertices non-finite {_nonfinite(first['pred_right_hand_verts'][b]) + _nonfinite(first['pred_left_hand_verts'][b])}")

"""Preconditions of tests/test_gpu_nonfinite.py, on the host: every sample of both control batches penetrates (float32 oracle), so the
victim AND its neighbours are in the collision kernels' work queues; a poisoned batch differs from its control in the victim alone; the
numpy replay of the select rule is the reference's rule on finite snapshots and differs from it exactly where a NaN select loss passes
the filter.  The oracle's C grid code is called on the control batches only -- never on a non-finite vertex."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nc


@pytest.mark.parametrize("kind", nc.CONTROL_KINDS)
def test_every_sample_of_the_control_batches_penetrates(mano_arrays, kind):
    from oracle.sdf_ref import SDFLossRef
    right, left = mano_arrays
    hv, batch = nc.control(mano_arrays, kind)
    assert hv.shape == (nc.B, 2, 778, 3) and bool(torch.isfinite(hv).all())
    assert all(bool(torch.isfinite(v.float()).all()) for v in batch.values())
    assert bool((batch["hand_type_array"] == 1).all()), "every control sample is two-handed (the collision mask is 1)"
    loss, per_vert, _ = SDFLossRef(right["faces"], left["faces"])(hv, return_per_vert_loss=True, return_origin_scale_loss=True)
    pen = (per_vert > 0).view(nc.B, 2, 778).sum(dim=2)
    print(f"[nonfinite] {kind}: penetrating vertices per sample and hand {pen.tolist()}, loss {loss.tolist()}")
    assert bool((pen.sum(dim=1) > 0).all()), pen.tolist()
    # the vertices the kernels see at the loop's first iteration are these: the batch's initial parameters give hv
    assert batch["init_pose_params"].shape == (nc.B, 96) and batch["init_hand_trans"].shape == (nc.B, 1, 4)


def test_a_poisoned_batch_differs_from_its_control_in_the_victim_alone(mano_arrays):
    _, batch = nc.control(mano_arrays, "deep")
    for position in range(nc.B):
        placed = nc.place(batch, 1, position)
        for k in batch:          # a permutation of the control's samples
            assert torch.equal(placed[k][position], batch[k][1]) and torch.equal(placed[k][1], batch[k][position]), k
        for kind, (key, index, value) in nc.LOOP_KINDS.items():
            poisoned = nc.poison_batch(placed, position, kind)
            assert nc.differs_only_in(placed, poisoned, position), (kind, position)
            got = float(poisoned[key][(position,) + index])
            assert (np.isnan(got) and np.isnan(value)) or got == np.float32(value), kind
    assert set(nc.LOOP_KINDS) == set(nc.TARGET_KINDS) | set(nc.STATE_KINDS) and len(nc.LOOP_KINDS) == 9


def test_vertex_kinds_touch_only_the_victims_hands(mano_arrays):
    hv, _ = nc.control(mano_arrays, "default")
    vertex = nc.deepest_vertices(mano_arrays, "default")
    assert all(0 <= v < 778 for v in vertex + nc.deepest_vertices(mano_arrays, "deep"))
    for kind in nc.VERTEX_KINDS:
        for hands in nc.HANDS.values():
            for b in range(nc.B):
                p = nc.poison_vertices(hv, b, kind, hands, vertex)
                changed = (p.view(torch.int32) != hv.view(torch.int32)).view(nc.B, 2, -1).any(dim=2)
                want = torch.zeros(nc.B, 2, dtype=torch.bool)
                want[b, list(hands)] = True
                assert torch.equal(changed, want), (kind, hands, b)
    # what each kind does to the hand's box (max - min per axis, float32): the classes the audit table names
    v = nc.poison_vertices(hv, 0, "extent-overflow", (0,), vertex)[0, 0]
    assert bool(torch.isinf(v.max(dim=0)[0] - v.min(dim=0)[0]).all()) and bool(torch.isfinite((v.max(dim=0)[0] + v.min(dim=0)[0]) * 0.5).all())
    v = nc.poison_vertices(hv, 0, "all-equal", (0,), vertex)[0, 0]
    assert float((v.max(dim=0)[0] - v.min(dim=0)[0]).abs().max()) == 0.0
    v = nc.poison_vertices(hv, 0, "vertex-1e30", (0,), vertex)[0, 0]
    assert bool(torch.isfinite(v.max(dim=0)[0] - v.min(dim=0)[0]).all())


def test_select_replay_is_the_references_rule_except_for_a_nan_that_passes_the_filter():
    assert int(torch.argmin(torch.tensor([1.0, float("nan"), 0.0, float("nan")]))) == 1, "torch.argmin takes the first NaN for the minimum"
    rng = np.random.default_rng(5)
    S, nb = 4, 64
    snap = rng.uniform(0.5, 1.5, (S, 3, nb)).astype(np.float32)
    snap[2, :, :8] = snap[0, :, :8]                         # ties: the first minimum wins in both
    for use, fac, sel in (((1, 0, 0), (1.001, 1.0, 1.0), 0), ((1, 0, 1), (1.051, 1.0, 0.9), 1), ((1, 0, 0), (1.05, 1.0, 1.0), 2), ((0, 0, 1), (1.0, 1.0, 0.9), 0)):
        assert np.array_equal(nc.select_replay(snap, use, fac, sel), nc.reference_select(snap, use, fac, sel)), (use, sel)
    # NaN in a FILTERED select loss: the row fails the filter in both rules
    bad = snap.copy()
    bad[1, 0, :] = np.nan
    assert np.array_equal(nc.select_replay(bad, (1, 0, 0), (2.0, 1.0, 1.0), 0), nc.reference_select(bad, (1, 0, 0), (2.0, 1.0, 1.0), 0))
    # NaN from snapshot 0 on: both select 0
    bad = snap.copy()
    bad[:, :, :] = np.nan
    assert not nc.select_replay(bad, (1, 0, 0), (2.0, 1.0, 1.0), 0).any() and not nc.reference_select(bad, (1, 0, 0), (2.0, 1.0, 1.0), 0).any()
    # the one difference: the select loss carries no filter criterion and is NaN in a row that passes the filter
    bad = snap.copy()
    bad[:, 0, :] = 1.0                                      # every row passes the filter on loss 0
    bad[2, 2, :] = np.nan
    mine, ref = nc.select_replay(bad, (1, 0, 0), (1.001, 1.0, 1.0), 2), nc.reference_select(bad, (1, 0, 0), (1.001, 1.0, 1.0), 2)
    assert (ref == 2).all() and (mine != 2).all()
    finite = np.where(np.isnan(bad[:, 2, :]), np.inf, bad[:, 2, :])
    assert np.array_equal(mine, finite.argmin(axis=0))

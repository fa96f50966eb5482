"""The Evaluator's one packing of its metric families (base, PA, volume, curves: `packed_sums` / `metrics_from_packed`, what
`run_optimize` all-reduces) and its one list of device accumulators, on the host: the packed vector is the concatenation of the
families' own `*_sums()`, the dict of a reduced vector the union of their `*_from_sums`, and the list is what `clear()` empties and
what an older pickle may lack."""
import itertools
import pickle

import numpy as np
import pytest
import torch

import curve_cases as CC
from ihmr_amd import evaluator as E


@pytest.fixture(scope="module")
def batch():
    res, data_list, _ = CC.evaluator_batch()
    return res, data_list


def _volume_rows(seed, B):
    """What update_device_volume leaves behind for one batch, made up on the host (tests/test_volume_cpu.py)."""
    rng = np.random.RandomState(seed)
    kept = rng.rand(B) < 0.8
    counted = kept & (rng.rand(B) < 0.6)
    return torch.from_numpy(np.stack([np.where(counted, rng.rand(B) * 7.0, 0.0), kept.astype(np.float64), counted.astype(np.float64),
                                      (kept & ~counted).astype(np.float64)], axis=1))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("pa,vol,curves", list(itertools.product((False, True), repeat=3)))
def test_the_packed_vector_is_the_families_sums_and_unpacks_to_their_metrics(batch, pa, vol, curves):
    res, data_list = batch
    ev = E.Evaluator(CC.mano_models(), data_list=data_list, pa_metrics=pa, volume_metric=vol, curve_metrics=curves)
    ev.update(np.arange(3), {k: v[:3].copy() for k, v in res.items()})
    if vol:
        ev._device_volume_parts += [_volume_rows(3, 13), _volume_rows(4, 6)]
    parts = ([ev.metric_sums()] + ([ev.pa_metric_sums()] if pa else []) + ([ev.volume_sums()] if vol else []) + ([ev.curve_sums()] if curves else []))
    packed = ev.packed_sums()
    assert packed.dtype == np.float64 and packed.tobytes() == np.concatenate(parts).tobytes()
    assert len(packed) == 9 + 6 * pa + 4 * vol + (5 * 101 + 2 * 3 + 2 * 51) * curves
    assert packed[1] > 0 and (not pa or packed[10] > 0) and (not vol or packed[9 + 6 * pa + 1] > 0) and (not curves or packed[9 + 6 * pa + 4 * vol + 100] > 0)
    for reduced in (packed, 2.0 * packed, np.zeros_like(packed)):          # one rank, two equal ranks, nothing counted (NaN metrics)
        want, at = {}, 0
        for used, n, from_sums in ((True, 9, E.Evaluator.metrics_from_sums), (pa, 6, E.Evaluator.pa_metrics_from_sums),
                                   (vol, 4, E.Evaluator.volume_metrics_from_sums), (curves, len(reduced), E.Evaluator.curve_metrics_from_sums)):
            if used:
                want.update(from_sums(reduced[at:at + n]))
                at += n
        got = ev.metrics_from_packed(reduced)
        assert list(got) == list(want) and all(_same(got[k], want[k]) for k in want), (pa, vol, curves)
        assert ("pa_mpjpe_3d" in got) == pa and ("pen_volume" in got) == vol and ("auc_j3d" in got) == curves and "mpjpe_3d" in got
    with pytest.raises(AssertionError):
        ev.metrics_from_packed(packed[:-1])


def test_the_curve_family_unpacks_with_the_evaluators_own_tables(batch):
    res, data_list = batch
    thr, fthr = CC.pck_table(CC.EVAL_T), CC.F_TABLES[CC.EVAL_F]
    ev = E.Evaluator(CC.mano_models(), data_list=data_list, curve_metrics=True, thresholds=thr, f_thresholds=fthr)
    ev.update(np.arange(2), {k: v[:2].copy() for k, v in res.items()})
    got, want = ev.metrics_from_packed(ev.packed_sums()), E.Evaluator.curve_metrics_from_sums(ev.curve_sums(), thr, fthr)
    assert all(_same(got[k], want[k]) for k in want) and len(got["pck_j3d"]) == len(thr)


def test_clear_empties_every_accumulator_and_an_old_pickle_still_sums_to_zeros(batch):
    names = E.Evaluator.DEVICE_ACCUMULATORS
    assert len(names) == 7 and names[-1] == "_device_volume_parts"
    ev = E.Evaluator(CC.mano_models(), pa_metrics=True, curve_metrics=True, volume_metric=True)
    assert [k for k in ev.__dict__ if k.startswith("_device_")] == list(names)
    assert [k for k in E.Evaluator(CC.mano_models()).__dict__ if k.startswith("_device_")] == list(names[:-1])
    T, F = len(ev.thresholds), len(ev.f_thresholds)
    made_up = {"_device_parts": torch.ones(2, 7, dtype=torch.float64), "_device_vert_parts": torch.ones(2, 2, dtype=torch.float64),
               "_device_pa_parts": torch.ones(2, 4, dtype=torch.float64), "_device_pa_vert_parts": torch.ones(2, 2, dtype=torch.float64),
               "_device_curve_parts": torch.ones(2, 3, T + 1, dtype=torch.float64),
               "_device_curve_vert_parts": (torch.ones(2, 2, T + 1, dtype=torch.float64), torch.ones(2, 2, 2, 2, F, dtype=torch.float64),
                                            torch.ones(2, 2, 2, dtype=torch.float64)),
               "_device_volume_parts": _volume_rows(3, 5)}
    for name in names:
        for _ in range(2):
            getattr(ev, name).append(made_up[name])
    assert ev.metric_sums().tolist() == [4.0] * 9 and ev.pa_metric_sums().tolist() == [4.0] * 6 and ev.volume_sums()[1] > 0
    c = ev.curve_sums()
    assert (c[:5 * (T + 1)] == 4.0).all() and c[5 * (T + 1) + F] == 8.0 and c[-1] == 4.0       # counts; 4 rows x 2 hands; interacting rows
    assert ev._device_column_sums("_device_pa_parts").tolist() == [4.0] * 4
    ev.clear()
    assert all(getattr(ev, name) == [] for name in names) and ev.pred_results == []
    assert all(ev._device_column_sums(name) is None for name in names)
    zeros = [ev.metric_sums(), ev.pa_metric_sums(), ev.volume_sums(), ev.curve_sums()]
    assert [len(z) for z in zeros] == [9, 6, 4, 5 * (T + 1) + 2 * (F + 1) + 2 * 51] and not any(z.any() for z in zeros)
    # an Evaluator pickled before the PA, curve and volume metrics existed has none of their attributes
    old = pickle.loads(pickle.dumps(ev))
    for k in ("pa_metrics", "curve_metrics", "volume_metric", "volume_subdiv") + names[2:]:
        old.__dict__.pop(k)
    assert all(old._device_column_sums(name) is None for name in names)
    for got, want in zip((old.metric_sums(), old.pa_metric_sums(), old.volume_sums(), old.curve_sums()), zeros):
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert len(old.packed_sums()) == 9 and list(old.metrics_from_packed(old.packed_sums())) == ["mpjpe_3d", "inter_mpjpe_3d", "collision_ave", "collision_max"]
    old.clear()                                                            # as before: clear() gives such an object its lists, but no volume
    assert [k for k in old.__dict__ if k.startswith("_device_")] == list(names[:2]) + list(names[2:-1])


def test_keep_is_a_selection_on_every_part():
    """`Evaluator._kept`, the one keep rule of the `update_device_*` methods: a kept row keeps its bits, a dropped row is +0 whatever it held."""
    keep = torch.tensor([True, False, True])
    a = torch.tensor([[1.5, 0.0], [float("nan"), float("inf")], [3.0, 7.0]], dtype=torch.float64)
    b = torch.arange(24, dtype=torch.float64).reshape(3, 2, 4)
    b[1, 0, 0] = float("nan")
    ev = E.Evaluator()
    ka, kb = ev._kept(keep, a, b)
    assert ka.dtype == kb.dtype == torch.float64 and ka.shape == a.shape and kb.shape == b.shape
    assert ka.numpy().tobytes() == np.array([[1.5, 0.0], [0.0, 0.0], [3.0, 7.0]]).tobytes()
    assert kb[0].equal(b[0]) and kb[2].equal(b[2]) and kb[1].numpy().tobytes() == np.zeros((2, 4)).tobytes()
    assert ev._kept(None, a, b) == (a, b)
    finite = torch.tensor([[1.5, 0.0], [2.5, 4.0], [3.0, 7.0]], dtype=torch.float64)
    assert ev._kept(keep, finite)[0].numpy().tobytes() == (finite * keep.to(torch.float64)[:, None]).numpy().tobytes()

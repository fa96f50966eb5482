"""The cases of tests/test_gpu_mano_layer.py (tests/mano_cases.py) checked on the CPU: that the generators are deterministic, that the
`zero` class is an exactly zero rotation, which term of `within`'s bound governs in which pose class (the float32 oracle's own distance
from float64, or the floor), and that the hand counts of the GPU tests reach every slot of the skin kernel's workgroups."""
import numpy as np
import pytest
import torch

import mano_cases as MC

N_COND = 16


@pytest.fixture(scope="module")
def conditioning(mano_arrays):
    """{class: {output: (|oracle32 - f64|, floor, max|f64|)}} at 16 hands of the right asset."""
    right, _ = mano_arrays
    out = {}
    for name in MC.CLASSES:
        c = MC.case(name, N_COND, 31, right["hands_mean"])
        f64, o32 = MC.reference(right, c, torch.float64), MC.reference(right, c, torch.float32)
        out[name] = {k: (MC.distances(o32[k], f64[k], o32[k])[0], MC.floor_of(k, f64[k]), float(np.abs(f64[k]).max())) for k in MC.OUTPUTS}
    return out


def test_generators_are_deterministic(mano_arrays):
    hm = mano_arrays[0]["hands_mean"]
    for name in MC.CLASSES + ("mixed",):
        a, b, other = MC.case(name, 9, 5, hm), MC.case(name, 9, 5, hm), MC.case(name, 9, 6, hm)
        for k in ("orient", "pose", "betas", "gv", "gj"):
            assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), (name, k)
        assert not np.array_equal(a["gv"], other["gv"])
        if name != "zero":
            assert not np.array_equal(a["orient"], other["orient"]), name
    a = MC.case("mixed", 12, 5, hm)
    perm = np.random.RandomState(0).permutation(12)
    p = MC.permuted(a, perm)
    assert np.array_equal(p["pose"], a["pose"][perm]) and np.array_equal(p["gj"], a["gj"][perm]) and p["pose"].flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("side", [0, 1], ids=["right", "left"])
def test_zero_class_is_an_exactly_zero_full_pose(mano_arrays, side):
    arr = mano_arrays[side]
    c = MC.case("zero", 5, 1, arr["hands_mean"])
    assert np.array_equal(MC.full_pose(c, arr["hands_mean"]), np.zeros((5, 48), np.float32))
    assert not c["betas"].any()
    # ... and in the oracle, in both precisions: what it feeds to Rodrigues
    from oracle.mano_ref import ManoRef
    for dtype in (torch.float32, torch.float64):
        ref = ManoRef(MC.rounded_asset(arr), dtype=dtype)
        out = ref(global_orient=torch.tensor(c["orient"], dtype=dtype), hand_pose=torch.tensor(c["pose"], dtype=dtype),
                  betas=torch.tensor(c["betas"], dtype=dtype))
        assert not out.full_pose.numpy().any(), dtype


@pytest.mark.parametrize("name,scale", sorted(MC.TINY.items()))
def test_tiny_classes_have_the_full_pose_they_are_named_for(mano_arrays, name, scale):
    """float64 sees the angles float32 sees to within the one rounding of pose + hands_mean (exact by Sterbenz's lemma wherever the
    angle is below half the mean's entry, i.e. almost everywhere in tiny6 and tiny4); their spread is the class's."""
    hm = mano_arrays[0]["hands_mean"]
    c = MC.case(name, 64, 2, hm)
    fp32 = MC.full_pose(c, hm)
    fp64 = np.concatenate([c["orient"].astype(np.float64), c["pose"].astype(np.float64) + np.float32(hm).astype(np.float64)[None]], 1)
    assert np.abs(fp32.astype(np.float64) - fp64).max() <= 2.0 ** -24 * np.abs(c["pose"]).max()
    if name != "tiny3":
        assert np.mean(fp32.astype(np.float64) == fp64) > 0.99
    assert 0.9 * scale < fp32.std() < 1.1 * scale and np.abs(fp32).max() < 6 * scale


def test_mixed_class_deals_the_classes_round_robin(mano_arrays):
    hm = mano_arrays[0]["hands_mean"]
    N = 33
    c = MC.case("mixed", N, 3, hm)
    fp = np.abs(MC.full_pose(c, hm)).max(axis=1)
    cls = MC.class_of_hand("mixed", N)
    assert np.array_equal(cls, np.arange(N) % 6)
    for k in range(N):
        name = MC.CLASSES[cls[k]]
        if name == "zero":
            assert fp[k] == 0
        elif name in MC.TINY:
            assert 0.5 * MC.TINY[name] < fp[k] < 6 * MC.TINY[name], (k, name, fp[k])
        else:
            assert fp[k] > 0.3, (k, name, fp[k])
    # a packed pair of the skin kernel (slots 2q, 2q + 1: hands 8 apart) never holds one class twice, and a group holds at least three
    big = MC.class_of_hand("mixed", 64)
    for HG in (4, 8):
        hands = [MC.lbs_group_hand(HG, 3, 0, i) for i in range(HG)]
        assert all(big[hands[2 * q]] != big[hands[2 * q + 1]] for q in range(HG // 2))
        assert len({int(big[h]) for h in hands}) >= 3


def test_conditioning_table(conditioning):
    """Which term of the bound max(floor, 1.5 |oracle32 - f64|) governs where: the float32 oracle is inside the floor in every output
    of `mild`, `zero`, `tiny6` and `large` (there the floor is the bound, as in the existing LBS tests), and OUTSIDE it in the rotation
    gradients of `tiny4`, where `cos a - sin a / a` cancels in float32 (there the bound is 1.5 x the oracle's own distance)."""
    for name, row in conditioning.items():
        print(f"[mano cases] {name:6s} " + "  ".join(f"{k} {d / (top if k.startswith('d_') else 1.0):.2e} (floor {f / (top if k.startswith('d_') else 1.0):.1e})"
                                                       for k, (d, f, top) in row.items()))
    for name in ("mild", "zero", "tiny6", "large"):
        for k, (d, f, _) in conditioning[name].items():
            assert d < f, (name, k, d, f)
    for k in ("d_orient", "d_pose"):
        d, f, _ = conditioning["tiny4"][k]
        assert d > f, ("tiny4", k, d, f)
    for name in MC.TINY:                                      # the shape gradient and the forward are conditioned everywhere
        for k in ("verts", "joints", "d_betas"):
            d, f, _ = conditioning[name][k]
            assert d < f, (name, k, d, f)


def test_within_takes_the_larger_of_floor_and_ratio():
    f64 = np.array([1.0, -2.0, 0.5])
    o32 = f64 + np.array([1e-3, 0, 0])
    assert MC.within(f64 + np.array([0, 1.4e-3, 0]), f64, o32, 1e-6) == pytest.approx(1.4)
    with pytest.raises(AssertionError):
        MC.within(f64 + np.array([0, 1.6e-3, 0]), f64, o32, 1e-6)
    MC.within(f64 + np.array([0, 0, 9e-3]), f64, o32, 1e-2)                 # the floor governs
    with pytest.raises(AssertionError):
        MC.within(f64 + np.array([0, 0, 1.1e-2]), f64, o32, 1e-2)
    with pytest.raises(AssertionError):
        MC.within(np.array([1.0, np.nan, 0.5]), f64, o32, 1e-2)
    assert MC.floor_of("d_pose", f64) == 2e-5 * 2.0
    assert MC.floor_of("verts", np.array([0.1])) == 2e-6 and MC.floor_of("joints", np.array([0.8])) == pytest.approx(8e-6)


def test_hand_counts_reach_every_slot_of_a_skin_workgroup():
    """`lbs_group_hand(x, s, i) = x + 8 (HG s + i)`: for each of HG = 4 (up to 256 hands) and HG = 8 (above), the hand counts of the
    GPU tests hold a launch with a workgroup whose slots 0 .. HG - 1 are all real hands, and one with a workgroup where a real hand
    sits next to an empty slot (the `hid < N` / `min(h, N - 1)` clamps with real neighbours)."""
    full, ragged = set(), set()
    for N in MC.N_LIST:
        slots = MC.skin_slots(N)
        HG = MC.skin_hands_per_group(N)
        assert slots.shape == ((N + 8 * HG - 1) // (8 * HG) * 8, HG)
        assert int(slots.sum()) == N                                             # every hand has exactly one slot
        hands = sorted(MC.lbs_group_hand(HG, g % 8, g // 8, i) for g in range(slots.shape[0]) for i in range(HG) if slots[g, i])
        assert hands == list(range(N))
        if slots.all(axis=1).any():
            full.add(HG)
        if (slots.any(axis=1) & ~slots.all(axis=1)).any():
            ragged.add(HG)
    assert full == {4, 8} and ragged == {4, 8}
    # what the counts up to 8 cannot do: slot 1 is never a real hand
    for N in range(1, 9):
        assert not MC.skin_slots(N)[:, 1:].any()
    assert MC.skin_slots(9)[0, 1] and not MC.skin_slots(9)[0, 2]
    assert MC.skin_slots(33).shape[0] == 16 and MC.skin_slots(32).shape[0] == 8     # the second hand group starts at 33 (small form)
    assert MC.skin_slots(321).shape[0] == 48 and MC.skin_slots(320).shape[0] == 40   # 321 opens the SIXTH group of the large form (64 hands each)
    assert MC.skin_slots(257).shape[0] == 40                                         # ... whose groups 1 - 4 the first large launch already has
    assert MC.skin_hands_per_group(256) == 4 and MC.skin_hands_per_group(257) == 8

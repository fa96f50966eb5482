"""``ihmr_sdf_volume`` on the GPU against the float32 statement of tests/volume_ref.py: counts, bits (every word), status and box bit
for bit -- an integer-equal count is the bar, there is no tolerance -- inside guarded buffers; batch independence, the keep mask, the
other statuses, the refusals; then ``penetration_volume``, ``Evaluator.update_device_volume`` and ``run_optimize --volume_metric``."""
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import volume_ref as VR  # noqa: E402
from guarded import Guarded, assert_guards  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(cases, n, keep=None, with_bits=True, fill=0xFF, override=None):
    """One call of the C ABI on a batch of cases of one group, every buffer guarded, the outputs pre-filled with ``fill``.  Returns
    (rc, dict of numpy outputs); the guards are checked."""
    from ihmr_amd import hip
    B, T = len(cases), n ** 3
    c0 = cases[0]
    assert all(c.group == c0.group for c in cases)
    va, vb = np.stack([c.va for c in cases]), np.stack([c.vb for c in cases])
    g = dict(va=Guarded(va.nbytes), vb=Guarded(vb.nbytes), fa=Guarded(c0.fa.nbytes), fb=Guarded(c0.fb.nbytes),
             box=Guarded(B * 16, fill=fill), status=Guarded(B * 4, fill=fill), counts=Guarded(B * T * 4, fill=fill))
    if with_bits:
        g["bits"] = Guarded(B * T * 4096, fill=fill)
    if keep is not None:
        g["keep"] = Guarded(B)
        g["keep"].copy_in(torch.from_numpy(np.asarray(keep, np.uint8)).cuda())
    for name, a in (("va", va), ("vb", vb), ("fa", c0.fa), ("fb", c0.fb)):
        g[name].copy_in(torch.from_numpy(a).cuda())
    a = dict(n_verts_a=va.shape[1], n_faces_a=len(c0.fa), n_verts_b=vb.shape[1], n_faces_b=len(c0.fb), B=B, subdiv=n)
    a.update(override or {})
    ptr = lambda k: None if (override or {}).get("null") == k else g[k].data_ptr
    rc = hip.lib().ihmr_sdf_volume(ptr("va"), ptr("fa"), a["n_verts_a"], a["n_faces_a"], ptr("vb"), ptr("fb"), a["n_verts_b"], a["n_faces_b"],
                                   a["B"], a["subdiv"], g["keep"].data_ptr if keep is not None else None, ptr("box"), ptr("status"),
                                   ptr("counts"), g["bits"].data_ptr if with_bits else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_sdf_volume B={B} subdiv={n}")
    out = dict(box=g["box"].view(torch.float32, (B, 4)).cpu().numpy(), status=g["status"].view(torch.int32, (B,)).cpu().numpy(),
               counts=g["counts"].view(torch.int32, (B, T)).cpu().numpy().view(np.uint32))
    if with_bits:
        out["bits"] = g["bits"].view(torch.int32, (B, T, 1024)).cpu().numpy().view(np.uint32)
    return rc, out


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a if k in b) and a.keys() & b.keys() >= {"box", "status", "counts"}


def _run(cases, n, keep=None):
    """The call with 0xFF-filled outputs; the same call with zero-filled outputs must give the same bytes (so every word was written),
    and so must the call without the bits buffer."""
    rc, out = _launch(cases, n, keep)
    assert rc == 0
    rc0, out0 = _launch(cases, n, keep, fill=0x00)
    rcn, outn = _launch(cases, n, keep, with_bits=False)
    assert rc0 == 0 and rcn == 0 and _same(out, out0) and "bits" in out0 and _same(out, outn) and "bits" not in outn
    return out


def _check(cases, n, out, keep=None):
    for b, c in enumerate(cases):
        what = f"{c.name} subdiv {n} row {b}"
        if keep is not None and not keep[b]:
            assert out["status"][b] == 0 and not out["box"][b].view(np.uint32).any() and not out["counts"][b].any() and not out["bits"][b].any(), what
            continue
        s = VR.statement(c, n)
        assert out["status"][b] == s["status"] == c.status, (what, out["status"][b])
        assert out["box"][b].tobytes() == s["box"].tobytes(), (what, out["box"][b], s["box"])
        assert np.array_equal(out["counts"][b], s["counts"]), (what, out["counts"][b], s["counts"])
        assert np.array_equal(out["bits"][b], s["bits"]), (what, int((out["bits"][b] != s["bits"]).sum()))


def _chunks(cases):
    """Batches of 5, 3 and 1 samples, in turn (ten cases: 5, 3, 1, 1)."""
    out, i, turn = [], 0, 0
    while i < len(cases):
        k = (5, 3, 1)[turn % 3]
        turn += 1
        if k <= len(cases) - i:
            out.append(cases[i:i + k])
            i += k
    return out


def _groups():
    g = {}
    for c in VR.case_table().values():
        g.setdefault(c.group, []).append(c)
    return g


GROUPS = ("hand", "hand_open", "fingers", "sphere162", "sphere642", "tetra", "sphere_vs_hand")


def test_every_case_at_subdiv_1_is_the_statement_bit_for_bit():
    groups = _groups()
    assert sorted(groups) == sorted(GROUPS)
    sizes = set()
    for name in GROUPS:
        for batch in _chunks(groups[name]):
            sizes.add(len(batch))
            _check(batch, 1, _run(batch, 1))
    assert sizes == {1, 3, 5}


@pytest.mark.parametrize("group", GROUPS)
def test_every_class_at_subdiv_2_is_the_statement_bit_for_bit(group):
    cases = _groups()[group]
    if group == "hand":          # a counted case of every hand class next to the samples that are not counted
        t = VR.case_table()
        cases = [t[k] for k in ("hand_default_0", "nan_vertex", "hand_deep_0", "far_vertex", "disjoint")]
    batch = _chunks(cases)[0]
    _check(batch, 2, _run(batch, 2))


@pytest.mark.parametrize("name", ["hand_default_0", "hand_deep_0", "far_vertex", "shifted_2m", "hand_open", "fingers_0", "sphere162", "sphere642",
                                  "tetra", "sphere_vs_hand", "disjoint", "touching", "nan_vertex", "tiny_cube"])
def test_every_class_at_subdiv_4_is_the_statement_bit_for_bit(name):
    batch = [VR.case_table()[name]]
    _check(batch, 4, _run(batch, 4))


def test_batch_independence_and_the_keep_mask():
    t = VR.case_table()
    cases = [t[k] for k in ("hand_default_0", "hand_deep_0", "disjoint", "far_vertex", "hand_default_1")]
    for n in (1, 2):
        base = _run(cases, n)
        perm = [3, 0, 4, 2, 1]
        got = _run([cases[p] for p in perm], n)
        for k in base:
            assert got[k].tobytes() == base[k][perm].tobytes(), (n, k)
        rep = _run([cases[1]] * 5, n)
        for k in base:
            assert all(rep[k][b].tobytes() == base[k][1].tobytes() for b in range(5)), (n, k)
        keep = np.array([1, 0, 1, 0, 1], np.uint8)
        masked = _run(cases, n, keep=keep)
        _check(cases, n, masked, keep=keep)
        for k in base:
            assert masked[k][keep > 0].tobytes() == base[k][keep > 0].tobytes(), (n, k)


def test_other_statuses_next_to_counted_samples():
    t = VR.case_table()
    hands = [t[k] for k in ("hand_default_0", "disjoint", "nan_vertex", "tiny_cube", "hand_deep_0")]
    out = _run(hands, 1)
    assert out["status"].tolist() == [0, 1, 2, 2, 0]
    balls = [t[k] for k in ("sphere162", "touching", "sphere162")]
    out2 = _run(balls, 2)
    assert out2["status"].tolist() == [0, 1, 0]
    for cases, n, o in ((hands, 1, out), (balls, 2, out2)):
        _check(cases, n, o)
        for b, c in enumerate(cases):
            if c.status != VR.COUNTED:
                assert not o["box"][b].view(np.uint32).any() and not o["counts"][b].any() and not o["bits"][b].any()
            else:
                assert o["counts"][b].sum() > 0


@pytest.mark.parametrize("override", [dict(subdiv=3), dict(subdiv=0), dict(n_verts_a=1025), dict(n_verts_b=1025), dict(n_faces_a=2049),
                                      dict(n_faces_b=2049), dict(B=0), dict(null="va"), dict(null="fb"), dict(null="box"),
                                      dict(null="status"), dict(null="counts")])
def test_refusals_launch_nothing(override):
    cases = [VR.case_table()["tetra"]]
    rc, out = _launch(cases, 1, override=override)
    assert rc != 0
    for k, v in out.items():
        assert (v.view(np.uint8) == 0xFF).all(), k          # nothing was written


# ------------------------------------------------------------------------------------------------------------------ the Python wrappers
def _hand_cases():
    return _groups()["hand"]


def test_penetration_volume_is_count_times_cell_volume():
    from ihmr_amd.assets import synthetic_mano
    from ihmr_amd.sdf import penetration_volume
    cases = _hand_cases()[:5]
    fr, fl = synthetic_mano(True)["faces"], synthetic_mano(False)["faces"]         # open: the wrapper closes them
    va = torch.from_numpy(np.stack([c.va for c in cases])).cuda()
    vb = torch.from_numpy(np.stack([c.vb for c in cases])).cuda()
    for n in (1, 2):
        vol, counts, box, status, bits = penetration_volume(va, vb, fr, fl, subdiv=n, return_bits=True)
        assert vol.dtype == torch.float64 and vol.shape == (5,) and counts.shape == (5, n ** 3) and bits.shape == (5, n ** 3, 1024)
        for b, c in enumerate(cases):
            s = VR.statement(c, n)
            assert np.array_equal(counts[b].cpu().numpy(), s["counts"].astype(np.int64)) and int(status[b]) == s["status"]
            assert np.array_equal(bits[b].cpu().numpy().view(np.uint32), s["bits"]) and box[b].cpu().numpy().tobytes() == s["box"].tobytes()
            assert float(vol[b]) == VR.volume_m3(c, n), (c.name, n, float(vol[b]), VR.volume_m3(c, n))
    assert len(penetration_volume(va, vb, fr, fl)) == 4
    # the uncapped table goes through as it is with close=False
    open_case = VR.case_table()["hand_open"]
    v1 = penetration_volume(va[:1], vb[:1], fr, fl, subdiv=1, close=False)
    assert np.array_equal(v1[1][0].cpu().numpy(), VR.statement(open_case, 1)["counts"].astype(np.int64))
    with pytest.raises(ValueError):
        penetration_volume(va, vb, fr, fl, subdiv=3)


def test_evaluator_volume_sums_over_two_batches_with_masks():
    from ihmr_amd.assets import synthetic_mano
    from ihmr_amd.evaluator import Evaluator
    cases = _hand_cases()
    assert len(cases) == 10
    mano = dict(right=types.SimpleNamespace(faces=synthetic_mano(True)["faces"]), left=types.SimpleNamespace(faces=synthetic_mano(False)["faces"]))
    ev = Evaluator(mano, volume_metric=True, volume_subdiv=1)
    keep = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1, 1], bool)
    inter = np.array([1, 0, 1, 1, 1, 1, 1, 1, 0, 1], bool)
    for lo, hi in ((0, 5), (5, 10)):
        va = torch.from_numpy(np.stack([c.va for c in cases[lo:hi]])).cuda()
        vb = torch.from_numpy(np.stack([c.vb for c in cases[lo:hi]])).cuda()
        ev.update_device_volume(va, vb, keep=torch.from_numpy(keep[lo:hi]), interacting=torch.from_numpy(inter[lo:hi]))
    use = keep & inter
    vols = np.array([VR.volume_m3(c, 1) * 1e6 for c in cases])
    stat = np.array([VR.statement(c, 1)["status"] for c in cases])
    want = np.array([vols[use].sum(), use.sum(), (use & (vols > 0)).sum(), (use & (stat == 2)).sum()], np.float64)
    got = ev.volume_sums()
    assert want[1] == 7 and want[2] >= 3 and want[3] >= 1
    assert np.array_equal(got[1:], want[1:]) and abs(got[0] - want[0]) <= 1e-12 * want[0], (got, want)
    m = Evaluator.volume_metrics_from_sums(got)
    assert abs(m["pen_volume"] - want[0] / 7) <= 1e-12 * want[0] and m["pen_rate"] == want[2] / 7
    # the metric leaves the other sums alone
    assert not ev.metric_sums().any() and not ev.pa_metric_sums().any() and ev.pred_results == []


def test_run_optimize_volume_metric_one_process_equals_two_ranks():
    from ihmr_amd import run_optimize
    args = ["--num_samples", "14", "--batchSize", "4", "--opt_epoch", "2", "--volume_metric"]
    one = run_optimize.main(args)
    assert one["pen_volume"] >= 0 and 0 <= one["pen_rate"] <= 1
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, IHMR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "ihmr_amd.run_optimize"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "pen_volume : " in r.stdout and "pen_rate : " in r.stdout
    two = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert two["world"] == 2
    assert two["pen_rate"] == one["pen_rate"]
    assert abs(two["pen_volume"] - one["pen_volume"]) <= 1e-12 * max(1.0, abs(one["pen_volume"])), (two["pen_volume"], one["pen_volume"])
    for k in ("mpjpe_3d", "collision_ave"):
        assert abs(two[k] - one[k]) <= 1e-12 * max(1.0, abs(one[k])), k
    # without the option the line carries neither key
    plain = run_optimize.main(args[:-1])
    assert "pen_volume" not in plain and "pen_rate" not in plain
    for k in ("mpjpe_3d", "inter_mpjpe_3d", "collision_ave", "collision_max"):
        assert plain[k] == one[k], k

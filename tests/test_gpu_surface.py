"""``ihmr_surface_distance`` / ``ihmr_surface_distance_bwd`` on the GPU against the float64 statement of tests/surface_ref.py, through the
C ABI in guarded buffers pre-filled with 0xFF and again with 0x00, in batches of 1, 3 and 5: ``|dist|`` and the weights within 1e-9 of
the statement, signs, inside counts and every contact count EXACT, the face condition, ``is_signed = 0``, the ``use`` mask, batch
independence bit for bit, the refusals; the backward against the statement's gradient and bit-identical on a second run; then
``sdf.surface_distance`` under ``torch.autograd``, ``Evaluator.update_device_surface`` and ``run_optimize --surface_metrics``.

Measured on the MI355X (the prints below): the worst ``||dist| - statement|``, weight and gradient deviations over the whole table are
recorded in DESIGN.md section 8, row (f)8."""
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
import surface_ref as SR  # noqa: E402
from guarded import Guarded, assert_guards  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = SR.TOL


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ the C ABI, guarded
def _inputs(cases, use=None):
    c0 = cases[0]
    assert all(c.shape == c0.shape and c.faces.tobytes() == c0.faces.tobytes() for c in cases)
    arrays = dict(points=np.stack([c.points for c in cases]), verts=np.stack([c.verts for c in cases]), faces=c0.faces)
    if use is not None:
        arrays["use"] = np.asarray(use, np.uint8)
    g = {k: Guarded(a.nbytes) for k, a in arrays.items()}
    for k, a in arrays.items():
        g[k].copy_in(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return g


def _launch(cases, signed=1, use=None, fill=0xFF, override=None):
    """One call of ``ihmr_surface_distance`` on a batch of cases of one shape and face table, every buffer guarded, the outputs
    pre-filled with ``fill``.  Returns (rc, dict of numpy outputs); the guards are checked."""
    from ihmr_amd import hip
    override = override or {}
    B = len(cases)
    P, V, F_total, F_dist = cases[0].shape
    g = _inputs(cases, use)
    g.update(dist=Guarded(B * P * 8, fill=fill), face=Guarded(B * P * 4, fill=fill), bary=Guarded(B * P * 3 * 8, fill=fill))
    ptr = lambda k: None if override.get("null") == k else g[k].data_ptr
    rc = hip.lib().ihmr_surface_distance(ptr("points"), override.get("P", P), ptr("verts"), override.get("V", V), ptr("faces"),
                                         override.get("F_dist", F_dist), override.get("F_total", F_total),
                                         g["use"].data_ptr if use is not None else None, override.get("B", B), signed, ptr("dist"),
                                         ptr("face"), ptr("bary"), hip.stream_ptr())
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_surface_distance B={B} P={P}")
    return rc, dict(dist=g["dist"].view(torch.float64, (B, P)).cpu().numpy(), face=g["face"].view(torch.int32, (B, P)).cpu().numpy(),
                    bary=g["bary"].view(torch.float64, (B, P, 3)).cpu().numpy())


def _bytes_equal(a, b):
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


def _run(cases, signed=1, use=None):
    """The call with 0xFF-filled outputs; the same call with zero-filled outputs must give the same bytes: every word was written."""
    rc, out = _launch(cases, signed, use)
    rc0, out0 = _launch(cases, signed, use, fill=0x00)
    assert rc == 0 and rc0 == 0 and _bytes_equal(out, out0)
    return out


def _row(out, b):
    return dict(dist=out["dist"][b], face=out["face"][b].astype(np.int64), bary=out["bary"][b])


def _groups():
    """The case table grouped by (shape, face table), each group cut into batches of 5, 3 and 1 in turn."""
    groups = {}
    for c in SR.cases().values():
        groups.setdefault((c.shape, c.faces.tobytes()), []).append(c)
    out = []
    for cases in groups.values():
        i, turn = 0, 0
        while i < len(cases):
            k = (5, 3, 1)[turn % 3]
            turn += 1
            if k <= len(cases) - i:
                out.append(cases[i:i + k])
                i += k
    return out


WORST = dict(dist=0.0, bary=0.0)


def test_every_case_is_the_statement():
    sizes = set()
    for batch in _groups():
        sizes.add(len(batch))
        out = _run(batch)
        for b, c in enumerate(batch):
            st, got = SR.statement(c.name), _row(out, b)
            d, w = SR.check_against_statement(c, st, got, TOL, TOL, c.name)
            WORST["dist"], WORST["bary"] = max(WORST["dist"], d), max(WORST["bary"], w)
            assert int((got["dist"] < 0).sum()) == int((st["dist"] < 0).sum()), c.name                # inside counts EXACT
            if c.hand:                                                                               # and every contact count
                for table in SR.TABLES.values():
                    thr = np.asarray(table)[:, None]
                    with np.errstate(all="ignore"):
                        assert ((got["dist"][None] / np.float64(c.scale) < thr) == (st["dist"][None] / np.float64(c.scale) < thr)).all(), c.name
    assert sizes == {1, 3, 5}
    print(f"[surface] worst ||dist| - statement| = {WORST['dist']:.3e} m, worst |weight - statement| = {WORST['bary']:.3e}")


def test_known_answers_are_exact_in_any_batch():
    t = SR.cases()
    for name in ("cube", "cube_bad_faces", "nothing_usable"):
        c = t[name]
        out = _run([c] * 3)
        for b in range(3):
            for i, (q, dist, face, bary) in enumerate(c.known):
                assert _same(out["dist"][b, i], dist) and out["face"][b, i] == face and out["bary"][b, i].tolist() == list(bary), (name, b, i)


def test_unsigned_distance_skips_the_sign_only():
    t = SR.cases()
    for batch in ([t["deep_0_r_on_l"], t["deep_1_r_on_l"], t["apart_1m"]], [t["cube_bad_faces"]], [t["sphere_P257"]]):
        signed, plain = _run(batch), _run(batch, signed=0)
        assert _same(plain["dist"], np.abs(signed["dist"])) and (signed["dist"] < 0).any()
        assert plain["face"].tobytes() == signed["face"].tobytes() and plain["bary"].tobytes() == signed["bary"].tobytes()
        assert _bytes_equal(_run(batch, signed=7), signed)                                         # any non-zero value asks for the sign


def test_batch_independence_and_the_use_mask():
    t = SR.cases()
    cases = [t[k] for k in ("deep_0_r_on_l", "default_1_r_on_l", "shifted_2m", "apart_1m", "deep_2_r_on_l")]
    base = _run(cases)
    perm = [3, 0, 4, 2, 1]
    got = _run([cases[p] for p in perm])
    for k in base:
        assert got[k].tobytes() == base[k][perm].tobytes(), k
    rep = _run([cases[1]] * 5)
    single = _run([cases[1]])
    for k in base:
        assert all(rep[k][b].tobytes() == base[k][1].tobytes() for b in range(5)) and single[k][0].tobytes() == base[k][1].tobytes(), k
    use = np.array([1, 0, 1, 0, 1], np.uint8)
    masked = _run(cases, use=use)
    for k in base:
        assert masked[k][use > 0].tobytes() == base[k][use > 0].tobytes(), k
    assert not masked["dist"][use == 0].view(np.uint64).any() and not masked["bary"][use == 0].view(np.uint64).any()
    assert (masked["face"][use == 0] == -1).all()
    assert _bytes_equal(_run(cases, use=np.array([1, 2, 255, 1, 7], np.uint8)), base)              # any non-zero byte is "use"
    # more chunks than one, the last partial, in a batch: P = 1025 is five chunks of 256
    big = [t["sphere_P1025"]] * 3
    out = _run(big)
    assert out["dist"][0].tobytes() == out["dist"][1].tobytes() == out["dist"][2].tobytes()


@pytest.mark.parametrize("override", [dict(B=0), dict(B=-1), dict(P=0), dict(V=0), dict(V=1025), dict(F_dist=0), dict(F_dist=13),
                                      dict(F_total=2049, F_dist=12), dict(F_total=11), dict(null="points"), dict(null="verts"),
                                      dict(null="faces"), dict(null="dist"), dict(null="face"), dict(null="bary")])
def test_refusals_write_nothing(override):
    rc, out = _launch([SR.cases()["cube"]], override=override)
    assert rc != 0
    for k, v in out.items():
        assert (v.view(np.uint8) == 0xFF).all(), k


# ------------------------------------------------------------------------------------------------------------------ backward
def _launch_bwd(cases, fwd, g_dist, use=None, fill=0xFF, override=None, outputs=("d_points", "d_verts")):
    from ihmr_amd import hip
    override = override or {}
    B = len(cases)
    P, V, F_total, F_dist = cases[0].shape
    g = _inputs(cases, use)
    for k, a in dict(dist=fwd["dist"], face=fwd["face"].astype(np.int32), bary=fwd["bary"], g_dist=np.asarray(g_dist, np.float64)).items():
        g[k] = Guarded(a.nbytes)
        g[k].copy_in(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    g.update(d_points=Guarded(B * P * 3 * 4, fill=fill), d_verts=Guarded(B * V * 3 * 4, fill=fill))
    ptr = lambda k: None if override.get("null") == k else g[k].data_ptr
    rc = hip.lib().ihmr_surface_distance_bwd(ptr("points"), override.get("P", P), ptr("verts"), override.get("V", V), ptr("faces"),
                                             override.get("F_dist", F_dist), override.get("F_total", F_total),
                                             g["use"].data_ptr if use is not None else None, override.get("B", B), ptr("dist"), ptr("face"),
                                             ptr("bary"), ptr("g_dist"), ptr("d_points") if "d_points" in outputs else None,
                                             ptr("d_verts") if "d_verts" in outputs else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert_guards(g, f"ihmr_surface_distance_bwd B={B} P={P}")
    return rc, dict(d_points=g["d_points"].view(torch.float32, (B, P, 3)).cpu().numpy(), d_verts=g["d_verts"].view(torch.float32, (B, V, 3)).cpu().numpy())


BWD_BATCHES = (("deep_0_r_on_l", "deep_1_r_on_l", "default_0_r_on_l", "shifted_2m", "apart_1m"), ("fingers_0_l_on_r",), ("cube_bad_faces",) * 3,
               ("tetrahedron",), ("sphere_P257",), ("sphere_P1025",))


@pytest.mark.parametrize("names", BWD_BATCHES, ids=lambda n: f"{n[0]}x{len(n)}")
def test_backward_is_the_statements_gradient_and_the_same_bits_twice(names):
    """The bar (the issue's): 3 x the distance of a float32 evaluation of the same formula from the float64 statement, plus one float32
    ulp of the largest term.  Measured on the MI355X: see DESIGN.md section 8, row (f)8."""
    cases = [SR.cases()[n] for n in names]
    B, P = len(cases), cases[0].shape[0]
    g = np.random.RandomState(len(names) * 1000 + P).uniform(0.5, 1.5, (B, P))
    fwd = _run(cases)
    rc, out = _launch_bwd(cases, fwd, g)
    rc0, out0 = _launch_bwd(cases, fwd, g, fill=0x00)
    assert rc == 0 and rc0 == 0 and _bytes_equal(out, out0)                                         # every word written, the same bits twice
    only_p = _launch_bwd(cases, fwd, g, outputs=("d_points",))[1]
    only_v = _launch_bwd(cases, fwd, g, outputs=("d_verts",))[1]
    assert only_p["d_points"].tobytes() == out["d_points"].tobytes() and (only_p["d_verts"].view(np.uint8) == 0xFF).all()
    assert only_v["d_verts"].tobytes() == out["d_verts"].tobytes() and (only_v["d_points"].view(np.uint8) == 0xFF).all()
    for b, c in enumerate(cases):
        st = SR.statement(c.name)
        want = SR.gradient(c.points, c.verts, c.faces, st, g[b])
        f32 = SR.gradient(c.points, c.verts, c.faces, st, g[b], np.float32)
        ok = st["face"] >= 0
        term = float(np.abs(st["bary"][ok] * g[b][ok, None]).max()) if ok.any() else 0.0
        for k, name, largest in ((0, "d_points", float(g[b].max())), (1, "d_verts", term)):
            yard = float(np.abs(f32[k].astype(np.float64) - want[k]).max())
            bar = 3.0 * yard + float(np.spacing(np.float32(largest)))
            err = float(np.abs(out[name][b].astype(np.float64) - want[k]).max())
            print(f"[surface bwd] {c.name} {name}: |device - statement| {err:.3e}, float32 formula {yard:.3e}, bar {bar:.3e}")
            assert np.isfinite(out[name][b]).all() and err <= bar, (c.name, name, err, bar)
        nan = np.isnan(st["dist"])
        assert not out["d_points"][b][nan].any()
    use = np.zeros(B, np.uint8)
    use[0] = 1
    rc, masked = _launch_bwd(cases, fwd, g, use=use)
    assert rc == 0 and masked["d_points"][0].tobytes() == out["d_points"][0].tobytes() and masked["d_verts"][0].tobytes() == out["d_verts"][0].tobytes()
    assert not masked["d_points"][1:].any() and not masked["d_verts"][1:].any()


def test_backward_reads_a_foreign_face_buffer_safely():
    """The forward's words are inputs of the backward: ids outside the table add nothing and nothing is read through them."""
    c = SR.cases()["cube_bad_faces"]
    fwd = _run([c])
    fwd["face"][0, :4] = [-5, 15, 2 ** 31 - 1, 16]                       # 15 and 16 lie in the cap part or behind the table
    fwd["face"][0, 4] = 1                                              # a surface face that names vertex 10 of 10
    rc, out = _launch_bwd([c], fwd, np.ones((1, c.shape[0])))
    assert rc == 0 and not out["d_points"][0, :5].any() and np.isfinite(out["d_verts"]).all() and out["d_points"][0, 5:8].any()


@pytest.mark.parametrize("override", [dict(B=0), dict(P=0), dict(V=1025), dict(F_dist=0), dict(F_dist=18), dict(F_total=2049), dict(null="points"),
                                      dict(null="verts"), dict(null="faces"), dict(null="dist"), dict(null="face"), dict(null="bary"),
                                      dict(null="g_dist")])
def test_backward_refusals_write_nothing(override):
    c = SR.cases()["cube_bad_faces"]
    st = SR.statement(c.name)
    fwd = dict(dist=st["dist"][None], face=st["face"][None], bary=st["bary"][None])
    rc, out = _launch_bwd([c], fwd, np.ones((1, c.shape[0])), override=override)
    assert rc != 0
    for k, v in out.items():
        assert (v.view(np.uint8) == 0xFF).all(), k


# ------------------------------------------------------------------------------------------------------------------ the public function
def _hand_models():
    from ihmr_amd.assets import synthetic_mano
    return dict(right=types.SimpleNamespace(faces=synthetic_mano(True)["faces"]), left=types.SimpleNamespace(faces=synthetic_mano(False)["faces"]))


def test_autograd_through_surface_distance_gives_the_entry_points_tensors():
    from ihmr_amd import sdf
    names = ("deep_0_r_on_l", "default_1_r_on_l", "apart_1m")
    cases = [SR.cases()[n] for n in names]
    B, P = len(cases), 778
    g = np.random.RandomState(77).uniform(0.5, 1.5, (B, P))
    fwd = _run(cases)
    want = _launch_bwd(cases, fwd, g)[1]
    points = torch.from_numpy(np.stack([c.points for c in cases])).cuda().requires_grad_(True)
    verts = torch.from_numpy(np.stack([c.verts for c in cases])).cuda().requires_grad_(True)
    dist, face, bary = sdf.surface_distance(points, verts, _hand_models()["left"].faces)          # close=True: the table of the cases
    assert dist.dtype == torch.float64 and face.dtype == torch.int32 and not face.requires_grad and not bary.requires_grad and dist.requires_grad
    assert dist.detach().cpu().numpy().tobytes() == fwd["dist"].tobytes() and face.cpu().numpy().tobytes() == fwd["face"].tobytes()
    assert bary.cpu().numpy().tobytes() == fwd["bary"].tobytes()
    (dist * torch.from_numpy(g).cuda()).sum().backward()
    assert points.grad.dtype == torch.float32 and points.grad.cpu().numpy().tobytes() == want["d_points"].tobytes()
    assert verts.grad.cpu().numpy().tobytes() == want["d_verts"].tobytes()
    # an attraction term reaches a hand far outside the other hand's box, where the grid loss has no gradient
    assert points.grad[2].abs().sum() > 100 and verts.grad[2].abs().sum() > 1
    # only the points: the vertex gradient is not formed; unsigned, open table, use mask
    p2 = points.detach().clone().requires_grad_(True)
    d2 = sdf.surface_distance(p2, verts.detach(), _hand_models()["left"].faces, signed=False, close=False,
                              use=torch.tensor([True, False, True]))[0]
    assert d2[1].abs().sum() == 0 and (d2[0] >= 0).all() and torch.equal(d2[0], dist[0].detach().abs())
    d2.sum().backward()
    assert p2.grad[1].abs().sum() == 0 and p2.grad[0].abs().sum() > 0
    with pytest.raises(ValueError):
        sdf.surface_distance(points[0], verts, _hand_models()["left"].faces)


@pytest.mark.parametrize("K", [2, 8])
def test_evaluator_device_path_over_two_masked_batches_is_the_statement(K):
    from ihmr_amd.evaluator import Evaluator
    table = SR.TABLES[K]
    e = SR.evaluator_batch()
    B = len(e["keep"])
    ev = Evaluator(_hand_models(), surface_metrics=True, surface_thresholds=table)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for lo, hi in ((0, 2), (2, B)):
        sl = slice(lo, hi)
        ev.update_device_surface(up(e["pred_right"][sl]), up(e["pred_left"][sl]), up(e["gt_right"][sl]), up(e["gt_left"][sl]),
                                 up(e["weight"][sl]), scale=up(e["scale"][sl]), keep=torch.from_numpy(e["keep"][sl]),
                                 interacting=torch.from_numpy(e["inter"][sl]))
    got, want = ev.surface_sums(), SR.expected_surface_sums(table)
    print(f"[evaluator] K={K} device {got[:5]!r} statement {want[:5]!r}")
    assert _same(got[2:], want[2:]), (got, want)                                                  # integer entries element for element
    assert want[3] >= 3 and 0 < want[4] < want[3] and want[5:].all()
    for k in (0, 1):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])
    m = ev.metrics_from_packed(ev.packed_sums())
    assert 1.0 < m["pen_depth_max"] < 60 and 0 < m["pen_depth_ave"] < m["pen_depth_max"] and len(m["surface_contact_f1"]) == K
    assert not ev.metric_sums().any() and ev.pred_results == []                                   # the family leaves the other sums alone
    # without GT meshes: the depth part alone
    plain = Evaluator(_hand_models(), surface_metrics=True, surface_thresholds=table)
    plain.update_device_surface(up(e["pred_right"]), up(e["pred_left"]), scale=up(e["scale"]), keep=torch.from_numpy(e["keep"]),
                                interacting=torch.from_numpy(e["inter"]))
    s = plain.surface_sums()
    assert _same(s[2:4], want[2:4]) and not s[4:].any() and abs(s[0] - want[0]) <= 1e-9 * want[0]
    ev.clear()
    assert not ev.surface_sums().any()
    with pytest.raises(RuntimeError):
        Evaluator(_hand_models()).update_device_surface(up(e["pred_right"]), up(e["pred_left"]))
    with pytest.raises(ValueError):
        plain.update_device_surface(up(e["pred_right"]), up(e["pred_left"]), up(e["gt_right"]), up(e["gt_left"]))


def test_run_optimize_surface_metrics_one_process_and_two_ranks_agree():
    from ihmr_amd import run_optimize
    args = ["--num_samples", "14", "--batchSize", "4", "--opt_epoch", "2", "--surface_metrics"]
    one = run_optimize.main(args)
    plain = run_optimize.main(args[:-1])
    new = ["pen_depth_max", "pen_depth_ave", "pen_vertex_rate"]
    assert sorted(one) == sorted(list(plain) + new) and not any(k in plain for k in new)         # no GT meshes: no contact part
    for k in plain:
        assert one[k] == plain[k], k
    print(f"[surface] run_optimize {[(k, one[k]) for k in new]} collision_max {one['collision_max']!r} collision_ave {one['collision_ave']!r}")
    assert one["pen_depth_max"] >= one["pen_depth_ave"] >= 0 and 0 <= one["pen_vertex_rate"] < 1
    with pytest.raises(SystemExit):
        run_optimize.main(args + ["--host_eval"])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, IHMR_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "ihmr_amd.run_optimize"] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "pen_depth_max : " in r.stdout
    two = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert two["world"] == 2 and not any(k.startswith("surface_contact_") for k in two)
    for k in new + ["mpjpe_3d", "collision_ave"]:
        assert abs(two[k] - one[k]) <= 1e-12 * max(1.0, abs(one[k])), (k, two[k], one[k])

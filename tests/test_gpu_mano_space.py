"""The MANO layer's pose space and output stage on the GPU (include/ihmr_mano_ext.h; the statement is tests/mano_space_ref.py): the four
entry points through the C ABI in guarded buffers pre-filled with 0xFF and again with 0x00, at N = 1 (one hand), 9 (a ragged first
tile) and 257 (a ragged last tile, and one past 256, where the skin launch changes form), K = 1, 6, 45; then the layer through
``mano.create``; then today's call, which must launch none of the four and give the bits of ``_LbsFunction.apply``.

The bounds are the derived ones of tests/test_mano_space_cpu.py (gamma_K for the PCA chains, bit equality for the translation and the
tips, one float32 ulp for d_transl); the layer is held to the rule of tests/mano_cases.py (``within``: 1.5 x the float32 oracle's own
distance from float64, or the floor of the older LBS tests)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mano_cases as MC  # noqa: E402
import mano_space_ref as SP  # noqa: E402
from guarded import Guarded, assert_guards  # noqa: E402

pytestmark = pytest.mark.gpu
NS, KS = (1, 9, 257), (1, 6, 45)
NEW = ("ihmr_mano_pca_fwd", "ihmr_mano_pca_bwd", "ihmr_mano_post_fwd", "ihmr_mano_post_bwd")
TIPS = np.array([744, 320, 443, 554, 671], np.int32)


def _comps(K, is_rhand=True):
    from ihmr_amd.assets import get_hand_components
    return np.ascontiguousarray(get_hand_components("", is_rhand)[:K])


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------------ the C ABI, guarded
def _call(name, inputs, outputs, args, fill=0xFF, null=None, alias=None):
    """One call of entry point `name`.  `inputs`: name -> array or None (a NULL pointer); `outputs`: name -> (dtype, shape); `args`: the
    argument list with buffer names where pointers go; `alias`: {output: input} for an in-place call.  Every buffer is guarded, the
    outputs pre-filled with `fill`.  Returns (rc, {output: array}); the guards are checked."""
    from ihmr_amd import hip
    g = {}
    for k, a in inputs.items():
        if a is not None:
            a = np.ascontiguousarray(a)
            g[k] = Guarded(a.nbytes)
            g[k].copy_in(torch.from_numpy(a).cuda())
    for k, (dtype, shape) in outputs.items():
        if not (alias and k in alias):
            g[k] = Guarded(int(np.prod(shape)) * np.dtype(dtype).itemsize, fill=fill)
    where = lambda k: g[(alias or {}).get(k, k)]
    ptr = lambda k: None if (k == null or (k in inputs and inputs[k] is None)) else where(k).data_ptr
    rc = getattr(hip.lib(), name)(*[ptr(a) if isinstance(a, str) else a for a in args], hip.stream_ptr())
    torch.cuda.synchronize()
    assert_guards(g, name)
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}
    return rc, {k: where(k).view(tdt[np.dtype(dt)], tuple(shape)).cpu().numpy() for k, (dt, shape) in outputs.items()}


def _twice(name, inputs, outputs, args, **kw):
    """The call with 0xFF-filled outputs; the same call with zero-filled outputs must give the same bytes: every word was written."""
    rc, out = _call(name, inputs, outputs, args, fill=0xFF, **kw)
    rc0, out0 = _call(name, inputs, outputs, args, fill=0x00, **kw)
    assert rc == 0 and rc0 == 0 and all(_bits(out[k], out0[k]) for k in out), name
    return out


def _pca_fwd(coeffs, comps, **kw):
    N, K = coeffs.shape
    return _twice("ihmr_mano_pca_fwd", dict(coeffs=coeffs, comps=comps), dict(pose45=(np.float32, (N, 45))), ["coeffs", "comps", N, K, "pose45"], **kw)["pose45"]


def _pca_bwd(d_pose45, comps, **kw):
    N, K = d_pose45.shape[0], comps.shape[0]
    return _twice("ihmr_mano_pca_bwd", dict(d_pose45=d_pose45, comps=comps), dict(d_coeffs=(np.float32, (N, K))),
                  ["d_pose45", "comps", N, K, "d_coeffs"], **kw)["d_coeffs"]


def _post_fwd(verts, joints16, transl, tips, inplace=False):
    N, J = verts.shape[0], 16 if tips is None else 21
    return _twice("ihmr_mano_post_fwd", dict(verts_in=verts, joints16_in=joints16, transl=transl, tip_ids=tips),
                  dict(verts_out=(np.float32, (N, 778, 3)), joints_out=(np.float32, (N, J, 3))),
                  ["verts_in", "joints16_in", "transl", "tip_ids", N, "verts_out", "joints_out"], alias=dict(verts_out="verts_in") if inplace else None)


def _post_bwd(d_verts_out, d_joints_out, tips, want_transl=True, twice=_twice):
    N = d_verts_out.shape[0]
    outputs = dict(d_verts_in=(np.float32, (N, 778, 3)), d_joints16=(np.float32, (N, 16, 3)), d_transl=(np.float32, (N, 3)))
    return twice("ihmr_mano_post_bwd", dict(d_verts_out=d_verts_out, d_joints_out=d_joints_out, tip_ids=tips), outputs,
                 ["d_verts_out", "d_joints_out", "tip_ids", N, "d_verts_in", "d_joints16", "d_transl"], null=None if want_transl else "d_transl")


def _normal(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ PCA entry points alone
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_pca_forward_and_backward_meet_the_derived_bound(N, K):
    comps = _comps(K)
    coeffs, g = 0.6 * _normal((N, K), 10 * N + K), _normal((N, 45), 20 * N + K)
    pose45, d_coeffs = _pca_fwd(coeffs, comps), _pca_bwd(g, comps)
    exact, mag = SP.pca_exact(coeffs, comps)
    err = np.abs(pose45 - exact)
    print(f"[pca] N={N} K={K}: worst |fwd - exact| / (gamma_K sum|c C|) = {float((err / np.maximum(SP.gamma(K) * mag, 1e-300)).max()):.3f}")
    assert (err <= SP.gamma(K) * mag).all()
    b_exact, b_mag = SP.pca_bwd_exact(g, comps)
    assert (np.abs(d_coeffs - b_exact) <= SP.gamma(45) * b_mag).all()
    zero = _pca_fwd(np.zeros((N, K), np.float32), comps)                                   # the zero class: exactly +0
    assert not zero.view(np.uint32).any()


@pytest.mark.parametrize("K", KS)
def test_pca_dyadic_known_answer_is_exact(K):
    rng = np.random.RandomState(K)
    dy = lambda s: (rng.randint(-8, 9, size=s) * 0.125).astype(np.float32)
    coeffs, comps, g = dy((9, K)), dy((K, 45)), dy((9, 45))
    assert _bits(_pca_fwd(coeffs, comps), (coeffs.astype(np.float64) @ comps.astype(np.float64)).astype(np.float32) + np.float32(0))
    assert _bits(_pca_bwd(g, comps), (g.astype(np.float64) @ comps.astype(np.float64).T).astype(np.float32) + np.float32(0))


def test_pca_permuted_and_repeated_hands_give_the_same_bits():
    K, N = 6, 257
    comps = _comps(K)
    coeffs, g = 0.6 * _normal((N, K), 3), _normal((N, 45), 4)
    base_f, base_b = _pca_fwd(coeffs, comps), _pca_bwd(g, comps)
    perm = np.random.RandomState(5).permutation(N)
    assert _bits(_pca_fwd(coeffs[perm], comps), base_f[perm]) and _bits(_pca_bwd(g[perm], comps), base_b[perm])
    rep_f, rep_b = _pca_fwd(np.repeat(coeffs[7:8], 33, 0), comps), _pca_bwd(np.repeat(g[7:8], 33, 0), comps)
    assert all(_bits(rep_f[i], base_f[7]) and _bits(rep_b[i], base_b[7]) for i in range(33))
    assert _bits(_pca_fwd(coeffs[200:201], comps)[0], base_f[200]) and _bits(_pca_bwd(g[200:201], comps)[0], base_b[200])


@pytest.mark.parametrize("override", [dict(K=0), dict(K=46), dict(K=-1), dict(N=0), dict(N=-3), dict(null="rows"), dict(null="comps"), dict(null="out")])
def test_pca_refusals_write_nothing(override):
    comps = _comps(6)
    for name, rows, width in (("ihmr_mano_pca_fwd", _normal((9, 6), 1), 45), ("ihmr_mano_pca_bwd", _normal((9, 45), 2), 6)):
        rc, out = _call(name, dict(rows=rows, comps=comps), dict(out=(np.float32, (9, width))),
                        ["rows", "comps", override.get("N", 9), override.get("K", 6), "out"], null=override.get("null"))
        assert rc == -1 and (out["out"].view(np.uint8) == 0xFF).all(), (name, override)


# ------------------------------------------------------------------------------------------------------------------ post entry points alone
@pytest.mark.parametrize("N", NS)
def test_post_forward_passes_through_translates_and_gathers(N):
    verts, joints, transl = _normal((N, 778, 3), N), _normal((N, 16, 3), N + 1), _normal((N, 3), N + 2)
    verts[0, 5, 1] = -0.0                                                              # passes through as -0.0: nothing is added
    plain = _post_fwd(verts, joints, None, None)
    assert _bits(plain["verts_out"], verts) and _bits(plain["joints_out"], joints)
    moved = _post_fwd(verts, joints, transl, TIPS)
    want_v = verts + transl[:, None]
    assert _bits(moved["verts_out"], want_v) and _bits(moved["joints_out"][:, :16], joints + transl[:, None])
    assert _bits(moved["joints_out"][:, 16:], want_v[:, TIPS])
    tips_only = _post_fwd(verts, joints, None, TIPS)
    assert _bits(tips_only["verts_out"], verts) and _bits(tips_only["joints_out"], np.concatenate([joints, verts[:, TIPS]], 1))
    transl_only = _post_fwd(verts, joints, transl, None)
    assert _bits(transl_only["verts_out"], want_v) and transl_only["joints_out"].shape == (N, 16, 3)
    for t, tips in ((transl, TIPS), (None, TIPS), (transl, None)):
        inplace = _post_fwd(verts, joints, t, tips, inplace=True)
        ref = _post_fwd(verts, joints, t, tips)
        assert _bits(inplace["verts_out"], ref["verts_out"]) and _bits(inplace["joints_out"], ref["joints_out"])
    odd = np.array([777, 0, -1, 778, 0], np.int32)                                      # the ends, a repeat, two ids outside the hand
    got = _post_fwd(verts, joints, transl, odd)["joints_out"][:, 16:]
    assert _bits(got[:, [0, 1, 4]], want_v[:, [777, 0, 0]]) and not got[:, [2, 3]].view(np.uint32).any()


@pytest.mark.parametrize("N", NS)
def test_post_backward_is_exact_and_the_same_bits_twice(N):
    gv, gj = _normal((N, 778, 3), 7 * N), _normal((N, 21, 3), 7 * N + 1)
    out = _post_bwd(gv, gj, TIPS)
    want = gv.copy()
    want[:, TIPS] += gj[:, 16:]
    assert _bits(out["d_verts_in"], want) and _bits(out["d_joints16"], gj[:, :16])
    total = SP.transl_sum(gv, gj)
    assert (np.abs(out["d_transl"] - total) <= SP.one_ulp_of(total)).all()
    again = _post_bwd(gv, gj, TIPS)
    assert all(_bits(out[k], again[k]) for k in out)
    # without tips: 16 rows, the vertices pass through; without d_transl: it is not written
    no_tips = _post_bwd(gv, gj[:, :16], None)
    assert _bits(no_tips["d_verts_in"], gv) and _bits(no_tips["d_joints16"], gj[:, :16])
    total16 = SP.transl_sum(gv, gj[:, :16])
    assert (np.abs(no_tips["d_transl"] - total16) <= SP.one_ulp_of(total16)).all()
    rc, skipped = _call("ihmr_mano_post_bwd", dict(d_verts_out=gv, d_joints_out=gj, tip_ids=TIPS),
                        dict(d_verts_in=(np.float32, (N, 778, 3)), d_joints16=(np.float32, (N, 16, 3)), d_transl=(np.float32, (N, 3))),
                        ["d_verts_out", "d_joints_out", "tip_ids", N, "d_verts_in", "d_joints16", "d_transl"], null="d_transl")
    assert rc == 0 and _bits(skipped["d_verts_in"], want) and (skipped["d_transl"].view(np.uint8) == 0xFF).all()
    if N == 9:                                                                          # a hand's sums do not depend on its place
        perm = np.random.RandomState(1).permutation(N)
        moved = _post_bwd(gv[perm], gj[perm], TIPS)
        assert all(_bits(moved[k], out[k][perm]) for k in out)


@pytest.mark.parametrize("override", [dict(N=0), dict(N=-1), dict(null="verts_in"), dict(null="joints16_in"), dict(null="verts_out"), dict(null="joints_out")])
def test_post_forward_refusals_write_nothing(override):
    rc, out = _call("ihmr_mano_post_fwd", dict(verts_in=_normal((2, 778, 3), 1), joints16_in=_normal((2, 16, 3), 2), transl=None, tip_ids=TIPS),
                    dict(verts_out=(np.float32, (2, 778, 3)), joints_out=(np.float32, (2, 21, 3))),
                    ["verts_in", "joints16_in", "transl", "tip_ids", override.get("N", 2), "verts_out", "joints_out"], null=override.get("null"))
    assert rc == -1 and all((v.view(np.uint8) == 0xFF).all() for v in out.values())


@pytest.mark.parametrize("override", [dict(N=0), dict(null="d_verts_out"), dict(null="d_joints_out"), dict(null="d_verts_in"), dict(null="d_joints16")])
def test_post_backward_refusals_write_nothing(override):
    rc, out = _call("ihmr_mano_post_bwd", dict(d_verts_out=_normal((2, 778, 3), 1), d_joints_out=_normal((2, 21, 3), 2), tip_ids=TIPS),
                    dict(d_verts_in=(np.float32, (2, 778, 3)), d_joints16=(np.float32, (2, 16, 3)), d_transl=(np.float32, (2, 3))),
                    ["d_verts_out", "d_joints_out", "tip_ids", override.get("N", 2), "d_verts_in", "d_joints16", "d_transl"], null=override.get("null"))
    assert rc == -1 and all((v.view(np.uint8) == 0xFF).all() for v in out.values())


# ------------------------------------------------------------------------------------------------------------------ the layer
def _up(a, grad=False):
    return None if a is None else torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


@functools.lru_cache(maxsize=None)
def _layer(K=None, flat=False, is_rhand=True):
    from ihmr_amd import mano
    return mano.create("", "mano", use_pca=K is not None, num_pca_comps=K or 6, flat_hand_mean=flat, is_rhand=is_rhand).cuda()


@functools.lru_cache(maxsize=None)
def _truth(name, N, K, flat):
    """(case, float64 statement, float32 statement) on the right hand: computed once, read-only."""
    from ihmr_amd.assets import synthetic_mano
    arrays = synthetic_mano(True)
    c = SP.case(name, N, K, 900 + N, arrays["hands_mean"])
    comps = None if K is None else _comps(K)
    f64, o32 = SP.reference(arrays, c, torch.float64, comps, flat), SP.reference(arrays, c, torch.float32, comps, flat)
    for d in (c, f64, o32):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c, f64, o32


def _run_layer(layer, c):
    leaves = {k: _up(c[k], True) for k in ("orient", "hand_pose", "betas", "transl")}
    out = layer(global_orient=leaves["orient"], hand_pose=leaves["hand_pose"], betas=leaves["betas"], transl=leaves["transl"],
                return_tips=c["gj"].shape[1] == 21, return_full_pose=True)
    ((out.vertices * _up(c["gv"])).sum() + (out.joints * _up(c["gj"])).sum()).backward()
    torch.cuda.synchronize()
    f = lambda t: t.detach().cpu().numpy()
    return dict(verts=f(out.vertices), joints=f(out.joints), full_pose=f(out.full_pose), d_orient=f(leaves["orient"].grad),
                d_hand_pose=f(leaves["hand_pose"].grad), d_betas=f(leaves["betas"].grad), d_transl=f(leaves["transl"].grad))


# mild: drawn coefficients on the mean hand; zero: zero coefficients on the flat hand mean -- the full pose is exactly zero, the angle
# ||0 + 1e-8|| (the `zero` class of tests/mano_cases.py reached through the new arguments)
@pytest.mark.parametrize("name,N,K", [("mild", N, K) for N in NS for K in KS] + [("zero", N, 6) for N in NS])
def test_the_pca_layer_is_the_statement_forward_and_in_all_four_gradients(name, N, K):
    flat = name == "zero"
    c, f64, o32 = _truth(name, N, K, flat)
    got = _run_layer(_layer(K, flat), c)
    assert got["d_hand_pose"].shape == (N, K) and got["joints"].shape == (N, 21, 3) and got["d_transl"].shape == (N, 3)
    for k in SP.OUTPUTS:
        MC.within(got[k], f64[k], o32[k], SP.floor_of(k, f64[k]), f"{name} N={N} K={K} {k}")
    # the full pose: the bits of the float32 additions on the entry point's pose45
    pose45 = _pca_fwd(np.array(c["hand_pose"]), _comps(K))
    mean = np.zeros(45, np.float32) if flat else MC._f32(_layer(K, flat).hand_mean.cpu().numpy())
    assert _bits(got["full_pose"], np.concatenate([c["orient"], pose45 + mean[None]], 1))
    if flat:
        assert not got["full_pose"].any()


def test_flat_hand_mean_is_the_asset_with_a_zeroed_mean():
    from ihmr_amd import mano
    from ihmr_amd.assets import synthetic_mano
    for is_rhand in (True, False):
        arrays = synthetic_mano(is_rhand)
        by_hand = mano.MANO(dict(arrays, hands_mean=np.zeros_like(arrays["hands_mean"])), is_rhand=is_rhand).cuda()
        flat = _layer(None, True, is_rhand)
        assert not flat.hand_mean.any() and flat.flat_hand_mean and _layer(None, False, is_rhand).hand_mean.any()
        o, p, b = MC.inputs("mild", 9, 77, arrays["hands_mean"])
        outs = []
        for layer in (by_hand, flat, _layer(None, False, is_rhand)):
            leaves = [_up(a, True) for a in (o, p, b)]
            out = layer(global_orient=leaves[0], hand_pose=leaves[1], betas=leaves[2])
            (out.vertices.sum() + out.joints.sum()).backward()
            outs.append([out.vertices.detach().cpu().numpy(), out.joints.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in leaves])
        assert all(_bits(a, b_) for a, b_ in zip(outs[0], outs[1]))
        assert not _bits(outs[0][0], outs[2][0])


@pytest.mark.parametrize("K", [None, 6])
def test_arguments_left_out_are_zeros(K):
    from ihmr_amd import mano
    layer = mano.create("", "mano", use_pca=K is not None, num_pca_comps=K or 6, batch_size=3).cuda()
    width = K or 45
    z = lambda w, n=3: torch.zeros(n, w, device="cuda")
    want = layer(global_orient=z(3), hand_pose=z(width), betas=z(10))
    got = layer()
    assert type(got) is mano.ManoOutput and got.vertices.shape == (3, 778, 3) and got.joints.shape == (3, 16, 3)
    assert torch.equal(got.vertices, want.vertices) and torch.equal(got.joints, want.joints)
    assert got.betas.shape == (3, 10) and got.hand_pose.shape == (3, width) and not got.hand_pose.any()
    # the row count comes from the arguments that are there
    b = torch.from_numpy(MC._f32(np.random.RandomState(2).standard_normal((5, 10)))).cuda()
    some = layer(betas=b)
    full = layer(global_orient=z(3, 5), hand_pose=z(width, 5), betas=b)
    assert some.vertices.shape == (5, 778, 3) and torch.equal(some.vertices, full.vertices) and torch.equal(some.joints, full.joints)
    only_t = layer(transl=torch.ones(2, 3, device="cuda"))
    assert only_t.vertices.shape == (2, 778, 3) and torch.equal(only_t.vertices, want.vertices[:2] + 1.0)
    assert layer(return_verts=False).vertices is None and torch.equal(layer(return_verts=False).joints, want.joints)
    with pytest.raises(ValueError):
        layer(hand_pose=z(width + 1) if K else z(6))


def test_tips_and_full_pose_of_the_plain_layer():
    from ihmr_amd import mano
    from ihmr_amd.assets import synthetic_mano
    layer = _layer()
    arrays = synthetic_mano(True)
    o, p, b = (_up(a) for a in MC.inputs("mild", 9, 5, arrays["hands_mean"]))
    t = _up(_normal((9, 3), 8))
    base = layer(global_orient=o, hand_pose=p, betas=b)
    tips = torch.as_tensor(TIPS.astype(np.int64), device="cuda")
    for transl in (None, t):
        out = layer(global_orient=o, hand_pose=p, betas=b, transl=transl, return_tips=True)
        v = base.vertices if transl is None else base.vertices + transl[:, None]
        j = base.joints if transl is None else base.joints + transl[:, None]
        assert type(out) is mano.ManoOutput and torch.equal(out.vertices, v)
        assert torch.equal(out.joints, torch.cat([j, v[:, tips]], dim=1))
    full = layer(global_orient=o, hand_pose=p, betas=b, return_full_pose=True)
    assert type(full) is mano.ManoOutputFullPose and full._fields[:5] == mano.ManoOutput._fields
    assert torch.equal(full.vertices, base.vertices) and torch.equal(full.joints, base.joints)
    want = np.concatenate([o.cpu().numpy(), p.cpu().numpy() + MC._f32(arrays["hands_mean"])[None]], 1)
    assert _bits(full.full_pose.cpu().numpy(), want)
    # the tips' gradient flows into the vertices: only tip rows of the joints are asked for
    leaves = [x.clone().requires_grad_(True) for x in (o, p, b)]
    out = layer(global_orient=leaves[0], hand_pose=leaves[1], betas=leaves[2], return_tips=True)
    out.joints[:, 16:].sum().backward()
    again = [x.clone().requires_grad_(True) for x in (o, p, b)]
    layer(global_orient=again[0], hand_pose=again[1], betas=again[2]).vertices[:, tips].sum().backward()
    assert all(torch.equal(a.grad, b_.grad) and a.grad.abs().sum() > 0 for a, b_ in zip(leaves, again))


# ------------------------------------------------------------------------------------------------------------------ today's callers
def test_todays_call_launches_none_of_the_four_and_keeps_its_bits(monkeypatch):
    from ihmr_amd import hip, mano
    from ihmr_amd.assets import synthetic_mano
    layer = mano.create("", "mano", use_pca=False, is_rhand=True, batch_size=9).cuda()
    c = MC.case("mild", 9, 31, synthetic_mano(True)["hands_mean"])

    def refuse(*a, **k):
        raise AssertionError("a kernel of ihmr_mano_ext.h was launched on today's path")
    L = hip.lib()
    for name in NEW:
        assert callable(getattr(L, name))
        monkeypatch.setattr(L, name, refuse)
    with pytest.raises(AssertionError):
        L.ihmr_mano_post_fwd()
    runs = []
    for direct in (False, True):
        o, p, b = (_up(c[k], True) for k in ("orient", "pose", "betas"))
        if direct:
            verts, joints = mano._LbsFunction.apply(o, p, b, layer)
        else:
            out = layer(betas=b, global_orient=o, hand_pose=p)
            assert type(out) is mano.ManoOutput and len(out) == 5 and out.betas is b and out.global_orient is o and out.hand_pose is p
            verts, joints = out.vertices, out.joints
        ((verts * _up(c["gv"])).sum() + (joints * _up(c["gj"])).sum()).backward()
        runs.append([t.detach().cpu().numpy() for t in (verts, joints, o.grad, p.grad, b.grad)])
    assert all(_bits(a, b_) for a, b_ in zip(*runs))
    assert joints.shape == (9, 16, 3)
    with pytest.raises(AssertionError):                                                # the guard is live: a new argument does launch
        layer(betas=_up(c["betas"]), global_orient=_up(c["orient"]), hand_pose=_up(c["pose"]), return_tips=True)

"""The pure arithmetic helpers the kernels inline (ihmr_amd/csrc/ihmr_pure.h: point-triangle distance, the +x ray test of a grid column,
the three-instruction division, the collision sampler's query cell / cell word / corner mask / trilinear interpolation and its
gradient, Rodrigues, the kinematic chain step, the optimizer step) compiled for the HOST by g++ with
-fsanitize=address,undefined and compared bit for bit with the CPU oracle (oracle/sdf_grid.c) and numpy float32 arithmetic, and
against torch where the oracle is torch.  The GPU-less container can therefore unit-test the very functions whose bits the GPU
parity claims rest on; the GPU tests compare the kernels that inline them.  Plus the oracle's own C code under the sanitizers."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pure")
    exe = hostbuild.build("pure_host_driver.cpp", d, hostbuild.X86_V3)

    def run(op, records, out_dtype=np.float32):
        records = np.ascontiguousarray(records, np.float32)
        fin, fout = str(d / f"{op}.in"), str(d / f"{op}.out")
        with open(fin, "wb") as fh:
            fh.write(np.int32(records.shape[0]).tobytes())
            fh.write(records.tobytes())
        hostbuild.run(exe, op, fin, fout)
        return np.fromfile(fout, out_dtype).reshape(records.shape[0], -1)
    return run


def _oracle():
    from oracle import sdf_ref
    return sdf_ref._lib()


def _tris(rng, n, spread=1.0, size=0.3):
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.normal(0, size, (n, 3, 3))).astype(np.float32)


def test_point_triangle_distance_is_the_oracles_bit_for_bit(driver):
    rng = np.random.default_rng(0)
    n = 20000
    tri = _tris(rng, n)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    # degenerate and special cases: a point ON a corner / edge / face, zero-area and collinear triangles, a duplicated corner
    tri[:50, 1] = tri[:50, 0]
    tri[50:100, 2] = tri[50:100, 0] + 2 * (tri[50:100, 1] - tri[50:100, 0])
    p[100:150] = tri[100:150, 0]
    p[150:200] = 0.5 * (tri[150:200, 0] + tri[150:200, 1])
    p[200:250] = (tri[200:250, 0] + tri[200:250, 1] + tri[200:250, 2]) / 3
    got = driver("ptd", np.concatenate([tri.reshape(n, 9), p], 1))[:, 0]
    L = _oracle()
    ref = np.array([L.ihmr_oracle_point_tri_dist2(tri[i, 0].ctypes.data, tri[i, 1].ctypes.data, tri[i, 2].ctypes.data, p[i].ctypes.data)
                    for i in range(n)], np.float32)
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (int((~same).sum()), got[~same][:4], ref[~same][:4])


def test_column_ray_mask_is_the_oracles_per_voxel_test(driver):
    """sdf_ray_column_hits (one (u, v) test per column + the loop-free t > 0 mask, sdf_ray_hits) against the oracle's per-voxel
    ray_hit_px at all 32 voxel centres of the column -- including near-degenerate triangles (huge 1/det: the mask falls back to the
    per-voxel loop) and triangles that are degenerate in yz (never counted)."""
    rng = np.random.default_rng(1)
    n = 6000
    col = rng.integers(0, 1024, n)
    j, k = col & 31, col >> 5
    py, pz = (2 * j + 1) / 32.0 - 1.0, (2 * k + 1) / 32.0 - 1.0
    tri = np.zeros((n, 3, 3), np.float32)
    tri[:, :, 0] = rng.uniform(-1.2, 1.2, (n, 3))
    tri[:, :, 1] = py[:, None] + rng.normal(0, 0.15, (n, 3))
    tri[:, :, 2] = pz[:, None] + rng.normal(0, 0.15, (n, 3))
    tri[:300, :, 1:] = tri[:300, :1, 1:] + 1e-5 * rng.normal(0, 1, (300, 3, 2))          # slivers in yz: |det| tiny, 1/det huge
    tri[300:400, 2] = tri[300:400, 0]                                                      # degenerate
    tri[400:500, :, 0] = rng.uniform(-1, 1, (100, 1))                                      # planes x = const (crossing exactly between voxels possible)
    out = driver("raycol", np.concatenate([tri.reshape(n, 9), col[:, None].astype(np.float32)], 1), np.uint32)
    L = _oracle()
    px = ((2 * np.arange(32) + 1) / 32.0 - 1.0).astype(np.float32)
    bad = 0
    for i in range(n):
        ref = 0
        p = np.array([0, py[i], pz[i]], np.float32)
        for v in range(32):
            p[0] = px[v]
            ref |= L.ihmr_oracle_ray_hit_px(tri[i, 0].ctypes.data, tri[i, 1].ctypes.data, tri[i, 2].ctypes.data, p.ctypes.data) << v
        bad += int(ref != int(out[i, 2]))
    assert bad == 0, bad
    assert (out[:, 1] == 1).sum() > n // 10 and (out[:, 2] != 0).sum() > n // 20          # (the cases do exercise hits)
    # a restricted `need` mask gives the restriction of the full mask (the static-hand path tests only voxels that are new)
    need = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rec = np.concatenate([tri.reshape(n, 9), col[:, None].astype(np.float32), need.view(np.float32)[:, None]], 1)
    sub = driver("raycol_need", rec, np.uint32)[:, 0]
    assert np.array_equal(sub, out[:, 2] & need)


def test_three_instruction_division_is_ieee_division(driver):
    rng = np.random.default_rng(2)
    n = 200000
    a = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    b = (10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    # the plain-division path: divisors outside [1e-6, 1e6] (a degenerate hand keeps the oracle's infinities / NaNs); a non-finite
    # numerator is only meaningful there (the three-instruction form needs finite operands: documented at sdf_div)
    b[:100] = np.float32(1e-7); b[100:220] = np.float32(1e7); b[200:210] = 0.0; a[210:220] = np.inf
    got = driver("div", np.stack([a, b], 1))[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = (a / b).astype(np.float32)
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), int((~same).sum())


def test_column_range_and_grid_coordinates(driver):
    rng = np.random.default_rng(3)
    n = 5000
    yz = rng.uniform(-1.3, 1.3, (n, 6)).astype(np.float32)
    got = driver("colrange", yz, np.int32)
    centres = (2 * np.arange(32) + 1) / 32.0 - 1.0
    for i in range(0, n, 7):
        y, z = yz[i, :3], yz[i, 3:]
        for lo, hi, (c0, c1) in ((float(y.min()), float(y.max()), got[i, :2]), (float(z.min()), float(z.max()), got[i, 2:])):
            inside = np.nonzero((centres >= lo - 1e-4) & (centres <= hi + 1e-4))[0]
            strict = np.nonzero((centres >= lo) & (centres <= hi))[0]
            have = set(range(c0, c1 + 1))
            assert set(strict) <= have <= set(inside) | {x for x in have if abs(centres[x] - lo) < 2e-4 or abs(centres[x] - hi) < 2e-4}
    x = rng.uniform(-1.5, 1.5, n).astype(np.float32)
    ac = rng.integers(0, 2, n).astype(np.float32)
    out = driver("unnorm", np.stack([x, ac], 1))
    ref = np.where(ac > 0, ((x + np.float32(1)) / np.float32(2)) * np.float32(31), ((x + np.float32(1)) * np.float32(32) - np.float32(1)) / np.float32(2))
    assert np.array_equal(out[:, 0], ref.astype(np.float32))
    ids = np.arange(n) % 32768
    assert np.array_equal(out[:, 1], ((2 * (ids & 31) + 1) / np.float32(32) - np.float32(1)).astype(np.float32))
    assert np.array_equal(out[:, 3], ((2 * (ids >> 10) + 1) / np.float32(32) - np.float32(1)).astype(np.float32))


def test_rodrigues_forward_and_backward_match_the_oracle(driver):
    from oracle.mano_ref import rodrigues_smplx
    rng = np.random.default_rng(4)
    n = 4000
    r = (rng.normal(0, 1, (n, 3)) * rng.uniform(0, 2.5, (n, 1))).astype(np.float32)
    r[:20] = 0.0                                                     # the + 1e-8 branch point
    r[20:40] *= 1e-4
    got = driver("rod_fwd", r).reshape(n, 3, 3)
    rt = torch.tensor(r, dtype=torch.float64, requires_grad=True)
    ref = rodrigues_smplx(rt)
    assert np.abs(got - ref.detach().numpy()).max() < 2e-6
    dR = rng.normal(0, 1, (n, 9)).astype(np.float32)
    (ref * torch.tensor(dR.reshape(n, 3, 3), dtype=torch.float64)).sum().backward()
    gb = driver("rod_bwd", np.concatenate([r, dR], 1))
    big = np.linalg.norm(r, axis=1) > 1e-2                           # (near zero the analytic form divides by the angle: compared where it is conditioned)
    err = np.abs(gb[big] - rt.grad.numpy()[big]).max()
    assert err < 2e-4, err


@pytest.mark.parametrize("scale", [0.0, 1e-6, 1e-4, 1e-3, 1e-2], ids=["zero", "1e-6", "1e-4", "1e-3", "1e-2"])
def test_rodrigues_backward_near_a_zero_rotation(driver, scale):
    """The angles the test above leaves out (||r|| <= 1e-2, where the analytic form divides by the angle and `cos a - sin a / a`
    cancels): no fixed tolerance is right across them, so `rodrigues_bwd` may be 1.5 times as far from the float64 oracle as the oracle's
    own float32 autograd is, or 2e-5 of the largest gradient -- the criterion of tests/mano_cases.py, which tests/test_gpu_mano_layer.py
    applies to the kernels at the same angles (with the device's sinf / cosf)."""
    import mano_cases as MC
    from oracle.mano_ref import rodrigues_smplx
    rng = np.random.default_rng(14)
    n = 2000
    r = (rng.normal(0, 1, (n, 3)) * scale).astype(np.float32)
    dR = rng.normal(0, 1, (n, 9)).astype(np.float32)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        rt = torch.tensor(r, dtype=dtype, requires_grad=True)
        (rodrigues_smplx(rt) * torch.tensor(dR.reshape(n, 3, 3), dtype=dtype)).sum().backward()
        grads[dtype] = rt.grad.numpy().astype(np.float64)
    got = driver("rod_bwd", np.concatenate([r, dR], 1))
    f64 = grads[torch.float64]
    MC.within(got, f64, grads[torch.float32], MC.floor_of("d_pose", f64), f"rodrigues_bwd on the host, r ~ N(0, {scale:g})")


def test_optimizer_steps_are_torch_optim_in_float32(driver):
    rng = np.random.default_rng(5)
    n = 5000
    x, g = rng.normal(0, 1, n).astype(np.float32), (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
    m, v = (0.1 * rng.normal(0, 1, n)).astype(np.float32), (rng.uniform(0, 1, n) ** 4).astype(np.float32)
    t, lr = 7, 1e-2
    step, bc2 = np.float32(lr / (1 - 0.9 ** t)), np.float32(np.sqrt(1 - 0.999 ** t))
    out = driver("adam", np.stack([x, g, m, v, np.full(n, step, np.float32), np.full(n, bc2, np.float32)], 1))
    f = np.float32
    m2 = m + f(0.1) * (g - m)
    v2 = v * f(0.999)
    v2 = v2 + (f(0.001) * g) * g
    x2 = x + (-step) * (m2 / (np.sqrt(v2) / bc2 + f(1e-8)))
    assert np.array_equal(out[:, 1], m2) and np.array_equal(out[:, 2], v2) and np.array_equal(out[:, 0], x2.astype(np.float32))
    p = torch.nn.Parameter(torch.tensor(x))
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999))
    p.grad = torch.tensor(g)
    opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.tensor(m), exp_avg_sq=torch.tensor(v))
    opt.step()
    # (torch's CPU kernels may order the products of addcmul / addcdiv differently: equal to rounding, i.e. relative to the size of the step)
    upd = np.abs(out[:, 0] - x)
    assert np.all(np.abs(out[:, 0] - p.detach().numpy()) <= 2e-4 * upd + 4e-7) and np.abs(out[:, 1] - opt.state[p]["exp_avg"].numpy()).max() < 1e-6
    out = driver("sgd", np.stack([x, g, m, np.full(n, lr, np.float32)], 1))
    mb = m * f(0.9) + g
    assert np.array_equal(out[:, 1], mb) and np.array_equal(out[:, 0], (x + f(-lr) * mb).astype(np.float32))


def test_chain_step_and_loss_helpers(driver):
    rng = np.random.default_rng(6)
    n = 3000
    rec = rng.normal(0, 1, (n, 27)).astype(np.float32)
    out = driver("chain", rec)
    Gp, R, Jj, Jp = rec[:, :12].reshape(n, 3, 4).astype(np.float64), rec[:, 12:21].reshape(n, 3, 3).astype(np.float64), rec[:, 21:24].astype(np.float64), rec[:, 24:].astype(np.float64)
    G = np.concatenate([Gp[:, :, :3] @ R, (Gp[:, :, :3] @ (Jj - Jp)[:, :, None]) + Gp[:, :, 3:]], 2)
    assert np.abs(out[:, :12].reshape(n, 3, 4) - G).max() < 2e-5
    A = G.copy()
    A[:, :, 3] = G[:, :, 3] - (G[:, :, :3] @ Jj[:, :, None])[:, :, 0]
    assert np.abs(out[:, 12:].reshape(n, 3, 4) - A).max() < 5e-5
    ab = rng.normal(0, 1, (n, 6)).astype(np.float32)
    w = rng.choice(np.array([0.0, 1e-8, 0.3, 0.5, 0.51, 1.0], np.float32), n)
    o = driver("misc", np.concatenate([ab, w[:, None]], 1))
    assert np.abs(o[:, :3] - np.cross(ab[:, :3].astype(np.float64), ab[:, 3:].astype(np.float64))).max() < 1e-6
    assert np.array_equal(o[:, 3], np.where(w > 0.5, 0, np.where(w < 1e-7, 21, -1)).astype(np.float32))


# ----------------------------------------------------------------------------------- the collision sampler's arithmetic
G = 32
F = np.float32


def test_cell_word_round_trips(driver):
    """Pack -> unpack is the identity for every cell (i0, j0, k0) in [-1, 31]^3, the mask insert / extract round-trips all 256 masks,
    and a query outside the grid has the word 0 (whatever cell it names)."""
    r = np.arange(-1, G)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    n = cells.shape[0]
    m8 = np.arange(n) % 256
    out = driver("qcell", np.concatenate([np.ones((n, 1)), cells, m8[:, None]], 1), np.uint32)
    assert np.array_equal(out[:, 1:4].view(np.int32), cells)
    assert np.array_equal(out[:, 0], 0x80000000 | (cells[:, 0] + 1) | ((cells[:, 1] + 1) << 6) | ((cells[:, 2] + 1) << 12))
    assert np.array_equal(out[:, 5], m8) and np.array_equal(out[:, 4], out[:, 0] | (m8 << 18)) and set(m8) == set(range(256))
    out = driver("qcell", np.concatenate([np.zeros((n, 1)), cells, np.zeros((n, 1))], 1), np.uint32)
    assert not out[:, 0].any() and not out[:, 5].any()


def _unnorm_ref(x, align_corners):
    return (x + F(1)) / F(2) * F(G - 1) if align_corners else ((x + F(1)) * F(G) - F(1)) / F(2)


def _query_ref(q, c, s, swap_xz, align_corners):
    """sdf_query_cell in numpy float32, operation for operation (sdf_div is the IEEE division: its own test above)."""
    with np.errstate(all="ignore"):
        n = (q - c) / s
        if swap_xz:
            n = n[:, ::-1]
        ic = _unnorm_ref(n, align_corners).astype(F)
        f0 = np.floor(ic)
        return ic, f0, ((f0 >= -1) & (f0 <= G - 1)).all(1)


def _trilinear_ref(ic, pv):
    """sdf_trilinear<false> in numpy float32, operation for operation: the corners in the order c8 = di + 2 dj + 4 dk, a corner outside
    the grid skipped."""
    f0 = np.floor(ic)
    w1, w0 = ic - f0, (f0 + F(1)) - ic
    c0 = f0.astype(np.int64)
    val, g = np.zeros(len(ic), F), [np.zeros(len(ic), F) for _ in range(3)]
    for c8 in range(8):
        d = (c8 & 1, (c8 >> 1) & 1, c8 >> 2)
        ok = np.all([(c0[:, a] + d[a] >= 0) & (c0[:, a] + d[a] < G) for a in range(3)], 0)
        wx, wy, wz = (w1[:, a] if d[a] else w0[:, a] for a in range(3))
        p = pv[:, c8]
        val = np.where(ok, val + p * (wx * wy * wz), val)
        for a, w in enumerate((wy * wz, wx * wz, wx * wy)):
            g[a] = np.where(ok, g[a] + (p if d[a] else -p) * w, g[a])
    return val, np.stack(g, 1)


def _corner_values(phi, c0, junk):
    """pv[c8] of the cells c0 (N, 3) = (i0, j0, k0) from phi[k][j][i]; `junk` where the corner lies outside the grid."""
    pv = np.full((len(c0), 8), junk, F)
    for c8 in range(8):
        i, j, k = c0[:, 0] + (c8 & 1), c0[:, 1] + ((c8 >> 1) & 1), c0[:, 2] + (c8 >> 2)
        ok = (i >= 0) & (i < G) & (j >= 0) & (j < G) & (k >= 0) & (k < G)
        pv[ok, c8] = phi[k[ok], j[ok], i[ok]]
    return pv


def _sampler_queries(rng, align_corners, n=20000):
    """Normalised queries in [-1.15, 1.15]^3; the first 200 exactly on lattice coordinates (every component: the float32 whose grid
    coordinate is an integer), the next 12 with floor = -1 and floor = 31 on each axis; the last two non-finite."""
    x = rng.uniform(-1.15, 1.15, (n, 3)).astype(F)
    lat = rng.integers(0, G, (200, 3))
    want = (2.0 * lat / (G - 1) - 1.0) if align_corners else ((2.0 * lat + 1.0) / G - 1.0)
    best = want.astype(F)
    for cand in (np.nextafter(best, F(2)), np.nextafter(best, F(-2))):         # (align_corners: 2 i / 31 - 1 is not a float32)
        hit = (_unnorm_ref(cand, align_corners) == lat) & (_unnorm_ref(best, align_corners) != lat)
        best = np.where(hit, cand, best)
    x[:200] = best
    edge = (F(-1.0), F(1.0)) if not align_corners else (F(-1.03), F(1.03))      # grid coordinates -0.5 / 31.5 and -0.97 / 31.97
    for a in range(3):
        x[200 + 4 * a:202 + 4 * a, a] = edge[0]
        x[202 + 4 * a:204 + 4 * a, a] = edge[1]
    x[-2] = (np.nan, 0.1, 0.2)
    x[-1] = (0.1, np.inf, 0.2)
    return x, lat


@pytest.fixture(scope="module")
def sampler_grid():
    rng = np.random.default_rng(7)
    return (rng.uniform(0.0, 0.3, (G, G, G)) * (rng.random((G, G, G)) > 0.6)).astype(F)       # phi[k][j][i]: ~60 % of the voxels zero


@pytest.mark.parametrize("swap_xz", [0, 1])
@pytest.mark.parametrize("align_corners", [0, 1])
def test_query_cell_and_trilinear_core_are_the_numpy_float32_restatement(driver, sampler_grid, align_corners, swap_xz):
    """sdf_query_cell (grid coordinates, in-grid flag, cell word) and sdf_trilinear (value, gradient, value-only form) + sdf_grad_to_vertex
    against the same operations in numpy float32, bit for bit, at 20 000 queries against a random grid: in a hand-sized box (the
    three-instruction division) and in the unit box, where the first 200 queries lie exactly on lattice coordinates."""
    rng = np.random.default_rng(100 + 2 * align_corners + swap_xz)
    phi = sampler_grid
    x, lat = _sampler_queries(rng, align_corners)
    n = len(x)
    for c, s in ((np.zeros(3, F), F(1.0)), (np.array([0.013, -0.021, 0.034], F), F(0.1137))):
        q = (c + s * x).astype(F)
        rec = np.concatenate([q, np.tile(c, (n, 1)), np.full((n, 1), s), np.full((n, 1), swap_xz), np.full((n, 1), align_corners)], 1)
        out = driver("query", rec, np.uint32)
        ic, f0, ing = _query_ref(q, c, s, swap_xz, align_corners)
        got_ic = out[:, :3].view(F)
        # (a non-finite query: the three-instruction division turns an infinite numerator into NaN -- documented at sdf_div; either is "outside")
        assert ((got_ic.view(np.uint32) == ic.view(np.uint32)) | (~np.isfinite(got_ic) & ~np.isfinite(ic))).all()
        assert np.isfinite(ic[:-2]).all()
        assert np.array_equal(out[:, 3], ing.astype(np.uint32))
        assert not out[-2:, 3].any() and not out[-2:, 4].any(), "a non-finite query is outside the grid"
        c0 = np.where(ing[:, None], f0, 0).astype(np.int64)
        assert np.array_equal(out[:, 4], np.where(ing, 0x80000000 | (c0[:, 0] + 1) | ((c0[:, 1] + 1) << 6) | ((c0[:, 2] + 1) << 12), 0))
        if s == 1.0:
            on_lattice = ic[:200] == (lat[:, ::-1] if swap_xz else lat)
            assert on_lattice.all(1).sum() >= 150 and on_lattice.mean() > 0.9, on_lattice.mean()
        for a in range(3):
            assert (ing & (f0[:, a] == -1)).sum() >= 2 and (ing & (f0[:, a] == G - 1)).sum() >= 2, "both border cells on every axis"
        assert 0.5 * n < ing.sum() < n - 2
        # the interpolation at the in-grid queries; corners outside the grid hold junk, which must not be read
        icg, c0g = ic[ing], c0[ing]
        pv = _corner_values(phi, c0g, 1e30)
        m = len(icg)
        rec = np.concatenate([icg, pv, np.full((m, 1), s), np.full((m, 1), swap_xz), np.full((m, 1), align_corners)], 1)
        out = driver("trilin", rec)
        val, g = _trilinear_ref(icg, pv)
        chain = (F(0.5) * F(G - 1 if align_corners else G)) / s
        gv = g * chain
        if swap_xz:
            gv = gv[:, ::-1]
        assert np.array_equal(out[:, 0].view(np.uint32), val.view(np.uint32)) and np.array_equal(out[:, 4].view(np.uint32), val.view(np.uint32))
        assert np.array_equal(out[:, 1:4].view(np.uint32), g.view(np.uint32))
        assert np.array_equal(out[:, 5:8].view(np.uint32), np.ascontiguousarray(gv).view(np.uint32))
        assert (val > 0).sum() > m // 2


@pytest.mark.parametrize("swap_xz", [0, 1])
@pytest.mark.parametrize("align_corners", [0, 1])
def test_trilinear_core_is_as_close_to_float64_grid_sample_as_torch_float32(driver, sampler_grid, align_corners, swap_xz):
    """Value and vertex gradient of the pure functions (unit box: the normalised coordinate IS the query) against
    torch.nn.functional.grid_sample (bilinear, zeros padding) and its autograd.  The arbiter is torch in float64 on the same float32
    inputs; the pure functions' largest error against it is at most 1.5 x the largest error of torch's own float32 grid_sample (the
    factor of the project's float64 arbiter tests).  The queries of the bit-for-bit test without the 200 on lattice coordinates: the
    gradient jumps there, and the float64 un-normalisation of the same input may fall into the neighbouring cell."""
    import torch.nn.functional as TF
    rng = np.random.default_rng(100 + 2 * align_corners + swap_xz)
    phi = sampler_grid
    x = _sampler_queries(rng, align_corners)[0][200:-2]
    n = len(x)
    ic, f0, ing = _query_ref(x, np.zeros(3, F), F(1.0), swap_xz, align_corners)
    pv = _corner_values(phi, np.where(ing[:, None], f0, 0).astype(np.int64), 1e30)
    rec = np.concatenate([np.where(ing[:, None], ic, 0), pv, np.full((n, 1), 1.0), np.full((n, 1), swap_xz), np.full((n, 1), align_corners)], 1)
    out = driver("trilin", rec)
    got_val, got_g = np.where(ing, out[:, 0], 0), np.where(ing[:, None], out[:, 5:8], 0)

    def torch_ref(dtype):
        qt = torch.tensor(x, dtype=dtype, requires_grad=True)
        grid = (qt.flip(1) if swap_xz else qt).view(1, n, 1, 1, 3)
        v = TF.grid_sample(torch.tensor(phi, dtype=dtype).view(1, 1, G, G, G), grid, mode="bilinear", padding_mode="zeros",
                           align_corners=bool(align_corners)).view(n)
        v.sum().backward()
        return v.detach().numpy().astype(np.float64), qt.grad.numpy().astype(np.float64)

    v64, g64 = torch_ref(torch.float64)
    v32, g32 = torch_ref(torch.float32)
    ev, eg = np.abs(got_val - v64).max(), np.abs(got_g - g64).max()
    tv, tg = np.abs(v32 - v64).max(), np.abs(g32 - g64).max()
    print(f"[pure] grid_sample align_corners={align_corners} swap_xz={swap_xz}: value error {ev:.2e} (torch float32 {tv:.2e}), gradient error {eg:.2e} (torch float32 {tg:.2e})")
    assert (np.abs(v64) > 0).sum() > n // 2 and np.abs(g64).max() > 1.0
    assert ev <= 1.5 * tv and eg <= 1.5 * tg, (ev, tv, eg, tg)


def test_corner_mask_is_the_per_corner_bitmap_lookup(driver):
    """sdf_corner_mask against a plain per-corner lookup in random 32 x 32-word bitmaps (sparse, half full, dense), at every cell
    (i0, j0, k0) in [-1, 31]^3: bit 2 c4 is voxel i0 and bit 2 c4 + 1 voxel i0 + 1 of column c4 = (j - j0) + 2 (k - k0)."""
    rng = np.random.default_rng(8)
    r = np.arange(-1, G)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    i0, j0, k0 = cells.T
    seen = set()
    for fill in (0.1, 0.5, 0.9):
        inside = rng.random((G, G, G)) < fill                                            # [k][j][i]
        words = (inside.astype(np.uint64) << np.arange(G, dtype=np.uint64)).sum(-1).astype(np.uint32)     # [k][j]: bit i
        rec = np.zeros((len(cells), 5), np.uint32)
        ref = np.zeros(len(cells), np.uint32)
        for c4 in range(4):
            j, k = j0 + (c4 & 1), k0 + (c4 >> 1)
            col = (j >= 0) & (j < G) & (k >= 0) & (k < G)
            rec[col, c4] = words[k[col], j[col]]
            for di in range(2):
                i = i0 + di
                ok = col & (i >= 0) & (i < G)
                ref[ok] |= inside[k[ok], j[ok], i[ok]].astype(np.uint32) << np.uint32(2 * c4 + di)
        rec[:, 4] = i0.astype(np.int32).view(np.uint32)
        got = driver("cmask", rec.view(np.float32), np.uint32)[:, 0]
        assert np.array_equal(got, ref)
        seen |= set(ref.tolist())
    assert len(seen) == 256


def test_oracle_c_code_runs_clean_under_the_sanitizers():
    """`make -C oracle asan`: oracle/sdf_grid.c + its known-answer tests (oracle/sdf_kat.c) as one program under ASan / UBSan."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "asan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sdf_kat: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])

"""The statement of the two-hand intersection volume (``ihmr_sdf_volume``), independent of ``ihmr_amd``: the frame
arithmetic in numpy float32 exactly as the issue of record defines it, the inside grids from the oracle (``oracle.sdf_ref.sdf_grid`` on
the tile-normalised vertices: float32 for the spec, float64 on the same float32 frame for the arbiter; inside is ``phi > 0``),
``close_boundary`` restated, and the seeded case table.

    lo = max(min A, min B), hi = min(max A, max B) per axis;  empty (status 1) when any hi <= lo;
    invalid (status 2) when a vertex is non-finite or s < 1e-5;  c = (lo + hi) * 0.5f, s = 0.5f * max_axis(hi - lo);
    tile (tx, ty, tz) of n^3: off = (float)(2t + 1) / (float)n - 1.0f, ct = c + s * off (two roundings), st = s / (float)n;
    vn = (v - ct) / st;  voxel (k, j, i) = (z, y, x) has its centre at (2 idx + 1) / 32 - 1;  count = #(inside A and inside B);
    volume = count * (2 st / 32)^3 in float64.

Order of the status rules: non-finite first, then empty, then s.  A sample that is not counted has box 0 and no voxels.  Tile index
``(tz * n + ty) * n + tx``; column ``k * 32 + j``, bit ``i``."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

G = 32
S_MIN = np.float32(1e-5)
COUNTED, EMPTY, INVALID = 0, 1, 2
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ closing a mesh
def boundary_edges(faces):
    """Directed edges (a, b) of the faces whose opposite (b, a) is no edge of any face."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    have = set(map(tuple, e.tolist()))
    return [(a, b) for a, b in e.tolist() if (b, a) not in have]


def close_boundary(faces, n_verts):
    """Every boundary loop closed by a triangle fan from the loop's lowest-numbered vertex; no vertex is added.  A loop v0 -> v1 ->
    ... -> v_{m-1} -> v0 (v0 the lowest) gets the m - 2 faces (v0, v_{i+1}, v_i), i = 1 .. m-2, which run against the boundary."""
    f = np.asarray(faces)
    assert f.ndim == 2 and f.shape[1] == 3 and f.min() >= 0 and f.max() < n_verts
    nxt = {}
    for a, b in boundary_edges(f):
        assert a not in nxt, "a boundary vertex with two outgoing boundary edges: not a simple loop"
        nxt[a] = b
    added, left = [], set(nxt)
    while left:
        v0 = min(left)
        loop, v = [v0], nxt[v0]
        while v != v0:
            loop.append(v)
            v = nxt[v]
        left -= set(loop)
        added += [(v0, loop[i + 1], loop[i]) for i in range(1, len(loop) - 1)]
    if not added:
        return f.copy()
    return np.concatenate([f, np.asarray(added, f.dtype)])


# ------------------------------------------------------------------------------------------------------------------ the frame
def cube(va, vb):
    """(box (4,) float32 = cx, cy, cz, s; status) of one sample."""
    va, vb = np.asarray(va, F32), np.asarray(vb, F32)
    zero = np.zeros(4, F32)
    if not (np.isfinite(va).all() and np.isfinite(vb).all()):
        return zero, INVALID
    lo = np.maximum(va.min(axis=0), vb.min(axis=0))
    hi = np.minimum(va.max(axis=0), vb.max(axis=0))
    if (hi <= lo).any():
        return zero, EMPTY
    s = F32(0.5) * np.max(hi - lo)
    if s < S_MIN:
        return zero, INVALID
    c = (lo + hi) * F32(0.5)
    return np.array([c[0], c[1], c[2], s], F32), COUNTED


def tile_frame(box, n, tile):
    """(ct (3,) float32, st float32) of tile (tz * n + ty) * n + tx."""
    t = np.array([tile % n, (tile // n) % n, tile // (n * n)])
    off = (2 * t + 1).astype(F32) / F32(n) - F32(1.0)
    so = box[3] * off                         # one rounding
    return (box[:3] + so).astype(F32), F32(box[3] / F32(n))


def voxel_volume(box, n):
    """(2 st / 32)^3 in float64 from the float32 s: the cell's side multiplied out, (a * a) * a."""
    st = np.float64(F32(box[3] / F32(n)))
    a = 2.0 * st / 32.0
    return (a * a) * a


def _words(inside):
    """(T,32,32,32) bool [k][j][i] -> (T,1024) uint32, bit i of word k * 32 + j."""
    w = (inside.astype(np.uint64) << np.arange(G, dtype=np.uint64)).sum(axis=-1)
    return w.reshape(inside.shape[0], G * G).astype(np.uint32)


_CACHE = {}


def statement(case, n, f64=False):
    """dict(box (4,) f32, status, counts (n^3,) uint32, bits (n^3,1024) uint32, inside_a / inside_b (n^3,32,32,32) bool) of one case
    at subdivision n; ``f64``: the grids in double precision on the same float32 frame.  Computed once per (case, n, precision)."""
    key = (case.name, n, f64)
    if key in _CACHE:
        return _CACHE[key]
    from oracle.sdf_ref import sdf_grid
    T = n ** 3
    box, status = cube(case.va, case.vb)
    out = dict(box=box, status=status, counts=np.zeros(T, np.uint32), bits=np.zeros((T, G * G), np.uint32),
               inside_a=np.zeros((T, G, G, G), bool), inside_b=np.zeros((T, G, G, G), bool))
    if status == COUNTED:
        for key_in, v, faces in (("inside_a", case.va, case.fa), ("inside_b", case.vb, case.fb)):
            vn = []
            for t in range(T):
                ct, st = tile_frame(box, n, t)
                if f64:
                    vn.append((v.astype(np.float64) - ct.astype(np.float64)) / np.float64(st))
                else:
                    vn.append(((v - ct) / st).astype(F32))
                    assert vn[-1].dtype == F32
            phi = sdf_grid(torch.from_numpy(np.stack(vn)), torch.from_numpy(np.asarray(faces, np.int32)))
            out[key_in] = phi.numpy() > 0
        both = out["inside_a"] & out["inside_b"]
        out["bits"] = _words(both)
        out["counts"] = both.reshape(T, -1).sum(axis=1).astype(np.uint32)
    _CACHE[key] = out
    return out


def volume_m3(case, n):
    s = statement(case, n)
    return float(s["counts"].astype(np.float64).sum() * voxel_volume(s["box"], n))


# ------------------------------------------------------------------------------------------------------------------ meshes
def icosphere(level, radius=1.0):
    """Icosahedron subdivided ``level`` times, vertices pushed onto the sphere: 42 / 80 (1), 162 / 320 (2), 642 / 1280 (3)."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius), np.asarray(f, np.int32)


def rotation(seed):
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


SPHERE_R, SPHERE_D = 0.03, 0.03


def lens_volume(r=SPHERE_R, d=SPHERE_D):
    """Two spheres of radius r, centres d apart: pi (4 r + d) (2 r - d)^2 / 12."""
    return np.pi * (4 * r + d) * (2 * r - d) ** 2 / 12.0


def sphere_pair(level, seed=5):
    """Two icospheres of radius 0.03 m, centres 0.03 m apart, each rotated into general position, the pair off the origin."""
    v, f = icosphere(level, SPHERE_R)
    d = rotation(seed) @ np.array([1.0, 0.0, 0.0]) * SPHERE_D
    origin = np.array([0.013, -0.021, 0.417])
    a = v @ rotation(seed + 1).T + origin
    b = v @ rotation(seed + 2).T + origin + d
    return a.astype(F32), f, b.astype(F32), f


def tetra_pair():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * 0.03
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    a = v @ rotation(21).T + [0.1, 0.2, 0.5]
    b = v @ rotation(22).T + [0.1, 0.2, 0.5] + np.array([0.011, -0.007, 0.005])
    return a.astype(F32), f, b.astype(F32), f


class Case:
    def __init__(self, name, group, va, fa, vb, fb, status=COUNTED, known_answer=False):
        self.name, self.group, self.status, self.known_answer = name, group, status, known_answer
        self.va, self.vb = np.ascontiguousarray(va, F32), np.ascontiguousarray(vb, F32)
        self.fa, self.fb = np.ascontiguousarray(fa, np.int32), np.ascontiguousarray(fb, np.int32)


_TABLE = None


def case_table():
    """name -> Case.  ``group``: cases of one group share their face tables and vertex counts, so they can form one batch.  The hand
    pairs carry the capped faces (``close_boundary``) except ``hand_open``, the uncapped MANO-shaped mesh the C ABI takes as well."""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    import helpers as H
    from ihmr_amd.assets import synthetic_mano
    mitten = synthetic_mano(True), synthetic_mano(False)
    fingers = synthetic_mano(True, kind="fingers"), synthetic_mano(False, kind="fingers")
    cap = lambda arrays: tuple(close_boundary(np.asarray(m["faces"], np.int32), 778) for m in arrays)
    t = OrderedDict()

    def add(name, group, va, fa, vb, fb, **kw):
        t[name] = Case(name, group, va, fa, vb, fb, **kw)

    fr, fl = cap(mitten)
    hv, _ = H.oracle_two_hand_verts(mitten, 3, 11)
    hv = hv.numpy()
    for b in range(3):
        add(f"hand_default_{b}", "hand", hv[b, 0], fr, hv[b, 1], fl)
    deep, _ = H.oracle_two_hand_verts(mitten, 2, H.DEEP_SEED, overlap="deep")
    deep = deep.numpy()
    for b in range(2):
        add(f"hand_deep_{b}", "hand", deep[b, 0], fr, deep[b, 1], fl)
    a, b = deep[0, 0], deep[0, 1]
    box, _ = cube(a, b)
    add("disjoint", "hand", a, fr, b + F32([1.0, 0.0, 0.0]), fl, status=EMPTY)
    nan = a.copy()
    nan[345, 1] = np.nan
    add("nan_vertex", "hand", nan, fr, b, fl, status=INVALID)
    add("tiny_cube", "hand", a * F32(1e-4), fr, b * F32(1e-4), fl, status=INVALID)
    add("shifted_2m", "hand", a + F32(2.0), fr, b + F32(2.0), fl)
    far = a.copy()
    far[100] = box[:3] + F32([0.3, box[3] + 1.0, -(box[3] + 1.0)])        # 1 m outside the cube in y and in z
    add("far_vertex", "hand", far, fr, b, fl)
    add("hand_open", "hand_open", hv[0, 0], np.asarray(mitten[0]["faces"], np.int32), hv[0, 1], np.asarray(mitten[1]["faces"], np.int32))
    gr, gl = cap(fingers)
    fv, _ = H.oracle_two_hand_verts(fingers, 2, 12, interlock=True)
    fv = fv.numpy()
    for b in range(2):
        add(f"fingers_{b}", "fingers", fv[b, 0], gr, fv[b, 1], gl)
    add("sphere162", "sphere162", *sphere_pair(2), known_answer=True)
    sa, sf, sb, _ = sphere_pair(2, seed=9)
    sb = sb + F32([0.2, 0.0, 0.0])
    sb[np.argmin(sb[:, 0]), 0] = sa[:, 0].max()                            # the boxes touch in x: hi == lo
    assert sb[:, 0].min() == sa[:, 0].max()
    add("touching", "sphere162", sa, sf, sb, sf, status=EMPTY)
    add("sphere642", "sphere642", *sphere_pair(3), known_answer=True)
    add("tetra", "tetra", *tetra_pair(), known_answer=True)
    ball, bf = icosphere(2, 0.03)
    add("sphere_vs_hand", "sphere_vs_hand", (ball + deep[1, 0].mean(axis=0)).astype(F32), bf, deep[1, 1], fl)
    _TABLE = t
    return t


SUBDIV_2_4_CASES = ("hand_default_0", "hand_deep_0", "sphere162", "far_vertex")     # the four cases also stated at subdiv 2 and 4

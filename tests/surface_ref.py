"""The exact point-to-surface signed distance stated in float64 numpy, its analytic gradient, and the
seeded case table of the CPU and GPU tests.  Nothing here imports ``ihmr_amd.sdf`` or reads ``csrc/surface_pure.h``.

All arithmetic is float64 on float32 arrays.  One face table ``[surface faces 0..F_dist) | cap faces F_dist..F_total)``: distances are
taken to the surface faces, the sign over all faces.

* a face is usable when its ids lie in [0, V), its vertices are finite and ``n = (b - a) x (c - a)`` has ``(nx*nx + ny*ny) + nz*nz != 0``.
* unsigned distance -- NOT the region method of the header but the textbook decomposition: the foot of the perpendicular on the face's
  plane where it lies inside the triangle (its weights from the Gram system of the two edges), else the nearest of the three closed edge
  segments (the parameter of the foot on the edge's line, clamped to [0, 1]).  The minimum over the faces is taken on the squares
  (``argmin``: the lowest face id wins an exact tie), one root at the end.
* sign -- the +x ray: ``det = (b_y-a_y)(c_z-a_z) - (c_y-a_y)(b_z-a_z)``, a face with ``det == 0`` does not count, ``u`` and ``v`` by two
  divisions, a crossing needs ``u >= 0, v >= 0, u + v <= 1`` and ``(a_x + u (b_x-a_x)) + v (c_x-a_x) > q_x``.  Odd parity: inside.
* a query with a non-finite coordinate, or a mesh without a usable surface face: ``dist = NaN, face = -1, bary = 0``.
* gradient -- with the closest point ``c`` and ``n = sign (q - c) / |q - c|``: ``d dist / d q = n``, ``d dist / d vertex_k = -w_k n`` on
  the three vertices of the closest face; 0 where ``|q - c| == 0`` or ``dist`` is NaN.

MARGIN.  A sign is exact only if no ray passes within rounding of a triangle's edge or starts within rounding of its plane: for every
query and every face whose ``min(u, v, 1 - u - v) > -RAY_MARGIN`` both that minimum and ``|x_hit - q_x|`` are at least ``RAY_MARGIN`` =
1e-9 in magnitude; and every ``dist / scale`` of the hand cases lies at least ``THR_MARGIN`` = 1e-8 from every threshold it meets.
``python tests/surface_ref.py`` prints what violates either (nothing, as committed); seeds were searched on the CPU until both held.
"""
import functools
import os
import sys
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

F32, F64 = np.float32, np.float64
TOL = 1e-9                                           # the project's bar on a float64 device value [m]
RAY_MARGIN, THR_MARGIN = 1e-9, 1e-8
THRESHOLDS = (0.003, 0.005)                          # the Evaluator's default surface_thresholds
TABLES = {1: (0.003,), 2: THRESHOLDS, 8: tuple(np.linspace(0.003, 0.0171, 8))}
NV, NF = 778, 1538
CHUNK = 128                                          # queries per numpy block: (CHUNK, F, 3) float64 temporaries


# ------------------------------------------------------------------------------------------------------------------ statement
def usable_faces(verts, faces):
    """(F_total,) bool: the faces that count."""
    v, f = np.asarray(verts).astype(F64), np.asarray(faces).astype(np.int64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    g = np.where(ok[:, None], f, 0)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        ok &= np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ok &= ((nx * nx + ny * ny) + nz * nz) != 0.0
    return ok


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _pair_sq(q, a, b, c):
    """q (n,1,3), a / b / c (1,F,3) -> (sq (n,F), weights (n,F,3)): the plane foot where it is inside, else the nearest edge segment."""
    e1, e2, p = b - a, c - a, q - a
    n = np.cross(e1, e2)
    nn = _dot(n, n)
    g11, g12, g22, r1, r2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(p, e1), _dot(p, e2)
    D = g11 * g22 - g12 * g12
    with np.errstate(all="ignore"):
        v, w = (g22 * r1 - g12 * r2) / D, (g11 * r2 - g12 * r1) / D
        pn = _dot(p, n)
        plane = pn * pn / nn
    inside = (v >= 0) & (w >= 0) & (v + w <= 1)
    best = np.where(inside, plane, np.inf)
    wts = np.stack([1.0 - v - w, v, w], axis=-1)
    wts = np.where(inside[..., None], wts, 0.0)
    for (x0, x1), (k0, k1) in (((a, b), (0, 1)), ((a, c), (0, 2)), ((b, c), (1, 2))):
        e = x1 - x0
        with np.errstate(all="ignore"):
            t = np.clip(_dot(q - x0, e) / _dot(e, e), 0.0, 1.0)
        d = (q - x0) - t[..., None] * e
        sq = _dot(d, d)
        take = sq < best
        best = np.where(take, sq, best)
        ew = np.zeros(t.shape + (3,))
        ew[..., k0], ew[..., k1] = 1.0 - t, t
        wts = np.where(take[..., None], ew, wts)
    return best, wts


def ray_terms(q, a, b, c):
    """q (n,1,3), a / b / c (1,F,3) -> (crosses (n,F) bool, edge margin min(u, v, 1-u-v) (n,F), x_hit - q_x (n,F), det != 0 (1,F))."""
    e1y, e1z, e2y, e2z = b[..., 1] - a[..., 1], b[..., 2] - a[..., 2], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
    det = e1y * e2z - e2y * e1z
    py, pz = q[..., 1] - a[..., 1], q[..., 2] - a[..., 2]
    with np.errstate(all="ignore"):
        u = (py * e2z - e2y * pz) / det
        v = (e1y * pz - py * e1z) / det
        xh = (a[..., 0] + u * (b[..., 0] - a[..., 0])) + v * (c[..., 0] - a[..., 0])
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        return ok & (xh > q[..., 0]), np.minimum(np.minimum(u, v), 1.0 - u - v), xh - q[..., 0], det != 0


def surface_distance(points, verts, faces, F_dist, signed=True):
    """dict(dist (P,) float64, face (P,) int, bary (P,3), sq (P,) the minimum square, margin: the smallest |ray margin| met) of one
    sample: points (P,3), verts (V,3) float32, faces (F_total,3) integer."""
    q_all, v = np.asarray(points).astype(F64), np.asarray(verts).astype(F64)
    f = np.asarray(faces).astype(np.int64)
    P = len(q_all)
    use = usable_faces(verts, faces)
    out = dict(dist=np.full(P, np.nan), face=np.full(P, -1, np.int64), bary=np.zeros((P, 3)), sq=np.full(P, np.nan), margin=np.inf)
    surf = np.nonzero(use[:F_dist])[0]
    every = np.nonzero(use)[0]
    if len(surf) == 0:
        return out
    tri = lambda ids: tuple(v[f[ids, k]][None] for k in range(3))
    sa, sb, sc = tri(surf)
    ea, eb, ec = tri(every)
    finite = np.isfinite(q_all).all(axis=1)
    for lo in range(0, P, CHUNK):
        rows = np.nonzero(finite[lo:lo + CHUNK])[0] + lo
        if len(rows) == 0:
            continue
        q = q_all[rows][:, None, :]
        sq, wts = _pair_sq(q, sa, sb, sc)
        k = np.argmin(sq, axis=1)
        r = np.arange(len(rows))
        best = sq[r, k]
        inside = np.zeros(len(rows), bool)
        if signed:
            cross, edge, ahead, det = ray_terms(q, ea, eb, ec)
            inside = (cross.sum(axis=1) % 2) == 1
            cand = det & (edge > -RAY_MARGIN)                   # every face the ray passes through or within the margin of
            with np.errstate(all="ignore"):
                m = np.where(cand, np.minimum(np.abs(edge), np.abs(ahead)), np.inf)
            out["margin"] = min(out["margin"], float(m.min()))
        out["sq"][rows] = best
        out["dist"][rows] = np.where(inside, -np.sqrt(best), np.sqrt(best))
        out["face"][rows] = surf[k]
        out["bary"][rows] = wts[r, k]
    return out


def distance_to_face(points, verts, faces, face_ids):
    """(P,) the statement's squared distance from query i to face ``face_ids[i]`` (NaN where the id is < 0)."""
    q, v, f = np.asarray(points).astype(F64), np.asarray(verts).astype(F64), np.asarray(faces).astype(np.int64)
    ids = np.asarray(face_ids).astype(np.int64)
    ok = ids >= 0
    g = f[np.where(ok, ids, 0)]
    with np.errstate(all="ignore"):
        sq = np.array([_pair_sq(q[i][None, None], v[g[i, 0]][None, None], v[g[i, 1]][None, None], v[g[i, 2]][None, None])[0][0, 0]
                       if ok[i] else np.nan for i in range(len(q))])
    return sq


def closest_points(verts, faces, face_ids, bary, dtype=F64):
    """(P,3) the points ``sum_k bary_k vertex_k`` of the given faces (0 where the id is < 0)."""
    v, f = np.asarray(verts).astype(dtype), np.asarray(faces).astype(np.int64)
    ids = np.asarray(face_ids).astype(np.int64)
    g = f[np.where(ids >= 0, ids, 0)]
    c = (np.asarray(bary).astype(dtype)[:, :, None] * v[g]).sum(axis=1)
    return np.where((ids >= 0)[:, None], c, dtype(0))


def gradient(points, verts, faces, st, g_dist, dtype=F64):
    """(d_points (P,3), d_verts (V,3)) of ``sum(g_dist * dist)`` from the statement ``st`` of :func:`surface_distance``, every operation
    in ``dtype``: float64 is the statement, float32 the same formula at the precision of the outputs (the yardstick of the device bar)."""
    q, v, f = np.asarray(points).astype(dtype), np.asarray(verts).astype(dtype), np.asarray(faces).astype(np.int64)
    g = np.asarray(g_dist).astype(dtype)
    st = dict(st, bary=st["bary"].astype(dtype), dist=st["dist"].astype(dtype))
    c = closest_points(v, faces, st["face"], st["bary"], dtype)
    d = q - c
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(d, d))
        ok = (st["face"] >= 0) & np.isfinite(st["dist"]) & (ln > 0)
        n = np.where(ok[:, None], np.sign(st["dist"])[:, None] * d / np.where(ok, ln, dtype(1))[:, None], dtype(0))
    d_points = g[:, None] * n
    d_verts = np.zeros_like(v)
    ids = f[np.where(ok, st["face"], 0)]
    for k in range(3):
        np.add.at(d_verts, ids[ok, k], -(st["bary"][ok, k] * g[ok])[:, None] * n[ok])
    return d_points, d_verts


def vertex_distance(points, verts):
    """(P,) the distance to the nearest VERTEX: what the contact metrics of row (f)7 call ``near``."""
    d = np.asarray(points).astype(F64)[:, None, :] - np.asarray(verts).astype(F64)[None, :, :]
    with np.errstate(all="ignore"):
        sq = np.where(np.isnan(_dot(d, d)), np.inf, _dot(d, d))
    return np.sqrt(sq.min(axis=1))


def _same(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check_against_statement(c, st, got, dist_tol, bary_tol, what=""):
    """The checks of a distance result ``got`` (dist, face, bary) against the statement ``st`` of case ``c``; returns the worst
    |dist| and weight deviations."""
    nan = np.isnan(st["dist"])
    assert _same(np.isnan(got["dist"]), nan) and (got["face"][nan] == -1).all() and not got["bary"][nan].any(), what
    ok = ~nan
    assert (np.signbit(got["dist"][ok]) == np.signbit(st["dist"][ok])).all(), what                       # signs EXACT
    worst_d = float(np.abs(np.abs(got["dist"][ok]) - np.abs(st["dist"][ok])).max()) if ok.any() else 0.0
    assert worst_d <= dist_tol, (what, worst_d)
    assert ((got["face"][ok] >= 0) & (got["face"][ok] < c.F_dist)).all(), what
    # the face condition: the statement's distance from the query to the face named equals the statement's minimum
    sq = distance_to_face(c.points[ok], c.verts, c.faces, got["face"][ok])
    assert np.abs(np.sqrt(sq) - np.abs(st["dist"][ok])).max() <= dist_tol if ok.any() else True, what
    same = ok & (got["face"] == st["face"])
    worst_w = float(np.abs(got["bary"][same] - st["bary"][same]).max()) if same.any() else 0.0
    assert worst_w <= bary_tol, (what, worst_w)
    assert np.abs(got["bary"][ok].sum(axis=1) - 1).max() <= 1e-12 if ok.any() else True, what
    # where the closest point is unique, the two closest points are one point whichever face names it
    pts = closest_points(c.verts, c.faces, got["face"], got["bary"]), closest_points(c.verts, c.faces, st["face"], st["bary"])
    n = len(c.known or ())                  # the known answers come first: some of them are ties between two closest points
    free = ok & (np.arange(len(ok)) >= n)
    if free.any():
        assert np.abs(pts[0][free] - pts[1][free]).max() <= bary_tol, what
    assert _same(got["dist"][:n], st["dist"][:n]) and _same(got["face"][:n], st["face"][:n]) and _same(got["bary"][:n], st["bary"][:n]), what
    return worst_d, worst_w


# ------------------------------------------------------------------------------------------------------------------ meshes
def close_faces(faces, n_verts):
    from ihmr_amd.sdf import close_boundary
    return np.ascontiguousarray(close_boundary(np.asarray(faces), n_verts), np.int32)


@functools.lru_cache(maxsize=None)
def hand_faces(kind):
    """((F_total,3) closed right table, closed left table) int32 of the synthetic hand ``kind``; F_dist = 1538 for both."""
    from ihmr_amd.assets import synthetic_mano
    return tuple(close_faces(synthetic_mano(r, kind=kind)["faces"], NV) for r in (True, False))


CUBE_VERTS = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F32)      # id = x + 2 y + 4 z
# the x = 1 side is cut along y + z = 1, the others along the diagonal through their lowest vertex
CUBE_FACES = np.array([[0, 2, 3], [0, 3, 1],          # z = 0
                       [4, 5, 7], [4, 7, 6],          # z = 1
                       [0, 1, 5], [0, 5, 4],          # y = 0
                       [2, 6, 7], [2, 7, 3],          # y = 1
                       [0, 4, 6], [0, 6, 2],          # x = 0
                       [1, 3, 5], [3, 7, 5]], np.int32)   # x = 1: diagonal 3-5
# query, dist, face, weights: dyadic coordinates, every answer exact (the roots are the correctly rounded ones)
CUBE_KNOWN = [
    ((0.5, 0.25, 1.5), 0.5, 2, (0.5, 0.25, 0.25)),                     # face region of (4, 5, 7), outside
    ((1.5, 1.5, 0.5), np.sqrt(0.5), 7, (0.0, 0.5, 0.5)),               # edge 3-7, shared by faces 7 and 11: the lower id
    ((2.0, 2.0, 2.0), np.sqrt(3.0), 2, (0.0, 0.0, 1.0)),               # vertex 7: faces 2, 3, 6, 7, 11
    ((-1.0, -0.5, -0.25), np.sqrt(1.3125), 0, (1.0, 0.0, 0.0)),        # vertex 0
    ((0.5, 0.25, 0.875), -0.125, 2, (0.5, 0.25, 0.25)),                # inside, under the z = 1 side
    ((0.875, 0.875, 0.5), -0.125, 7, (0.125, 0.5, 0.375)),             # inside, the y = 1 and x = 1 sides tie: the lower id (2, 7, 3)
    ((0.75, -0.25, 0.5), 0.25, 4, (0.25, 0.25, 0.5)),                  # face region of (0, 1, 5)
    ((0.25, 0.5, 0.375), -0.25, 9, (0.5, 0.375, 0.125)),               # inside, nearest the x = 0 side
]


def icosphere(level=2, radius=1.0):
    """(verts float32, faces int32) of an icosahedron subdivided ``level`` times: 2 -> 162 vertices, 320 faces."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(x, F64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(F32), np.array(f, np.int32)


def sphere_bounds(verts, faces):
    """(r_in, r_out) of a polyhedron around the origin: every point of its surface has r_in <= |x| <= r_out."""
    v = np.asarray(verts).astype(F64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    return float(np.abs(_dot(a, n) / np.sqrt(_dot(n, n))).min()), float(np.sqrt(_dot(v, v)).max())


# ------------------------------------------------------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, points, verts, faces, F_dist, scale=1.0, known=None, hand=False):
        self.name, self.points, self.verts = name, np.ascontiguousarray(points, F32), np.ascontiguousarray(verts, F32)
        self.faces, self.F_dist, self.scale, self.known, self.hand = np.ascontiguousarray(faces, np.int32), int(F_dist), F32(scale), known, hand

    @property
    def shape(self):
        return len(self.points), len(self.verts), len(self.faces), self.F_dist


def _shell(rng, n, lo, hi):
    """n points with a norm in [lo, hi], directions uniform."""
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))


SIZES = (1, 255, 256, 257, 778, 1025)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case."""
    import contact_cases as CT
    t = OrderedDict()

    def add(name, *a, **kw):
        t[name] = Case(name, *a, **kw)

    for name, (r, l) in CT.gt_pairs().items():
        fr, fl = hand_faces("fingers" if name.startswith("fingers") else "mitten")
        add(f"{name}_r_on_l", r, l, fl, NF, hand=True)
        add(f"{name}_l_on_r", l, r, fr, NF, hand=True)
    r, l = CT.gt_pairs()["deep_0"]
    fr, fl = hand_faces("mitten")
    add("scale_1p7", r, l, fl, NF, scale=1.7, hand=True)
    add("scale_0p25", r, l, fl, NF, scale=0.25, hand=True)
    add("apart_1m", r, l + F32([1.0, 0.0, 0.0]), fl, NF, hand=True)
    add("shifted_2m", r + F32(2.0), l + F32(2.0), fl, NF, hand=True)
    add("open_mesh", r, l, fl[:NF], NF, hand=True)                                       # no cap faces: F_dist = F_total
    # queries around the middle of the left hand's wrist opening: the cap is the nearest triangle, and it is not skin
    loop = np.unique(fl[NF:])
    rng = np.random.RandomState(8150)
    add("cap_probe", l[loop].astype(F64).mean(axis=0) + rng.uniform(-0.004, 0.004, (64, 3)), l, fl, NF)
    q = np.array([k[0] for k in CUBE_KNOWN], F32)
    add("cube", q, CUBE_VERTS, CUBE_FACES, 12, known=CUBE_KNOWN)
    # the cube with three faces that do not count put in FRONT of it (ids shift by 3), and a NaN query at the end
    bad_v = np.concatenate([CUBE_VERTS, F32([[np.nan, 0.5, 0.5], [0.5, 0.5, 3.0]])])
    bad_f = np.concatenate([np.array([[0, 1, 1], [0, 1, 10], [0, 8, 3]], np.int32), CUBE_FACES, np.array([[2, -1, 3], [0, 9, 9]], np.int32)])
    known = [(k[0], k[1], k[2] + 3, k[3]) for k in CUBE_KNOWN] + [((0.5, np.nan, 0.5), np.nan, -1, (0.0, 0.0, 0.0)),
                                                                   ((np.inf, 0.5, 0.5), np.nan, -1, (0.0, 0.0, 0.0))]
    add("cube_bad_faces", np.array([k[0] for k in known], F32), bad_v, bad_f, 15, known=known)
    add("nothing_usable", q[:3], bad_v, bad_f[:3], 3, known=[(tuple(x), np.nan, -1, (0.0, 0.0, 0.0)) for x in q[:3]])
    tet_v = F32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    known = [((-1.0, -1.0, -1.0), np.sqrt(3.0), 0, (1.0, 0.0, 0.0)),
             ((0.125, 0.25, 0.0625), -0.0625, 0, (0.625, 0.25, 0.125)),                  # inside, nearest the z = 0 side
             ((0.25, 0.25, -0.5), 0.5, 0, (0.5, 0.25, 0.25)),
             ((2.0, -1.0, -1.0), np.sqrt(3.0), 0, (0.0, 0.0, 1.0))]                      # vertex 1: faces 0, 1, 3
    rng = np.random.RandomState(8101)
    add("tetrahedron", np.concatenate([F32([k[0] for k in known]), rng.uniform(-0.5, 1.5, (60, 3)).astype(F32)]), tet_v, tet_f, 4, known=known)
    sv, sf = icosphere(2, 0.5)
    r_in, r_out = sphere_bounds(sv, sf)
    for i, P in enumerate(SIZES):
        rng = np.random.RandomState(8200 + i)
        n_in = P // 2
        pts = np.concatenate([_shell(rng, n_in, 0.05, r_in - 0.01), _shell(rng, P - n_in, r_out + 0.01, 1.5)])
        add(f"sphere_P{P}", pts[rng.permutation(P)], sv, sf, len(sf))
    return t


_ST = {}


def statement(name):
    """:func:`surface_distance` of one case, computed once and shared by every test."""
    if name not in _ST:
        c = cases()[name]
        _ST[name] = surface_distance(c.points, c.verts, c.faces, c.F_dist)
    return _ST[name]


def margin_violations():
    """[(case, what, value)]: rays within RAY_MARGIN of an edge or a plane, hand distances within THR_MARGIN of a threshold."""
    bad = []
    for name, c in cases().items():
        st = statement(name)
        if st["margin"] < RAY_MARGIN:
            bad.append((name, "ray", st["margin"]))
        if c.hand:
            d = st["dist"] / F64(c.scale)
            for table in TABLES.values():
                near = np.abs(d[:, None] - np.asarray(table)[None, :])
                if np.nanmin(near) < THR_MARGIN:
                    bad.append((name, "threshold", float(np.nanmin(near))))
    return bad


# ------------------------------------------------------------------------------------------------------------------ an Evaluator batch
EVAL_PAIRS = ("deep_0", "default_1", "fingers_0", "deep_2", "default_0", "deep_1", "default_2")      # sample 2 is of the other asset
EVAL_SCALES = (1.0, 1.7, 1.0, 0.25, 1.0, 1.0, 1.3)
EVAL_WEIGHTS = ((1, 1), (1, 1), (1, 1), (1, 0), (1, 1), (1e-8, 1), (1, 1))
EVAL_KEEP = (True, False, True, True, True, True, True)
EVAL_INTER = (True, True, True, True, False, True, True)
EVAL_MITTEN = tuple(b for b, n in enumerate(EVAL_PAIRS) if not n.startswith("fingers"))
NOISE = 0.002


@functools.lru_cache(maxsize=None)
def evaluator_batch():
    """dict(pred_right, pred_left, gt_right, gt_left (B,778,3) float32, weight (B,2), scale (B), keep, inter (B) bool) of the mitten
    samples of the table above: prediction = ground truth + 2 mm of seeded noise."""
    import contact_cases as CT
    rows = EVAL_MITTEN
    gt = [CT.gt_pairs()[EVAL_PAIRS[b]] for b in rows]
    pred = []
    for b, (r, l) in zip(rows, gt):
        rng = np.random.RandomState(8300 + b)
        pred.append(((r + rng.normal(0, NOISE, r.shape)).astype(F32), (l + rng.normal(0, NOISE, l.shape)).astype(F32)))
    pick = lambda seq: np.array([seq[b] for b in rows])
    return dict(pred_right=np.stack([p[0] for p in pred]), pred_left=np.stack([p[1] for p in pred]), gt_right=np.stack([g[0] for g in gt]),
                gt_left=np.stack([g[1] for g in gt]), weight=pick(EVAL_WEIGHTS).astype(F32), scale=pick(EVAL_SCALES).astype(F32),
                keep=pick(EVAL_KEEP).astype(bool), inter=pick(EVAL_INTER).astype(bool))


@functools.lru_cache(maxsize=None)
def evaluator_distances():
    """(pred (B,1556), gt (B,1556)) float64: each hand's vertices against the other hand's closed mesh, right hand first."""
    e = evaluator_batch()
    fr, fl = hand_faces("mitten")
    out = []
    for r, l in ((e["pred_right"], e["pred_left"]), (e["gt_right"], e["gt_left"])):
        out.append(np.stack([np.concatenate([surface_distance(r[b], l[b], fl, NF)["dist"], surface_distance(l[b], r[b], fr, NF)["dist"]])
                             for b in range(len(r))]))
    return tuple(out)


def expected_surface_sums(table, rows=None, with_gt=True, scale=None):
    """The vector ``Evaluator.surface_sums()`` is to return for the rows of :func:`evaluator_batch`: [sum of max, sum of mean (mm),
    inside vertices, samples counted, samples counted with GT, (tp, pp, gp) x K].  ``scale``: one value in place of the samples' own."""
    e = evaluator_batch()
    dp, dg = evaluator_distances()
    thr = np.asarray(table, F64)
    s = np.zeros(5 + 3 * len(thr))
    for b in (range(len(dp)) if rows is None else rows):
        if not (e["keep"][b] and e["inter"][b]):
            continue
        sc = F64(e["scale"][b] if scale is None else scale)
        depth = np.where(dp[b] < 0, -dp[b], 0.0) / sc
        s[0] += depth.max() * 1000
        s[1] += depth.mean() * 1000
        s[2] += (dp[b] < 0).sum()
        s[3] += 1
        if with_gt and e["weight"][b, 0] > 0 and e["weight"][b, 1] > 0:
            s[4] += 1
            ip, ig = dp[b][None, :] / sc < thr[:, None], dg[b][None, :] / sc < thr[:, None]
            s[5:] += np.stack([(ip & ig).sum(axis=1), ip.sum(axis=1), ig.sum(axis=1)], axis=1).reshape(-1)
    return s


def evaluator_threshold_violations():
    e = evaluator_batch()
    bad = []
    for which, d in zip(("pred", "gt"), evaluator_distances()):
        for table in TABLES.values():
            near = np.abs((d / e["scale"].astype(F64)[:, None])[:, :, None] - np.asarray(table)[None, None, :])
            if near.min() < THR_MARGIN:
                bad.append((which, float(near.min())))
    return bad


if __name__ == "__main__":       # prints what violates the margins (nothing, as committed) and the cases' figures
    print("margin violations:", margin_violations(), evaluator_threshold_violations())
    for name, c in cases().items():
        st = statement(name)
        d = st["dist"]
        with np.errstate(all="ignore"):
            print(f"{name:20s} P {c.shape[0]:4d} V {c.shape[1]:4d} F {c.shape[3]:4d}|{c.shape[2] - c.shape[3]:2d}  inside {(d < 0).sum():4d}  "
                  f"deepest {(np.nanmin(d) if np.isfinite(d).any() else np.nan) * 1000:8.3f} mm  ray margin {st['margin']:.2e}")

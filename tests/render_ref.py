"""numpy restatement of the mesh renderer (``ihmr_amd/csrc/render_pure.h``), the oracle of tests/test_render_cpu.py (against a g++
build of the header) and tests/test_gpu_render.py (against the kernels).  Like tests/augment_ref.py it restates the operation order of
the header, one IEEE binary32 operation per numpy operation, so that all three agree bit for bit.

PARITY UNPINNED: the reference renders through OpenDR (utils/render_color_utils.py, utils/vis_util.py), which is not available; what
its own code computes before it calls OpenDR is pinned by tests/golden/render.npz, the pixel arithmetic here is this build's decision
(DESIGN.md section 2).  Every constant is a float32 before it meets an array."""
import numpy as np

f32 = np.float32
SUB = 256
MAX_PX = f32(16384.0)
NEAR = f32(0.1)
FOCAL = f32(5.0)
BAD = np.iinfo(np.int32).min
DISC = (3, 3, 2, 1)                     # half-widths of the filled radius-3 disc on rows |dy| = 0..3


def lights():
    """The three lights of simple_renderer (render_color_utils.py:171-196): positions times Ry(120 deg) in float64, then float32."""
    a = np.radians(120)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    pos = np.stack([np.dot(np.array(p, np.float64), ry) for p in ([-200, -100, -100], [800, 10, 300], [-500, 500, 1000])])
    col = np.stack([np.array([1.0, 1.0, 1.0]), np.array([1.0, 1.0, 1.0]), np.array([0.7, 0.7, 0.7])])
    return pos.astype(f32), col.astype(f32)


def build_csr(faces, n_verts):
    """Per vertex its incident faces in ascending face index: offsets (n_verts+1), ids (3 n_faces)."""
    faces = np.asarray(faces, np.int64)
    flat_v = faces.reshape(-1)
    flat_f = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    order = np.lexsort((flat_f, flat_v))
    off = np.zeros(n_verts + 1, np.int64)
    np.add.at(off, flat_v + 1, 1)
    return np.cumsum(off).astype(np.int32), flat_f[order].astype(np.int32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalise(a):
    a = np.asarray(a, f32)
    s = dot(a, a)
    with np.errstate(all="ignore"):
        out = a / np.sqrt(s)[..., None]
    return np.where((s == 0)[..., None], f32(0), out).astype(f32)


def vertex_normals(verts, faces, csr=None):
    verts = np.asarray(verts, f32)
    faces = np.asarray(faces, np.int64)
    off, ids = csr if csr is not None else build_csr(faces, verts.shape[0])
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    a, b = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        cr = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    n = np.zeros_like(verts)
    deg = off[1:] - off[:-1]
    for r in range(int(deg.max()) if len(deg) else 0):          # the r-th incident face of every vertex that has one: ascending order kept
        has = np.nonzero(deg > r)[0]
        with np.errstate(all="ignore"):
            n[has] = n[has] + cr[ids[off[has] + r]]
    return normalise(n)


def shade(normals, p, albedo, light=None):
    """albedo (nV,3) per vertex; p camera-space positions."""
    pos, col = light if light is not None else lights()
    acc = np.zeros_like(p)
    with np.errstate(all="ignore"):
        for l in range(3):
            d = normalise(pos[l][None, :] - p)
            t = dot(normals, d)
            t = np.where(t > 0, t, f32(0)).astype(f32)
            acc = acc + col[l][None, :] * t[:, None]
        v = np.asarray(albedo, f32) * acc
        return np.where(~(v > 0), f32(0), np.where(v > 1, f32(1), v)).astype(f32)


def cam_ok(s):
    s = f32(s)
    return bool(np.isfinite(s) and s > 0)


def translate(verts, cam):
    cam = np.asarray(cam, f32)
    tz = FOCAL / cam[0]
    return (np.asarray(verts, f32) + np.array([cam[1], cam[2], tz], f32)[None, :]).astype(f32)


def project(p, S):
    half = f32(0.5) * f32(S)
    F = half * FOCAL
    with np.errstate(all="ignore"):
        u = (F * p[:, 0]) / p[:, 2] + half
        v = (F * p[:, 1]) / p[:, 2] + half
        ok = (p[:, 2] >= NEAR) & (np.abs(u) <= MAX_PX) & (np.abs(v) <= MAX_PX)
        X = np.where(ok, np.rint(np.where(ok, u, 0) * f32(SUB)), BAD).astype(np.int64).astype(np.int32)
        Y = np.where(ok, np.rint(np.where(ok, v, 0) * f32(SUB)), 0).astype(np.int64).astype(np.int32)
        iz = np.where(ok, f32(1) / np.where(ok, p[:, 2], f32(1)), f32(0)).astype(f32)
    return X, Y, iz, ok


def rasterise(X, Y, iz, colours, faces, S, background=None, face_mask=None):
    """The z-buffered image of the prepared vertices: (S,S,3) uint8, (S,S) int32 face ids (-1 = none)."""
    faces = np.asarray(faces, np.int64)
    best_w = np.zeros((S, S), f32)
    best_id = np.full((S, S), -1, np.int32)
    img = np.full((S, S, 3), 255, np.uint8) if background is None else np.array(background, np.uint8).copy()
    for f in range(faces.shape[0]):
        if face_mask is not None and not face_mask[f]:
            continue
        i = faces[f]
        if np.any(i < 0) or np.any(i >= X.shape[0]) or np.any(X[i] == BAD):
            continue
        x = [int(X[k]) for k in i]
        y = [int(Y[k]) for k in i]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area == 0:
            continue
        s = 1 if area > 0 else -1
        c0, c1 = max(-(-min(x) // SUB), 0), min(max(x) // SUB, S - 1)
        r0, r1 = max(-(-min(y) // SUB), 0), min(max(y) // SUB, S - 1)
        if c0 > c1 or r0 > r1:
            continue
        px = (np.arange(c0, c1 + 1, dtype=np.int64) * SUB)[None, :]
        py = (np.arange(r0, r1 + 1, dtype=np.int64) * SUB)[:, None]
        cover = np.ones((r1 - r0 + 1, c1 - c0 + 1), bool)
        q = []
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            dx, dy = s * (x[k2] - x[k1]), s * (y[k2] - y[k1])
            owns = dy < 0 or (dy == 0 and dx > 0)
            e = dx * (py - y[k1]) - dy * (px - x[k1])
            cover &= (e > 0) | ((e == 0) & owns)
            q.append((e.astype(f32) / f32(s * area)) * iz[i[k]])
        if not cover.any():
            continue
        w = (q[0] + q[1]) + q[2]
        bw, bi = best_w[r0:r1 + 1, c0:c1 + 1], best_id[r0:r1 + 1, c0:c1 + 1]
        win = cover & ((w > bw) | ((w == bw) & (f < bi)))
        if not win.any():
            continue
        bw[win] = w[win]
        bi[win] = f
        sub = img[r0:r1 + 1, c0:c1 + 1]
        for ch in range(3):
            with np.errstate(all="ignore"):
                c = ((q[0] * colours[i[0], ch] + q[1] * colours[i[1], ch]) + q[2] * colours[i[2], ch]) / w
                byte = np.minimum((np.where(win, c, 0) * f32(255)).astype(np.int32), 255)
            sub[..., ch][win] = byte[win].astype(np.uint8)
    return img, best_id


def render_sample(verts, faces, cam, S, albedo, face_split, present=(1, 1), background=None, csr=None, light=None):
    """One sample as ihmr_render_meshes draws it: verts (nV,3) merged, albedo (2,3) per hand, faces < face_split are hand 0."""
    verts = np.asarray(verts, f32)
    faces = np.asarray(faces, np.int64)
    nV = verts.shape[0]
    bg = None if background is None else np.asarray(background, np.uint8)
    if not cam_ok(np.asarray(cam, f32)[0]):
        return (np.full((S, S, 3), 255, np.uint8) if bg is None else bg.copy()), np.full((S, S), -1, np.int32)
    csr = csr if csr is not None else build_csr(faces, nV)
    off, ids = csr
    hand = np.zeros(nV, np.int64)
    has = off[1:] > off[:-1]
    hand[has] = ids[off[:-1][has]] >= face_split
    n = vertex_normals(verts, faces, csr)
    p = translate(verts, cam)
    colours = shade(n, p, np.asarray(albedo, f32)[hand], light)
    X, Y, iz, _ = project(p, S)
    mask = np.where(np.arange(faces.shape[0]) < face_split, bool(present[0]), bool(present[1]))
    return rasterise(X, Y, iz, colours, faces, S, bg, mask)


def draw_keypoints(img, kps, weight, colour):
    """In place on (S,S,3) uint8: kps (K,2) float32 in [-1,1], weight (K)."""
    S = img.shape[0]
    kps = np.asarray(kps, f32)
    for k in range(kps.shape[0]):
        if not (np.asarray(weight, f32)[k] > 0) or not np.all(np.abs(kps[k]) < f32(1.0e6)):
            continue
        cx, cy = (int(((kps[k, a] + f32(1)) * f32(0.5)) * f32(S)) for a in (0, 1))
        for dy in range(-3, 4):
            for dx in range(-DISC[abs(dy)], DISC[abs(dy)] + 1):
                x, y = cx + dx, cy + dy
                if 0 <= x < S and 0 <= y < S:
                    img[y, x] = colour
    return img

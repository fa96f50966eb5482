"""numpy restatement of the rotated views and the penetration heat map of the mesh renderer (``rnd_view_point``, ``rnd_bbox_mid``,
``rnd_heat_colour`` of ``ihmr_amd/csrc/render_pure.h``), built on tests/render_ref.py: the oracle of tests/test_render_views_cpu.py
(against a g++ build of the header) and tests/test_gpu_render_views.py (against the kernels).  One IEEE binary32 operation per numpy
operation, in the header's bracketing, so that all three agree bit for bit.

Deviations from the reference (``SMPLRenderer.rotated``, ``get_alpha``; utils/vis_util.py:159-188,258-275): the
default pivot is the middle of the bounding box of the drawn hands' finite vertices, not the vertex mean; alpha is 255 where a face is
visible, not where the pixel is not white."""
import functools

import numpy as np

import render_ref as R

f32 = np.float32
VIEWS = (("y", 90), ("y", -90), ("x", 90), ("y", 180), ("z", 37))


def view_rotation(axis, deg):
    """cv2.Rodrigues of a turn about one coordinate axis, written out ('y', 'x', anything else = z), float64."""
    c, s = np.cos(np.radians(float(deg))), np.sin(np.radians(float(deg)))
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def view_points(p, c, rot):
    """q = (p - c) R + c for (n,3) points: q_j = ((d0 R[0][j] + d1 R[1][j]) + d2 R[2][j]) + c_j."""
    p, c, rot = np.asarray(p, f32), np.asarray(c, f32), np.asarray(rot, f32)
    with np.errstate(all="ignore"):
        d = p - c[None, :]
        q = [((d[:, 0] * rot[0, j] + d[:, 1] * rot[1, j]) + d[:, 2] * rot[2, j]) + c[j] for j in range(3)]
    return np.stack(q, 1).astype(f32)


def _extreme(x, low):
    """Minimum (low) or maximum of a non-empty finite float32 vector with -0 ordered below +0."""
    m = x.min() if low else x.max()
    if m == 0:
        neg = np.signbit(x[x == 0])
        m = f32(-0.0) if (neg.any() if low else neg.all()) else f32(0.0)
    return f32(m)


def bbox_mid(verts, n_split, present=(1, 1)):
    """The default pivot: 0.5 * (min + max) per axis over the finite vertices of the hands that are drawn; zeros when there is none."""
    verts = np.asarray(verts, f32)
    v = np.arange(verts.shape[0])
    take = np.where(v < n_split, bool(present[0]), bool(present[1])) & np.isfinite(verts).all(1)
    if not take.any():
        return np.zeros(3, f32)
    sel = verts[take]
    return np.array([f32(0.5) * (_extreme(sel[:, a], True) + _extreme(sel[:, a], False)) for a in range(3)], f32)


def heat_entry(n_verts, n_split, layout):
    """Per vertex the depth entry it reads."""
    v = np.arange(n_verts)
    return v if layout == 0 else np.where(v < n_split, n_split + v, v - n_split)


def heat_colours(depth, albedo, hot, lo, hi, n_split, layout):
    """depth (nV), albedo (2,3) -> (nV,3)."""
    depth, albedo, hot, lo, hi = np.asarray(depth, f32), np.asarray(albedo, f32), np.asarray(hot, f32), f32(lo), f32(hi)
    nV = depth.shape[0]
    d = depth[heat_entry(nV, n_split, layout)]
    with np.errstate(all="ignore"):
        t = (d - lo) / (hi - lo)
        t = np.where(~(t > 0), f32(0), np.where(t > 1, f32(1), t)).astype(f32)
        base = albedo[(np.arange(nV) >= n_split).astype(np.int64)]
        return (base + t[:, None] * (hot[None, :] - base)).astype(f32)


def render_sample_painted(verts, faces, cam, S, vertex_albedo, face_split, present=(1, 1), background=None, csr=None):
    """One sample as ihmr_paint_meshes draws it: render_ref.render_sample with one albedo per vertex."""
    verts, faces = np.asarray(verts, f32), np.asarray(faces, np.int64)
    bg = None if background is None else np.asarray(background, np.uint8)
    if not R.cam_ok(np.asarray(cam, f32)[0]):
        return (np.full((S, S, 3), 255, np.uint8) if bg is None else bg.copy()), np.full((S, S), -1, np.int32)
    csr = csr if csr is not None else R.build_csr(faces, verts.shape[0])
    n = R.vertex_normals(verts, faces, csr)
    p = R.translate(verts, cam)
    colours = R.shade(n, p, np.asarray(vertex_albedo, f32))
    X, Y, iz, _ = R.project(p, S)
    mask = np.where(np.arange(faces.shape[0]) < face_split, bool(present[0]), bool(present[1]))
    return R.rasterise(X, Y, iz, colours, faces, S, bg, mask)


def render_sample_view(verts, faces, cam, S, albedo, face_split, n_split, rot, pivot=None, present=(1, 1), background=None, csr=None,
                       vertex_albedo=None):
    """One sample turned by ``rot`` (3,3) about ``pivot`` (default: bbox_mid of the drawn hands) and drawn with its own camera."""
    c = bbox_mid(verts, n_split, present) if pivot is None else np.asarray(pivot, f32)
    turned = view_points(verts, c, np.asarray(rot, np.float64).astype(f32))
    if vertex_albedo is not None:
        return render_sample_painted(turned, faces, cam, S, vertex_albedo, face_split, present, background, csr)
    return R.render_sample(turned, faces, cam, S, albedo, face_split, present, background, csr)


@functools.lru_cache(maxsize=None)
def view_reference(name, view):
    """(B,S,S,3) images on WHITE and (B,S,S) face ids of a scene of tests/render_cases.py under ``view`` = (axis, deg), about the default
    pivot; computed once per process, read-only."""
    import render_cases as RC
    sc, f = RC.scene(name), RC.faces()
    csr = R.build_csr(f, 1556)
    rot = view_rotation(*view)
    out = [render_sample_view(sc["verts"][b], f, sc["cam"][b], sc["S"], sc["albedo"][b], RC.SPLIT, 778, rot, None, sc["present"][b], None, csr)
           for b in range(sc["verts"].shape[0])]
    img, ids = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    img.setflags(write=False)
    ids.setflags(write=False)
    return img, ids

// Pure arithmetic of the mesh renderer (csrc/render.h inlines it) -- compilable for the HOST as well, like augment_pure.h: under hipcc
// `__host__ __device__`, under g++ ordinary inline functions (tests/test_render_cpu.py builds tests/render_host_driver.cpp with
// -fsanitize=address,undefined and compares every stage bit for bit with tests/render_ref.py).  It stands where the reference hands its
// scene to OpenDR's ColoredRenderer + three LambertianPointLights (utils/render_color_utils.py:46-66,162-198, utils/vis_util.py:78-88,
// 219-255); OpenDR is not available, so the pixel arithmetic below is THIS BUILD'S DECISION (PARITY UNPINNED) and
// the operation order written here is the specification.  Every float operation is a single IEEE binary32 +, -, *, / or sqrt
// (compile with -ffp-contract=off); sums are taken left to right as bracketed.
//
//   scene      tz = 5 / cam[0];  p = v + (cam[1], cam[2], tz);  F = (0.5 * S) * 5;  cx = cy = 0.5 * S
//   normal     n(v) = normalise( sum over incident faces, ascending face index, of (v1 - v0) x (v2 - v0) ), on the untranslated vertices;
//              normalise(a) = a / sqrt((ax*ax + ay*ay) + az*az), the zero vector when that sum of squares is 0
//   shading    c[ch] = clamp01( albedo[ch] * (((0 + col0[ch]*d0) + col1[ch]*d1) + col2[ch]*d2) ),  d_l = max(n . normalise(L_l - p), 0),
//              a . b = (ax*bx + ay*by) + az*bz;  max(d, 0) = d > 0 ? d : 0;  clamp01(c) = !(c > 0) ? 0 : (c > 1 ? 1 : c)
//   projection u = (F * px) / pz + cx, v likewise;  X = (int)rint(u * 256), Y = (int)rint(v * 256) (nearest even);  iz = 1 / pz;
//              a vertex is USABLE iff pz >= 0.1 and |u| <= 16384 and |v| <= 16384 (false for NaN); a face with an unusable vertex is skipped
//   coverage   2A = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0) in int64; 2A == 0 covers nothing; s = sign(2A).  Edge i runs from vertex i+1 to
//              vertex i+2 (mod 3), d = s * (end - start), E_i(P) = dx * (Py - Ystart) - dy * (Px - Xstart), P = (256 i, 256 j) for pixel
//              column i, row j.  The pixel is covered iff every E_i > 0, or E_i == 0 on an edge that owns its points: dy < 0, or dy == 0
//              and dx > 0 (top-left rule; an edge and its reverse never both own, so a shared edge is covered exactly once).
//   depth      l_i = (float)E_i / (float)|2A|;  w = (l0*iz0 + l1*iz1) + l2*iz2;  the visible face has the largest w, ties to the lowest index
//   colour     c[ch] = (((l0*iz0)*c0[ch] + (l1*iz1)*c1[ch]) + (l2*iz2)*c2[ch]) / w;  byte = min((int)(c * 255), 255)
//   keypoints  centre = (int)(((k + 1) * 0.5) * S) per axis (truncation); filled disc of half-widths 3, 3, 2, 1 on rows |dy| = 0..3
// Rotated views and the penetration heat map (ihmr_view_vertices / ihmr_heat_colours; tests/render_views_ref.py restates them):
//   view       d = p - c;  q[j] = ((d0*R[0][j] + d1*R[1][j]) + d2*R[2][j]) + c[j]: the row vector (p - c) times R, plus c, as
//              np.dot(verts - center, around) + center of SMPLRenderer.rotated (utils/vis_util.py:177-178).  (p - c) + c rounds, so the
//              identity matrix does not give p back: "no view" skips the transform, it is never an identity rotation
//   pivot      c = 0.5 * (mn + mx) per axis, mn / mx over the vertices of the hands that are drawn (vertex v belongs to hand 0 iff
//              v < n_split) whose three coordinates are all finite; c = 0 when there is none.  min and max order -0 below +0, so the
//              result is one float however the reduction is arranged (the reference takes verts.mean(axis=0): DESIGN.md section 8.1)
//   heat       t = (d - lo) / (hi - lo);  t = !(t > 0) ? 0 : (t > 1 ? 1 : t) (a NaN depth gives the base colour);
//              out[ch] = base[ch] + t * (hot[ch] - base[ch]);  under layout 1 vertex v reads the depth entry of rnd_heat_entry
// Nothing here touches memory other than its arguments.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ihmr_hip.h"

#if defined(__HIPCC__)
#define RND_PURE __host__ __device__ __forceinline__
#else
#define RND_PURE static inline
#endif

#define RND_SUBPIXEL 256               /* fixed-point steps per pixel */
#define RND_MAX_PX 16384.0f            /* |u|, |v| beyond this: the vertex is unusable */
#define RND_NEAR 0.1f
#define RND_FOCAL 5.0f
#define RND_BAD_COORD INT32_MIN        /* X of an unusable vertex */

// one shaded, projected vertex: what the vertex kernel leaves in the workspace (24 bytes)
typedef struct rnd_vertex { int32_t X, Y; float iz; float c[3]; } rnd_vertex;

// one face prepared for a tile: E_i(col, row) + bias_i = A[i] * (256 col) + B[i] * (256 row) + C[i]
typedef struct rnd_face_rec {
    int64_t C[3];        // constant terms WITH the fill-rule bias folded in (E_i - 1 on an edge that does not own its points)
    int32_t A[3], B[3];
    float area2;         // (float)|2A|
    float iz[3];
    int32_t id;
    int32_t unbias;      // bit i: C[i] holds E_i - 1
} rnd_face_rec;          // 72 bytes

RND_PURE void rnd_cross_face(const float* v0, const float* v1, const float* v2, float* n) {
    const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
    const float bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
    n[0] = ay * bz - az * by;
    n[1] = az * bx - ax * bz;
    n[2] = ax * by - ay * bx;
}

RND_PURE float rnd_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RND_PURE void rnd_normalise(float* a) {
    const float s = rnd_dot(a, a);
    if (s == 0.0f) { a[0] = a[1] = a[2] = 0.0f; return; }
    const float len = sqrtf(s);
    a[0] = a[0] / len; a[1] = a[1] / len; a[2] = a[2] / len;
}

RND_PURE int rnd_cam_ok(float s) { return s > 0.0f && s <= 3.4028234663852886e38f; }        // finite and positive (false for NaN)

// camera-space position of a vertex (scene set-up); the caller has checked rnd_cam_ok(cam[0])
RND_PURE void rnd_translate(const float* v, const float* cam, float* p) {
    const float tz = RND_FOCAL / cam[0];
    p[0] = v[0] + cam[1]; p[1] = v[1] + cam[2]; p[2] = v[2] + tz;
}

// Lambertian shading of one vertex: n the normalised normal, p the camera-space position, albedo (3) of its hand
RND_PURE void rnd_shade(const float* n, const float* p, const float* albedo, const ihmr_render_lights* L, float* c) {
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < 3; ++l) {
        float d[3] = {L->pos[l][0] - p[0], L->pos[l][1] - p[1], L->pos[l][2] - p[2]};
        rnd_normalise(d);
        float t = rnd_dot(n, d);
        t = t > 0.0f ? t : 0.0f;
        for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + L->color[l][ch] * t;
    }
    for (int ch = 0; ch < 3; ++ch) {
        const float v = albedo[ch] * acc[ch];
        c[ch] = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
    }
}

// projection + snap of a camera-space point; returns 0 (and X = RND_BAD_COORD) for an unusable vertex
RND_PURE int rnd_project(const float* p, int S, rnd_vertex* out) {
    const float half = 0.5f * (float)S, F = half * RND_FOCAL;
    const float u = (F * p[0]) / p[2] + half, v = (F * p[1]) / p[2] + half;
    const int ok = p[2] >= RND_NEAR && fabsf(u) <= RND_MAX_PX && fabsf(v) <= RND_MAX_PX;
    out->X = ok ? (int32_t)rintf(u * (float)RND_SUBPIXEL) : RND_BAD_COORD;
    out->Y = ok ? (int32_t)rintf(v * (float)RND_SUBPIXEL) : 0;
    out->iz = ok ? 1.0f / p[2] : 0.0f;
    return ok;
}

// edge set-up of one face from its three projected vertices; returns 0 when the face covers nothing (unusable vertex, zero area)
RND_PURE int rnd_face_setup(const rnd_vertex* a, const rnd_vertex* b, const rnd_vertex* c, int id, rnd_face_rec* r) {
    if (a->X == RND_BAD_COORD || b->X == RND_BAD_COORD || c->X == RND_BAD_COORD) return 0;
    const int64_t X[3] = {a->X, b->X, c->X}, Y[3] = {a->Y, b->Y, c->Y};
    const int64_t area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (area == 0) return 0;
    const int64_t s = area > 0 ? 1 : -1;
    r->unbias = 0;
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        const int64_t dx = s * (X[i2] - X[i1]), dy = s * (Y[i2] - Y[i1]);
        const int owns = dy < 0 || (dy == 0 && dx > 0);
        r->A[i] = (int32_t)(-dy);
        r->B[i] = (int32_t)dx;
        r->C[i] = dy * X[i1] - dx * Y[i1] - (owns ? 0 : 1);
        r->unbias |= owns ? 0 : (1 << i);
    }
    r->area2 = (float)(s * area);
    r->iz[0] = a->iz; r->iz[1] = b->iz; r->iz[2] = c->iz;
    r->id = id;
    return 1;
}

// the three biased edge values of a face at pixel (col, row): covered iff none is negative
RND_PURE void rnd_edges(const rnd_face_rec* r, int col, int row, int64_t* e) {
    const int64_t px = (int64_t)col * RND_SUBPIXEL, py = (int64_t)row * RND_SUBPIXEL;
    for (int i = 0; i < 3; ++i) e[i] = (int64_t)r->A[i] * px + (int64_t)r->B[i] * py + r->C[i];
}

// barycentrics (times 1/z) and the depth key of a covered pixel from its biased edge values
RND_PURE float rnd_weights(const rnd_face_rec* r, const int64_t* e, float* q) {
    for (int i = 0; i < 3; ++i) q[i] = ((float)(e[i] + ((r->unbias >> i) & 1)) / r->area2) * r->iz[i];
    return (q[0] + q[1]) + q[2];
}

RND_PURE int rnd_wins(float w, int id, float best_w, int best_id) { return w > best_w || (w == best_w && id < best_id); }

// one channel of the visible face's colour as a byte
RND_PURE int rnd_colour_byte(const float* q, float w, float c0, float c1, float c2) {
    const float c = ((q[0] * c0 + q[1] * c1) + q[2] * c2) / w;
    const int b = (int)(c * 255.0f);
    return b > 255 ? 255 : b;
}

// keypoints (vis_util.draw_keypoints): centre coordinate and the half-width of the filled radius-3 disc on row |dy|
RND_PURE int rnd_kp_ok(float k) { return fabsf(k) < 1.0e6f; }                       // false for NaN / infinities: (int) would be undefined
RND_PURE int rnd_kp_centre(float k, int S) { return (int)(((k + 1.0f) * 0.5f) * (float)S); }
RND_PURE int rnd_disc_half_width(int ady) { return ady <= 1 ? 3 : (ady == 2 ? 2 : (ady == 3 ? 1 : -1)); }

// ------------------------------------------------------------------------------------------ rotated views, penetration heat map
RND_PURE int rnd_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }              // false for NaN and the infinities
// minimum / maximum of two numbers (never NaN here) under the order that puts -0 below +0: commutative and associative
RND_PURE float rnd_min(float a, float b) { return (b < a || (b == a && __builtin_signbit(b))) ? b : a; }
RND_PURE float rnd_max(float a, float b) { return (b > a || (b == a && !__builtin_signbit(b))) ? b : a; }

// q = (p - c) R + c, R row major (R[3 * i + j])
RND_PURE void rnd_view_point(const float* p, const float* c, const float* R, float* q) {
    const float d0 = p[0] - c[0], d1 = p[1] - c[1], d2 = p[2] - c[2];
    for (int j = 0; j < 3; ++j) q[j] = ((d0 * R[j] + d1 * R[3 + j]) + d2 * R[6 + j]) + c[j];
}

// the bounding box of the default pivot: empty (mn > mx), one more vertex, two boxes merged, and the pivot of a box
RND_PURE void rnd_bbox_empty(float* mn, float* mx) {
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
}
RND_PURE void rnd_bbox_take(const float* p, float* mn, float* mx) {
    if (!(rnd_finite(p[0]) && rnd_finite(p[1]) && rnd_finite(p[2]))) return;
    for (int a = 0; a < 3; ++a) { mn[a] = rnd_min(mn[a], p[a]); mx[a] = rnd_max(mx[a], p[a]); }
}
RND_PURE void rnd_bbox_merge(const float* mn2, const float* mx2, float* mn, float* mx) {
    for (int a = 0; a < 3; ++a) { mn[a] = rnd_min(mn[a], mn2[a]); mx[a] = rnd_max(mx[a], mx2[a]); }
}
RND_PURE void rnd_bbox_centre(const float* mn, const float* mx, float* c) {
    const int any = mn[0] <= mx[0];                                                          // a box that took a vertex has mn <= mx on every axis
    for (int a = 0; a < 3; ++a) c[a] = any ? 0.5f * (mn[a] + mx[a]) : 0.0f;
}
// the default pivot of one sample: verts (n_verts,3), draw0 / draw1 say which hands are drawn
RND_PURE void rnd_bbox_mid(const float* verts, int n_verts, int n_split, int draw0, int draw1, float* c) {
    float mn[3], mx[3];
    rnd_bbox_empty(mn, mx);
    for (int v = 0; v < n_verts; ++v)
        if (v < n_split ? draw0 : draw1) rnd_bbox_take(verts + 3 * (size_t)v, mn, mx);
    rnd_bbox_centre(mn, mx, c);
}

// the depth entry vertex v reads: layout 0 its own; layout 1 the collision module's order (entry h * n_split + k was sampled at vertex
// k of hand 1 - h: include/ihmr_hip.h, ihmr_sdf_collision), which needs n_verts == 2 * n_split
RND_PURE int rnd_heat_entry(int v, int n_split, int layout) { return layout ? (v < n_split ? n_split + v : v - n_split) : v; }

RND_PURE void rnd_heat_colour(float d, float lo, float hi, const float* base, const float* hot, float* out) {
    float t = (d - lo) / (hi - lo);
    t = !(t > 0.0f) ? 0.0f : (t > 1.0f ? 1.0f : t);
    for (int ch = 0; ch < 3; ++ch) out[ch] = base[ch] + t * (hot[ch] - base[ch]);
}

// Pure arithmetic of the exact point-to-surface signed distance (csrc/surface.h inlines it) -- compilable for the HOST as well, like
// contact_pure.h and volume_pure.h: under hipcc `__host__ __device__`, under g++ ordinary inline functions (tests/test_surface_cpu.py
// builds tests/surface_host_driver.cpp with -fsanitize=address,undefined and compares every word with the float64 statement of
// tests/surface_ref.py).  float64 throughout on the float32 inputs, every operation a single IEEE binary64 +, -, *, / or sqrt (compile
// with -ffp-contract=off).
//
//   statement    A query q, a vertex array, one face table [surface faces 0..F_dist) | cap faces
//              F_dist..F_total).  The distance is taken to the surface faces, the sign over all faces.
//   usable     a face counts (for distance and sign) when its three ids lie in [0, V), its nine coordinates are finite and the squared
//              length of its normal n = (b - a) x (c - a), (nx*nx + ny*ny) + nz*nz, is not exactly 0  (srf_face_usable).
//   distance   the closest point of the closed triangle by the region method (Ericson, Real-Time Collision Detection 5.1.5), written
//              with p = q - a, e1 = b - a, e2 = c - a and the six products
//                  d1 = e1.p   d2 = e2.p   d3 = e1.(q - b)   d4 = e2.(q - b)   d5 = e1.(q - c)   d6 = e2.(q - c)
//              every dot product (x*x' + y*y') + z*z'.  The closest point is a + v e1 + w e2 with (v, w) from the FIRST rule that holds:
//                  d1 <= 0 and d2 <= 0                                    vertex a   v = 0, w = 0
//                  d3 >= 0 and d4 <= d3                                   vertex b   v = 1, w = 0
//                  vc = d1 d4 - d3 d2 <= 0, d1 >= 0, d3 <= 0              edge ab    v = d1 / (d1 - d3), w = 0
//                  d6 >= 0 and d5 <= d6                                   vertex c   v = 0, w = 1
//                  vb = d5 d2 - d1 d6 <= 0, d2 >= 0, d6 <= 0              edge ac    v = 0, w = d2 / (d2 - d6)
//                  va = d3 d6 - d5 d4 <= 0, d4 - d3 >= 0, d5 - d6 >= 0    edge bc    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
//                  otherwise                                              face       v = vb / ((va + vb) + vc), w = vc / ((va + vb) + vc)
//              weights (w_a, w_b, w_c) = ((1 - v) - w, v, w);  s = v e1 + w e2;  sq = evp_sq_dist(p, s) = |p - s|^2.
//              The minimum is taken on the squares, faces ascending, strict `<` (the lowest face id wins an exact tie, a NaN never
//              replaces the running minimum), one root at the end.
//   sign       parity of the +x ray over all usable faces: det = e1y e2z - e2y e1z; a face with det == 0 does not count;
//              u = (py e2z - e2y pz) / det, v = (e1y pz - py e1z) / det (two divisions); a crossing needs u >= 0, v >= 0, u + v <= 1
//              and (a_x + u e1x) + v e2x > q_x.  Odd parity: inside, dist = -sqrt(sq).
//   nothing    a query with a non-finite coordinate, or a mesh without a usable surface face: dist = NaN, face = -1, weights 0.
//   gradient   with c = (w_a a + w_b b) + w_c c and n = sign (q - c) / |q - c|: d dist / d q = n, d dist / d vertex_k = -w_k n for
//              the three vertices of the closest face; exactly 0 where |q - c| == 0 or dist is NaN  (srf_grad_dir).
// Nothing here touches memory other than its arguments.
#pragma once
#include "eval_pure.h"

#define SRF_MAX_VERTS 1024                // IHMR_SURFACE_MAX_VERTS: a vertex id has 10 bits in a packed face record
#define SRF_MAX_FACES 2048                // IHMR_SURFACE_MAX_FACES
#define SRF_THREADS 256
#define SRF_BWD_SLOTS 4                   // surface_dist_bwd_kernel: a thread owns the vertices tid + 256 k, k < 4
// LDS of surface_dist_kernel: the sample's vertices (float32 xyz) and its packed face records
#define SRF_LDS_BYTES (SRF_MAX_VERTS * 3 * 4 + SRF_MAX_FACES * 4)                                    // 20 480
// LDS of surface_dist_bwd_kernel: per query of a chunk of 256 the three vertex ids of its face, its three weights and g n (xyz)
#define SRF_BWD_LDS_BYTES (SRF_THREADS * 3 * 4 + SRF_THREADS * 3 * 8 + SRF_THREADS * 3 * 8)          // 15 360

#define SRF_FACE_USABLE (1u << 30)

EVP_PURE bool srf_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for NaN and +-Inf

EVP_PURE double srf_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// A face record of the kernels: the three vertex ids (10 bits each) | SRF_FACE_USABLE.  An unusable face is the record 0.
EVP_PURE unsigned srf_pack_face(unsigned ia, unsigned ib, unsigned ic) { return ia | (ib << 10) | (ic << 20) | SRF_FACE_USABLE; }
EVP_PURE void srf_unpack_face(unsigned r, int& ia, int& ib, int& ic) {
    ia = (int)(r & 1023u); ib = (int)((r >> 10) & 1023u); ic = (int)((r >> 20) & 1023u);
}

// The face-usable predicate on the coordinates (the caller has checked the ids against [0, V)).
EVP_PURE bool srf_face_usable(const double* a, const double* b, const double* c) {
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && srf_finite(a[k]) && srf_finite(b[k]) && srf_finite(c[k]);
    if (!finite) return false;
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    return (nx * nx + ny * ny) + nz * nz != 0.0;
}

// The squared distance from q to the closed triangle (a, b, c) and the weights (v, w) of its closest point a + v (b - a) + w (c - a).
EVP_PURE double srf_point_tri(const double* q, const double* a, const double* b, const double* c, double& v, double& w) {
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double px = q[0] - a[0], py = q[1] - a[1], pz = q[2] - a[2];
    const double d1 = srf_dot(e1x, e1y, e1z, px, py, pz), d2 = srf_dot(e2x, e2y, e2z, px, py, pz);
    const double bx = q[0] - b[0], by = q[1] - b[1], bz = q[2] - b[2];
    const double d3 = srf_dot(e1x, e1y, e1z, bx, by, bz), d4 = srf_dot(e2x, e2y, e2z, bx, by, bz);
    const double cx = q[0] - c[0], cy = q[1] - c[1], cz = q[2] - c[2];
    const double d5 = srf_dot(e1x, e1y, e1z, cx, cy, cz), d6 = srf_dot(e2x, e2y, e2z, cx, cy, cz);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; }
    else if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; }
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { v = d1 / (d1 - d3); w = 0.0; }
    else if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; }
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { v = 0.0; w = d2 / (d2 - d6); }
    else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) { w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w; }
    else { const double den = (va + vb) + vc; v = vb / den; w = vc / den; }
    const double sx = v * e1x + w * e2x, sy = v * e1y + w * e2y, sz = v * e1z + w * e2z;
    return evp_sq_dist(px, py, pz, sx, sy, sz);
}

// The three weights of the closest point from (v, w).
EVP_PURE void srf_weights(double v, double w, double* bary) { bary[0] = (1.0 - v) - w; bary[1] = v; bary[2] = w; }

// Does the +x ray from q cross the triangle (a, b, c)?
EVP_PURE bool srf_ray_crosses(const double* q, const double* a, const double* b, const double* c) {
    const double e1y = b[1] - a[1], e1z = b[2] - a[2], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double det = e1y * e2z - e2y * e1z;
    if (det == 0.0) return false;
    const double py = q[1] - a[1], pz = q[2] - a[2];
    const double u = (py * e2z - e2y * pz) / det;
    const double v = (e1y * pz - py * e1z) / det;
    if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0)) return false;
    return (a[0] + u * (b[0] - a[0])) + v * (c[0] - a[0]) > q[0];
}

// The running minimum over squared distances with its face: strict `<`, so the lowest face id wins a tie and a NaN never enters.
EVP_PURE bool srf_min_update(double& best, double sq) {
    if (sq < best) { best = sq; return true; }
    return false;
}

// What a query leaves: dist from the minimum square and the parity; NaN / -1 / 0 when there was no usable surface face (face < 0).
EVP_PURE double srf_finish(double best, int face, bool inside) {
    if (face < 0) return (double)NAN;
    const double d = sqrt(best);
    return inside ? -d : d;
}

// The gradient direction n = sign (q - c) / |q - c| from the closest face's vertices and weights; 0 where |q - c| == 0, where dist is
// NaN or where anything of it is not finite.
EVP_PURE void srf_grad_dir(const double* q, const double* a, const double* b, const double* c, const double* bary, double dist,
                           double* n) {
    n[0] = n[1] = n[2] = 0.0;
    if (dist != dist || dist == 0.0) return;
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = q[k] - ((bary[0] * a[k] + bary[1] * b[k]) + bary[2] * c[k]);
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(len > 0.0) || !srf_finite(len)) return;
    for (int k = 0; k < 3; ++k) n[k] = dist < 0.0 ? -(d[k] / len) : d[k] / len;
}

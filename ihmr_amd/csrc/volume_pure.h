// Pure arithmetic of the two-hand intersection volume (csrc/volume.h inlines it) -- compilable for the HOST as well, like render_pure.h
// and eval_pure.h: under hipcc `__host__ __device__`, under g++ ordinary inline functions (tests/test_volume_cpu.py builds
// tests/volume_host_driver.cpp with -fsanitize=address,undefined and compares every column word with the statement of
// tests/volume_ref.py).  float32 throughout, every operation a single IEEE binary32 operation (compile with -ffp-contract=off).
//
//   statement  ("intersection volume")  Two closed meshes A, B.  lo = max(min A, min B), hi = min(max A, max B)
//              per axis;  c = (lo + hi) * 0.5f, s = 0.5f * max_axis(hi - lo): the common cube.  It is cut into n^3 tiles (n = 1, 2, 4),
//              tile (tx, ty, tz) with off = (float)(2t + 1) / (float)n - 1.0f, centre ct = c + s * off, half side st = s / (float)n.
//              Both meshes are normalised into the tile's frame, vn = (v - ct) / st, and voxel (k, j, i) of the tile's 32^3
//              cell-centred grid is inside a mesh when the +x ray from its centre crosses an odd number of the mesh's triangles:
//              oracle/sdf_grid.c ray_hit_px, expression for expression (composed from ihmr_pure.h: sdf_tri_yz_det, sdf_ray_t).
//              count = the voxels inside both meshes.
//   status     0 counted | 1 empty (some hi <= lo) | 2 invalid (a non-finite vertex, or s < 1e-5).  Non-finite is looked at first,
//              then empty, then s.  A sample that is not counted has box 0 and count 0.
//   columns    A triangle is tested only against the grid columns (k, j) inside its yz bounding box + a margin.  The meshes reach
//              far outside the tile (normalised coordinates in the hundreds), so, unlike tri_col_range (ihmr_pure.h), the float is
//              clamped to [-4, 36] BEFORE the conversion to int (no undefined conversion for a far vertex over a small cube) and the
//              margin grows with the triangle: m = 1e-4 * max(1, L), L its larger yz extent.  Why: a column a distance d outside
//              the box has a real barycentric coordinate below -d / L; the float (u, v) of ray_hit_px carry an error of about
//              6 * 2^-24 * kappa with kappa = L^2 / |det| the triangle's shape factor, so the oracle can only count a column with
//              d <= 18 * 2^-24 * kappa * L ~ 1.1e-6 * kappa * L.  The margin covers kappa <= 90 (for L <= 1 it is tri_col_range's).
//   t > 0      sdf_ray_hits' loop-free mask (ihmr_pure.h) rests on |p - a| <= 2, a mesh inside its own box; that does not hold
//              here, so all 32 voxels of a column that passes the (u, v) test are evaluated with sdf_ray_t.
// Nothing here touches memory other than its arguments.
#pragma once
#include "ihmr_pure.h"

#define VOL_MAX_VERTS IHMR_VOLUME_MAX_VERTS      // 1024 per mesh: the tile-normalised vertices of both meshes sit in LDS
#define VOL_MAX_FACES IHMR_VOLUME_MAX_FACES      // 2048 per mesh: the list of both meshes' triangles sits in LDS
#define VOL_COLS (SDF_G * SDF_G)   // 1024 columns (k, j) of 32 voxels: one 32-bit word each
#define VOL_THREADS 256
#define VOL_S_MIN 1e-5f
// LDS of vol_count_kernel: vertices of both meshes, the two column tables, the list of (triangle, column range) records, 4 partial sums
// and the list length
#define VOL_LDS_BYTES (2 * VOL_MAX_VERTS * 3 * 4 + 2 * VOL_COLS * 4 + 2 * VOL_MAX_FACES * 4 + (VOL_THREADS / 64) * 4 + 4)

enum { VOL_COUNTED = 0, VOL_EMPTY = 1, VOL_INVALID = 2 };

IHMR_PURE bool vol_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN and +-Inf

struct VolCube { float c[3]; float s; int status; };

// the common cube of two vertex boxes; `finite`: every vertex of both meshes is finite
IHMR_PURE VolCube vol_cube(const float* min_a, const float* max_a, const float* min_b, const float* max_b, bool finite) {
    VolCube q;
    q.c[0] = q.c[1] = q.c[2] = q.s = 0.0f;
    if (!finite) { q.status = VOL_INVALID; return q; }
    float lo[3], hi[3];
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        lo[a] = fmaxf(min_a[a], min_b[a]);
        hi[a] = fminf(max_a[a], max_b[a]);
        empty = empty || hi[a] <= lo[a];
    }
    if (empty) { q.status = VOL_EMPTY; return q; }
    const float s = 0.5f * fmaxf(hi[0] - lo[0], fmaxf(hi[1] - lo[1], hi[2] - lo[2]));
    if (s < VOL_S_MIN) { q.status = VOL_INVALID; return q; }
    for (int a = 0; a < 3; ++a) q.c[a] = (lo[a] + hi[a]) * 0.5f;
    q.s = s;
    q.status = VOL_COUNTED;
    return q;
}

// tile t = (tz * n + ty) * n + tx of the cube (c, s): its centre and half side
struct VolTile { float c[3]; float s; };
IHMR_PURE VolTile vol_tile_frame(float cx, float cy, float cz, float s, int n, int tile) {
    const int t[3] = {tile % n, (tile / n) % n, tile / (n * n)};
    const float c[3] = {cx, cy, cz};
    VolTile f;
    for (int a = 0; a < 3; ++a) {
        const float off = (float)(2 * t[a] + 1) / (float)n - 1.0f;
        const float so = s * off;
        f.c[a] = c[a] + so;
    }
    f.s = s / (float)n;
    return f;
}
IHMR_PURE float vol_normalise(float v, float ct, float st) { return (v - ct) / st; }      // one subtraction, one IEEE division

// first / last grid index whose centre (2 idx + 1) / 32 - 1 lies in [vmin, vmax]: the float is clamped before the conversion
IHMR_PURE int vol_index_lo(float vmin) {
    const float f = fminf(fmaxf(ceilf((vmin + 1.0f) * 16.0f - 0.5f), -4.0f), 36.0f);
    return ihmr_imax(0, (int)f);
}
IHMR_PURE int vol_index_hi(float vmax) {
    const float f = fminf(fmaxf(floorf((vmax + 1.0f) * 16.0f - 0.5f), -4.0f), 36.0f);
    return ihmr_imin(SDF_G - 1, (int)f);
}
// columns (k, j) whose ray can cross the triangle; false when there is none
IHMR_PURE bool vol_col_range(float y0, float y1, float y2, float z0, float z1, float z2, int& j0, int& j1, int& k0, int& k1) {
    const float ylo = fminf(y0, fminf(y1, y2)), yhi = fmaxf(y0, fmaxf(y1, y2));
    const float zlo = fminf(z0, fminf(z1, z2)), zhi = fmaxf(z0, fmaxf(z1, z2));
    const float m = 1e-4f * fmaxf(1.0f, fmaxf(yhi - ylo, zhi - zlo));
    j0 = vol_index_lo(ylo - m);
    j1 = vol_index_hi(yhi + m);
    k0 = vol_index_lo(zlo - m);
    k1 = vol_index_hi(zhi + m);
    return j0 <= j1 && k0 <= k1;
}

// one triangle of a tile-normalised mesh, ready for its columns: ray_hit_px up to `inv`.  False: dropped (|det| < 1e-12).
struct VolTri { float ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z, inv; };
IHMR_PURE bool vol_tri_setup(const float* a, const float* b, const float* c, VolTri& t) {
    const float det = sdf_tri_yz_det(a[1], a[2], b[1], b[2], c[1], c[2]);
    if (fabsf(det) < 1e-12f) return false;
    t.ax = a[0]; t.ay = a[1]; t.az = a[2];
    t.e1x = b[0] - a[0]; t.e1y = b[1] - a[1]; t.e1z = b[2] - a[2];
    t.e2x = c[0] - a[0]; t.e2y = c[1] - a[1]; t.e2z = c[2] - a[2];
    t.inv = 1.0f / det;
    return true;
}

// hit mask of one (triangle, column) pair: bit i = the +x ray from voxel (k, j, i), col = k * 32 + j, crosses the triangle at t > 0.
// The comparisons are ray_hit_px's own (a NaN passes them and fails t > 0).
IHMR_PURE unsigned vol_column_hits(const VolTri& t, int col) {
    const int j = col & (SDF_G - 1), k = col >> 5;
    const float py = (float)(2 * j + 1) / (float)SDF_G - 1.0f;
    const float pz = (float)(2 * k + 1) / (float)SDF_G - 1.0f;
    const float sy = py - t.ay, sz = pz - t.az;
    const float u = __builtin_fmaf(sz, t.e2y, -(sy * t.e2z)) * t.inv;
    if (u < 0.0f || u > 1.0f) return 0u;
    const float qx = __builtin_fmaf(sy, t.e1z, -(sz * t.e1y));
    const float v = qx * t.inv;
    if (v < 0.0f || u + v > 1.0f) return 0u;
    unsigned hits = 0u;
    for (int i = 0; i < SDF_G; ++i)
        if (sdf_ray_t(i, t.ax, t.e1x, t.e1y, t.e1z, t.e2x, t.e2y, t.e2z, t.inv, sy, sz, qx) > 0.0f) hits |= 1u << i;
    return hits;
}

// a list record of vol_count_kernel: the triangle's three vertex ids (10 bits each, VOL_MAX_VERTS = 1024) | mesh << 30
IHMR_PURE unsigned vol_pack_record(unsigned ia, unsigned ib, unsigned ic, int mesh) {
    return ia | (ib << 10) | (ic << 20) | ((unsigned)mesh << 30);
}
IHMR_PURE void vol_unpack_record(unsigned r, int& ia, int& ib, int& ic, int& mesh) {
    ia = (int)(r & 1023u); ib = (int)((r >> 10) & 1023u); ic = (int)((r >> 20) & 1023u); mesh = (int)((r >> 30) & 1u);
}

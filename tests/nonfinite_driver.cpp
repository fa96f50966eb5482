// Host driver for the pure helpers of libihmr_hip (ihmr_amd/csrc/ihmr_pure.h) on NON-FINITE and huge arguments: the same header the
// kernels inline, compiled by g++ with -fsanitize=address,undefined,float-cast-overflow (tests/test_nonfinite_host_cpu.py).  Every helper
// is fed the full cross product of VALS in each argument that carries caller data; a helper that converts a float to an integer is
// called the way the kernels call it (behind `in_grid`, behind the yz-degeneracy test of a hand normalised by its own box), and the
// driver counts every call that breaks a rule.  Test infrastructure, not product.
//
//   nonfinite_driver            prints `key value` lines; a sanitizer report aborts the program (non-zero exit)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ihmr_amd/csrc/ihmr_pure.h"

static const float NORMAL = 0.37f;
static const float VALS[8] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e30f, -0.0f, NORMAL};
static const int NV8 = 8;
// the query helpers also take a second ordinary value, so that some combinations do land inside the grid
static const float QVALS[9] = {NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e30f, -0.0f, NORMAL, -0.21f};
static const int NQ = 9;

static long long g_sink = 0;          // (keeps every result alive)
static void sink(float x) { uint32_t u; memcpy(&u, &x, 4); g_sink += u; }
static void report(const char* key, long long v) { printf("%s %lld\n", key, v); }

// ---- sdf_divisor / sdf_div
static void run_div() {
    long long calls = 0, differs = 0, differs_finite = 0;
    for (int i = 0; i < NV8; ++i)
        for (int j = 0; j < NV8; ++j) {
            const float a = VALS[i], b = VALS[j];
            const SdfDivisor d = sdf_divisor(b);
            const float q = sdf_div(a, d), ref = a / b;
            ++calls;
            // outside the fast range the helper IS the plain division; inside it both are the correctly rounded quotient -- unless the
            // quotient overflows: then the plain division gives +-inf and the fast form inf - inf = NaN (neither is a grid coordinate)
            if (!((std::isnan(q) && std::isnan(ref)) || q == ref)) {
                ++differs;
                if (std::isfinite(q) || std::isfinite(ref)) ++differs_finite;
            }
            sink(q);
        }
    report("div_calls", calls);
    report("div_differs_from_plain_division", differs);
    report("div_differs_with_a_finite_quotient", differs_finite);
}

// ---- sdf_query_cell -> sdf_qcell_pack -> sdf_qcell_cell, sdf_trilinear<false>, sdf_grad_to_vertex (the samplers' order of calls)
static void run_query() {
    long long calls = 0, in_grid = 0, in_grid_nonfinite = 0, bad_cell = 0, bad_word = 0, trilin = 0;
    for (int sa = 0; sa < 4; ++sa) {
        const int swap_xz = sa & 1, align = sa >> 1;
        int ix[7];
        for (ix[0] = 0; ix[0] < NQ; ++ix[0]) for (ix[1] = 0; ix[1] < NQ; ++ix[1]) for (ix[2] = 0; ix[2] < NQ; ++ix[2])
        for (ix[3] = 0; ix[3] < NQ; ++ix[3]) for (ix[4] = 0; ix[4] < NQ; ++ix[4]) for (ix[5] = 0; ix[5] < NQ; ++ix[5])
        for (ix[6] = 0; ix[6] < NQ; ++ix[6]) {
            float a[7];
            bool finite = true;
            for (int k = 0; k < 7; ++k) { a[k] = QVALS[ix[k]]; finite = finite && std::isfinite(a[k]); }
            const SdfQuery q = sdf_query_cell(a[0], a[1], a[2], a[3], a[4], a[5], sdf_divisor(a[6]), swap_xz, align);
            ++calls;
            // the prep kernel's lines, in its order (csrc/sdf_collision.h, "normalise own vertices"): the conversions for EVERY query,
            // guarded by in_grid, then the cell word -- under the float-cast-overflow check
            const int i0 = q.in_grid ? (int)floorf(q.ix) : 0, j0 = q.in_grid ? (int)floorf(q.iy) : 0, k0 = q.in_grid ? (int)floorf(q.iz) : 0;
            const unsigned c = sdf_qcell_pack(q.in_grid, i0, j0, k0);
            if (!q.in_grid) {
                if (c != 0u) ++bad_word;
                continue;
            }
            ++in_grid;
            if (!finite) ++in_grid_nonfinite;
            if (i0 < -1 || i0 > SDF_G - 1 || j0 < -1 || j0 > SDF_G - 1 || k0 < -1 || k0 > SDF_G - 1) ++bad_cell;
            int i1, j1, k1;
            sdf_qcell_cell(c, i1, j1, k1);
            if (!(c & SDF_QCELL_IN) || i1 != i0 || j1 != j0 || k1 != k0 || sdf_qcell_mask(c) != 0u) ++bad_word;
            // the cell's eight corner values: every rotation of VALS (a corner outside the mesh or the grid takes no part)
            for (int s = 0; s < NV8; ++s) {
                float pv[8], val, gx, gy, gz;
                for (int c8 = 0; c8 < 8; ++c8) pv[c8] = VALS[(c8 + s) % NV8];
                sdf_trilinear<false>(q.ix, q.iy, q.iz, pv, val, gx, gy, gz);
                sdf_grad_to_vertex(gx, gy, gz, a[6], swap_xz, align);
                sink(val); sink(gx); sink(gy); sink(gz);
                ++trilin;
            }
        }
    }
    report("query_calls", calls);
    report("query_in_grid", in_grid);
    report("query_in_grid_with_nonfinite_argument", in_grid_nonfinite);
    report("query_cell_outside_minus1_31", bad_cell);
    report("query_bad_cell_word", bad_word);
    report("trilinear_calls", trilin);
    // the chain rule on its own: gradient and box scale from VALS
    long long calls_g = 0;
    for (int sa = 0; sa < 4; ++sa)
        for (int i = 0; i < NV8; ++i) for (int j = 0; j < NV8; ++j) for (int k = 0; k < NV8; ++k) for (int l = 0; l < NV8; ++l) {
            float gx = VALS[i], gy = VALS[j], gz = VALS[k];
            sdf_grad_to_vertex(gx, gy, gz, VALS[l], sa & 1, sa >> 1);
            sink(gx); sink(gy); sink(gz);
            ++calls_g;
        }
    report("grad_to_vertex_calls", calls_g);
}

// ---- sdf_corner_mask: every i0 the cell word can hold (6-bit fields: -1 .. 62), bitmap words of every kind
static void run_corner_mask() {
    const unsigned words[4] = {0u, 0xffffffffu, 0xa5a5a5a5u, 0x80000001u};
    long long calls = 0, bad = 0;
    for (int i0 = -1; i0 <= 62; ++i0)
        for (int s = 0; s < 4; ++s) {
            unsigned w4[4];
            for (int c = 0; c < 4; ++c) w4[c] = words[(c + s) & 3];
            const unsigned m = sdf_corner_mask(w4, i0);
            ++calls;
            if (m > 0xffu) ++bad;
            unsigned zero[4] = {0u, 0u, 0u, 0u};
            if (sdf_corner_mask(zero, i0) != 0u) ++bad;
        }
    report("corner_mask_calls", calls);
    report("corner_mask_bad", bad);
}

// ---- the prep kernel's path to tri_col_range: a hand's box (fminf / fmaxf from +-inf, as sdf_prep_kernel forms it), its vertices
// normalised by sdf_div, the yz-degeneracy test -- and only then the column range.  The triangle's y and z (six values) and one x are the
// cross product; two ordinary vertices belong to the hand as well.  Restates the kernel's box lines (csrc/sdf_collision.h, "bounding
// box" and "normalise own vertices"): min / max are order-free, so the 5-vertex hand goes through the expressions of the 778-vertex one.
static void run_prep_range() {
    long long calls = 0, passed = 0, passed_nonfinite = 0, above_one = 0, bad_range = 0, nonempty = 0;
    const float extra[2][3] = {{0.11f, -0.05f, 0.02f}, {-0.07f, 0.09f, -0.04f}};
    int ix[7];
    for (ix[0] = 0; ix[0] < NV8; ++ix[0]) for (ix[1] = 0; ix[1] < NV8; ++ix[1]) for (ix[2] = 0; ix[2] < NV8; ++ix[2])
    for (ix[3] = 0; ix[3] < NV8; ++ix[3]) for (ix[4] = 0; ix[4] < NV8; ++ix[4]) for (ix[5] = 0; ix[5] < NV8; ++ix[5])
    for (ix[6] = 0; ix[6] < NV8; ++ix[6])
    for (int with_extra = 0; with_extra < 2; ++with_extra) {
        float v[5][3] = {{VALS[ix[6]], VALS[ix[0]], VALS[ix[3]]}, {0.02f, VALS[ix[1]], VALS[ix[4]]}, {-0.03f, VALS[ix[2]], VALS[ix[5]]},
                         {extra[0][0], extra[0][1], extra[0][2]}, {extra[1][0], extra[1][1], extra[1][2]}};
        const int n = with_extra ? 5 : 3;
        bool finite = true;
        for (int p = 0; p < 3; ++p) for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(v[p][k]);
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int p = 0; p < n; ++p) for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], v[p][k]); hi[k] = fmaxf(hi[k], v[p][k]); }
        const float cx = (lo[0] + hi[0]) * 0.5f, cy = (lo[1] + hi[1]) * 0.5f, cz = (lo[2] + hi[2]) * 0.5f;
        const float sc = 0.6f * fmaxf(hi[0] - lo[0], fmaxf(hi[1] - lo[1], hi[2] - lo[2]));
        const SdfDivisor dsc = sdf_divisor(sc);
        float nrm[3][3];
        for (int p = 0; p < 3; ++p) { nrm[p][0] = sdf_div(v[p][0] - cx, dsc); nrm[p][1] = sdf_div(v[p][1] - cy, dsc); nrm[p][2] = sdf_div(v[p][2] - cz, dsc); }
        ++calls;
        const float det = sdf_tri_yz_det(nrm[0][1], nrm[0][2], nrm[1][1], nrm[1][2], nrm[2][1], nrm[2][2]);
        if (!(fabsf(det) >= 1e-12f)) continue;                      // (the kernel's test, in the kernel's words)
        ++passed;
        if (!finite) ++passed_nonfinite;
        bool inside = true;
        for (int p = 0; p < 3; ++p) for (int k = 1; k < 3; ++k) inside = inside && (fabsf(nrm[p][k]) <= 1.0f);
        if (!inside) { ++above_one; continue; }                    // the precondition is broken: counted, tri_col_range not called
        int j0, j1, k0, k1;
        tri_col_range(nrm[0][1], nrm[1][1], nrm[2][1], nrm[0][2], nrm[1][2], nrm[2][2], j0, j1, k0, k1);
        const bool empty = j1 < j0 || k1 < k0;
        if (!empty) ++nonempty;
        if (!empty && (j0 < 0 || j1 > SDF_G - 1 || k0 < 0 || k1 > SDF_G - 1)) ++bad_range;
        // what the kernel makes of the range: the j mask (shift amounts) and the packed k range
        if (!empty) {
            const unsigned jmask = (j1 - j0 == 31 ? 0xffffffffu : ((1u << (j1 - j0 + 1)) - 1u)) << j0;
            const int kr = k0 | (k1 << 8);
            if (jmask == 0u || (kr & 255) != k0 || (kr >> 8) != k1) ++bad_range;
        }
    }
    report("prep_calls", calls);
    report("prep_passed_det_test", passed);
    report("prep_passed_det_test_with_nonfinite_vertex", passed_nonfinite);
    report("prep_normalised_above_one", above_one);
    report("prep_nonempty_ranges", nonempty);
    report("prep_bad_range", bad_range);
    // ... and the whole reachable domain directly: every y, z in [-1, 1] (the box bounds |normalised| by 0.5 / 0.6)
    const float dom[9] = {-1.0f, -0.8334f, -0.5f, -1e-30f, -0.0f, 1e-30f, 0.37f, 0.8334f, 1.0f};
    long long dcalls = 0, dbad = 0;
    int d[6];
    for (d[0] = 0; d[0] < 9; ++d[0]) for (d[1] = 0; d[1] < 9; ++d[1]) for (d[2] = 0; d[2] < 9; ++d[2])
    for (d[3] = 0; d[3] < 9; ++d[3]) for (d[4] = 0; d[4] < 9; ++d[4]) for (d[5] = 0; d[5] < 9; ++d[5]) {
        int j0, j1, k0, k1;
        tri_col_range(dom[d[0]], dom[d[1]], dom[d[2]], dom[d[3]], dom[d[4]], dom[d[5]], j0, j1, k0, k1);
        ++dcalls;
        if (!(j1 < j0 || k1 < k0) && (j0 < 0 || j1 > SDF_G - 1 || k0 < 0 || k1 > SDF_G - 1)) ++dbad;
    }
    report("range_domain_calls", dcalls);
    report("range_domain_bad", dbad);
}

// ---- sdf_tri_yz_det on raw VALS: how many non-finite triangles the degeneracy test ALONE would let through (a det of +-inf passes
// it) -- the reason the audit rests on the box normalisation above, not on the test
static void run_det() {
    long long calls = 0, pass_nonfinite = 0;
    int ix[6];
    for (ix[0] = 0; ix[0] < NV8; ++ix[0]) for (ix[1] = 0; ix[1] < NV8; ++ix[1]) for (ix[2] = 0; ix[2] < NV8; ++ix[2])
    for (ix[3] = 0; ix[3] < NV8; ++ix[3]) for (ix[4] = 0; ix[4] < NV8; ++ix[4]) for (ix[5] = 0; ix[5] < NV8; ++ix[5]) {
        bool finite = true;
        for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(VALS[ix[k]]);
        const float det = sdf_tri_yz_det(VALS[ix[0]], VALS[ix[1]], VALS[ix[2]], VALS[ix[3]], VALS[ix[4]], VALS[ix[5]]);
        ++calls;
        if (fabsf(det) >= 1e-12f && !finite) ++pass_nonfinite;
        sink(det);
    }
    report("det_calls", calls);
    report("det_test_alone_passes_nonfinite", pass_nonfinite);
}

// ---- sdf_ray_column_hits: all nine corner coordinates from VALS, a column in the middle of the grid, three `need` words
static void run_ray() {
    const unsigned needs[3] = {0xffffffffu, 0x9249a5c3u, 0x00010000u};
    const int col = 16 * SDF_G + 17;
    long long calls = 0, outside_need = 0, uv = 0, hit = 0;
    int ix[9];
    for (ix[0] = 0; ix[0] < NV8; ++ix[0]) for (ix[1] = 0; ix[1] < NV8; ++ix[1]) for (ix[2] = 0; ix[2] < NV8; ++ix[2])
    for (ix[3] = 0; ix[3] < NV8; ++ix[3]) for (ix[4] = 0; ix[4] < NV8; ++ix[4]) for (ix[5] = 0; ix[5] < NV8; ++ix[5])
    for (ix[6] = 0; ix[6] < NV8; ++ix[6]) for (ix[7] = 0; ix[7] < NV8; ++ix[7]) for (ix[8] = 0; ix[8] < NV8; ++ix[8]) {
        float t[9];
        for (int k = 0; k < 9; ++k) t[k] = VALS[ix[k]];
        const unsigned need = needs[(ix[0] + ix[4] + ix[8]) % 3];
        bool uv_pass = false;
        const unsigned hits = sdf_ray_column_hits(t, t + 3, t + 6, col, need, uv_pass);
        ++calls;
        if (hits & ~need) ++outside_need;
        if (!uv_pass && hits) ++outside_need;
        uv += uv_pass ? 1 : 0;
        hit += hits ? 1 : 0;
    }
    report("ray_calls", calls);
    report("ray_bits_outside_need", outside_need);
    report("ray_uv_passes", uv);
    report("ray_with_hits", hit);
}

// ---- align_root, the optimizer steps, Rodrigues
static void run_small() {
    for (int i = 0; i < NV8; ++i) printf("align_root_%d %d\n", i, align_root(VALS[i]));
    long long adam = 0, sgd = 0, rod = 0;
    for (int i = 0; i < NV8; ++i) for (int j = 0; j < NV8; ++j) for (int k = 0; k < NV8; ++k) {
        float ms = VALS[k];
        sink(opt_sgd_update(VALS[i], VALS[j], ms, 1e-2f)); sink(ms);
        ++sgd;
        for (int l = 0; l < NV8; ++l) {
            float m = VALS[k], v = VALS[l];
            sink(opt_adam_update(VALS[i], VALS[j], m, v, 1e-2f / 0.1f, sqrtf(0.001f))); sink(m); sink(v);
            ++adam;
        }
        const float r[3] = {VALS[i], VALS[j], VALS[k]};
        float R[9], dr[3];
        rodrigues_fwd(r, R);
        for (int e = 0; e < 9; ++e) sink(R[e]);
        for (int s = 0; s < NV8; ++s) {
            float dR[9];
            for (int e = 0; e < 9; ++e) dR[e] = VALS[(e + s) % NV8];
            rodrigues_bwd(r, dR, dr);
            sink(dr[0]); sink(dr[1]); sink(dr[2]);
            ++rod;
        }
    }
    report("adam_calls", adam);
    report("sgd_calls", sgd);
    report("rodrigues_bwd_calls", rod);
}

int main() {
    run_div();
    run_query();
    run_corner_mask();
    run_prep_range();
    run_det();
    run_ray();
    run_small();
    report("sink", g_sink & 1);
    return 0;
}

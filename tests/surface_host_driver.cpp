// Host build of csrc/surface_pure.h (tests/test_surface_cpu.py: g++ -fsanitize=address,undefined -ffp-contract=off): one sample of
// ihmr_surface_distance and ihmr_surface_distance_bwd computed on the CPU in the kernels' order -- the face records packed once per face
// (ids checked against [0, V), srf_face_usable), per query the walk over the records ascending (srf_point_tri + srf_min_update on the
// surface faces, srf_ray_crosses on all), srf_weights and srf_finish; then per query srf_grad_dir and g n, and per vertex the sum of
// -w_k g n over the queries ascending in float64, rounded to float32 once.
//
//   surface_host_driver IN OUT
//   IN : int32 P, V, F_total, F_dist, is_signed; float32 points (P,3); float32 verts (V,3); int32 faces (F_total,3); float64 g (P)
//   OUT: float64 dist (P), face (P), bary (P,3), d_points (P,3), d_verts (V,3)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ihmr_amd/csrc/surface_pure.h"

template <class T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = read_n<int32_t>(f, 5);
    const int P = hd[0], V = hd[1], F_total = hd[2], F_dist = hd[3], is_signed = hd[4];
    if (P < 1 || V < 1 || V > SRF_MAX_VERTS || F_total > SRF_MAX_FACES || F_dist < 1 || F_dist > F_total) { fprintf(stderr, "refused\n"); return 3; }
    const std::vector<float> points = read_n<float>(f, (size_t)P * 3), verts = read_n<float>(f, (size_t)V * 3);
    const std::vector<int32_t> faces = read_n<int32_t>(f, (size_t)F_total * 3);
    const std::vector<double> g = read_n<double>(f, (size_t)P);
    fclose(f);

    auto vertex = [&](int i, double* x) { for (int k = 0; k < 3; ++k) x[k] = (double)verts[(size_t)3 * i + k]; };
    std::vector<unsigned> rec((size_t)F_total, 0u);
    for (int t = 0; t < F_total; ++t) {
        const unsigned ia = (unsigned)faces[3 * t], ib = (unsigned)faces[3 * t + 1], ic = (unsigned)faces[3 * t + 2];
        if (ia < (unsigned)V && ib < (unsigned)V && ic < (unsigned)V) {
            double a[3], b[3], c[3];
            vertex((int)ia, a); vertex((int)ib, b); vertex((int)ic, c);
            if (srf_face_usable(a, b, c)) rec[t] = srf_pack_face(ia, ib, ic);
        }
    }
    std::vector<double> dist((size_t)P), face((size_t)P), bary((size_t)P * 3), d_points((size_t)P * 3, 0.0), d_verts((size_t)V * 3, 0.0);
    std::vector<double> acc((size_t)V * 3, 0.0);
    for (int p = 0; p < P; ++p) {
        const double q[3] = {(double)points[3 * p], (double)points[3 * p + 1], (double)points[3 * p + 2]};
        double best = (double)INFINITY, bv = 0.0, bw = 0.0;
        int bf = -1;
        bool inside = false;
        if (srf_finite(q[0]) && srf_finite(q[1]) && srf_finite(q[2])) {
            for (int t = 0; t < F_total; ++t) {
                if (!(rec[t] & SRF_FACE_USABLE)) continue;
                int ia, ib, ic;
                srf_unpack_face(rec[t], ia, ib, ic);
                double a[3], b[3], c[3];
                vertex(ia, a); vertex(ib, b); vertex(ic, c);
                if (t < F_dist) {
                    double v, w;
                    const double sq = srf_point_tri(q, a, b, c, v, w);
                    if (srf_min_update(best, sq)) { bf = t; bv = v; bw = w; }
                }
                if (is_signed && srf_ray_crosses(q, a, b, c)) inside = !inside;
            }
        }
        double wts[3] = {0.0, 0.0, 0.0};
        if (bf >= 0) srf_weights(bv, bw, wts);
        dist[p] = srf_finish(best, bf, inside);
        face[p] = (double)bf;
        for (int k = 0; k < 3; ++k) bary[3 * p + k] = wts[k];
        // the backward of this query, as surface_dist_bwd_kernel forms it from the forward's words
        if (bf >= 0 && bf < F_dist) {
            const unsigned ids[3] = {(unsigned)faces[3 * bf], (unsigned)faces[3 * bf + 1], (unsigned)faces[3 * bf + 2]};
            if (ids[0] < (unsigned)V && ids[1] < (unsigned)V && ids[2] < (unsigned)V) {
                double a[3], b[3], c[3], n[3];
                vertex((int)ids[0], a); vertex((int)ids[1], b); vertex((int)ids[2], c);
                srf_grad_dir(q, a, b, c, wts, dist[p], n);
                if (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0) {
                    const double gn[3] = {g[p] * n[0], g[p] * n[1], g[p] * n[2]};
                    for (int k = 0; k < 3; ++k) d_points[3 * p + k] = (double)(float)gn[k];
                    for (int k = 0; k < 3; ++k)
                        for (int x = 0; x < 3; ++x) acc[(size_t)3 * ids[k] + x] -= wts[k] * gn[x];
                }
            }
        }
    }
    for (size_t i = 0; i < acc.size(); ++i) d_verts[i] = (double)(float)acc[i];

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    for (const std::vector<double>* v : {&dist, &face, &bary, &d_points, &d_verts})
        if (fwrite(v->data(), sizeof(double), v->size(), o) != v->size()) { fprintf(stderr, "short output\n"); return 2; }
    fclose(o);
    return 0;
}

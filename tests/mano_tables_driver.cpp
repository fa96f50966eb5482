// Host driver of ihmr_amd/csrc/mano_tables.h for tests/test_mano_tables_cpu.py (g++ -fsanitize=address,undefined):
//   mano_tables_driver <op> <in> <out>
// <in>: the arrays of ihmr_mano_arrays in the order of the struct, raw (float32 / int32), each read into a heap block of exactly its
// size; for `update` a second shapedirs follows.
//   build    build_mano_tables
//   update   build_mano_tables, then build_shape_tables with the second shapedirs on the same tables
// <out>: int32 rc; for rc == 0 int32 sparse4 max_depth nnz nseg, then every vector of ManoTables in the order of `put` below as an int64
// element count followed by the elements.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../ihmr_amd/csrc/mano_tables.h"

template <typename T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T>
static bool put(FILE* f, const std::vector<T>& v) {
    const long long n = (long long)v.size();
    return fwrite(&n, sizeof n, 1, f) == 1 && fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc != 4 || (strcmp(argv[1], "build") && strcmp(argv[1], "update"))) { fprintf(stderr, "usage: %s build|update in out\n", argv[0]); return 2; }
    const bool update = !strcmp(argv[1], "update");
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) { perror(argv[2]); return 2; }
    std::vector<float> vt, sd, pd, jr, w, hm, sd2;
    std::vector<int32_t> par, faces, tips;
    const bool read = get(fi, vt, NV3) && get(fi, sd, (size_t)NV3 * 10) && get(fi, pd, (size_t)NPF * NV3) && get(fi, jr, (size_t)NJ * NV) &&
                      get(fi, w, (size_t)NV * NJ) && get(fi, par, NJ) && get(fi, hm, 45) && get(fi, faces, (size_t)NF * 3) &&
                      get(fi, tips, IHMR_NUM_TIPS) && (!update || get(fi, sd2, (size_t)NV3 * 10));
    if (!read || fgetc(fi) != EOF) { fprintf(stderr, "bad input size\n"); return 2; }
    fclose(fi);
    const ihmr_mano_arrays h = {vt.data(), sd.data(), pd.data(), jr.data(), w.data(), par.data(), hm.data(), faces.data(), tips.data()};
    ManoTables t;
    const int32_t rc = build_mano_tables(h, t);
    if (rc == 0 && update) build_shape_tables(sd2.data(), t);
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    bool ok = fwrite(&rc, sizeof rc, 1, fo) == 1;
    if (rc == 0) {
        const int32_t s[4] = {t.sparse4, t.max_depth, t.nnz, t.nseg};
        ok = ok && fwrite(s, sizeof s, 1, fo) == 1;
        ok = ok && put(fo, t.v_template) && put(fo, t.shapedirs_t) && put(fo, t.posedirs) && put(fo, t.pd4) && put(fo, t.sd4) && put(fo, t.vt4) &&
             put(fo, t.J_template) && put(fo, t.J_shapedirs) && put(fo, t.weights) && put(fo, t.w4_w) && put(fo, t.w4_j) && put(fo, t.pose_mean) &&
             put(fo, t.parents) && put(fo, t.depth) && put(fo, t.tip_ids) && put(fo, t.wj_start) && put(fo, t.wj_vert) && put(fo, t.wj_w) &&
             put(fo, t.seg_q) && put(fo, t.jseg_start) && put(fo, t.faces) && put(fo, t.faces_pk) && put(fo, t.J_regressor);
    }
    return (fclose(fo) == 0 && ok) ? 0 : 2;
}

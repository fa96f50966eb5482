// Host build of csrc/volume_pure.h (tests/test_volume_cpu.py: g++ -fsanitize=address,undefined -ffp-contract=off): one sample of
// ihmr_sdf_volume computed on the CPU by walking the face tables exactly as vol_count_kernel does -- vertex boxes, vol_cube, per tile
// vol_tile_frame and vol_normalise, per triangle the index check, vol_col_range, the yz determinant and the packed list record, per
// record vol_tri_setup and vol_column_hits XORed into the mesh's column word -- and writes box, status, counts and the AND-words.
//
//   volume_host_driver IN OUT
//   IN : int32 n_verts_a, n_faces_a, n_verts_b, n_faces_b, subdiv; float32 verts_a; int32 faces_a; float32 verts_b; int32 faces_b
//   OUT: float32 box[4]; int32 status; uint32 counts[subdiv^3]; uint32 bits[subdiv^3][1024]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ihmr_amd/csrc/volume_pure.h"

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
    const int nv[2] = {hd[0], hd[2]}, nf[2] = {hd[1], hd[3]}, n = hd[4];
    if (nv[0] < 1 || nv[0] > VOL_MAX_VERTS || nv[1] < 1 || nv[1] > VOL_MAX_VERTS || nf[0] < 1 || nf[0] > VOL_MAX_FACES || nf[1] < 1 ||
        nf[1] > VOL_MAX_FACES || (n != 1 && n != 2 && n != 4)) { fprintf(stderr, "refused\n"); return 3; }
    std::vector<float> verts[2];
    std::vector<int32_t> faces[2];
    for (int m = 0; m < 2; ++m) {
        verts[m] = read_n<float>(f, (size_t)nv[m] * 3);
        faces[m] = read_n<int32_t>(f, (size_t)nf[m] * 3);
    }
    fclose(f);

    float mn[2][3], mx[2][3];
    bool finite = true;
    for (int m = 0; m < 2; ++m) {
        for (int a = 0; a < 3; ++a) { mn[m][a] = INFINITY; mx[m][a] = -INFINITY; }
        for (int i = 0; i < nv[m]; ++i)
            for (int a = 0; a < 3; ++a) {
                const float x = verts[m][3 * i + a];
                finite = finite && vol_finite(x);
                mn[m][a] = fminf(mn[m][a], x);
                mx[m][a] = fmaxf(mx[m][a], x);
            }
    }
    const VolCube q = vol_cube(mn[0], mx[0], mn[1], mx[1], finite);
    const int n3 = n * n * n;
    std::vector<uint32_t> counts(n3, 0u), bits((size_t)n3 * VOL_COLS, 0u);
    for (int tile = 0; tile < n3 && q.status == VOL_COUNTED; ++tile) {
        const VolTile fr = vol_tile_frame(q.c[0], q.c[1], q.c[2], q.s, n, tile);
        std::vector<float> vn[2];
        std::vector<uint32_t> word[2];
        std::vector<unsigned> list;
        for (int m = 0; m < 2; ++m) {
            vn[m].resize((size_t)nv[m] * 3);
            for (int i = 0; i < nv[m] * 3; ++i) vn[m][i] = vol_normalise(verts[m][i], fr.c[i % 3], fr.s);
            word[m].assign(VOL_COLS, 0u);
            for (int t = 0; t < nf[m]; ++t) {
                const unsigned ia = (unsigned)faces[m][3 * t], ib = (unsigned)faces[m][3 * t + 1], ic = (unsigned)faces[m][3 * t + 2];
                if (ia >= (unsigned)nv[m] || ib >= (unsigned)nv[m] || ic >= (unsigned)nv[m]) continue;
                const float *a = &vn[m][3 * ia], *b = &vn[m][3 * ib], *c = &vn[m][3 * ic];
                int j0, j1, k0, k1;
                if (!vol_col_range(a[1], b[1], c[1], a[2], b[2], c[2], j0, j1, k0, k1)) continue;
                if (fabsf(sdf_tri_yz_det(a[1], a[2], b[1], b[2], c[1], c[2])) < 1e-12f) continue;
                list.push_back(vol_pack_record(ia, ib, ic, m));
            }
        }
        for (size_t r = 0; r < list.size(); ++r) {
            int ia, ib, ic, m, j0, j1, k0, k1;
            vol_unpack_record(list[r], ia, ib, ic, m);
            const float *a = &vn[m].at(3 * ia), *b = &vn[m].at(3 * ib), *c = &vn[m].at(3 * ic);
            VolTri tri;
            if (!vol_col_range(a[1], b[1], c[1], a[2], b[2], c[2], j0, j1, k0, k1) || !vol_tri_setup(a, b, c, tri)) continue;
            const int nj = j1 - j0 + 1, ncol = nj * (k1 - k0 + 1);
            for (int p = 0; p < ncol; ++p) {
                const int col = (k0 + p / nj) * SDF_G + j0 + p % nj;
                word[m].at(col) ^= vol_column_hits(tri, col);
            }
        }
        for (int c = 0; c < VOL_COLS; ++c) {
            const uint32_t both = word[0][c] & word[1][c];
            bits[(size_t)tile * VOL_COLS + c] = both;
            counts[tile] += (uint32_t)__builtin_popcount(both);
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const float box[4] = {q.c[0], q.c[1], q.c[2], q.s};
    const int32_t status = q.status;
    fwrite(box, 4, 4, o);
    fwrite(&status, 4, 1, o);
    fwrite(counts.data(), 4, counts.size(), o);
    fwrite(bits.data(), 4, bits.size(), o);
    fclose(o);
    return 0;
}

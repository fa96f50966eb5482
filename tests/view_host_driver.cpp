// Host driver of the view and heat-map functions of ihmr_amd/csrc/render_pure.h for tests/test_render_views_cpu.py
// (g++ -fsanitize=address,undefined -ffp-contract=off): runs the very functions view_vertices_kernel and heat_colours_kernel inline and
// writes what they give to a file for comparison with tests/render_views_ref.py.
//   view_host_driver view <in> <out>
//       in : int32 nV, n_split, draw0, draw1, has_pivot, nR;  float32 pivot[3], rot[nR][3][3], verts[nV][3]
//       out: float32 c[3] (the pivot used), then q[nR][nV][3]
//       The default pivot is taken twice: serially (rnd_bbox_mid) and as the kernel arranges it (256 strided partial boxes, merged in
//       DESCENDING order); the two must be the same bits or the driver fails.
//   view_host_driver heat <in> <out>
//       in : int32 nV, n_split, layout;  float32 lo, hi, hot[3], albedo[2][3], depth[nV]
//       out: float32 colour[nV][3]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ihmr_amd/csrc/render_pure.h"

static void die(const char* m) { fprintf(stderr, "%s\n", m); exit(2); }

template <typename T> static std::vector<T> read_all(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) die("short read");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 4) die("usage: view_host_driver <view|heat> <in> <out>");
    FILE* fin = fopen(argv[2], "rb");
    FILE* fout = fopen(argv[3], "wb");
    if (!fin || !fout) die("cannot open files");
    if (!strcmp(argv[1], "view")) {
        const std::vector<int32_t> h = read_all<int32_t>(fin, 6);
        const int nV = h[0], n_split = h[1], draw0 = h[2], draw1 = h[3], has_pivot = h[4], nR = h[5];
        const std::vector<float> pivot = read_all<float>(fin, 3), rot = read_all<float>(fin, (size_t)nR * 9),
                                 verts = read_all<float>(fin, (size_t)nV * 3);
        float c[3] = {pivot[0], pivot[1], pivot[2]};
        if (!has_pivot) {
            rnd_bbox_mid(verts.data(), nV, n_split, draw0, draw1, c);
            const int T = 256;
            std::vector<float> mn((size_t)T * 3), mx((size_t)T * 3);
            for (int t = 0; t < T; ++t) {
                rnd_bbox_empty(&mn[3 * t], &mx[3 * t]);
                for (int v = t; v < nV; v += T)
                    if (v < n_split ? draw0 : draw1) rnd_bbox_take(&verts[3 * (size_t)v], &mn[3 * t], &mx[3 * t]);
            }
            float amn[3], amx[3], c2[3];
            rnd_bbox_empty(amn, amx);
            for (int t = T - 1; t >= 0; --t) rnd_bbox_merge(&mn[3 * t], &mx[3 * t], amn, amx);
            rnd_bbox_centre(amn, amx, c2);
            if (memcmp(c, c2, sizeof(c))) die("the pivot depends on the order of the reduction");
        }
        fwrite(c, 4, 3, fout);
        std::vector<float> q((size_t)nV * 3);
        for (int r = 0; r < nR; ++r) {
            for (int v = 0; v < nV; ++v) rnd_view_point(&verts[3 * (size_t)v], c, &rot[9 * (size_t)r], &q[3 * (size_t)v]);
            fwrite(q.data(), 4, q.size(), fout);
        }
    } else if (!strcmp(argv[1], "heat")) {
        const std::vector<int32_t> h = read_all<int32_t>(fin, 3);
        const int nV = h[0], n_split = h[1], layout = h[2];
        const std::vector<float> p = read_all<float>(fin, 11), depth = read_all<float>(fin, (size_t)nV);
        if (layout != 0 && layout != 1) die("layout");
        if (layout == 1 && nV != 2 * n_split) die("layout 1 needs n_verts == 2 n_split");
        std::vector<float> out((size_t)nV * 3);
        for (int v = 0; v < nV; ++v)
            rnd_heat_colour(depth[rnd_heat_entry(v, n_split, layout)], p[0], p[1], &p[5 + 3 * (v >= n_split)], &p[2], &out[3 * (size_t)v]);
        fwrite(out.data(), 4, out.size(), fout);
    } else {
        die("unknown op");
    }
    fclose(fin);
    fclose(fout);
    return 0;
}

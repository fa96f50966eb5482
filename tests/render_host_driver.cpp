// Host driver of ihmr_amd/csrc/render_pure.h for tests/test_render_cpu.py (g++ -fsanitize=address,undefined -ffp-contract=off): runs the
// very functions the render kernels inline, in the kernels' order, and writes every stage to a file for comparison with tests/render_ref.py.
//   render_host_driver render <in> <out>
//       in : int32 nV, nF, split, S, present0, present1, has_bg;  float32 cam[3], albedo[2][3], lights (pos[3][3], color[3][3]);
//            float32 verts[nV][3];  int32 faces[nF][3], csr_offsets[nV+1], csr_ids[3 nF];  bytes background[S][S][3] when has_bg
//       out: per vertex 9 words (normal[3], colour[3] float32, X, Y int32, iz float32);  bytes image[S][S][3];  int32 face ids[S][S]
//   render_host_driver keypoints <in> <out>
//       in : int32 S, K;  bytes colour[3], pad;  float32 kps[K][2], weight[K];  bytes image[S][S][3]      out: bytes image[S][S][3]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../ihmr_amd/csrc/render_pure.h"

static void die(const char* m) { fprintf(stderr, "%s\n", m); exit(2); }

template <typename T> static std::vector<T> read_all(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) die("short read");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 4) die("usage: render_host_driver <render|keypoints> <in> <out>");
    FILE* fin = fopen(argv[2], "rb");
    FILE* fout = fopen(argv[3], "wb");
    if (!fin || !fout) die("cannot open files");
    if (!strcmp(argv[1], "render")) {
        const std::vector<int32_t> h = read_all<int32_t>(fin, 7);
        const int nV = h[0], nF = h[1], split = h[2], S = h[3], present[2] = {h[4], h[5]}, has_bg = h[6];
        const std::vector<float> cam = read_all<float>(fin, 3), albedo = read_all<float>(fin, 6);
        ihmr_render_lights L;
        if (fread(&L, sizeof(L), 1, fin) != 1) die("short read");
        const std::vector<float> verts = read_all<float>(fin, (size_t)nV * 3);
        const std::vector<int32_t> faces = read_all<int32_t>(fin, (size_t)nF * 3), off = read_all<int32_t>(fin, (size_t)nV + 1),
                                   ids = read_all<int32_t>(fin, (size_t)nF * 3);
        std::vector<uint8_t> img = has_bg ? read_all<uint8_t>(fin, (size_t)S * S * 3) : std::vector<uint8_t>((size_t)S * S * 3, 255);
        // vertex stage, as render_vertex_kernel
        std::vector<rnd_vertex> ws((size_t)nV);
        const bool cam_ok = rnd_cam_ok(cam[0]);
        for (int v = 0; v < nV; ++v) {
            rnd_vertex out;
            out.X = RND_BAD_COORD; out.Y = 0; out.iz = 0.0f; out.c[0] = out.c[1] = out.c[2] = 0.0f;
            float n[3] = {0.0f, 0.0f, 0.0f};
            if (cam_ok) {
                int hand = 0, first = 1;
                for (int k = off[v]; k < off[v + 1]; ++k) {
                    const int f = ids[k];
                    const float* a0 = &verts[3 * (size_t)faces[3 * f]];
                    const float* a1 = &verts[3 * (size_t)faces[3 * f + 1]];
                    const float* a2 = &verts[3 * (size_t)faces[3 * f + 2]];
                    if (first) { hand = f >= split; first = 0; }
                    float c[3];
                    rnd_cross_face(a0, a1, a2, c);
                    n[0] = n[0] + c[0]; n[1] = n[1] + c[1]; n[2] = n[2] + c[2];
                }
                rnd_normalise(n);
                float p[3];
                rnd_translate(&verts[3 * (size_t)v], cam.data(), p);
                rnd_shade(n, p, &albedo[3 * hand], &L, out.c);
                rnd_project(p, S, &out);
            }
            ws[v] = out;
            fwrite(n, 4, 3, fout); fwrite(out.c, 4, 3, fout); fwrite(&out.X, 4, 1, fout); fwrite(&out.Y, 4, 1, fout); fwrite(&out.iz, 4, 1, fout);
        }
        // raster stage: every face against the pixels of its bounding box, in DESCENDING face order (the result must not depend on it)
        std::vector<float> best_w((size_t)S * S, 0.0f), best_q((size_t)S * S * 3, 0.0f);
        std::vector<int32_t> best_id((size_t)S * S, -1);
        for (int f = nF - 1; f >= 0; --f) {
            if (!(f < split ? present[0] : present[1])) continue;
            const rnd_vertex &a = ws[faces[3 * f]], &b = ws[faces[3 * f + 1]], &c = ws[faces[3 * f + 2]];
            rnd_face_rec r;
            if (!rnd_face_setup(&a, &b, &c, f, &r)) continue;
            const int64_t xmin = std::min(a.X, std::min(b.X, c.X)), xmax = std::max(a.X, std::max(b.X, c.X));
            const int64_t ymin = std::min(a.Y, std::min(b.Y, c.Y)), ymax = std::max(a.Y, std::max(b.Y, c.Y));
            for (int row = 0; row < S; ++row) {
                if ((int64_t)row * RND_SUBPIXEL < ymin || (int64_t)row * RND_SUBPIXEL > ymax) continue;
                for (int col = 0; col < S; ++col) {
                    if ((int64_t)col * RND_SUBPIXEL < xmin || (int64_t)col * RND_SUBPIXEL > xmax) continue;
                    int64_t e[3];
                    rnd_edges(&r, col, row, e);
                    if ((e[0] | e[1] | e[2]) < 0) continue;
                    float q[3];
                    const float w = rnd_weights(&r, e, q);
                    const size_t at = (size_t)row * S + col;
                    if (rnd_wins(w, f, best_w[at], best_id[at])) {
                        best_w[at] = w; best_id[at] = f;
                        best_q[3 * at] = q[0]; best_q[3 * at + 1] = q[1]; best_q[3 * at + 2] = q[2];
                    }
                }
            }
        }
        for (size_t at = 0; at < (size_t)S * S; ++at) {
            const int f = best_id[at];
            if (f < 0) continue;
            const rnd_vertex &a = ws[faces[3 * f]], &b = ws[faces[3 * f + 1]], &c = ws[faces[3 * f + 2]];
            for (int ch = 0; ch < 3; ++ch) img[3 * at + ch] = (uint8_t)rnd_colour_byte(&best_q[3 * at], best_w[at], a.c[ch], b.c[ch], c.c[ch]);
        }
        fwrite(img.data(), 1, img.size(), fout);
        fwrite(best_id.data(), 4, best_id.size(), fout);
    } else if (!strcmp(argv[1], "keypoints")) {
        const std::vector<int32_t> h = read_all<int32_t>(fin, 2);
        const int S = h[0], K = h[1];
        const std::vector<uint8_t> colour = read_all<uint8_t>(fin, 4);
        const std::vector<float> kps = read_all<float>(fin, (size_t)K * 2), weight = read_all<float>(fin, (size_t)K);
        std::vector<uint8_t> img = read_all<uint8_t>(fin, (size_t)S * S * 3);
        for (int k = 0; k < K; ++k) {
            if (!(weight[k] > 0.0f) || !rnd_kp_ok(kps[2 * k]) || !rnd_kp_ok(kps[2 * k + 1])) continue;
            const int cx = rnd_kp_centre(kps[2 * k], S), cy = rnd_kp_centre(kps[2 * k + 1], S);
            for (int dy = -3; dy <= 3; ++dy)
                for (int dx = -3; dx <= 3; ++dx) {
                    const int x = cx + dx, y = cy + dy;
                    if (abs(dx) <= rnd_disc_half_width(abs(dy)) && x >= 0 && x < S && y >= 0 && y < S)
                        for (int ch = 0; ch < 3; ++ch) img[((size_t)y * S + x) * 3 + ch] = colour[ch];
                }
        }
        fwrite(img.data(), 1, img.size(), fout);
    } else {
        die("unknown op");
    }
    fclose(fin);
    fclose(fout);
    return 0;
}

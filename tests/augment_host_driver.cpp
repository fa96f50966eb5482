// Host driver of ihmr_amd/csrc/augment_pure.h for tests/test_augment_cpu.py (g++ -fsanitize=address,undefined): runs the very functions
// the augmentation kernels inline and writes their results to a file for comparison with tests/augment_ref.py.
//   augment_host_driver rgb2hsv <out>            every (r,g,b) in r-major order -> 3 bytes h,s,v each
//   augment_host_driver hsv2rgb <out>            every (h,s,v) -> 3 bytes r,g,b each
//   augment_host_driver blend <in> <out>         in: int32 n, n float32 factors; out: per factor 256*256 bytes [a][d] + the same against gray
//   augment_host_driver warp <in> <out>          in: int32 S, 6 doubles (inverted matrix); out: S*S records of 8 int32 sx,sy,fx,fy,w0..w3
//   augment_host_driver orient <in> <out>        in: int32 n, n records of 4 float32 (orient, rot_z); out: n x 3 float32
//   augment_host_driver reflect <out>            aug_reflect101(p, len) for len 1..40, p -40..79 -> int32
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ihmr_amd/csrc/augment_pure.h"

static void die(const char* m) { fprintf(stderr, "%s\n", m); exit(2); }

template <typename T> static std::vector<T> read_all(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) die("short read");
    return v;
}

int main(int argc, char** argv) {
    if (argc < 3) die("usage: augment_host_driver <op> [in] <out>");
    const char* op = argv[1];
    FILE* fout = fopen(argv[argc - 1], "wb");
    if (!fout) die("cannot open output");
    if (!strcmp(op, "rgb2hsv") || !strcmp(op, "hsv2rgb")) {
        const bool fwd = !strcmp(op, "rgb2hsv");
        std::vector<uint8_t> out((size_t)3 << 24);
        size_t k = 0;
        for (int a = 0; a < 256; ++a)
            for (int b = 0; b < 256; ++b)
                for (int c = 0; c < 256; ++c) {
                    int r[3];
                    if (fwd) aug_rgb2hsv(a, b, c, r); else aug_hsv2rgb(a, b, c, r);
                    out[k++] = (uint8_t)r[0]; out[k++] = (uint8_t)r[1]; out[k++] = (uint8_t)r[2];
                }
        fwrite(out.data(), 1, out.size(), fout);
    } else if (!strcmp(op, "blend")) {
        FILE* fin = fopen(argv[2], "rb");
        if (!fin) die("cannot open input");
        const int n = read_all<int32_t>(fin, 1)[0];
        const std::vector<float> fac = read_all<float>(fin, (size_t)n);
        fclose(fin);
        std::vector<uint8_t> out((size_t)n * 65536);
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 256; ++a)
                for (int d = 0; d < 256; ++d) out[((size_t)i * 256 + a) * 256 + d] = (uint8_t)aug_blend(a, d, fac[i]);
        fwrite(out.data(), 1, out.size(), fout);
    } else if (!strcmp(op, "warp")) {
        FILE* fin = fopen(argv[2], "rb");
        if (!fin) die("cannot open input");
        const int S = read_all<int32_t>(fin, 1)[0];
        const std::vector<double> m = read_all<double>(fin, 6);
        fclose(fin);
        std::vector<int32_t> out((size_t)S * S * 8);
        for (int y = 0; y < S; ++y)
            for (int x = 0; x < S; ++x) {
                const AugWarp w = aug_warp_coord(m.data(), x, y);
                int wt[4];
                aug_warp_weights(w, wt);
                int32_t* o = &out[((size_t)y * S + x) * 8];
                o[0] = w.sx; o[1] = w.sy; o[2] = w.fx; o[3] = w.fy; o[4] = wt[0]; o[5] = wt[1]; o[6] = wt[2]; o[7] = wt[3];
            }
        fwrite(out.data(), sizeof(int32_t), out.size(), fout);
    } else if (!strcmp(op, "orient")) {
        FILE* fin = fopen(argv[2], "rb");
        if (!fin) die("cannot open input");
        const int n = read_all<int32_t>(fin, 1)[0];
        const std::vector<float> rec = read_all<float>(fin, (size_t)n * 4);
        fclose(fin);
        std::vector<float> out((size_t)n * 3);
        for (int i = 0; i < n; ++i) aug_rotate_orient(&rec[(size_t)i * 4], rec[(size_t)i * 4 + 3], &out[(size_t)i * 3]);
        fwrite(out.data(), sizeof(float), out.size(), fout);
    } else if (!strcmp(op, "reflect")) {
        std::vector<int32_t> out;
        for (int len = 1; len <= 40; ++len)
            for (int p = -40; p < 80; ++p) out.push_back(aug_reflect101(p, len));
        fwrite(out.data(), sizeof(int32_t), out.size(), fout);
    } else {
        die("unknown op");
    }
    fclose(fout);
    return 0;
}

// Host build of csrc/eval_pure.h (g++, -fsanitize=address,undefined; tests/test_pa_metrics_cpu.py runs it directly).
//   eval_pure_driver moments IN OUT   IN: records of 17 doubles [n, mean1[3], mean2[3], M[3][3] row-major, var1]
//                                     OUT: records of 13 doubles [R[3][3] row-major, scale, t[3]]
//   eval_pure_driver errors IN OUT    IN: one record as above, then points as 6 doubles [p[3], g[3]];  OUT: one double per point,
//                                     |scale * R * p + t - g|
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ihmr_amd/csrc/eval_pure.h"

static std::vector<double> read_all(const char* path) {
    std::vector<double> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    double buf[1024];
    size_t k;
    while ((k = fread(buf, sizeof(double), 1024, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static evp_transform solve(const double* r) {
    double M[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][b] = r[7 + 3 * a + b];
    return procrustes_from_moments(r[0], r + 1, r + 4, M, r[16]);
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s moments|errors IN OUT\n", argv[0]); return 2; }
    const std::vector<double> in = read_all(argv[2]);
    std::vector<double> out;
    if (!strcmp(argv[1], "moments")) {
        if (in.size() % 17) { fprintf(stderr, "moments: input is not a whole number of records\n"); return 2; }
        for (size_t i = 0; i + 17 <= in.size(); i += 17) {
            const evp_transform T = solve(&in[i]);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) out.push_back(T.R[a][b]);
            out.push_back(T.scale);
            for (int a = 0; a < 3; ++a) out.push_back(T.t[a]);
        }
    } else if (!strcmp(argv[1], "errors")) {
        if (in.size() < 17 || (in.size() - 17) % 6) { fprintf(stderr, "errors: bad input size\n"); return 2; }
        const evp_transform T = solve(&in[0]);
        for (size_t i = 17; i + 6 <= in.size(); i += 6) out.push_back(evp_aligned_error(T, &in[i], &in[i + 3]));
    } else {
        fprintf(stderr, "unknown operation %s\n", argv[1]);
        return 2;
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 2;
    const size_t written = out.empty() ? 0 : fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    return written == out.size() ? 0 : 2;
}

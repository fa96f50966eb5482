// Host build of the curve helpers of csrc/eval_pure.h (g++, -fsanitize=address,undefined; tests/test_curve_metrics_cpu.py runs it).
//   eval_curve_driver index IN OUT    IN: [T, t[0..T), values...];  OUT: per value two doubles, evp_threshold_index and
//                                     evp_threshold_index_strict.  The table is copied into a heap block of exactly T doubles, so a
//                                     probe outside it is an AddressSanitizer report
//   eval_curve_driver sqdist IN OUT   IN: records of 6 doubles [a[3], b[3]];  OUT: one double per record, evp_sq_dist
//   eval_curve_driver fscore IN OUT   IN: records of 3 doubles [n_pg, n_gp, n];  OUT: one double per record, evp_fscore
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

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s index|sqdist|fscore IN OUT\n", argv[0]); return 2; }
    const std::vector<double> in = read_all(argv[2]);
    std::vector<double> out;
    if (!strcmp(argv[1], "index")) {
        if (in.empty() || in[0] < 0 || (size_t)in[0] + 1 > in.size()) { fprintf(stderr, "index: bad input\n"); return 2; }
        const int T = (int)in[0];
        double* table = new double[T > 0 ? T : 1];
        for (int k = 0; k < T; ++k) table[k] = in[1 + k];
        for (size_t i = 1 + (size_t)T; i < in.size(); ++i) {
            out.push_back((double)evp_threshold_index(in[i], table, T));
            out.push_back((double)evp_threshold_index_strict(in[i], table, T));
        }
        delete[] table;
    } else if (!strcmp(argv[1], "sqdist")) {
        if (in.size() % 6) { fprintf(stderr, "sqdist: input is not a whole number of records\n"); return 2; }
        for (size_t i = 0; i + 6 <= in.size(); i += 6) out.push_back(evp_sq_dist(in[i], in[i + 1], in[i + 2], in[i + 3], in[i + 4], in[i + 5]));
    } else if (!strcmp(argv[1], "fscore")) {
        if (in.size() % 3) { fprintf(stderr, "fscore: input is not a whole number of records\n"); return 2; }
        for (size_t i = 0; i + 3 <= in.size(); i += 3) out.push_back(evp_fscore(in[i], in[i + 1], in[i + 2]));
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

// Host driver of csrc/contact_pure.h (tests/test_contact_metrics_cpu.py builds it with g++ -fsanitize=address,undefined and runs it as a
// program): the header's functions on arrays of float64 read from a file, the results written to another.
//   contact_host_driver OP IN OUT
//   sample  in  [sc, K, thr[K], pred_right (778*3), pred_left, gt_right, gt_left]
//           out [pair_sum, |C|, counts (2,K,3), near (2,2,778)]: one sample walked in the order of eval_contact_kernel -- workgroup h,
//               thread tid, its slots tid + 256 s, j ascending; the pair sum per slot, slots ascending, then ctp_block_sum
//   decide  in  [tau, sc, sq...]            out per sq [literal predicate, filtered predicate]
//   index   in  [K, thr[K], near...]        out per value ctp_contact_index
//   min     in  [values...]                 out [the running minimum from +inf over the values in order]
//   mrrpe   in  records of 15 [p0, p21, g0, g21, w0, w21, sc]      out per record [e, counted]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ihmr_amd/csrc/contact_pure.h"

static std::vector<double> read_all(const char* path) {
    std::vector<double> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    double buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static int sample(const std::vector<double>& in, std::vector<double>& out) {
    if (in.size() < 2) return 2;
    const double sc = in[0];
    const int K = (int)in[1];
    if (K < 1 || K > CTP_MAX_K || in.size() != (size_t)(2 + K + 4 * CTP_NV * 3)) return 2;
    const double* thr = &in[2];
    const double* mesh[4] = {thr + K, thr + K + CTP_NV * 3, thr + K + 2 * CTP_NV * 3, thr + K + 3 * CTP_NV * 3};   // pr, pl, gr, gl
    const double tau = thr[0], limit = ctp_pair_limit(tau, sc);
    out.assign(2 + 2 * K * 3 + 2 * 2 * CTP_NV, 0.0);
    double* counts = &out[2];
    double* near = &out[2 + 2 * K * 3];
    for (int h = 0; h < 2; ++h) {
        const double* Qp = mesh[h ? 1 : 0];
        const double* Qg = mesh[h ? 3 : 2];
        const double* Tp = mesh[h ? 0 : 1];
        const double* Tg = mesh[h ? 2 : 3];
        std::vector<double> thread_sum(CTP_THREADS, 0.0);
        int hist[3][CTP_MAX_K + 1];
        memset(hist, 0, sizeof(hist));
        long pairs = 0;
        for (int tid = 0; tid < CTP_THREADS; ++tid) {
            double acc[CTP_SLOTS] = {0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < CTP_SLOTS; ++s) {
                const int v = tid + CTP_THREADS * s;
                if (v >= CTP_NV) continue;
                double bp = INFINITY, bg = INFINITY;
                for (int j = 0; j < CTP_NV; ++j) {
                    // always sq_dist(right, left)
                    const double sp = h == 0 ? evp_sq_dist(Qp[3 * v], Qp[3 * v + 1], Qp[3 * v + 2], Tp[3 * j], Tp[3 * j + 1], Tp[3 * j + 2])
                                             : evp_sq_dist(Tp[3 * j], Tp[3 * j + 1], Tp[3 * j + 2], Qp[3 * v], Qp[3 * v + 1], Qp[3 * v + 2]);
                    const double sg = h == 0 ? evp_sq_dist(Qg[3 * v], Qg[3 * v + 1], Qg[3 * v + 2], Tg[3 * j], Tg[3 * j + 1], Tg[3 * j + 2])
                                             : evp_sq_dist(Tg[3 * j], Tg[3 * j + 1], Tg[3 * j + 2], Qg[3 * v], Qg[3 * v + 1], Qg[3 * v + 2]);
                    bp = ctp_min_update(bp, sp);
                    bg = ctp_min_update(bg, sg);
                    if (h == 0 && ctp_pair_in_contact_filtered(sg, sc, tau, limit)) {
                        if (!ctp_pair_in_contact(sg, sc, tau)) return 3;      // the filter never changes a decision
                        acc[s] += ctp_dist(sp, sc);
                        ++pairs;
                    } else if (h == 0 && ctp_pair_in_contact(sg, sc, tau)) {
                        return 3;
                    }
                }
                const double np = ctp_dist(bp, sc), ng = ctp_dist(bg, sc);
                near[(h * 2 + 0) * CTP_NV + v] = np;
                near[(h * 2 + 1) * CTP_NV + v] = ng;
                const int ip = ctp_contact_index(np, thr, K), ig = ctp_contact_index(ng, thr, K);
                ++hist[0][ctp_both_index(ip, ig)];
                ++hist[1][ip];
                ++hist[2][ig];
            }
            thread_sum[tid] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
        }
        if (h == 0) {
            out[0] = ctp_block_sum(thread_sum.data());
            out[1] = (double)pairs;
        }
        for (int k = 0; k < K; ++k)
            for (int c = 0; c < 3; ++c) {
                int n = 0;
                for (int i = 0; i <= k; ++i) n += hist[c][i];
                counts[(h * K + k) * 3 + c] = (double)n;
            }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    std::vector<double> out;
    int rc = 0;
    if (!strcmp(argv[1], "sample")) {
        rc = sample(in, out);
    } else if (!strcmp(argv[1], "decide")) {
        if (in.size() < 2) return 2;
        const double tau = in[0], sc = in[1], limit = ctp_pair_limit(tau, sc);
        for (size_t i = 2; i < in.size(); ++i) {
            out.push_back(ctp_pair_in_contact(in[i], sc, tau) ? 1.0 : 0.0);
            out.push_back(ctp_pair_in_contact_filtered(in[i], sc, tau, limit) ? 1.0 : 0.0);
        }
        out.push_back(limit);
    } else if (!strcmp(argv[1], "index")) {
        if (in.empty()) return 2;
        const int K = (int)in[0];
        if (K < 0 || in.size() < (size_t)(1 + K)) return 2;
        for (size_t i = 1 + K; i < in.size(); ++i) out.push_back((double)ctp_contact_index(in[i], in.data() + 1, K));
    } else if (!strcmp(argv[1], "min")) {
        double best = INFINITY;
        for (double v : in) best = ctp_min_update(best, v);
        out.push_back(best);
    } else if (!strcmp(argv[1], "mrrpe")) {
        if (in.size() % 15) return 2;
        for (size_t r = 0; r < in.size(); r += 15) {
            double e;
            const bool counted = ctp_mrrpe(&in[r], &in[r + 3], &in[r + 6], &in[r + 9], in[r + 12], in[r + 13], in[r + 14], e);
            out.push_back(e);
            out.push_back(counted ? 1.0 : 0.0);
        }
    } else {
        return 2;
    }
    if (rc) return rc;
    FILE* f = fopen(argv[3], "wb");
    if (!f) return 2;
    if (!out.empty()) fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    return 0;
}

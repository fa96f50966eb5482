// Host driver of ihmr_amd/csrc/launch_plan.h for tests/test_launch_plan_cpu.py (g++ -fsanitize=address,undefined):
//   launch_plan_driver <op> <in> <out>
// <in>: int64 count, then count records of int64 fields; <out>: count records of int64 plan fields, in the order of the structs.
//   fp32   N Cin Ho Wo Cout kh kw ldx ldw ldy cus workspace_bytes y_aligned16 force_tile force_ksplit sk_max_tiles sk_min_nk sk_workers
//          (force_tile = -2: a default-constructed ConvTuning, the other four ignored)
//   bf16   N Cin Ho Wo Cout kh kw ldx ldw ldy ldr act cus workspace_bytes x16 x8 y8 has_residual r8
//   wgrad  N Cin Ho Wo Cout kh kw ldx lddy ldw workspace_bytes
//   bn     M
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../ihmr_amd/csrc/launch_plan.h"

typedef long long i64;

static int fields_in(const char* op) {
    return !strcmp(op, "fp32") ? 18 : !strcmp(op, "bf16") ? 19 : !strcmp(op, "wgrad") ? 11 : !strcmp(op, "bn") ? 1 : -1;
}

int main(int argc, char** argv) {
    if (argc != 4 || fields_in(argv[1]) < 0) { fprintf(stderr, "usage: %s fp32|bf16|wgrad|bn in out\n", argv[0]); return 2; }
    const char* op = argv[1];
    const int nf = fields_in(op);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) { perror(argv[2]); return 2; }
    i64 n = 0;
    if (fread(&n, sizeof n, 1, fi) != 1 || n < 0) { fprintf(stderr, "bad count\n"); return 2; }
    std::vector<i64> in((size_t)n * nf), out;
    if (fread(in.data(), sizeof(i64), in.size(), fi) != in.size()) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);
    for (i64 i = 0; i < n; ++i) {
        const i64* r = &in[(size_t)i * nf];
        auto I = [&](int k) { return (int)r[k]; };
        if (!strcmp(op, "fp32")) {
            plan::ConvTuning t;
            if (r[13] != -2) { t.force_tile = I(13); t.force_ksplit = I(14); t.sk_max_tiles = I(15); t.sk_min_nk = I(16); t.sk_workers = I(17); }
            const plan::ConvPlan p = plan::plan_conv_fp32(I(0), I(1), I(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), I(10), (size_t)r[11], r[12] != 0, t);
            out.insert(out.end(), {p.ok, p.bm, p.bn, p.mode, p.threads, p.grid_x, p.grid_y, p.grid_z, p.ksplit, p.reduce, p.streamk, p.sk_workers,
                                   p.sk_tiles, p.tiles_m, p.nk});
        } else if (!strcmp(op, "bf16")) {
            const plan::ConvPlanBF16 p = plan::plan_conv_bf16(I(0), I(1), I(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), I(10), I(11), I(12), (size_t)r[13],
                                                              r[14] != 0, r[15] != 0, r[16] != 0, r[17] != 0, r[18] != 0);
            out.insert(out.end(), {p.ok, p.bn, p.mode, p.grid_x, p.grid_y, p.grid_z, p.ksplit, p.vec, p.nk});
        } else if (!strcmp(op, "wgrad")) {
            const plan::WgradPlan p = plan::plan_conv_wgrad(I(0), I(1), I(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), (size_t)r[10]);
            out.insert(out.end(), {p.ok, p.bm, p.bn, p.threads, p.grid_x, p.grid_y, p.grid_z, p.msplit, p.chunks_per, p.reduce});
        } else {
            const plan::BnChunks p = plan::plan_bn_chunks((long)r[0]);
            out.insert(out.end(), {p.rows_per, p.chunks});
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    const bool ok = fwrite(out.data(), sizeof(i64), out.size(), fo) == out.size();
    return (fclose(fo) == 0 && ok) ? 0 : 2;
}

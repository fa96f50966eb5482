// Host driver of the bf16 rounding helpers of ihmr_amd/csrc/ihmr_pure.h (the functions the bf16 encoder kernels inline), built by
// tests/test_encoder_bf16_cpu.py with g++ -fsanitize=address,undefined.
//   pure_bf16_driver narrow <in> <out>   in: int32 n, n float32 bit patterns   out: n uint16 (ihmr_f32_to_bf16)
//   pure_bf16_driver widen  <in> <out>   in: int32 n, n uint32 (low 16 bits = a bf16 pattern)   out: n float32 bit patterns (ihmr_bf16_to_f32)
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../ihmr_amd/csrc/ihmr_pure.h"

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s narrow|widen <in> <out>\n", argv[0]); return 2; }
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) { perror(argv[2]); return 2; }
    int32_t n = 0;
    if (fread(&n, 4, 1, fi) != 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<uint32_t> in((size_t)n);
    if (n && fread(in.data(), 4, (size_t)n, fi) != (size_t)n) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    if (!strcmp(argv[1], "narrow")) {
        std::vector<uint16_t> out((size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            float f;
            memcpy(&f, &in[(size_t)i], 4);
            out[(size_t)i] = ihmr_f32_to_bf16(f);
        }
        fwrite(out.data(), 2, (size_t)n, fo);
    } else if (!strcmp(argv[1], "widen")) {
        std::vector<uint32_t> out((size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            const float f = ihmr_bf16_to_f32((uint16_t)in[(size_t)i]);
            memcpy(&out[(size_t)i], &f, 4);
        }
        fwrite(out.data(), 4, (size_t)n, fo);
    } else {
        fprintf(stderr, "unknown op %s\n", argv[1]);
        return 2;
    }
    fclose(fo);
    return 0;
}

// Launch selection of the convolution and BatchNorm launchers of ihmr_hip.hip -- which tile, gather mode, split depth, grid and reduce
// kernel a shape gets -- as pure functions of plain integers: no HIP header, no pointer, no getenv, so the GPU-less container compiles
// them with g++ under AddressSanitizer / UBSan and compares them field for field with the Python restatements the GPU tests predict
// workspace fingerprints from (tests/test_launch_plan_cpu.py builds tests/launch_plan_driver.cpp).  A launcher checks its pointers, asks
// device_cu_count(), calls its planner and dispatches on the plan; every refusal on shape or stride grounds is `ok = 0` here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define BN_MAX_CHUNKS 1024

namespace plan {

constexpr int CONV_BK_F32 = 16, CONV_BK_BF16 = 32;     // K steps of csrc/encoder.h / csrc/encoder_bf16.h (ihmr_hip.hip asserts they agree)
enum Mode { GENERIC = 0, FAST = 1, C4 = 2 };            // the values of CONV_* and CONVB_* (asserted likewise)

inline long lmin(long a, long b) { return a < b ? a : b; }
inline long lmax(long a, long b) { return a > b ? a : b; }
inline long cdiv(long a, long b) { return (a + b - 1) / b; }
// threads of a (BM x BN) fp32 tile: one wave per 64 x 32 sub-tile (the __launch_bounds__ of conv_igemm_kernel and conv_wgrad_kernel)
inline int tile_threads(int bm, int bn) { return (bm / 64) * (bn / 32) * 64; }

// ------------------------------------------------------------------------------------------ ihmr_conv_igemm
// Tuning overrides; the defaults are the product values.  Only a library built with IHMR_TUNING_BUILD fills this from the environment
// (IHMR_CONV_FORCE, IHMR_CONV_SK: per-layer tile / split measurements, scripts/prof_encoder.py).
struct ConvTuning {
    int force_tile = -1;        // 0-3: 128x128, 64x128, 128x64, 64x64 (ignored when the weight stride cannot carry it)
    int force_ksplit = 1;       // with force_tile: the K split, still capped by the workspace and 4 steps per piece
    int sk_max_tiles = 768;     // Stream-K: at most this many 128 x 128 tiles,
    int sk_min_nk = 64;         //           at least this many K steps,
    int sk_workers = 0;         //           workers (0: two per CU); a multiple of 8, at least 8
};

struct ConvPlan {
    int ok;                     // 0: the launcher refuses the shape
    int bm, bn, mode, threads;  // the tile that LAUNCHES and its gather mode
    int grid_x, grid_y, grid_z;
    int ksplit;                 // gridDim.z of the tile kernel; 1 = no split (and 1 under Stream-K)
    int reduce;                 // 0: none; 4 / 1: conv_splitk_reduce_kernel<4> / <1>
    int streamk, sk_workers, sk_tiles, tiles_m;
    int nk;
};

// Stream-K workers: two per CU of THIS device, a multiple of 8 (conv_streamk_kernel numbers them by XCD), at most 512 (the workspace
// contract of include/ihmr_hip.h: two 64 KB tile slots per worker = 64 MiB)
inline int streamk_workers(int cus) { return (int)lmax(8, lmin(512, 2 * cus / 8 * 8)); }

inline ConvPlan plan_conv_fp32(int N, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int ldx, int ldw, int ldy, int cus,
                               size_t workspace_bytes /* 0: no workspace */, bool y_aligned16, const ConvTuning& t = ConvTuning()) {
    ConvPlan p{};
    if (N <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0) return p;
    const int M = N * Ho * Wo, nk = (int)cdiv((long)kh * kw * Cin, CONV_BK_F32);
    // Tile and K split, from per-layer measurements on MI355X (scripts/prof_encoder.py with IHMR_CONV_FORCE):
    // the 128 x 128 tile wins on every ResNet-50 layer, even when it leaves CUs without a workgroup -- smaller
    // tiles move twice the operands through LDS per MFMA.  Occupancy is repaired with split-K instead: layers with
    // fewer than 1.5 workgroups per CU and a long K loop run their K halves in separate workgroups (two resident
    // workgroups per CU also hide each other's barriers); partial sums go to the caller's workspace and
    // conv_splitk_reduce_kernel adds them in fixed order.  Single-image-row layers (the Linear layers at batch 64)
    // take the 64-row tile and the deepest split the K loop allows.
    const bool wide_ok = Cout > 64 && ldw % 128 == 0;
    if (!wide_ok && ldw % 64 != 0) return p;
    const int tiles[4][2] = {{128, 128}, {64, 128}, {128, 64}, {64, 64}};
    auto blocks = [&](int i) { return cdiv(M, tiles[i][0]) * cdiv(Cout, tiles[i][1]); };
    const long cap = workspace_bytes ? (long)(workspace_bytes / ((size_t)M * Cout * sizeof(float))) : 1;
    int pick = wide_ok ? 0 : 2, ksplit = 1;
    // Linear layers (a handful of workgroups): every K step costs a global-load round trip (~1 us) that nothing hides at this
    // occupancy, so the K loop is cut as deep as 4 steps per workgroup allow (measured on the IHMR-MLP training step:
    // 8-way 0.47 ms, 16-way 0.41 ms, 32-way 0.39 ms per step)
    if (M <= 64) {
        pick = wide_ok ? 1 : 3;
        ksplit = (int)lmax(1, lmin(lmin(32, cap), nk / 4));
    } else if (blocks(pick) < 64) {
        ksplit = (int)lmax(1, lmin(lmin(32, cap), nk / 4));
    } else if (blocks(pick) < 384 && nk >= 64 && cap >= 2) {
        ksplit = 2;
    } else if (wide_ok && blocks(0) > 768 && blocks(0) < 896) {
        // 784 tiles (the 14 x 14 layers with >= 1024 output channels): three resident workgroups per CU take 768, the last 16 run alone at ~2 us
        // per K step (8-33 us: scripts/experiments/conv_tail_generation.py); as 1568 half-height tiles (six resident per CU) the stragglers
        // are half as long.  Measured per layer (scripts/experiments/tile_sweep.sh): 145 -> 132 us (32 K steps), 82 -> 77.5 us (16 K steps)
        pick = 1;
    }
    if (t.force_tile >= 0 && t.force_tile < 4 && (tiles[t.force_tile][1] == 64 || wide_ok)) {
        pick = t.force_tile;
        ksplit = (int)lmax(1, lmin(lmin(t.force_ksplit, cap), lmax(1, nk / 4)));
    }
    const bool fast = (Cin % CONV_BK_F32) == 0 && (ldx % 4) == 0 && Cin <= 2048;   // (2048: the zero page the padding pixels are read from, csrc/encoder.h)
    p.nk = nk;
    // Stream-K (csrc/encoder.h): layers with a long K loop and at most three 128 x 128 tiles per CU -- at batch 64 every 3 x 3 layer and the
    // first 1 x 1 of every bottleneck from 28 x 28 down (100, 196 or 392 tiles: 0.4-1.5 per CU) -- are shared evenly by two workers per CU.
    // Measured per layer (scripts/prof_encoder_layers.sh, round 4): 3 x 3 layers 175-187 -> 144-158 us, 1 x 1 layers with K >= 1024
    // 90-155 -> 77-141 us; with 32 K steps the fix-up's traffic eats the gain (85 -> 88 us), so those keep one workgroup per tile.
    if (t.sk_workers != 0 && (t.sk_workers < 8 || t.sk_workers % 8 != 0)) return p;
    const int sk_workers = t.sk_workers ? t.sk_workers : streamk_workers(cus);
    const long sk_tiles = blocks(0);
    if (fast && pick == 0 && M > 64 && Cout % 128 == 0 && ldy % 4 == 0 && y_aligned16 && sk_tiles >= 64 && sk_tiles <= t.sk_max_tiles &&
        nk >= t.sk_min_nk && sk_tiles * nk >= 4L * sk_workers && workspace_bytes >= (size_t)sk_workers * 2 * 128 * 128 * sizeof(float)) {
        p.ok = 1; p.bm = p.bn = 128; p.mode = FAST; p.threads = 512;
        p.grid_x = sk_workers; p.grid_y = p.grid_z = 1;
        p.ksplit = 1; p.reduce = 0;
        p.streamk = 1; p.sk_workers = sk_workers; p.sk_tiles = (int)sk_tiles; p.tiles_m = (int)cdiv(M, 128);
        return p;
    }
    // (a persistent 1-D grid walking the tiles with a stride -- the cure for sdf_dist_kernel's slow slot refill -- was measured here too:
    // 6.95 -> 7.17 ms per 64-image pass at 6, 5 and 4 waves per SIMD alike; one workgroup per tile stays)
    // The stem on the image padded to 4 channels has its own gather, built for the two 64-column tiles only: it needs !wide_ok, which
    // is exactly when pick is 2 or 3, so the picked tile is always one the mode exists for.
    p.mode = fast ? FAST : (Cin == 4 && (ldx % 4) == 0 && kw >= 4 && !wide_ok) ? C4 : GENERIC;
    p.ok = 1; p.bm = tiles[pick][0]; p.bn = tiles[pick][1]; p.threads = tile_threads(p.bm, p.bn);
    p.grid_x = (int)cdiv(M, p.bm); p.grid_y = (int)cdiv(Cout, p.bn); p.grid_z = ksplit;
    p.ksplit = ksplit;
    p.reduce = ksplit == 1 ? 0 : Cout % 4 == 0 ? 4 : 1;
    return p;
}

// ------------------------------------------------------------------------------------------ ihmr_conv_igemm_bf16
struct ConvPlanBF16 {
    int ok;
    int bn, mode;               // the tile is 128 x bn, 256 threads
    int grid_x, grid_y, grid_z;
    int ksplit;
    int vec;                    // the epilogue stores (and reads the residual) four channels at a time
    int nk;
};

inline ConvPlanBF16 plan_conv_bf16(int N, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int ldx, int ldw, int ldy, int ldr, int act,
                                   int cus, size_t workspace_bytes /* 0: no workspace */, bool x_aligned16, bool x_aligned8,
                                   bool y_aligned8, bool has_residual, bool residual_aligned8) {
    ConvPlanBF16 p{};
    if (N <= 0 || Ho <= 0 || Wo <= 0 || Cout <= 0 || Cin <= 0 || (act != 0 && act != 1) || ldw % 64 != 0 || ldw < Cout) return p;
    const int M = N * Ho * Wo, nk = (int)cdiv((long)kh * kw * Cin, CONV_BK_BF16);
    const bool wide = Cout > 64 && ldw % 128 == 0;
    const int BN = wide ? 128 : 64;
    if (ldw < cdiv(Cout, BN) * BN) return p;
    // K split: a layer with fewer than two tiles per CU (at batch 64: the 14 x 14 and 7 x 7 stages) runs its K loop in up to 8 pieces of
    // at least 4 steps; the pieces' fp32 sums go to the workspace and are added in ascending K order (bit-identical from run to run;
    // the split follows the device's CU count, so results are bit-stable per device model)
    const long tiles = cdiv(M, 128) * cdiv(Cout, BN);
    int ksplit = 1;
    if (workspace_bytes && tiles < 2L * cus && nk >= 8) {
        const long cap = (long)(workspace_bytes / ((size_t)M * Cout * sizeof(float)));
        ksplit = (int)lmax(1, lmin(lmin(8, cap), lmin(nk / 4, cdiv(2L * cus, tiles))));
    }
    p.ok = 1; p.bn = BN; p.nk = nk; p.ksplit = ksplit;
    p.grid_x = (int)cdiv(M, 128); p.grid_y = (int)cdiv(Cout, BN); p.grid_z = ksplit;
    p.vec = Cout % 4 == 0 && ldy % 4 == 0 && y_aligned8 && (!has_residual || (ldr % 4 == 0 && residual_aligned8));
    p.mode = (Cin % CONV_BK_BF16 == 0 && ldx % 8 == 0 && Cin <= 4096 && x_aligned16) ? FAST : (Cin == 4 && ldx == 4 && x_aligned8) ? C4 : GENERIC;
    return p;
}

// ------------------------------------------------------------------------------------------ ihmr_conv_wgrad
enum WgradReduce { WGRAD_REDUCE = 0, WGRAD_SPLITK4 = 4, WGRAD_SPLITK1 = 1 };   // wgrad_reduce_kernel / conv_splitk_reduce_kernel<4> / <1>

struct WgradPlan {
    int ok;
    int bm, bn, threads;        // tile over (K, Cout)
    int grid_x, grid_y, grid_z;
    int msplit, chunks_per;     // pixel ranges (gridDim.z) and 16-pixel chunks per range
    int reduce;
};

inline WgradPlan plan_conv_wgrad(int N, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int ldx, int lddy, int ldw, size_t workspace_bytes) {
    WgradPlan p{};
    if (N <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || Cin % 4 || lddy % 4 || ldx % 4 || ldw < Cout) return p;
    // (conv_wgrad_kernel splits a pixel index by a float-reciprocal product with a +-1 correction: exact below 2^23 pixels)
    if ((long)N * Ho * Wo >= (1L << 23)) return p;
    const int M = N * Ho * Wo, K = kh * kw * Cin;
    p.bm = K > 64 ? 128 : 64; p.bn = Cout > 64 ? 128 : 64; p.threads = tile_threads(p.bm, p.bn);
    const long tiles = cdiv(K, p.bm) * cdiv(Cout, p.bn);
    const long nchunks = cdiv(M, CONV_BK_F32);
    const long cap = (long)(workspace_bytes / ((size_t)K * Cout * sizeof(float)));
    if (cap < 1) return p;
    long msplit = lmax(1, lmin(lmin(cap, 256), lmin(cdiv(1024, tiles), lmax(1, nchunks / 8))));
    p.chunks_per = (int)cdiv(nchunks, msplit);
    msplit = cdiv(nchunks, p.chunks_per);                         // the re-division: no empty pixel range
    p.ok = 1; p.msplit = (int)msplit;
    p.grid_x = (int)cdiv(K, p.bm); p.grid_y = (int)cdiv(Cout, p.bn); p.grid_z = (int)msplit;
    p.reduce = (Cout % 4 == 0 && ldw % 4 == 0 && msplit >= 32) ? WGRAD_REDUCE : Cout % 4 == 0 ? WGRAD_SPLITK4 : WGRAD_SPLITK1;
    return p;
}

// ------------------------------------------------------------------------------------------ BatchNorm column reductions
struct BnChunks { int rows_per, chunks; };                         // at most BN_MAX_CHUNKS chunks of at least 16 rows
inline BnChunks plan_bn_chunks(long M) {
    const long rp = lmax(16, cdiv(M, BN_MAX_CHUNKS));
    return BnChunks{(int)rp, (int)cdiv(M, rp)};
}

}  // namespace plan

// Opt-in bf16 form of the ResNet-50 trunk (InterHandEncoder with encoder_precision = "bf16"): bf16 activations (NHWC) and bf16 weights
// on the bf16 matrix cores, fp32 accumulation, fp32 epilogue, ONE round-to-nearest-even per stored activation.  The fp32 kernels of
// encoder.h are untouched and stay the default; fc1, feat_encoder, the IEF iterations and the hand classifier stay on them.
//
// Numerics contract ("bf16 encoder path"; tests/bf16_emulation.py is the CPU restatement):
//   y = bf16_rne( act( sum_k x[k] w[k]  (fp32 accumulate; bf16 x bf16 products are exact in fp32)  + bias_f32  (+ widen(residual_bf16)) ) )
// Partial sums that leave a workgroup (split-K) are fp32 and are added in ascending K order by conv_splitk_reduce_bf16_kernel.
//
// GEMM view as in encoder.h: Y[M = N*Ho*Wo][Cout] = A[M][K = kh*kw*Cin] . Wt[K][Cout], A gathered on the fly.
// MFMA: v_mfma_f32_32x32x16_bf16.  A lane's operand fragment is 8 consecutive k of one row (A) / one column (B): 8 consecutive
// CHANNELS of one pixel = one 16-byte load, and -- with the weights packed on the host as [Kpad / 8][ldw][8] -- 8 consecutive k of one
// output channel = one 16-byte load.  The product is computed TRANSPOSED (weights as the A operand, pixels as the B operand): the
// C/D map (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) then puts the PIXEL on the lane and 4 consecutive output channels
// in 4 consecutive registers, so the epilogue stores 8 bytes (4 bf16) per instruction, reads the residual 8 bytes at a time and tests
// the row bound once per lane.
// Tile: 128 pixels x BN channels (BN = 128 | 64) x 32 k per workgroup of 4 waves (BN = 128: 2 x 2 waves of 64 x 64; BN = 64: 4 waves of
// 32 x 64), LDS double-buffered, the loads of step t + 1 issued before the MFMAs of step t, one barrier per K step.
// LDS images: A rows are 64 B of data + 16 B of padding (80-byte pitch: the 16-byte fragment reads of 32 consecutive rows fall on
// disjoint banks); B is [4 k-chunks][BN] 16-byte words, read by consecutive lanes at consecutive addresses.
#pragma once
#include "encoder.h"
#include "ihmr_pure.h"

#define CONVB_BK 32
#define CONVB_GENERIC 0
#define CONVB_FAST 1
#define CONVB_C4 2

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 mfma_bf16x8 __attribute__((ext_vector_type(8)));
#define CONVB_OPERAND(v) __builtin_bit_cast(mfma_bf16x8, (v))

struct ConvArgsBF16 {
    const uint16_t* x;         // input, NHWC bf16 with pixel stride ldx
    const uint16_t* w;         // [Kpad / 8][ldw][8] bf16 (k-interleaved, BN folded in, RNE), Kpad = ceil32(kh*kw*Cin), zero padded
    const float* bias;         // [Cout] fp32
    const uint16_t* residual;  // optional [M][ldr] bf16
    uint16_t* y;               // [M][ldy] bf16
    int N, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad;
    int ldx, ldw, ldy, ldr;
    int act;                   // 0 none, 1 relu
    float* partial;            // split-K: [ksplit][M][Cout] raw fp32 partial sums
    int ksplit;                // gridDim.z; 1 = no split
    int vec;                   // 1: Cout, ldy, ldr multiples of 4 and y / residual 8-byte aligned -> 8-byte epilogue accesses
};

// Zero page of the fast gather: a padding pixel's loader reads from here (Cin <= 4096)
__device__ __attribute__((aligned(16))) uint16_t g_conv_zero_bf16[4096 + 64];

__device__ __forceinline__ float bf16_widen(uint16_t v) { return __uint_as_float((unsigned)v << 16); }

// y = bf16(act(v + bias (+ residual))) for 4 consecutive output channels of one pixel
__device__ __forceinline__ void convb_finish4(const ConvArgsBF16& a, float (&v)[4], int m, int n) {
    if (a.vec) {
        if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
        if (a.residual) {
            const u16x4 r = *reinterpret_cast<const u16x4*>(a.residual + (size_t)m * a.ldr + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bf16_widen(r[e]);
        }
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ihmr_f32_to_bf16(a.act == 1 ? fmaxf(v[e], 0.f) : v[e]);
        *reinterpret_cast<u16x4*>(a.y + (size_t)m * a.ldy + n) = o;
    } else {
        for (int e = 0; e < 4; ++e) {
            if (n + e >= a.Cout) break;
            float t = v[e] + (a.bias ? a.bias[n + e] : 0.f);
            if (a.residual) t += bf16_widen(a.residual[(size_t)m * a.ldr + n + e]);
            a.y[(size_t)m * a.ldy + n + e] = ihmr_f32_to_bf16(a.act == 1 ? fmaxf(t, 0.f) : t);
        }
    }
}

template <int BN, int MODE>                                // MODE: CONVB_GENERIC, CONVB_FAST (Cin % 32 == 0, ldx % 8 == 0), CONVB_C4 (Cin == ldx == 4: the padded stem)
__global__ __launch_bounds__(256)
void conv_igemm_bf16_kernel(ConvArgsBF16 a) {
    constexpr int BM = 128, THREADS = 256;
    constexpr int WN = BN / 64, WM = 4 / WN, MI = BM / WM / 32;   // waves along n / m, 32-pixel blocks per wave (each wave: 32 MI pixels x 64 channels)
    constexpr int LDA = 5;                                 // 16-byte words per A row: 4 k-chunks + 1 of padding
    constexpr int B_V = 4 * BN / THREADS;                  // 16-byte loads of B per thread (2 or 1)
    __shared__ bf16x8 As[2][BM * LDA];
    __shared__ bf16x8 Bs[2][4 * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN, h = lane >> 5, l31 = lane & 31;
    const int M = a.N * a.Ho * a.Wo, K = a.kh * a.kw * a.Cin, nk_all = (K + CONVB_BK - 1) / CONVB_BK;
    // XCD-aware tile order (encoder.h: conv_igemm_kernel): XCD k = L % 8 takes the k-th contiguous eighth of the tile sequence, the
    // column tiles of one row tile adjacent in time.  Placement is a performance assumption only: any map gives the same tiles.
    int m0, n0;
    {
        const unsigned gy = gridDim.y, T = gridDim.x * gy, L = blockIdx.x + gridDim.x * blockIdx.y;
        const unsigned q = T >> 3, r = T & 7u, xcd = L & 7u, seq = xcd * q + min(xcd, r) + (L >> 3);
        m0 = (int)(seq / gy) * BM; n0 = (int)(seq % gy) * BN;
    }
    const int nk_per = (nk_all + a.ksplit - 1) / a.ksplit;
    const int kc0 = blockIdx.z * nk_per, kc1 = min(nk_all, kc0 + nk_per);

    f32x16 acc[MI][2];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // A loaders: thread -> rows (tid >> 2) and (tid >> 2) + 64 of the tile, k-chunk tid & 3 (8 consecutive k)
    const int chunk = tid & 3;
    int an[2], hbase[2], wbase[2];
    bool am_ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int am = m0 + (tid >> 2) + 64 * i;
        am_ok[i] = am < M;
        int aho = 0, awo = 0;
        an[i] = 0;
        if (am_ok[i]) { an[i] = am / (a.Ho * a.Wo); const int r = am % (a.Ho * a.Wo); aho = r / a.Wo; awo = r % a.Wo; }
        hbase[i] = aho * a.stride - a.pad; wbase[i] = awo * a.stride - a.pad;
    }
    // B loaders: 16-byte word g = tid + 256 i of the step's [4][BN] image; ldw >= n0 + BN (zero padded)
    const bf16x8* pb[B_V];
#pragma unroll
    for (int i = 0; i < B_V; ++i) {
        const int g = tid + i * THREADS;
        pb[i] = reinterpret_cast<const bf16x8*>(a.w) + (size_t)(kc0 * 4 + g / BN) * a.ldw + n0 + g % BN;
    }
    const size_t bstep = (size_t)4 * a.ldw;

    // FAST: wave-uniform filter tap / channel offset of the NEXT step to load and carried pixel pointers (the gather's index arithmetic
    // runs only when the tap changes; a padding pixel or a row past M reads the zero page -- no select after the load)
    int tap_c = 0, tap_h = 0, tap_w = 0;
    const uint16_t* pa[2] = {nullptr, nullptr};
    auto retap = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hi = hbase[i] + tap_h, wi = wbase[i] + tap_w;
            const bool ok = am_ok[i] && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
            pa[i] = (ok ? a.x + ((size_t)(an[i] * a.H + hi) * a.W + wi) * a.ldx : g_conv_zero_bf16) + tap_c + chunk * 8;
        }
    };
    if constexpr (MODE == CONVB_FAST) {
        const int k0 = kc0 * CONVB_BK, tap = k0 / a.Cin;
        tap_c = k0 % a.Cin; tap_h = tap / a.kw; tap_w = tap % a.kw;
        retap();
    }
    int kload = kc0;                                       // K step the next load_step() fetches
    bf16x8 areg[2], breg[B_V];
    auto load_step = [&]() {
        if constexpr (MODE == CONVB_FAST) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { areg[i] = *reinterpret_cast<const bf16x8*>(pa[i]); pa[i] += CONVB_BK; }
            tap_c += CONVB_BK;
            if (tap_c >= a.Cin) { tap_c = 0; if (++tap_w == a.kw) { tap_w = 0; ++tap_h; } retap(); }
        } else if constexpr (MODE == CONVB_C4) {
            // a chunk is 2 consecutive taps x 4 channels: two 8-byte pixel loads; taps past the last one (zero-padded K) give zeros
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int tap = kload * 8 + chunk * 2 + t, fh = tap / a.kw, fw = tap % a.kw;
                    const int hi = hbase[i] + fh, wi = wbase[i] + fw;
                    if (am_ok[i] && fh < a.kh && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W) {
                        const u16x4 p = *reinterpret_cast<const u16x4*>(a.x + ((size_t)(an[i] * a.H + hi) * a.W + wi) * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[4 * t + e] = (short)p[e];
                    }
                }
                areg[i] = v;
            }
        } else {
            // generic gather: any Cin / ldx, one element at a time with its own bounds test
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = kload * CONVB_BK + chunk * 8 + e, tap = k / a.Cin, c = k % a.Cin, fh = tap / a.kw, fw = tap % a.kw;
                    const int hi = hbase[i] + fh, wi = wbase[i] + fw;
                    if (am_ok[i] && k < K && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W)
                        v[e] = (short)a.x[((size_t)(an[i] * a.H + hi) * a.W + wi) * a.ldx + c];
                }
                areg[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < B_V; ++i) { breg[i] = *pb[i]; pb[i] += bstep; }
        ++kload;
    };
    auto store_step = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) As[buf][((tid >> 2) + 64 * i) * LDA + chunk] = areg[i];
#pragma unroll
        for (int i = 0; i < B_V; ++i) Bs[buf][tid + i * THREADS] = breg[i];
    };
    auto mfma_step = [&](int cur) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int c = 2 * s + h;                       // this lane's k-chunk: k = 16 s + 8 h + j
            bf16x8 xa[MI], wb[2];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) xa[mi] = As[cur][(wm * 32 * MI + mi * 32 + l31) * LDA + c];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) wb[ni] = Bs[cur][c * BN + wn * 64 + ni * 32 + l31];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(CONVB_OPERAND(wb[ni]), CONVB_OPERAND(xa[mi]), acc[mi][ni], 0, 0, 0);
        }
    };
    if (kc0 < kc1) { load_step(); store_step(0); }
    __syncthreads();
    for (int kc = kc0; kc < kc1; ++kc) {
        const int cur = (kc - kc0) & 1;
        if (kc + 1 < kc1) load_step();                     // in flight during the MFMAs below
        mfma_step(cur);
        if (kc + 1 < kc1) store_step(cur ^ 1);             // the other buffer: its readers finished before the previous barrier
        __syncthreads();
    }

    // ---- epilogue.  D is the transposed product: lane -> pixel (col = lane & 31), registers 4 g .. 4 g + 3 -> channels 8 g + 4 h + 0..3
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = m0 + wm * 32 * MI + mi * 32 + l31;
        if (m >= M) continue;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * 64 + ni * 32 + 8 * g + 4 * h;
                if (n >= a.Cout) continue;
                float v[4] = {acc[mi][ni][4 * g], acc[mi][ni][4 * g + 1], acc[mi][ni][4 * g + 2], acc[mi][ni][4 * g + 3]};
                if (a.ksplit > 1) {                        // raw partial sums; the reduce kernel finishes the layer
                    float* part = a.partial + ((size_t)blockIdx.z * M + m) * a.Cout + n;
                    if (a.vec) *reinterpret_cast<float4*>(part) = make_float4(v[0], v[1], v[2], v[3]);
                    else for (int e = 0; e < 4 && n + e < a.Cout; ++e) part[e] = v[e];
                } else {
                    convb_finish4(a, v, m, n);
                }
            }
    }
}

// split-K epilogue: y = bf16(act(sum_z partial[z] (ascending z: a fixed order) + bias + residual)); one thread per 4 output channels
__global__ __launch_bounds__(256)
void conv_splitk_reduce_bf16_kernel(ConvArgsBF16 a) {
    const int M = a.N * a.Ho * a.Wo, cv = (a.Cout + 3) / 4;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * cv) return;
    const int m = (int)(idx / cv), n = (int)(idx % cv) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec) {
        for (int z = 0; z < a.ksplit; ++z) {
            const float4 p = *reinterpret_cast<const float4*>(a.partial + ((size_t)z * M + m) * a.Cout + n);
            if (z == 0) { v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w; }
            else { v[0] += p.x; v[1] += p.y; v[2] += p.z; v[3] += p.w; }
        }
    } else {
        for (int e = 0; e < 4 && n + e < a.Cout; ++e) {
            v[e] = a.partial[(size_t)m * a.Cout + n + e];
            for (int z = 1; z < a.ksplit; ++z) v[e] += a.partial[((size_t)z * M + m) * a.Cout + n + e];
        }
    }
    convb_finish4(a, v, m, n);
}

// NCHW fp32 image -> NHWC bf16 with 4 channels (channel 3 zero), RNE; one thread per pixel, 8-byte stores
__global__ void image_to_nhwc4_bf16_kernel(const float* __restrict__ img, uint16_t* __restrict__ y, int N, int HW) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * HW) return;
    const long n = idx / HW, p = idx % HW;
    const float* s = img + (size_t)n * 3 * HW + p;
    u16x4 o;
    o[0] = ihmr_f32_to_bf16(s[0]); o[1] = ihmr_f32_to_bf16(s[HW]); o[2] = ihmr_f32_to_bf16(s[2 * (size_t)HW]); o[3] = 0;
    *reinterpret_cast<u16x4*>(y + (size_t)idx * 4) = o;
}

// MaxPool2d(kernel 3, stride 2, padding 1) on NHWC bf16 (exact: the maximum of bf16 values is one of them); one thread per (pixel, 8 channels)
__global__ void maxpool3x3s2_bf16_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = C / 8;
    const long total = (long)N * Ho * Wo * c8;
    if (idx >= total) return;
    const int c = (int)(idx % c8) * 8;
    long p = idx / c8;
    const int wo = (int)(p % Wo); p /= Wo;
    const int ho = (int)(p % Ho);
    const int n = (int)(p / Ho);
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
    for (int dh = 0; dh < 3; ++dh) {
        const int hi = ho * 2 + dh - 1;
        if (hi < 0 || hi >= H) continue;
        for (int dw = 0; dw < 3; ++dw) {
            const int wi = wo * 2 + dw - 1;
            if (wi < 0 || wi >= W) continue;
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + ((size_t)(n * H + hi) * W + wi) * C + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], bf16_widen((uint16_t)v[e]));
        }
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (short)(__float_as_uint(m[e]) >> 16);
    *reinterpret_cast<bf16x8*>(y + ((size_t)(n * Ho + ho) * Wo + wo) * C + c) = o;
}

// AvgPool2d(7) over the whole map + ReLU: bf16 in, fp32 sum in pixel order, fp32 out (row stride ldy); one thread per (image, 8 channels)
__global__ void avgpool_relu_bf16_kernel(const uint16_t* __restrict__ x, float* __restrict__ y, int N, int HW, int C, int ldy) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, c8 = C / 8;
    if (idx >= N * c8) return;
    const int n = idx / c8, c = (idx % c8) * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < HW; ++p) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + ((size_t)n * HW + p) * C + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += bf16_widen((uint16_t)v[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) y[(size_t)n * ldy + c + e] = fmaxf(s[e] / (float)HW, 0.f);
}

// fp32 -> bf16, RNE (ihmr_pure.h: ihmr_f32_to_bf16)
__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = ihmr_f32_to_bf16(x[i]);
}

// Training-time augmentation of IHMR-Baseline for a whole batch on the device: what the reference does per image in its DataLoader
// workers when `bash/train_baseline.sh` switches the six augmentations on --
//   BaselineDataset.preprocess_data     data/baseline_dataset.py:67-108   (the order of the steps)
//   DataProcessor.random_flip           data/data_preprocess.py:63-93
//   DataProcessor.random_rescale        data/data_preprocess.py:96-119    (cv2.resize + placement on a zero canvas)
//   DataProcessor.random_rotate         data/data_preprocess.py:122-143   (utils/rotate_utils.py: cv2.warpAffine, label rotations)
//   DataProcessor.color_jitter          data/data_preprocess.py:146-152   (torchvision 0.7 ColorJitter on PIL images)
//   DataProcessor.add_motion_blur       data/data_preprocess.py:155-159   (cv2.filter2D)
//   ToTensor + Normalize(0.5, 0.5)      data/baseline_dataset.py:41-44,202
// Every image step quantises to uint8 as the reference does, so each kernel reads the previous kernel's bytes from one of two
// (B,S,S,3) uint8 buffers (9.6 MB at batch 64: resident in the last-level cache) and writes the other.  Arithmetic = augment_pure.h.
// Byte-bound style of preprocess.h: a thread owns FOUR horizontally adjacent pixels (S % 4 == 0), 12-byte uint8 stores, 16-byte
// float stores by whichever kernel runs last (img_out non-NULL); per-sample geometry once per workgroup.  A sample whose switch for a
// step is off passes through that step unchanged.
#pragma once
#include "augment_pure.h"
#include "ihmr_common.h"
#include "preprocess.h"

#define AUG_THREADS 256
#define AUG_BLUR_MAX 33                 // largest blur kernel side
#define AUG_BLUR_TILE 32                // output tile side of aug_blur_kernel

// four pixels (12 bytes, 4-byte aligned: ox0 % 4 == 0) of image `img` (S,S,3)
__device__ __forceinline__ void aug_load4(const uint8_t* __restrict__ img, int S, int oy, int ox0, int v[4][3]) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(img + ((size_t)oy * S + ox0) * 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    v[0][0] = w0 & 0xff; v[0][1] = (w0 >> 8) & 0xff; v[0][2] = (w0 >> 16) & 0xff; v[1][0] = w0 >> 24;
    v[1][1] = w1 & 0xff; v[1][2] = (w1 >> 8) & 0xff; v[2][0] = (w1 >> 16) & 0xff; v[2][1] = w1 >> 24;
    v[2][2] = w2 & 0xff; v[3][0] = (w2 >> 8) & 0xff; v[3][1] = (w2 >> 16) & 0xff; v[3][2] = w2 >> 24;
}

// the four pixels to the uint8 image of sample b and, when f_out is given, to its three float planes (ToTensor, Normalize(0.5, 0.5))
__device__ __forceinline__ void aug_store4(const int v[4][3], int b, int S, int oy, int ox0, uint8_t* __restrict__ u8_out,
                                           float* __restrict__ f_out) {
    const size_t plane = (size_t)S * S;
    uint32_t* uw = reinterpret_cast<uint32_t*>(u8_out + ((size_t)b * plane + (size_t)oy * S + ox0) * 3);
    uw[0] = (uint32_t)v[0][0] | ((uint32_t)v[0][1] << 8) | ((uint32_t)v[0][2] << 16) | ((uint32_t)v[1][0] << 24);
    uw[1] = (uint32_t)v[1][1] | ((uint32_t)v[1][2] << 8) | ((uint32_t)v[2][0] << 16) | ((uint32_t)v[2][1] << 24);
    uw[2] = (uint32_t)v[2][2] | ((uint32_t)v[3][0] << 8) | ((uint32_t)v[3][1] << 16) | ((uint32_t)v[3][2] << 24);
    if (f_out) {
        float* o = f_out + (size_t)b * 3 * plane + (size_t)oy * S + ox0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 f;
            f.x = ((float)v[0][c] / 255.0f - 0.5f) / 0.5f; f.y = ((float)v[1][c] / 255.0f - 0.5f) / 0.5f;
            f.z = ((float)v[2][c] / 255.0f - 0.5f) / 0.5f; f.w = ((float)v[3][c] / 255.0f - 0.5f) / 0.5f;
            *reinterpret_cast<float4*>(o + c * plane) = f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- rescale + position
// cv2.resize(img, (new_size, new_size)) of the S x S image (cv::resize's three modes, pre_axis's coefficients), placed at
// (x_pos, y_pos) on a zero canvas.  grid = (ceil(S*S / 4 / 256), B)
struct AugRescale { double step; int mode; };
__global__ __launch_bounds__(AUG_THREADS) void aug_rescale_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                  float* __restrict__ img_out,
                                                                  const ihmr_aug_params* __restrict__ params, int S) {
    __shared__ AugRescale gsh;
    const int b = blockIdx.y;
    const int on = params[b].flags & IHMR_AUG_RESCALE;
    const int ns = params[b].new_size, xp = params[b].x_pos, yp = params[b].y_pos;
    if (threadIdx.x == 0) {
        AugRescale g;
        g.step = 1.0 / ((double)ns / (double)S);
        g.mode = ns == S ? 0 : (fabs(g.step - 2.0) < 2.220446049250313e-16 ? 1 : 2);
        gsh = g;
    }
    __syncthreads();
    const AugRescale g = gsh;
    const int p4 = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (p4 * 4 >= S * S) return;
    const int oy = (p4 * 4) / S, ox0 = (p4 * 4) % S;
    const uint8_t* src = in + (size_t)b * S * S * 3;
    int v[4][3];
    if (!on) {
        aug_load4(src, S, oy, ox0, v);
    } else {
        const size_t row = (size_t)S * 3;
        const int dy = oy - yp;
        const bool row_in = dy >= 0 && dy < ns;
        PreAxis ay = {0, 0, 0};
        const uint8_t *r0 = src, *r1 = src;
        if (row_in) {
            if (g.mode == 2) {
                ay = pre_axis(dy, g.step, S, false);
                r0 = src + (size_t)min(max(ay.s, 0), S - 1) * row;
                r1 = src + (size_t)min(max(ay.s + 1, 0), S - 1) * row;
            } else if (g.mode == 1) {
                r0 = src + (size_t)min(2 * dy, S - 1) * row; r1 = src + (size_t)min(2 * dy + 1, S - 1) * row;
            } else {
                r0 = src + (size_t)min(dy, S - 1) * row;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = ox0 + i - xp;
            v[i][0] = v[i][1] = v[i][2] = 0;
            if (row_in && dx >= 0 && dx < ns) {
                if (g.mode == 0) {
                    const uint8_t* q = r0 + (size_t)min(dx, S - 1) * 3;
                    v[i][0] = q[0]; v[i][1] = q[1]; v[i][2] = q[2];
                } else if (g.mode == 1) {
                    const size_t c0 = (size_t)min(2 * dx, S - 1) * 3, c1 = (size_t)min(2 * dx + 1, S - 1) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[i][c] = ((int)r0[c0 + c] + (int)r0[c1 + c] + (int)r1[c0 + c] + (int)r1[c1 + c] + 2) >> 2;
                } else {
                    const PreAxis ax = pre_axis(dx, g.step, S, true);
                    const int x0 = min(max(ax.s, 0), S - 1), x1 = min(ax.s + 1, S - 1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int h0 = (int)r0[(size_t)x0 * 3 + c] * ax.w0 + (int)r0[(size_t)x1 * 3 + c] * ax.w1;
                        const int h1 = (int)r1[(size_t)x0 * 3 + c] * ax.w0 + (int)r1[(size_t)x1 * 3 + c] * ax.w1;
                        v[i][c] = ((((ay.w0 * (h0 >> 4)) >> 16) + ((ay.w1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xff;
                    }
                }
            }
        }
    }
    aug_store4(v, b, S, oy, ox0, out, img_out);
}

// --------------------------------------------------------------------------------------------------------------- rotation
// cv2.warpAffine(img, M, (S, S), flags=INTER_LINEAR), constant zero border; params[b].warp = the inverted matrix
__global__ __launch_bounds__(AUG_THREADS) void aug_rotate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                 float* __restrict__ img_out,
                                                                 const ihmr_aug_params* __restrict__ params, int S) {
    const int b = blockIdx.y;
    const int p4 = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (p4 * 4 >= S * S) return;
    const int oy = (p4 * 4) / S, ox0 = (p4 * 4) % S;
    const uint8_t* src = in + (size_t)b * S * S * 3;
    int v[4][3];
    if (!(params[b].flags & IHMR_AUG_ROTATE)) {
        aug_load4(src, S, oy, ox0, v);
    } else {
        double m[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = params[b].warp[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const AugWarp w = aug_warp_coord(m, ox0 + i, oy);
            int wt[4];
            aug_warp_weights(w, wt);
            const bool x0 = w.sx >= 0 && w.sx < S, x1 = w.sx + 1 >= 0 && w.sx + 1 < S;
            const bool y0 = w.sy >= 0 && w.sy < S, y1 = w.sy + 1 >= 0 && w.sy + 1 < S;
            const uint8_t* q00 = src + ((size_t)(y0 ? w.sy : 0) * S + (x0 ? w.sx : 0)) * 3;
            const uint8_t* q01 = src + ((size_t)(y0 ? w.sy : 0) * S + (x1 ? w.sx + 1 : 0)) * 3;
            const uint8_t* q10 = src + ((size_t)(y1 ? w.sy + 1 : 0) * S + (x0 ? w.sx : 0)) * 3;
            const uint8_t* q11 = src + ((size_t)(y1 ? w.sy + 1 : 0) * S + (x1 ? w.sx + 1 : 0)) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[i][c] = aug_warp_value(wt, (y0 && x0) ? q00[c] : 0, (y0 && x1) ? q01[c] : 0, (y1 && x0) ? q10[c] : 0,
                                         (y1 && x1) ? q11[c] : 0);
        }
    }
    aug_store4(v, b, S, oy, ox0, out, img_out);
}

// ----------------------------------------------------------------------------------------------------------------- colour
// per sample: integer sum of the L image as it stands where contrast applies in that sample's order (the operations before it applied
// on the fly).  Exact and order-independent, so integer atomics are fine; S*S*255 fits uint32 up to S = 4104.  sums zeroed by the caller.
__global__ __launch_bounds__(AUG_THREADS) void aug_gray_sum_kernel(const uint8_t* __restrict__ in, const ihmr_aug_params* __restrict__ params,
                                                                   int S, uint32_t* __restrict__ sums) {
    __shared__ uint32_t ssum;
    const int b = blockIdx.y;
    if (!(params[b].flags & IHMR_AUG_COLOR)) return;                 // (uniform per workgroup)
    const ihmr_aug_params P = params[b];
    const int pos = aug_contrast_pos(&P);
    if (pos == 4) return;
    if (threadIdx.x == 0) ssum = 0;
    __syncthreads();
    const int p4 = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (p4 * 4 < S * S) {
        const int oy = (p4 * 4) / S, ox0 = (p4 * 4) % S;
        int v[4][3];
        aug_load4(in + (size_t)b * S * S * 3, S, oy, ox0, v);
        uint32_t local = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            aug_color_pixel(v[i], &P, pos, 0);
            local += (uint32_t)aug_gray(v[i][0], v[i][1], v[i][2]);
        }
        atomicAdd(&ssum, local);
    }
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[b], ssum);
}

// all four operations of ColorJitter in the sample's order, pointwise
__global__ __launch_bounds__(AUG_THREADS) void aug_color_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                float* __restrict__ img_out, const ihmr_aug_params* __restrict__ params,
                                                                int S, const uint32_t* __restrict__ sums) {
    const int b = blockIdx.y;
    const int p4 = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (p4 * 4 >= S * S) return;
    const int oy = (p4 * 4) / S, ox0 = (p4 * 4) % S;
    int v[4][3];
    aug_load4(in + (size_t)b * S * S * 3, S, oy, ox0, v);
    if (params[b].flags & IHMR_AUG_COLOR) {
        const ihmr_aug_params P = params[b];
        const int deg = aug_contrast_degenerate(sums[b], S * S);
#pragma unroll
        for (int i = 0; i < 4; ++i) aug_color_pixel(v[i], &P, 4, deg);
    }
    aug_store4(v, b, S, oy, ox0, out, img_out);
}

// ------------------------------------------------------------------------------------------------------------------- blur
// cv2.filter2D(img, -1, k): correlation, anchor (kw/2, kh/2), BORDER_REFLECT_101; float32 sum over the non-zero taps in row-major
// order (no contraction), rounded half to even, clamped.  bank: n kernels in slots of 33*33 floats (kh*kw values row-major at the
// head of the slot), dims (n,2) int32 = kh, kw; params[b].blur_kernel = slot, -1 = copy.
// grid = (ceil(S/32)^2, B), block 256: a 32 x 32 output tile, a thread owns four adjacent pixels of one row; the tile with its
// halo (at most 64 x 64 pixels) and the taps sit in LDS.
__global__ __launch_bounds__(AUG_THREADS) void aug_blur_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                               float* __restrict__ img_out, const ihmr_aug_params* __restrict__ params,
                                                               int S, const float* __restrict__ bank, const int32_t* __restrict__ dims,
                                                               int n_kernels) {
    constexpr int T = AUG_BLUR_TILE, TW = T + AUG_BLUR_MAX - 1;      // 64
    __shared__ uint8_t tile[TW * TW * 3];
    __shared__ float taps[AUG_BLUR_MAX * AUG_BLUR_MAX];
    const int b = blockIdx.y;
    const int tiles_x = (S + T - 1) / T;
    const int ty0 = (blockIdx.x / tiles_x) * T, tx0 = (blockIdx.x % tiles_x) * T;
    const int oy = ty0 + (int)threadIdx.x / 8, ox0 = tx0 + ((int)threadIdx.x % 8) * 4;
    const bool inside = oy < S && ox0 < S;
    const uint8_t* src = in + (size_t)b * S * S * 3;
    const int kid = params[b].blur_kernel;
    int v[4][3];
    if (kid < 0 || kid >= n_kernels) {                               // (uniform per workgroup)
        if (!inside) return;
        aug_load4(src, S, oy, ox0, v);
        aug_store4(v, b, S, oy, ox0, out, img_out);
        return;
    }
    const int kh = min(max(dims[2 * kid], 1), AUG_BLUR_MAX), kw = min(max(dims[2 * kid + 1], 1), AUG_BLUR_MAX);
    const int ay = kh / 2, ax = kw / 2;
    const int th = T + kh - 1, tw = T + kw - 1;
    for (int i = threadIdx.x; i < kh * kw; i += AUG_THREADS) taps[i] = bank[(size_t)kid * AUG_BLUR_MAX * AUG_BLUR_MAX + i];
    for (int i = threadIdx.x; i < th * tw; i += AUG_THREADS) {
        const int ry = i / tw, rx = i % tw;
        const uint8_t* q = src + ((size_t)aug_reflect101(ty0 - ay + ry, S) * S + aug_reflect101(tx0 - ax + rx, S)) * 3;
        uint8_t* t = tile + (ry * TW + rx) * 3;
        t[0] = q[0]; t[1] = q[1]; t[2] = q[2];
    }
    __syncthreads();
    if (!inside) return;
    float acc[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0f;
    const int ly = oy - ty0, lx = ox0 - tx0;
    for (int ky = 0; ky < kh; ++ky) {
        const uint8_t* trow = tile + ((ly + ky) * TW + lx) * 3;
        for (int kx = 0; kx < kw; ++kx) {
            const float w = taps[ky * kw + kx];
            if (w == 0.0f) continue;                                 // (uniform: filter2D keeps the non-zero taps only)
            const uint8_t* t = trow + kx * 3;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[i][c] = acc[i][c] + w * (float)t[i * 3 + c];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[i][c] = min(255, max(0, __float2int_rn(acc[i][c])));
    aug_store4(v, b, S, oy, ox0, out, img_out);
}

// ----------------------------------------------------------------------------------------------------------------- labels
// one workgroup (64 threads) per sample: padding_and_resize's joint scaling, flip, rescale, rotation, normalize_joints_2d and
// hand_trans (baseline_dataset.py:192-199, from the augmented joints_3d)
#define AUG_LABEL_THREADS 64
__global__ __launch_bounds__(AUG_LABEL_THREADS) void aug_labels_kernel(const int32_t* __restrict__ sizes, const ihmr_aug_params* __restrict__ params,
                                                                       int S, const float* __restrict__ joints_2d, const float* __restrict__ joints_3d,
                                                                       const float* __restrict__ mano_pose, const float* __restrict__ mano_betas,
                                                                       const float* __restrict__ mano_weight, const float* __restrict__ hand_type,
                                                                       float* __restrict__ o_joints_2d, float* __restrict__ o_joints_3d,
                                                                       float* __restrict__ o_pose, float* __restrict__ o_betas,
                                                                       float* __restrict__ o_weight, float* __restrict__ o_hand_type,
                                                                       float* __restrict__ o_do_flip, float* __restrict__ o_hand_trans) {
    __shared__ float pose[96];
    __shared__ float j3[42][4];
    const int b = blockIdx.x, t = threadIdx.x;
    const ihmr_aug_params P = params[b];
    const bool flip = P.flip != 0, rot = P.flags & IHMR_AUG_ROTATE;
    const float ratio = pre_geometry(sizes[2 * b], sizes[2 * b + 1], S).ratio;
    const float rz[3] = {0.0f, 0.0f, P.rot_z};
    float Rx[9];
    aug_aa_to_rotmat(rz, Rx);
    if (t < 42) {
        const int src = flip ? (t + 21) % 42 : t;                    // the two hands swap on a flip
        const float* q = joints_2d + ((size_t)b * 42 + src) * 3;
        float* o = o_joints_2d + ((size_t)b * 42 + t) * 3;
        aug_joint_2d(q[0] * ratio, q[1] * ratio, &P, S, o);
        o[2] = q[2];
        const float* q3 = joints_3d + ((size_t)b * 42 + src) * 4;
        float p3[3] = {flip ? -q3[0] : q3[0], q3[1], q3[2]};
        if (rot) {
            float r3[3];
            aug_rotate_joint_3d(Rx, p3, r3);
            p3[0] = r3[0]; p3[1] = r3[1]; p3[2] = r3[2];
        }
        j3[t][0] = p3[0]; j3[t][1] = p3[1]; j3[t][2] = p3[2]; j3[t][3] = q3[3];
    }
    for (int i = t; i < 96; i += AUG_LABEL_THREADS) {                // flip_hand_pose: hands swapped, y and z of every rotation negated
        const float x = mano_pose[(size_t)b * 96 + (flip ? (i + 48) % 96 : i)];
        pose[i] = (flip && i % 3 != 0) ? -x : x;
    }
    if (t < 20) o_betas[(size_t)b * 20 + t] = flip ? 0.0f : mano_betas[(size_t)b * 20 + t];   // the reference returns its zero-initialised betas
    if (t < 2) {
        o_weight[(size_t)b * 2 + t] = mano_weight[(size_t)b * 2 + (flip ? 1 - t : t)];
        o_hand_type[(size_t)b * 2 + t] = hand_type[(size_t)b * 2 + (flip ? 1 - t : t)];
    }
    __syncthreads();
    if (t == 0) {
        if (rot) {                                                   // random_rotate turns mano_pose[:3] only
            float o3[3];
            aug_rotate_orient(pose, P.rot_z, o3);
            pose[0] = o3[0]; pose[1] = o3[1]; pose[2] = o3[2];
        }
        o_do_flip[b] = flip ? 1.0f : 0.0f;
        float* ht = o_hand_trans + (size_t)b * 4;
        if (j3[0][3] > 0.0f && j3[21][3] > 0.0f) {
            ht[0] = -j3[0][0] + j3[21][0]; ht[1] = -j3[0][1] + j3[21][1]; ht[2] = -j3[0][2] + j3[21][2]; ht[3] = 1.0f;
        } else {
            ht[0] = ht[1] = ht[2] = ht[3] = 0.0f;
        }
    }
    __syncthreads();
    for (int i = t; i < 96; i += AUG_LABEL_THREADS) o_pose[(size_t)b * 96 + i] = pose[i];
    for (int i = t; i < 42 * 4; i += AUG_LABEL_THREADS) o_joints_3d[(size_t)b * 168 + i] = j3[i / 4][i % 4];
}

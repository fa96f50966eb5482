// Pure arithmetic of the training-time augmentation (csrc/augment.h inlines it) -- compilable for the HOST as well, like ihmr_pure.h:
// under hipcc `__host__ __device__`, under g++ ordinary inline functions (tests/test_augment_cpu.py builds tests/augment_host_driver.cpp
// with -fsanitize=address,undefined and compares every function with tests/augment_ref.py).  What it restates:
//   Pillow ImageEnhance.Brightness / Contrast / Color  = Image.blend(degenerate, image, factor)    (torchvision 0.7 ColorJitter)
//   Pillow convert("L"), convert("HSV"), convert("RGB") from HSV                                   (torchvision adjust_hue)
//   cv2.warpAffine(INTER_LINEAR) coordinates and weights, 8-bit (OpenCV 4.2.0 imgwarp.cpp; PARITY UNPINNED, see tests/augment_ref.py)
//   the label half of DataProcessor.random_flip / random_rescale / random_rotate                  (data/data_preprocess.py:63-143,
//                                                                                                   utils/rotate_utils.py, geometry_utils.py)
// Nothing here touches memory other than its arguments.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ihmr_hip.h"

#if defined(__HIPCC__)
#define AUG_PURE __host__ __device__ __forceinline__
#else
#define AUG_PURE static inline
#endif

// ------------------------------------------------------------------------------------------------------------------ colour
// Pillow's RGB -> L (ImagingConvert rgb2l): channel 0 plays R (the reference hands its BGR array to PIL as RGB)
AUG_PURE int aug_gray(int c0, int c1, int c2) { return (19595 * c0 + 38470 * c1 + 7471 * c2 + 0x8000) >> 16; }

// Image.blend(degenerate d, image a, alpha): float32 `d + alpha * (a - d)`, truncated; outside 0 <= alpha <= 1 clipped first
AUG_PURE int aug_blend(int a, int d, float alpha) {
    const float t = (float)d + alpha * (float)(a - d);
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t;
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)t;
}

// Pillow rgb2hsv_row for one pixel
AUG_PURE void aug_rgb2hsv(int r, int g, int b, int* hsv) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    hsv[2] = maxc;
    if (minc == maxc) { hsv[0] = 0; hsv[1] = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    int uh = (int)((double)h * 255.0), us = (int)((double)s * 255.0);
    hsv[0] = uh < 0 ? 0 : (uh > 255 ? 255 : uh);
    hsv[1] = us < 0 ? 0 : (us > 255 ? 255 : us);
}

// Pillow hsv2rgb for one pixel
AUG_PURE void aug_hsv2rgb(int h, int s, int v, int* rgb) {
    if (s == 0) { rgb[0] = rgb[1] = rgb[2] = v; return; }
    const double h6 = (double)h * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const double f = h6 - (double)i, fs = (double)s / 255.0;
    const int p = (int)floor((double)v * (1.0 - fs) + 0.5);
    const int q = (int)floor((double)v * (1.0 - fs * f) + 0.5);
    const int t = (int)floor((double)v * (1.0 - fs * (1.0 - f)) + 0.5);
    switch (i % 6) {
        case 0: rgb[0] = v; rgb[1] = t; rgb[2] = p; break;
        case 1: rgb[0] = q; rgb[1] = v; rgb[2] = p; break;
        case 2: rgb[0] = p; rgb[1] = v; rgb[2] = t; break;
        case 3: rgb[0] = p; rgb[1] = q; rgb[2] = v; break;
        case 4: rgb[0] = t; rgb[1] = p; rgb[2] = v; break;
        default: rgb[0] = v; rgb[1] = p; rgb[2] = q; break;
    }
}

// the colour part of one sample's parameters: operation ids 0 brightness, 1 contrast, 2 saturation, 3 hue (ColorJitter's list order)
#define AUG_OP_BRIGHTNESS 0
#define AUG_OP_CONTRAST 1
#define AUG_OP_SATURATION 2
#define AUG_OP_HUE 3

// one pixel through the first n_ops operations of the sample's order (contrast_deg: int(mean(L) + 0.5) of the image as it stands
// where contrast applies; unused while contrast is not among the n_ops)
AUG_PURE void aug_color_pixel(int* c, const ihmr_aug_params* p, int n_ops, int contrast_deg) {
    for (int k = 0; k < n_ops; ++k) {
        const int op = p->order[k];
        if (op == AUG_OP_BRIGHTNESS) {
            for (int i = 0; i < 3; ++i) c[i] = aug_blend(c[i], 0, p->brightness);
        } else if (op == AUG_OP_CONTRAST) {
            for (int i = 0; i < 3; ++i) c[i] = aug_blend(c[i], contrast_deg, p->contrast);
        } else if (op == AUG_OP_SATURATION) {
            const int L = aug_gray(c[0], c[1], c[2]);
            for (int i = 0; i < 3; ++i) c[i] = aug_blend(c[i], L, p->saturation);
        } else {
            int hsv[3];
            aug_rgb2hsv(c[0], c[1], c[2], hsv);
            aug_hsv2rgb((hsv[0] + p->hue_shift) & 0xff, hsv[1], hsv[2], c);
        }
    }
}

// position of contrast in the order (4 when absent)
AUG_PURE int aug_contrast_pos(const ihmr_aug_params* p) {
    for (int k = 0; k < 4; ++k)
        if (p->order[k] == AUG_OP_CONTRAST) return k;
    return 4;
}

// ImageEnhance.Contrast's degenerate value: int(mean + 0.5), the mean of the L image in double
AUG_PURE int aug_contrast_degenerate(uint32_t gray_sum, int n_pixels) { return (int)((double)gray_sum / (double)n_pixels + 0.5); }

// -------------------------------------------------------------------------------------------------------------------- warp
// cv::warpAffine, 8-bit INTER_LINEAR: fixed-point source coordinate of destination (x, y) under the inverted matrix m (AB_BITS = 10,
// INTER_BITS = 5): source column / row and the 1/32 fractions
struct AugWarp { int sx, sy, fx, fy; };
AUG_PURE int aug_cvround(double v) { return (int)rint(v); }               // cvRound: to nearest, ties to even
AUG_PURE AugWarp aug_warp_coord(const double* m, int x, int y) {
    const int adelta = aug_cvround(m[0] * (double)x * 1024.0), bdelta = aug_cvround(m[3] * (double)x * 1024.0);
    const int X0 = aug_cvround((m[1] * (double)y + m[2]) * 1024.0) + 16, Y0 = aug_cvround((m[4] * (double)y + m[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    AugWarp w;
    w.sx = X >> 5; w.sy = Y >> 5; w.fx = X & 31; w.fy = Y & 31;
    return w;
}
// the four bilinear weights (sum 32768): taps (sx,sy), (sx+1,sy), (sx,sy+1), (sx+1,sy+1)
AUG_PURE void aug_warp_weights(const AugWarp& w, int* wt) {
    wt[0] = (32 - w.fx) * (32 - w.fy) * 32; wt[1] = w.fx * (32 - w.fy) * 32;
    wt[2] = (32 - w.fx) * w.fy * 32; wt[3] = w.fx * w.fy * 32;
}
AUG_PURE int aug_warp_value(const int* wt, int p00, int p01, int p10, int p11) {
    return (wt[0] * p00 + wt[1] * p01 + wt[2] * p10 + wt[3] * p11 + 16384) >> 15;
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
AUG_PURE int aug_reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------ labels
// geometry_utils.angle_axis_to_rotation_matrix (float32, torch's operation order), 3x3 row-major
AUG_PURE void aug_aa_to_rotmat(const float* r, float* R) {
    const float theta2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    if (theta2 > 1e-6f) {
        const float theta = sqrtf(theta2);
        const float wx = r[0] / (theta + 1e-6f), wy = r[1] / (theta + 1e-6f), wz = r[2] / (theta + 1e-6f);
        const float c = cosf(theta), s = sinf(theta), k = 1.0f - c;
        R[0] = c + wx * wx * k;        R[1] = wx * wy * k - wz * s;   R[2] = wy * s + wx * wz * k;
        R[3] = wz * s + wx * wy * k;   R[4] = c + wy * wy * k;        R[5] = -wx * s + wy * wz * k;
        R[6] = -wy * s + wx * wz * k;  R[7] = wx * s + wy * wz * k;   R[8] = c + wz * wz * k;
    } else {
        R[0] = 1.0f; R[1] = -r[2]; R[2] = r[1];
        R[3] = r[2]; R[4] = 1.0f;  R[5] = -r[0];
        R[6] = -r[1]; R[7] = r[0]; R[8] = 1.0f;
    }
}

// geometry_utils.rotation_matrix_to_angle_axis (rotation_matrix_to_quaternion + quaternion_to_angle_axis), R 3x3 row-major
AUG_PURE void aug_rotmat_to_aa(const float* R, float* aa) {
#define AUG_M(i, j) R[(j) * 3 + (i)]                                         // rmat_t = transpose(R)
    const bool d2 = AUG_M(2, 2) < 1e-6f, d0_d1 = AUG_M(0, 0) > AUG_M(1, 1), d0_nd1 = AUG_M(0, 0) < -AUG_M(1, 1);
    float q[4], t;
    if (d2 && d0_d1) {
        t = 1.0f + AUG_M(0, 0) - AUG_M(1, 1) - AUG_M(2, 2);
        q[0] = AUG_M(1, 2) - AUG_M(2, 1); q[1] = t; q[2] = AUG_M(0, 1) + AUG_M(1, 0); q[3] = AUG_M(2, 0) + AUG_M(0, 2);
    } else if (d2) {
        t = 1.0f - AUG_M(0, 0) + AUG_M(1, 1) - AUG_M(2, 2);
        q[0] = AUG_M(2, 0) - AUG_M(0, 2); q[1] = AUG_M(0, 1) + AUG_M(1, 0); q[2] = t; q[3] = AUG_M(1, 2) + AUG_M(2, 1);
    } else if (d0_nd1) {
        t = 1.0f - AUG_M(0, 0) - AUG_M(1, 1) + AUG_M(2, 2);
        q[0] = AUG_M(0, 1) - AUG_M(1, 0); q[1] = AUG_M(2, 0) + AUG_M(0, 2); q[2] = AUG_M(1, 2) + AUG_M(2, 1); q[3] = t;
    } else {
        t = 1.0f + AUG_M(0, 0) + AUG_M(1, 1) + AUG_M(2, 2);
        q[0] = t; q[1] = AUG_M(1, 2) - AUG_M(2, 1); q[2] = AUG_M(2, 0) - AUG_M(0, 2); q[3] = AUG_M(0, 1) - AUG_M(1, 0);
    }
#undef AUG_M
    const float rt = sqrtf(t);
    for (int i = 0; i < 4; ++i) q[i] = (q[i] / rt) * 0.5f;
    const float sin2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const float sin_t = sqrtf(sin2), cos_t = q[0];
    const float two_theta = 2.0f * (cos_t < 0.0f ? atan2f(-sin_t, -cos_t) : atan2f(sin_t, cos_t));
    const float k = sin2 > 0.0f ? two_theta / sin_t : 2.0f;
    aa[0] = q[1] * k; aa[1] = q[2] * k; aa[2] = q[3] * k;
}

// rotate_utils.rotate_orient: orient <- angle_axis(R_z(rot_z) . R(orient)), rot_z = (float)(-pi * angle / 180)
AUG_PURE void aug_rotate_orient(const float* orient, float rot_z, float* out) {
    float Rt[9], Rx[9], Rn[9];
    const float rz[3] = {0.0f, 0.0f, rot_z};
    aug_aa_to_rotmat(orient, Rt);
    aug_aa_to_rotmat(rz, Rx);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = Rx[i * 3 + 0] * Rt[0 * 3 + j] + Rx[i * 3 + 1] * Rt[1 * 3 + j] + Rx[i * 3 + 2] * Rt[2 * 3 + j];
    aug_rotmat_to_aa(Rn, out);
}

// rotate_utils.rotate_joints_3d: R_z(rot_z) . j in float32
AUG_PURE void aug_rotate_joint_3d(const float* Rx, const float* j, float* out) {
    for (int i = 0; i < 3; ++i) out[i] = Rx[i * 3 + 0] * j[0] + Rx[i * 3 + 1] * j[1] + Rx[i * 3 + 2] * j[2];
}

// 2-D joint (x, y already scaled by padding_and_resize's ratio) through flip / rescale / rotation / normalize_joints_2d.  numpy's types:
// float32 up to the rotation; rotate_joints_2d subtracts a float64 origin array, so from there on (normalisation included) the
// reference computes in float64 and rounds once at the end (`torch.from_numpy(joints_2d).float()`).
AUG_PURE void aug_joint_2d(float x, float y, const ihmr_aug_params* p, int S, float* out) {
    if (p->flip) x = (float)S - x;
    if (p->flags & IHMR_AUG_RESCALE) {
        x *= p->scale; y *= p->scale;
        x += (float)p->x_pos; y += (float)p->y_pos;
    }
    if (p->flags & IHMR_AUG_ROTATE) {
        const double o = (double)S / 2.0;
        const double dx = (double)x - o, dy = (double)y - o;
        const double rx = o + p->rot_cos * dx - p->rot_sin * dy, ry = o + p->rot_sin * dx + p->rot_cos * dy;
        out[0] = (float)((rx / (double)S) * 2.0 - 1.0);
        out[1] = (float)((ry / (double)S) * 2.0 - 1.0);
    } else {
        out[0] = (x / (float)S) * 2.0f - 1.0f;
        out[1] = (y / (float)S) * 2.0f - 1.0f;
    }
}

// The tables every LBS, tail and collision kernel reads, built from the MANO asset on the HOST: plain C++17, no HIP header, no globals.
// ihmr_mano_create (ihmr_hip.hip) uploads a ManoTables member by member; tests/mano_tables_driver.cpp is built by g++ with
// -fsanitize=address,undefined and tests/test_mano_tables_cpu.py checks what it builds against the layouts written at struct ihmr_mano
// (ihmr_common.h).  The sizes of those layouts are defined here, once, for the kernels too.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/ihmr_hip.h"

#define NV IHMR_NUM_VERTS      // 778
#define NF IHMR_NUM_FACES      // 1538
#define NJ IHMR_NUM_JOINTS     // 16
#define NV3 (NV * 3)           // 2334
#define NPF 135                // pose-feature length (15 joints x 9)
#define NFP 1600               // faces padded to a multiple of 64 (SoA row length)
#define NVP 832                // vertices padded to a multiple of 64 (float4 basis rows)
#define LBS_SEG 13             // CSR entries per dA segment
#define LBS_SEG_CAP 1024       // >= 778*16/13 + 16: every weight matrix fits

struct ManoTables {            // one vector per device buffer of ihmr_mano, same names, same layouts
    std::vector<float> v_template, shapedirs_t, posedirs, pd4, sd4, vt4, J_template, J_shapedirs, weights, w4_w, pose_mean, wj_w, J_regressor;
    std::vector<uint32_t> w4_j, faces_pk;
    std::vector<int32_t> parents, depth, tip_ids, wj_start, wj_vert, seg_q, jseg_start, faces;
    int sparse4 = 1, max_depth = 0, nnz = 0, nseg = 0;
};

// [rows][2334] -> [rows][NVP] float4 (x, y, z, 0), rows of zeros behind vertex 777
static inline void mano_pack4(const std::vector<float>& src, int rows, std::vector<float>& dst) {
    dst.assign((size_t)rows * NVP * 4, 0.f);
    for (int r = 0; r < rows; ++r)
        for (int v = 0; v < NV; ++v)
            for (int k = 0; k < 3; ++k) dst[((size_t)r * NVP + v) * 4 + k] = src[(size_t)r * NV3 + 3 * v + k];
}

// what depends on shapedirs (778,3,10): shapedirs_t, sd4, J_shapedirs -- and J_template, which shares the loop -- from t.J_regressor
// and t.v_template.  ihmr_mano_update_shapedirs calls this alone.
static inline void build_shape_tables(const float* shapedirs, ManoTables& t) {
    const float* Jreg = t.J_regressor.data();
    t.shapedirs_t.assign((size_t)10 * NV3, 0.f);
    for (int v = 0; v < NV; ++v)
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < 10; ++l) t.shapedirs_t[(size_t)l * NV3 + 3 * v + k] = shapedirs[(v * 3 + k) * 10 + l];
    t.J_template.assign(48, 0.f);
    t.J_shapedirs.assign(480, 0.f);
    for (int j = 0; j < NJ; ++j)
        for (int k = 0; k < 3; ++k) {
            double acc = 0.0;
            for (int v = 0; v < NV; ++v) acc += (double)Jreg[j * NV + v] * (double)t.v_template[3 * v + k];
            t.J_template[j * 3 + k] = (float)acc;
            for (int l = 0; l < 10; ++l) {
                double a2 = 0.0;
                for (int v = 0; v < NV; ++v) a2 += (double)Jreg[j * NV + v] * (double)shapedirs[(v * 3 + k) * 10 + l];
                t.J_shapedirs[(j * 3 + k) * 10 + l] = (float)a2;
            }
        }
    mano_pack4(t.shapedirs_t, 10, t.sd4);
}

// 0, or -1 for an asset the kernels cannot take: a parent that does not precede its joint, a face id outside [0, 778), more than
// LBS_SEG_CAP segments
static inline int build_mano_tables(const ihmr_mano_arrays& h, ManoTables& t) {
    t.v_template.assign(h.v_template, h.v_template + NV3);
    t.posedirs.assign(h.posedirs, h.posedirs + (size_t)NPF * NV3);
    t.weights.assign(h.lbs_weights, h.lbs_weights + NV * NJ);
    t.J_regressor.assign(h.J_regressor, h.J_regressor + NJ * NV);
    t.parents.assign(h.parents, h.parents + NJ);
    t.tip_ids.assign(h.tip_ids, h.tip_ids + IHMR_NUM_TIPS);
    build_shape_tables(h.shapedirs, t);
    mano_pack4(t.posedirs, NPF, t.pd4);
    mano_pack4(t.v_template, 1, t.vt4);
    t.pose_mean.assign(48, 0.f);
    for (int i = 0; i < 45; ++i) t.pose_mean[3 + i] = h.hands_mean[i];
    t.depth.assign(NJ, 0);
    t.max_depth = 0;
    for (int j = 1; j < NJ; ++j) {
        if (t.parents[j] < 0 || t.parents[j] >= j) return -1;
        t.depth[j] = t.depth[t.parents[j]] + 1;
        if (t.depth[j] > t.max_depth) t.max_depth = t.depth[j];
    }
    const std::vector<float>& wts = t.weights;
    t.wj_start.assign(NJ + 1, 0);
    t.wj_vert.clear();
    t.wj_w.clear();
    for (int j = 0; j < NJ; ++j) {
        for (int v = 0; v < NV; ++v)
            if (wts[v * NJ + j] != 0.f) { t.wj_vert.push_back(v); t.wj_w.push_back(wts[v * NJ + j]); }
        t.wj_start[j + 1] = (int32_t)t.wj_vert.size();
    }
    t.nnz = (int)t.wj_vert.size();
    // by vertex: the (up to) four non-zero weights in joint order (a zero weight adds an exact zero to the skinning sums, so
    // leaving the zeros out changes no bit); an asset with a denser vertex keeps the 16-joint loops
    t.w4_w.assign((size_t)NV * 4, 0.f);
    t.w4_j.assign(NV, 0u);
    t.sparse4 = 1;
    for (int v = 0; v < NV; ++v) {
        int n = 0;
        for (int j = 0; j < NJ; ++j)
            if (wts[v * NJ + j] != 0.f) {
                if (n < 4) { t.w4_w[(size_t)v * 4 + n] = wts[v * NJ + j]; t.w4_j[v] |= (uint32_t)j << (8 * n); }
                ++n;
            }
        if (n > 4) t.sparse4 = 0;
    }
    // segment s of joint j ends at min(next segment start, end of the joint's list)
    t.seg_q.clear();
    t.jseg_start.assign(NJ + 1, 0);
    for (int j = 0; j < NJ; ++j) {
        t.jseg_start[j] = (int32_t)t.seg_q.size();
        for (int q = t.wj_start[j]; q < t.wj_start[j + 1]; q += LBS_SEG) t.seg_q.push_back(q);
    }
    t.jseg_start[NJ] = (int32_t)t.seg_q.size();
    t.seg_q.push_back((int32_t)t.nnz);
    t.nseg = (int)t.seg_q.size() - 1;
    if (t.nseg > LBS_SEG_CAP) return -1;
    t.faces.assign((size_t)3 * NFP, 0);
    for (int f = 0; f < NFP; ++f)
        for (int k = 0; k < 3; ++k) {
            const int32_t id = h.faces[(f < NF ? f : 0) * 3 + k];
            if (id < 0 || id >= NV) return -1;
            t.faces[(size_t)k * NFP + f] = id;
        }
    t.faces_pk.assign(NFP, 0u);
    for (int f = 0; f < NFP; ++f)
        t.faces_pk[f] = (uint32_t)t.faces[f] | ((uint32_t)t.faces[(size_t)NFP + f] << 10) | ((uint32_t)t.faces[(size_t)2 * NFP + f] << 20);
    return 0;
}

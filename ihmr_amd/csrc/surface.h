// Exact point-to-surface signed distance and its gradient (statement and arithmetic: surface_pure.h).
//
//   surface_dist_kernel      one workgroup per (sample, chunk of 256 queries), the chunks of a sample consecutive.  The sample's
//                            vertices (float32) and its face table (packed ids + the usable flag, formed once per face by a thread
//                            per face) sit in LDS; every lane walks the SAME face for its own query, so each LDS read is one
//                            wave-uniform broadcast.  A thread keeps the running minimum (square, face, v, w) and the ray parity in
//                            registers and writes its query's words itself.
//   surface_dist_bwd_kernel  one workgroup per sample.  In chunks of 256 queries a thread forms its query's (face ids, weights, g n) into
//                            LDS and writes d_points; then every thread walks the chunk in ascending query order and adds, in float64,
//                            -w_k g n where the query's face names one of the (at most 4) vertices it owns.  One rounding to float32 at
//                            the end: the sum has one order, the result is the same on every run.
// A sample with use[b] == 0 writes zeros (face = -1) and does no work.  No float atomics, no scratch, nothing passes from one workgroup
// to another; a sample's words do not depend on its place in the batch.
#pragma once
#include "ihmr_common.h"
#include "surface_pure.h"

struct SurfaceLds {
    float v[SRF_MAX_VERTS * 3];
    unsigned face[SRF_MAX_FACES];
};
static_assert(sizeof(SurfaceLds) == SRF_LDS_BYTES, "surface_pure.h names the LDS of surface_dist_kernel");
static_assert(SRF_MAX_VERTS == IHMR_SURFACE_MAX_VERTS && SRF_MAX_FACES == IHMR_SURFACE_MAX_FACES, "surface_pure.h and ihmr_hip.h name one limit");
static_assert(SRF_MAX_VERTS <= 1024, "a vertex id has 10 bits in a face record");

__global__ __launch_bounds__(SRF_THREADS) void surface_dist_kernel(const float* __restrict__ points, int P, const float* __restrict__ verts,
                                                                    int V, const int32_t* __restrict__ faces, int F_dist, int F_total,
                                                                    const uint8_t* __restrict__ use, int n_chunks, int is_signed,
                                                                    double* __restrict__ dist, int32_t* __restrict__ face,
                                                                    double* __restrict__ bary) {
    __shared__ SurfaceLds L;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
    const int p = chunk * SRF_THREADS + tid;
    const size_t at = (size_t)b * P + p;
    if (use && !use[b]) {                       // (uniform)
        if (p < P) {
            dist[at] = 0.0;
            face[at] = -1;
            bary[3 * at] = 0.0; bary[3 * at + 1] = 0.0; bary[3 * at + 2] = 0.0;
        }
        return;
    }
    const float* vb = verts + (size_t)b * V * 3;
    for (int i = tid; i < 3 * V; i += SRF_THREADS) L.v[i] = vb[i];
    __syncthreads();
    for (int f = tid; f < F_total; f += SRF_THREADS) {
        const unsigned ia = (unsigned)faces[3 * f], ib = (unsigned)faces[3 * f + 1], ic = (unsigned)faces[3 * f + 2];
        unsigned rec = 0u;
        if (ia < (unsigned)V && ib < (unsigned)V && ic < (unsigned)V) {
            const double a[3] = {(double)L.v[3 * ia], (double)L.v[3 * ia + 1], (double)L.v[3 * ia + 2]};
            const double bb[3] = {(double)L.v[3 * ib], (double)L.v[3 * ib + 1], (double)L.v[3 * ib + 2]};
            const double c[3] = {(double)L.v[3 * ic], (double)L.v[3 * ic + 1], (double)L.v[3 * ic + 2]};
            if (srf_face_usable(a, bb, c)) rec = srf_pack_face(ia, ib, ic);
        }
        L.face[f] = rec;
    }
    __syncthreads();
    if (p >= P) return;                         // (no barrier follows)
    const float* qf = points + at * 3;
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    double best = (double)INFINITY, bv = 0.0, bw = 0.0;
    int bf = -1;
    bool inside = false;
    if (srf_finite(q[0]) && srf_finite(q[1]) && srf_finite(q[2])) {
        for (int f = 0; f < F_total; ++f) {
            const unsigned rec = L.face[f];     // the same word in every lane
            if (!(rec & SRF_FACE_USABLE)) continue;
            int ia, ib, ic;
            srf_unpack_face(rec, ia, ib, ic);
            const double a[3] = {(double)L.v[3 * ia], (double)L.v[3 * ia + 1], (double)L.v[3 * ia + 2]};
            const double bb[3] = {(double)L.v[3 * ib], (double)L.v[3 * ib + 1], (double)L.v[3 * ib + 2]};
            const double c[3] = {(double)L.v[3 * ic], (double)L.v[3 * ic + 1], (double)L.v[3 * ic + 2]};
            if (f < F_dist) {
                double v, w;
                const double sq = srf_point_tri(q, a, bb, c, v, w);
                if (srf_min_update(best, sq)) { bf = f; bv = v; bw = w; }
            }
            if (is_signed && srf_ray_crosses(q, a, bb, c)) inside = !inside;
        }
    }
    double wts[3] = {0.0, 0.0, 0.0};
    if (bf >= 0) srf_weights(bv, bw, wts);
    dist[at] = srf_finish(best, bf, inside);
    face[at] = bf;
    bary[3 * at] = wts[0]; bary[3 * at + 1] = wts[1]; bary[3 * at + 2] = wts[2];
}

struct SurfaceBwdLds {
    int id[SRF_THREADS][3];                     // the vertex ids of the query's face, -1 where the query adds nothing
    double w[SRF_THREADS][3];
    double gn[SRF_THREADS][3];                  // g * n
};
static_assert(sizeof(SurfaceBwdLds) == SRF_BWD_LDS_BYTES, "surface_pure.h names the LDS of surface_dist_bwd_kernel");
static_assert(SRF_BWD_SLOTS * SRF_THREADS >= SRF_MAX_VERTS, "a thread owns at most SRF_BWD_SLOTS vertices");

__global__ __launch_bounds__(SRF_THREADS) void surface_dist_bwd_kernel(const float* __restrict__ points, int P,
                                                                        const float* __restrict__ verts, int V,
                                                                        const int32_t* __restrict__ faces, int F_dist,
                                                                        const uint8_t* __restrict__ use, const double* __restrict__ dist,
                                                                        const int32_t* __restrict__ face, const double* __restrict__ bary,
                                                                        const double* __restrict__ g_dist, float* __restrict__ d_points,
                                                                        float* __restrict__ d_verts) {
    __shared__ SurfaceBwdLds L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* vb = verts + (size_t)b * V * 3;
    float* dv = d_verts ? d_verts + (size_t)b * V * 3 : nullptr;
    if (use && !use[b]) {                       // (uniform)
        if (d_points) for (int i = tid; i < 3 * P; i += SRF_THREADS) d_points[(size_t)b * P * 3 + i] = 0.f;
        if (dv) for (int i = tid; i < 3 * V; i += SRF_THREADS) dv[i] = 0.f;
        return;
    }
    double acc[SRF_BWD_SLOTS][3];
#pragma unroll
    for (int s = 0; s < SRF_BWD_SLOTS; ++s) { acc[s][0] = 0.0; acc[s][1] = 0.0; acc[s][2] = 0.0; }
    for (int base = 0; base < P; base += SRF_THREADS) {
        const int p = base + tid;
        int id[3] = {-1, -1, -1};
        double w[3] = {0.0, 0.0, 0.0}, gn[3] = {0.0, 0.0, 0.0};
        if (p < P) {
            const size_t at = (size_t)b * P + p;
            const int f = face[at];
            if (f >= 0 && f < F_dist) {
                const unsigned ia = (unsigned)faces[3 * f], ib = (unsigned)faces[3 * f + 1], ic = (unsigned)faces[3 * f + 2];
                if (ia < (unsigned)V && ib < (unsigned)V && ic < (unsigned)V) {
                    const double q[3] = {(double)points[3 * at], (double)points[3 * at + 1], (double)points[3 * at + 2]};
                    const double a[3] = {(double)vb[3 * ia], (double)vb[3 * ia + 1], (double)vb[3 * ia + 2]};
                    const double bb[3] = {(double)vb[3 * ib], (double)vb[3 * ib + 1], (double)vb[3 * ib + 2]};
                    const double c[3] = {(double)vb[3 * ic], (double)vb[3 * ic + 1], (double)vb[3 * ic + 2]};
                    w[0] = bary[3 * at]; w[1] = bary[3 * at + 1]; w[2] = bary[3 * at + 2];
                    double n[3];
                    srf_grad_dir(q, a, bb, c, w, dist[at], n);
                    const double g = g_dist[at];
                    if (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0) {
                        id[0] = (int)ia; id[1] = (int)ib; id[2] = (int)ic;
                        gn[0] = g * n[0]; gn[1] = g * n[1]; gn[2] = g * n[2];
                    }
                }
            }
            if (d_points) { d_points[3 * at] = (float)gn[0]; d_points[3 * at + 1] = (float)gn[1]; d_points[3 * at + 2] = (float)gn[2]; }
        }
        if (!dv) continue;                      // (uniform)
        __syncthreads();                        // the walk of the chunk before has read its entries
#pragma unroll
        for (int k = 0; k < 3; ++k) { L.id[tid][k] = id[k]; L.w[tid][k] = w[k]; L.gn[tid][k] = gn[k]; }
        __syncthreads();
        const int n_here = min(SRF_THREADS, P - base);
        for (int j = 0; j < n_here; ++j) {      // ascending query order; every lane reads the same entry
            const int i0 = L.id[j][0];
            if (i0 < 0) continue;               // (uniform)
            const int ids[3] = {i0, L.id[j][1], L.id[j][2]};
            const double m[3] = {L.gn[j][0], L.gn[j][1], L.gn[j][2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double wk = L.w[j][k];
#pragma unroll
                for (int s = 0; s < SRF_BWD_SLOTS; ++s)
                    if (ids[k] == tid + SRF_THREADS * s) {
                        acc[s][0] -= wk * m[0]; acc[s][1] -= wk * m[1]; acc[s][2] -= wk * m[2];
                    }
            }
        }
    }
    if (dv) {
#pragma unroll
        for (int s = 0; s < SRF_BWD_SLOTS; ++s) {
            const int v = tid + SRF_THREADS * s;
            if (v < V) { dv[3 * v] = (float)acc[s][0]; dv[3 * v + 1] = (float)acc[s][1]; dv[3 * v + 2] = (float)acc[s][2]; }
        }
    }
}

static bool srf_shape_ok(int P, int V, int F_dist, int F_total, int B) {
    return B >= 1 && P >= 1 && V >= 1 && V <= SRF_MAX_VERTS && F_total <= SRF_MAX_FACES && F_dist >= 1 && F_dist <= F_total;
}

static int srf_launch(const float* points, int P, const float* verts, int V, const int32_t* faces, int F_dist, int F_total,
                      const uint8_t* use, int B, int is_signed, double* dist, int32_t* face, double* bary, hipStream_t stream) {
    if (!points || !verts || !faces || !dist || !face || !bary || !srf_shape_ok(P, V, F_dist, F_total, B)) return -1;
    const long long n_chunks = ((long long)P + SRF_THREADS - 1) / SRF_THREADS;
    if (n_chunks * B > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(surface_dist_kernel, dim3((unsigned)(n_chunks * B)), dim3(SRF_THREADS), 0, stream, points, P, verts, V, faces, F_dist,
                       F_total, use, (int)n_chunks, is_signed, dist, face, bary);
    return (int)hipGetLastError();
}

static int srf_launch_bwd(const float* points, int P, const float* verts, int V, const int32_t* faces, int F_dist, int F_total,
                          const uint8_t* use, int B, const double* dist, const int32_t* face, const double* bary, const double* g_dist,
                          float* d_points, float* d_verts, hipStream_t stream) {
    if (!points || !verts || !faces || !dist || !face || !bary || !g_dist || !srf_shape_ok(P, V, F_dist, F_total, B)) return -1;
    if (!d_points && !d_verts) return 0;
    hipLaunchKernelGGL(surface_dist_bwd_kernel, dim3(B), dim3(SRF_THREADS), 0, stream, points, P, verts, V, faces, F_dist, use, dist, face,
                       bary, g_dist, d_points, d_verts);
    return (int)hipGetLastError();
}

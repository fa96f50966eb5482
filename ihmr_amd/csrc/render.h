// Mesh renderer of the visualisation path (ihmr_render_meshes / ihmr_draw_keypoints, include/ihmr_hip.h): a batched triangle
// rasteriser in place of the reference's OpenDR scene (utils/render_color_utils.py, utils/vis_util.py).  The arithmetic is
// csrc/render_pure.h, shared with the host build the CPU tests run; this file only distributes it over the machine:
//   render_vertex_kernel   grid (vertex blocks, B): vertex normal from the incident-face CSR (ascending faces, no atomics), shading,
//                          projection and snap -> one 24-byte rnd_vertex per vertex in the workspace
//   render_raster_kernel   grid (tiles, B), 256 threads per 32 x 32 pixel tile, four horizontally adjacent pixels per thread.  The face
//                          table is walked in chunks of 256: every thread sets up one face and tests its bounding box against the tile,
//                          the survivors are compacted in face order (ballot + per-wave counts) into an LDS list of at most 256 records
//                          -- a chunk can never overflow it --, then every thread walks the list with broadcast LDS reads.  Depth, face
//                          id and the interpolation weights of the visible face stay in registers: the z-buffer never touches memory.
//                          Colours are fetched once per pixel, for the visible face only.  One 12-byte run of output per thread.
//   paint_vertex_kernel    render_vertex_kernel with one albedo per vertex (ihmr_paint_meshes); both call render_vertex_body
//   view_vertices_kernel   one workgroup per sample: the default pivot (an exact min / max reduction by wave shuffles and LDS), then
//                          q = (p - c) R + c for every vertex (ihmr_view_vertices)
//   heat_colours_kernel    grid (vertex blocks, B): per-vertex albedo from a depth table (ihmr_heat_colours)
//   draw_keypoints_kernel  one workgroup of one wave per sample: the keypoints in order, one lane per cell of the 7 x 7 box, so that a
//                          later disc overwrites an earlier one.
// No float atomics, no hand-offs between workgroups, no scratch (tests/test_render_cpu.py reads the code-object metadata).
#pragma once
#include <hip/hip_runtime.h>

#include "render_pure.h"

#define RND_TILE 32
#define RND_THREADS 256
#define RND_PPT 4                      /* pixels per thread: one 12-byte run */
#define RND_KP_THREADS 64

// the vertex stage of both vertex kernels: PER_VERTEX reads the albedo of vertex v from a (B,nV,3) table, otherwise from the (B,2,3)
// table of the vertex's hand (the hand of its first incident face)
template <bool PER_VERTEX>
__device__ __forceinline__ void render_vertex_body(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                   const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_ids, int nV, int nF,
                                                   int split, const float* __restrict__ albedo, const float* __restrict__ cam,
                                                   const ihmr_render_lights& L, int S, rnd_vertex* __restrict__ ws) {
    const int v = blockIdx.x * RND_THREADS + threadIdx.x, b = blockIdx.y;
    if (v >= nV) return;
    rnd_vertex out;
    out.X = RND_BAD_COORD; out.Y = 0; out.iz = 0.0f; out.c[0] = out.c[1] = out.c[2] = 0.0f;
    const float cm[3] = {cam[3 * b], cam[3 * b + 1], cam[3 * b + 2]};
    if (rnd_cam_ok(cm[0])) {
        const float* vb = verts + (size_t)b * nV * 3;
        float n[3] = {0.0f, 0.0f, 0.0f};
        int hand = 0, first = 1;
        const int lo = max(csr_off[v], 0), hi = min(csr_off[v + 1], 3 * nF);
        for (int k = lo; k < hi; ++k) {
            const int f = csr_ids[k];
            if (f < 0 || f >= nF) continue;
            const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            if ((unsigned)i0 >= (unsigned)nV || (unsigned)i1 >= (unsigned)nV || (unsigned)i2 >= (unsigned)nV) continue;
            if (first) { hand = f >= split; first = 0; }
            const float a0[3] = {vb[3 * i0], vb[3 * i0 + 1], vb[3 * i0 + 2]};
            const float a1[3] = {vb[3 * i1], vb[3 * i1 + 1], vb[3 * i1 + 2]};
            const float a2[3] = {vb[3 * i2], vb[3 * i2 + 1], vb[3 * i2 + 2]};
            float c[3];
            rnd_cross_face(a0, a1, a2, c);
            n[0] = n[0] + c[0]; n[1] = n[1] + c[1]; n[2] = n[2] + c[2];
        }
        rnd_normalise(n);
        const float p0[3] = {vb[3 * v], vb[3 * v + 1], vb[3 * v + 2]};
        float p[3];
        rnd_translate(p0, cm, p);
        const float* al = albedo + (PER_VERTEX ? (size_t)b * nV + v : (size_t)b * 2 + hand) * 3;
        const float alb[3] = {al[0], al[1], al[2]};
        rnd_shade(n, p, alb, &L, out.c);
        rnd_project(p, S, &out);
    }
    ws[(size_t)b * nV + v] = out;
}

__global__ __launch_bounds__(RND_THREADS) void render_vertex_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                    const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_ids,
                                                                    int nV, int nF, int split, const float* __restrict__ albedo,
                                                                    const float* __restrict__ cam, ihmr_render_lights L, int S,
                                                                    rnd_vertex* __restrict__ ws) {
    render_vertex_body<false>(verts, faces, csr_off, csr_ids, nV, nF, split, albedo, cam, L, S, ws);
}

__global__ __launch_bounds__(RND_THREADS) void paint_vertex_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                   const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_ids,
                                                                   int nV, int nF, int split, const float* __restrict__ albedo,
                                                                   const float* __restrict__ cam, ihmr_render_lights L, int S,
                                                                   rnd_vertex* __restrict__ ws) {
    render_vertex_body<true>(verts, faces, csr_off, csr_ids, nV, nF, split, albedo, cam, L, S, ws);
}

// One workgroup per sample.  Without a pivot: every thread takes its vertices of the drawn hands into a bounding box, the boxes are
// merged across the wave by shuffles and across the four waves through LDS (rnd_min / rnd_max are order independent, so every thread
// ends with the same box whatever the arrangement).  Then every vertex of the sample is transformed, drawn or not.
__global__ __launch_bounds__(RND_THREADS) void view_vertices_kernel(const float* __restrict__ verts, const uint8_t* __restrict__ present,
                                                                    int nV, int split, const float* __restrict__ rot, int rot_per_sample,
                                                                    const float* __restrict__ pivot, float* __restrict__ out) {
    __shared__ float box[RND_THREADS / 64][6];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* vb = verts + (size_t)b * nV * 3;
    float c[3];
    if (pivot) {
        c[0] = pivot[3 * b]; c[1] = pivot[3 * b + 1]; c[2] = pivot[3 * b + 2];
    } else {
        const int draw0 = present ? present[2 * b] : 1, draw1 = present ? present[2 * b + 1] : 1;
        float mn[3], mx[3];
        rnd_bbox_empty(mn, mx);
        for (int v = t; v < nV; v += RND_THREADS) {
            if (!(v < split ? draw0 : draw1)) continue;
            const float p[3] = {vb[3 * v], vb[3 * v + 1], vb[3 * v + 2]};
            rnd_bbox_take(p, mn, mx);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            float mn2[3], mx2[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { mn2[a] = __shfl_xor(mn[a], m, 64); mx2[a] = __shfl_xor(mx[a], m, 64); }
            rnd_bbox_merge(mn2, mx2, mn, mx);
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { box[wave][a] = mn[a]; box[wave][3 + a] = mx[a]; }
        }
        __syncthreads();
        rnd_bbox_empty(mn, mx);
#pragma unroll
        for (int w = 0; w < RND_THREADS / 64; ++w) rnd_bbox_merge(&box[w][0], &box[w][3], mn, mx);
        rnd_bbox_centre(mn, mx, c);
    }
    const float* rb = rot + (rot_per_sample ? (size_t)b * 9 : 0);
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rb[k];
    float* ob = out + (size_t)b * nV * 3;
    for (int v = t; v < nV; v += RND_THREADS) {
        const float p[3] = {vb[3 * v], vb[3 * v + 1], vb[3 * v + 2]};
        float q[3];
        rnd_view_point(p, c, R, q);
        ob[3 * v] = q[0]; ob[3 * v + 1] = q[1]; ob[3 * v + 2] = q[2];
    }
}

// grid (vertex blocks, B): the colour of one vertex from the depth entry its layout names and its hand's base colour
__global__ __launch_bounds__(RND_THREADS) void heat_colours_kernel(const float* __restrict__ depth, const float* __restrict__ albedo,
                                                                   float hot0, float hot1, float hot2, float lo, float hi, int nV, int split,
                                                                   int layout, float* __restrict__ out) {
    const int v = blockIdx.x * RND_THREADS + threadIdx.x, b = blockIdx.y;
    if (v >= nV) return;
    const float d = depth[(size_t)b * nV + rnd_heat_entry(v, split, layout)];
    const float* al = albedo + ((size_t)b * 2 + (v >= split)) * 3;
    const float base[3] = {al[0], al[1], al[2]}, hot[3] = {hot0, hot1, hot2};
    float c[3];
    rnd_heat_colour(d, lo, hi, base, hot, c);
    float* o = out + ((size_t)b * nV + v) * 3;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
}

__global__ __launch_bounds__(RND_THREADS) void render_raster_kernel(const rnd_vertex* __restrict__ ws, const int32_t* __restrict__ faces,
                                                                    int nV, int nF, int split, const uint8_t* __restrict__ present,
                                                                    const uint8_t* __restrict__ bg, int S, int vec,
                                                                    uint8_t* __restrict__ out, int32_t* __restrict__ ids) {
    __shared__ rnd_face_rec recs[RND_THREADS];
    __shared__ int wave_cnt[RND_THREADS / 64];
    const int tiles_x = (S + RND_TILE - 1) / RND_TILE;
    const int ox = (blockIdx.x % tiles_x) * RND_TILE, oy = (blockIdx.x / tiles_x) * RND_TILE, b = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row = oy + t / (RND_TILE / RND_PPT), col0 = ox + RND_PPT * (t % (RND_TILE / RND_PPT));
    const int draw0 = present ? present[2 * b] : 1, draw1 = present ? present[2 * b + 1] : 1;
    const rnd_vertex* wb = ws + (size_t)b * nV;
    // the tile's pixel range in fixed point, clipped to the image
    const int64_t tx0 = (int64_t)ox * RND_SUBPIXEL, tx1 = (int64_t)min(ox + RND_TILE - 1, S - 1) * RND_SUBPIXEL;
    const int64_t ty0 = (int64_t)oy * RND_SUBPIXEL, ty1 = (int64_t)min(oy + RND_TILE - 1, S - 1) * RND_SUBPIXEL;

    float best_w[RND_PPT], best_q[RND_PPT][3];
    int best_id[RND_PPT];
#pragma unroll
    for (int p = 0; p < RND_PPT; ++p) { best_w[p] = 0.0f; best_id[p] = -1; best_q[p][0] = best_q[p][1] = best_q[p][2] = 0.0f; }

    for (int base = 0; base < nF; base += RND_THREADS) {
        const int f = base + t;
        rnd_face_rec r;
        int keep = 0;
        if (f < nF && (f < split ? draw0 : draw1)) {
            const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            if ((unsigned)i0 < (unsigned)nV && (unsigned)i1 < (unsigned)nV && (unsigned)i2 < (unsigned)nV) {
                const rnd_vertex a = wb[i0], bb = wb[i1], c = wb[i2];
                if (rnd_face_setup(&a, &bb, &c, f, &r)) {
                    const int xmin = min(a.X, min(bb.X, c.X)), xmax = max(a.X, max(bb.X, c.X));
                    const int ymin = min(a.Y, min(bb.Y, c.Y)), ymax = max(a.Y, max(bb.Y, c.Y));
                    keep = xmax >= tx0 && xmin <= tx1 && ymax >= ty0 && ymin <= ty1;
                }
            }
        }
        const unsigned long long ballot = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(ballot);
        __syncthreads();
        int start = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RND_THREADS / 64; ++w) {
            const int c = wave_cnt[w];
            start += w < wave ? c : 0;
            total += c;
        }
        if (keep) recs[start + __popcll(ballot & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const rnd_face_rec* q = &recs[k];
            int64_t e[3];
            rnd_edges(q, col0, row, e);
#pragma unroll
            for (int p = 0; p < RND_PPT; ++p) {
                if ((e[0] | e[1] | e[2]) >= 0) {
                    float w3[3];
                    const float w = rnd_weights(q, e, w3);
                    if (rnd_wins(w, q->id, best_w[p], best_id[p])) {
                        best_w[p] = w; best_id[p] = q->id;
                        best_q[p][0] = w3[0]; best_q[p][1] = w3[1]; best_q[p][2] = w3[2];
                    }
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) e[i] += (int64_t)q->A[i] * RND_SUBPIXEL;
            }
        }
        __syncthreads();
    }

    if (row >= S || col0 >= S) return;
    const size_t pix = ((size_t)b * S + row) * S + col0;
    uint32_t word[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (bg) {
        if (vec) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(bg + pix * 3);
            word[0] = s[0]; word[1] = s[1]; word[2] = s[2];
        } else {
            uint32_t acc[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 3 * RND_PPT; ++k)
                if (col0 + k / 3 < S) acc[k / 4] |= (uint32_t)bg[pix * 3 + k] << (8 * (k % 4));
            word[0] = acc[0]; word[1] = acc[1]; word[2] = acc[2];
        }
    }
#pragma unroll
    for (int p = 0; p < RND_PPT; ++p) {
        if (best_id[p] < 0) continue;
        const int f = best_id[p];
        const rnd_vertex* a = wb + faces[3 * f];
        const rnd_vertex* bb = wb + faces[3 * f + 1];
        const rnd_vertex* c = wb + faces[3 * f + 2];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t byte = (uint32_t)rnd_colour_byte(best_q[p], best_w[p], a->c[ch], bb->c[ch], c->c[ch]);
            const int k = 3 * p + ch;
            word[k / 4] = (word[k / 4] & ~(0xffu << (8 * (k % 4)))) | (byte << (8 * (k % 4)));
        }
    }
    if (vec) {
        uint32_t* d = reinterpret_cast<uint32_t*>(out + pix * 3);
        d[0] = word[0]; d[1] = word[1]; d[2] = word[2];
    } else {
#pragma unroll
        for (int k = 0; k < 3 * RND_PPT; ++k)
            if (col0 + k / 3 < S) out[pix * 3 + k] = (uint8_t)(word[k / 4] >> (8 * (k % 4)));
    }
    if (ids) {
#pragma unroll
        for (int p = 0; p < RND_PPT; ++p)
            if (col0 + p < S) ids[pix + p] = best_id[p];
    }
}

__global__ __launch_bounds__(RND_KP_THREADS) void draw_keypoints_kernel(uint8_t* __restrict__ img, const float* __restrict__ kps,
                                                                        const float* __restrict__ weight, int c0, int c1, int c2, int S, int K) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int dy = lane / 7 - 3, dx = lane % 7 - 3;                    // lanes 0..48: the cells of the 7 x 7 box around the centre
    const int inside = lane < 49 && (dx < 0 ? -dx : dx) <= rnd_disc_half_width(dy < 0 ? -dy : dy);
    uint8_t* im = img + (size_t)b * S * S * 3;
    for (int k = 0; k < K; ++k) {
        const float kx = kps[((size_t)b * K + k) * 2], ky = kps[((size_t)b * K + k) * 2 + 1];
        if (weight[(size_t)b * K + k] > 0.0f && rnd_kp_ok(kx) && rnd_kp_ok(ky)) {
            const int x = rnd_kp_centre(kx, S) + dx, y = rnd_kp_centre(ky, S) + dy;
            if (inside && x >= 0 && x < S && y >= 0 && y < S) {
                uint8_t* d = im + ((size_t)y * S + x) * 3;
                d[0] = (uint8_t)c0; d[1] = (uint8_t)c1; d[2] = (uint8_t)c2;
            }
        }
        __threadfence_block();
        __syncthreads();                                               // the next disc's stores come after this one's
    }
}

// Two-hand intersection volume: the voxels of a common grid that lie inside BOTH meshes (statement and arithmetic: volume_pure.h).
//
//   vol_box_kernel    one workgroup per sample: vertex boxes of both meshes, the common cube and its status -> box (B,4), status (B).
//   vol_count_kernel  one workgroup per (sample, tile), tiles consecutive within a sample.  Both meshes are normalised into the tile's
//                     frame in LDS; a thread per triangle finds its column range and the triangles with a non-empty range go into an LDS
//                     list; then 16 lanes per list record walk the record's columns, a lane per column: (u, v) test, 32-bit hit mask,
//                     atomicXor into that mesh's column word.  Integer LDS atomics only: the words do not depend on the order.  Last,
//                     popc(wordA & wordB) over the 1024 columns, an integer block sum, one store per tile.
// A sample with keep[b] == 0 or status != 0 stores zeros and does no ray work.  No float atomics, no scratch, nothing passes from
// one workgroup to another.
#pragma once
#include "ihmr_common.h"
#include "volume_pure.h"

__global__ __launch_bounds__(VOL_THREADS) void vol_box_kernel(const float* __restrict__ verts_a, int n_verts_a,
                                                               const float* __restrict__ verts_b, int n_verts_b,
                                                               const uint8_t* __restrict__ keep, float* __restrict__ box,
                                                               int32_t* __restrict__ status) {
    __shared__ float part[VOL_THREADS / WAVE][13];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (keep && !keep[b]) {                 // (uniform)
        if (tid < 4) box[4 * b + tid] = 0.0f;
        if (tid == 0) status[b] = VOL_COUNTED;
        return;
    }
    float mn[2][3], mx[2][3];
    bool finite = true;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int nv = m ? n_verts_b : n_verts_a;
        const float* v = (m ? verts_b : verts_a) + (size_t)b * nv * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[m][a] = INFINITY; mx[m][a] = -INFINITY; }
        for (int i = tid; i < nv; i += VOL_THREADS) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x = v[3 * i + a];
                finite = finite && vol_finite(x);
                mn[m][a] = fminf(mn[m][a], x);
                mx[m][a] = fmaxf(mx[m][a], x);
            }
        }
    }
    const int wave = tid / WAVE, lane = tid % WAVE;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = wave_reduce_min(mn[m][a]), hi = wave_reduce_max(mx[m][a]);
            if (lane == 0) { part[wave][6 * m + a] = lo; part[wave][6 * m + 3 + a] = hi; }
        }
    const float bad = wave_reduce_max(finite ? 0.0f : 1.0f);
    if (lane == 0) part[wave][12] = bad;
    __syncthreads();
    if (tid == 0) {
        float lo[2][3], hi[2][3];
        float anybad = 0.0f;
        for (int m = 0; m < 2; ++m)
            for (int a = 0; a < 3; ++a) {
                lo[m][a] = part[0][6 * m + a];
                hi[m][a] = part[0][6 * m + 3 + a];
                for (int w = 1; w < VOL_THREADS / WAVE; ++w) {
                    lo[m][a] = fminf(lo[m][a], part[w][6 * m + a]);
                    hi[m][a] = fmaxf(hi[m][a], part[w][6 * m + 3 + a]);
                }
            }
        for (int w = 0; w < VOL_THREADS / WAVE; ++w) anybad = fmaxf(anybad, part[w][12]);
        const VolCube q = vol_cube(lo[0], hi[0], lo[1], hi[1], anybad == 0.0f);
        box[4 * b + 0] = q.c[0]; box[4 * b + 1] = q.c[1]; box[4 * b + 2] = q.c[2]; box[4 * b + 3] = q.s;
        status[b] = q.status;
    }
}

struct VolLds {
    float vn[2][VOL_MAX_VERTS * 3];         // tile-normalised vertices, mesh A then mesh B
    unsigned word[2][VOL_COLS];             // column (k, j): bit i = parity of the crossings of the ray from voxel (k, j, i)
    unsigned list[2 * VOL_MAX_FACES];       // vol_pack_record of every triangle with a non-empty column range
    unsigned part[VOL_THREADS / WAVE];
    unsigned n_list;
};
static_assert(sizeof(VolLds) == VOL_LDS_BYTES, "VOL_LDS_BYTES is the size of vol_count_kernel's LDS");
static_assert(VOL_MAX_VERTS <= 1024, "a vertex id has 10 bits in a list record");
#define VOL_GROUP 16      // lanes per list record: most triangles cover a handful of columns, a whole wave per record would idle

__global__ __launch_bounds__(VOL_THREADS) void vol_count_kernel(const float* __restrict__ verts_a, const int32_t* __restrict__ faces_a,
                                                                 int n_verts_a, int n_faces_a, const float* __restrict__ verts_b,
                                                                 const int32_t* __restrict__ faces_b, int n_verts_b, int n_faces_b,
                                                                 int subdiv, const uint8_t* __restrict__ keep,
                                                                 const float* __restrict__ box, const int32_t* __restrict__ status,
                                                                 uint32_t* __restrict__ counts, uint32_t* __restrict__ bits) {
    __shared__ VolLds L;
    const int tid = threadIdx.x;
    const int n3 = subdiv * subdiv * subdiv;
    const int b = blockIdx.x / n3, tile = blockIdx.x % n3;
    uint32_t* my_bits = bits ? bits + (size_t)blockIdx.x * VOL_COLS : nullptr;
    if ((keep && !keep[b]) || status[b] != VOL_COUNTED) {         // (uniform)
        if (tid == 0) counts[blockIdx.x] = 0u;
        if (my_bits)
            for (int c = tid; c < VOL_COLS; c += VOL_THREADS) my_bits[c] = 0u;
        return;
    }
    const VolTile fr = vol_tile_frame(box[4 * b + 0], box[4 * b + 1], box[4 * b + 2], box[4 * b + 3], subdiv, tile);

    // 1. both meshes into the tile's frame; the column tables cleared
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int nv = m ? n_verts_b : n_verts_a;
        const float* v = (m ? verts_b : verts_a) + (size_t)b * nv * 3;
        for (int i = tid; i < nv; i += VOL_THREADS) {
#pragma unroll
            for (int a = 0; a < 3; ++a) L.vn[m][3 * i + a] = vol_normalise(v[3 * i + a], fr.c[a], fr.s);
        }
        for (int c = tid; c < VOL_COLS; c += VOL_THREADS) L.word[m][c] = 0u;
    }
    if (tid == 0) L.n_list = 0u;
    __syncthreads();

    // 2. a thread per triangle: its column range; the triangles that can be hit go into the list (a face that names a vertex outside
    //    its mesh is left out).  The list's order depends on the atomics; the words built from it do not.
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int nf = m ? n_faces_b : n_faces_a, nv = m ? n_verts_b : n_verts_a;
        const int32_t* faces = m ? faces_b : faces_a;
        for (int f = tid; f < nf; f += VOL_THREADS) {
            const unsigned ia = (unsigned)faces[3 * f], ib = (unsigned)faces[3 * f + 1], ic = (unsigned)faces[3 * f + 2];
            if (ia >= (unsigned)nv || ib >= (unsigned)nv || ic >= (unsigned)nv) continue;
            const float* a = &L.vn[m][3 * ia];
            const float* bb = &L.vn[m][3 * ib];
            const float* c = &L.vn[m][3 * ic];
            int j0, j1, k0, k1;
            if (!vol_col_range(a[1], bb[1], c[1], a[2], bb[2], c[2], j0, j1, k0, k1)) continue;
            if (fabsf(sdf_tri_yz_det(a[1], a[2], bb[1], bb[2], c[1], c[2])) < 1e-12f) continue;
            L.list[atomicAdd(&L.n_list, 1u)] = vol_pack_record(ia, ib, ic, m);
        }
    }
    __syncthreads();

    // 3. a group of VOL_GROUP lanes per record, a lane per column of its range (the record holds the vertex ids: nothing is read from
    //    global memory here, the range is found again from the same LDS values)
    const int group = tid / VOL_GROUP, glane = tid % VOL_GROUP;
    const int n_list = (int)L.n_list;
    for (int r = group; r < n_list; r += VOL_THREADS / VOL_GROUP) {
        int ia, ib, ic, m;
        vol_unpack_record(L.list[r], ia, ib, ic, m);
        const float* a = &L.vn[m][3 * ia];
        const float* bb = &L.vn[m][3 * ib];
        const float* c = &L.vn[m][3 * ic];
        int j0, j1, k0, k1;
        VolTri t;
        if (!vol_col_range(a[1], bb[1], c[1], a[2], bb[2], c[2], j0, j1, k0, k1) || !vol_tri_setup(a, bb, c, t)) continue;
        const int nj = j1 - j0 + 1, ncol = nj * (k1 - k0 + 1);
        for (int q = glane; q < ncol; q += VOL_GROUP) {
            const int col = (k0 + q / nj) * SDF_G + j0 + q % nj;
            const unsigned hits = vol_column_hits(t, col);
            if (hits) atomicXor(&L.word[m][col], hits);
        }
    }
    __syncthreads();

    // 4. the voxels inside both meshes
    const int wave = tid / WAVE, lane = tid % WAVE;
    unsigned n = 0u;
    for (int c = tid; c < VOL_COLS; c += VOL_THREADS) {
        const unsigned both = L.word[0][c] & L.word[1][c];
        if (my_bits) my_bits[c] = both;
        n += (unsigned)__popc(both);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) L.part[wave] = n;
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0u;
        for (int w = 0; w < VOL_THREADS / WAVE; ++w) total += L.part[w];
        counts[blockIdx.x] = total;
    }
}

static int vol_launch(const float* verts_a, const int32_t* faces_a, int n_verts_a, int n_faces_a, const float* verts_b,
                      const int32_t* faces_b, int n_verts_b, int n_faces_b, int B, int subdiv, const uint8_t* keep, float* box,
                      int32_t* status, uint32_t* counts, uint32_t* bits, hipStream_t stream) {
    if (!verts_a || !faces_a || !verts_b || !faces_b || !box || !status || !counts) return -1;
    if (B < 1 || (subdiv != 1 && subdiv != 2 && subdiv != 4)) return -1;
    if (n_verts_a < 1 || n_verts_a > VOL_MAX_VERTS || n_verts_b < 1 || n_verts_b > VOL_MAX_VERTS) return -1;
    if (n_faces_a < 1 || n_faces_a > VOL_MAX_FACES || n_faces_b < 1 || n_faces_b > VOL_MAX_FACES) return -1;
    if ((long long)B * subdiv * subdiv * subdiv > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(vol_box_kernel, dim3(B), dim3(VOL_THREADS), 0, stream, verts_a, n_verts_a, verts_b, n_verts_b, keep, box, status);
    hipLaunchKernelGGL(vol_count_kernel, dim3(B * subdiv * subdiv * subdiv), dim3(VOL_THREADS), 0, stream, verts_a, faces_a, n_verts_a,
                       n_faces_a, verts_b, faces_b, n_verts_b, n_faces_b, subdiv, keep, box, status, counts, bits);
    return (int)hipGetLastError();
}

// Host driver of csrc/mano_pose_space_pure.h (tests/test_mano_space_cpu.py builds it with g++ -fsanitize=address,undefined and runs it as a
// program): the four kernels of csrc/mano_pose_space.h restated on the host in their own order -- tiles of MPS_TILE hands with C and
// the tile's rows in arrays of the LDS layout, thread e of a tile, thread tid of a hand, block_sum_f64 as ctp_block_sum -- on buffers of
// exactly the sizes the entry points are handed, so that an index one past an end is a sanitizer report.
//
//   mano_space_driver IN OUT
//   IN   int32 N, K, J (16: no tips, 21), has_transl; then float32 coeffs (N,K), comps (K,45), d_pose45 (N,45), verts (N,778,3),
//        joints16 (N,16,3), transl (N,3), int32 tip_ids (5), float32 d_verts_out (N,778,3), d_joints_out (N,J,3)
//   OUT  float32 pose45 (N,45), d_coeffs (N,K), verts_out (N,778,3), joints_out (N,J,3), verts_inplace (N,778,3) (the forward run in
//        place), d_verts_in (N,778,3), d_joints16 (N,16,3), d_transl (N,3)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ihmr_amd/csrc/contact_pure.h"
#include "../ihmr_amd/csrc/mano_pose_space_pure.h"

static const int NV3 = MPS_VERTS * 3;

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

struct PcaLds {
    float C[MPS_POSE * MPS_C_STRIDE];
    float in[MPS_TILE * MPS_POSE];
};
static_assert(sizeof(PcaLds) == MPS_PCA_LDS_BYTES, "the layout the header names");

static void load_tile(PcaLds& L, const float* comps, int K, const float* rows, int n_in) {
    for (int e = 0; e < K * MPS_POSE; ++e) L.C[(e / MPS_POSE) * MPS_C_STRIDE + e % MPS_POSE] = comps[e];
    for (int e = 0; e < n_in; ++e) L.in[e] = rows[e];
}

static void pca_fwd(const float* coeffs, const float* comps, int N, int K, float* pose45) {
    for (int n0 = 0; n0 < N; n0 += MPS_TILE) {
        std::vector<PcaLds> lds(1);                                     // on the heap: its ends are guarded
        PcaLds& L = lds[0];
        const int hands = N - n0 < MPS_TILE ? N - n0 : MPS_TILE;
        load_tile(L, comps, K, coeffs + (size_t)n0 * K, hands * K);
        for (int e = 0; e < hands * MPS_POSE; ++e) {
            const int h = e / MPS_POSE, i = e % MPS_POSE;
            pose45[(size_t)n0 * MPS_POSE + e] = mps_fma_chain(L.in + h * K, 1, L.C + i, MPS_C_STRIDE, K);
        }
    }
}

static void pca_bwd(const float* d_pose45, const float* comps, int N, int K, float* d_coeffs) {
    for (int n0 = 0; n0 < N; n0 += MPS_TILE) {
        std::vector<PcaLds> lds(1);
        PcaLds& L = lds[0];
        const int hands = N - n0 < MPS_TILE ? N - n0 : MPS_TILE;
        load_tile(L, comps, K, d_pose45 + (size_t)n0 * MPS_POSE, hands * MPS_POSE);
        for (int e = 0; e < hands * K; ++e) {
            const int h = e / K, k = e % K;
            d_coeffs[(size_t)n0 * K + e] = mps_fma_chain(L.in + h * MPS_POSE, 1, L.C + k * MPS_C_STRIDE, 1, MPS_POSE);
        }
    }
}

static void post_fwd(const float* verts_in, const float* joints16_in, const float* transl, const int32_t* tip_ids, int N, float* verts_out,
                     float* joints_out) {
    const int J = tip_ids ? MPS_JOINTS + MPS_TIPS : MPS_JOINTS;
    for (int n = 0; n < N; ++n) {
        const float* vi = verts_in + (size_t)n * NV3;
        float* vo = verts_out + (size_t)n * NV3;
        float* jo = joints_out + (size_t)n * J * 3;
        for (int tid = 0; tid < MPS_THREADS; ++tid) {
            for (int e = tid; e < NV3; e += MPS_THREADS) {
                const int v = e / 3, c = e - 3 * v;
                const float x = mps_shift(vi[e], transl != nullptr, transl ? transl[3 * n + c] : 0.f);
                vo[e] = x;
                for (int k = 0; k < MPS_TIPS; ++k)
                    if (tip_ids && tip_ids[k] == v) jo[(MPS_JOINTS + k) * 3 + c] = x;
            }
            if (tid < MPS_JOINTS * 3)
                jo[tid] = mps_shift(joints16_in[(size_t)n * MPS_JOINTS * 3 + tid], transl != nullptr, transl ? transl[3 * n + tid % 3] : 0.f);
            if (tip_ids && tid < MPS_TIPS * 3 && !mps_tip_ok(tip_ids[tid / 3])) jo[MPS_JOINTS * 3 + tid] = 0.f;
        }
    }
}

static void post_bwd(const float* d_verts_out, const float* d_joints_out, const int32_t* tip_ids, int N, float* d_verts_in, float* d_joints16,
                     float* d_transl) {
    const int J = tip_ids ? MPS_JOINTS + MPS_TIPS : MPS_JOINTS;
    for (int n = 0; n < N; ++n) {
        const float* dvo = d_verts_out + (size_t)n * NV3;
        const float* djo = d_joints_out + (size_t)n * J * 3;
        std::vector<double> part(3 * MPS_THREADS);
        for (int tid = 0; tid < MPS_THREADS; ++tid) {
            for (int e = tid; e < NV3; e += MPS_THREADS) {
                const int v = e / 3, c = e - 3 * v;
                float g = dvo[e];
                for (int k = 0; k < MPS_TIPS; ++k)
                    if (tip_ids && tip_ids[k] == v) g += djo[(MPS_JOINTS + k) * 3 + c];
                d_verts_in[(size_t)n * NV3 + e] = g;
            }
            if (tid < MPS_JOINTS * 3) d_joints16[(size_t)n * MPS_JOINTS * 3 + tid] = djo[tid];
            double acc[3];
            mps_thread_rows(dvo, djo, J, tid, acc);
            for (int c = 0; c < 3; ++c) part[c * MPS_THREADS + tid] = acc[c];
        }
        for (int c = 0; c < 3; ++c) d_transl[3 * n + c] = (float)ctp_block_sum(part.data() + c * MPS_THREADS);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: mano_space_driver IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> head = read_n<int32_t>(f, 4);
    const int N = head[0], K = head[1], J = head[2], has_transl = head[3];
    if (N < 1 || K < 1 || K > MPS_POSE || (J != MPS_JOINTS && J != MPS_JOINTS + MPS_TIPS)) { fprintf(stderr, "refused\n"); return 3; }
    const std::vector<float> coeffs = read_n<float>(f, (size_t)N * K), comps = read_n<float>(f, (size_t)K * MPS_POSE);
    const std::vector<float> d_pose45 = read_n<float>(f, (size_t)N * MPS_POSE), verts = read_n<float>(f, (size_t)N * NV3);
    const std::vector<float> joints16 = read_n<float>(f, (size_t)N * MPS_JOINTS * 3), transl = read_n<float>(f, (size_t)N * 3);
    const std::vector<int32_t> tip_ids = read_n<int32_t>(f, MPS_TIPS);
    const std::vector<float> d_verts_out = read_n<float>(f, (size_t)N * NV3), d_joints_out = read_n<float>(f, (size_t)N * J * 3);
    fclose(f);
    const float* t = has_transl ? transl.data() : nullptr;
    const int32_t* tips = J > MPS_JOINTS ? tip_ids.data() : nullptr;

    std::vector<float> pose45((size_t)N * MPS_POSE), d_coeffs((size_t)N * K), verts_out((size_t)N * NV3), joints_out((size_t)N * J * 3);
    std::vector<float> inplace(verts), joints_inplace((size_t)N * J * 3), d_verts_in((size_t)N * NV3), d_joints16((size_t)N * MPS_JOINTS * 3);
    std::vector<float> d_transl((size_t)N * 3);
    pca_fwd(coeffs.data(), comps.data(), N, K, pose45.data());
    pca_bwd(d_pose45.data(), comps.data(), N, K, d_coeffs.data());
    post_fwd(verts.data(), joints16.data(), t, tips, N, verts_out.data(), joints_out.data());
    post_fwd(inplace.data(), joints16.data(), t, tips, N, inplace.data(), joints_inplace.data());
    if (joints_inplace != joints_out) { fprintf(stderr, "in place: other joints\n"); return 4; }
    post_bwd(d_verts_out.data(), d_joints_out.data(), tips, N, d_verts_in.data(), d_joints16.data(), d_transl.data());

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    for (const std::vector<float>* v : {&pose45, &d_coeffs, &verts_out, &joints_out, &inplace, &d_verts_in, &d_joints16, &d_transl})
        fwrite(v->data(), sizeof(float), v->size(), o);
    fclose(o);
    return 0;
}

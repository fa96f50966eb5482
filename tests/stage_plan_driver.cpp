// Host driver of ihmr_amd/csrc/stage_plan.h for tests/test_stage_plan_cpu.py (g++ -fsanitize=address,undefined):
//   stage_plan_driver <op> <in> <out>
// <in>: int64 count, then count records of float64 fields (integers are exact in them); <out>: count records of float64 plan fields, in
// the order of the structs.
//   stage   param_mask no_fused_tail tail_fits sdf_no_static_reuse force_generic_tail keep_lists              -> StagePlan
//   iter    (the six of `stage`) it n_iters                                                                  -> IterPlan
//   single  which: 0 forward + losses, 1 forward + backward, 2 forward verts, 10 + mode: an IHMR-MLP evaluation -> IterPlan
//   step    lr sgd it save_freq                                                                              -> step_size bc2_sqrt snap_idx
//   snaps   n_iters save_freq                                                                                -> snapshot count
//   sdf     lists static_mask sdf_no_candidate_lists sdf_no_static_reuse                                     -> SdfFlags
//   ok      param_mask optimizer n_iters save_freq select_loss                                               -> stage_ok
//   forms   hands dense force_streaming                                                                      -> skin_small prep_form bwd2_lds
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../ihmr_amd/csrc/stage_plan.h"

typedef long long i64;

static int fields_in(const char* op) {
    return !strcmp(op, "stage") ? 6 : !strcmp(op, "iter") ? 8 : !strcmp(op, "single") ? 1 : !strcmp(op, "step") ? 4 : !strcmp(op, "snaps") ? 2 :
           !strcmp(op, "sdf") ? 4 : !strcmp(op, "ok") ? 5 : !strcmp(op, "forms") ? 3 : -1;
}

int main(int argc, char** argv) {
    if (argc != 4 || fields_in(argv[1]) < 0) { fprintf(stderr, "usage: %s stage|iter|single|step|snaps|sdf|ok|forms in out\n", argv[0]); return 2; }
    const char* op = argv[1];
    const int nf = fields_in(op);
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) { perror(argv[2]); return 2; }
    i64 n = 0;
    if (fread(&n, sizeof n, 1, fi) != 1 || n < 0) { fprintf(stderr, "bad count\n"); return 2; }
    std::vector<double> in((size_t)n * nf), out;
    if (fread(in.data(), sizeof(double), in.size(), fi) != in.size()) { fprintf(stderr, "short input\n"); return 2; }
    fclose(fi);
    auto put_iter = [&](const plan::IterPlan& q) {
        for (int v : {q.head, q.skin, q.lists, q.tail, q.after, q.first, q.need_cam, q.need_mask, q.static_mask, q.keep_rot}) out.push_back(v);
    };
    for (i64 i = 0; i < n; ++i) {
        const double* r = &in[(size_t)i * nf];
        auto I = [&](int k) { return (int)r[k]; };
        if (!strcmp(op, "stage") || !strcmp(op, "iter")) {
            const plan::StagePlan p = plan::plan_stage(I(0), I(1), I(2), I(3), I(4), I(5));
            if (!strcmp(op, "iter")) put_iter(plan::plan_iter(p, I(6), I(7)));
            else
                for (int v : {p.need_mask, p.need_cam, p.vposed_fixed, p.pose_fixed, p.pose_stage, p.first_skin, p.later_skin, p.static_mask,
                              p.fused_tail, p.trans_tail, p.keep_rot, p.lists_first})
                    out.push_back(v);
        } else if (!strcmp(op, "single")) {
            put_iter(I(0) == 0 ? plan::kForwardLosses : I(0) == 1 ? plan::kForwardBackward : I(0) == 2 ? plan::kForwardVerts : plan::plan_mlp_eval(I(0) - 10));
        } else if (!strcmp(op, "step")) {
            const plan::StepPlan s = plan::plan_step((float)r[0], I(1), I(2), I(3));
            out.insert(out.end(), {(double)s.step_size, (double)s.bc2_sqrt, (double)s.snap_idx});
        } else if (!strcmp(op, "snaps")) {
            out.push_back(plan::snapshot_count(I(0), I(1)));
        } else if (!strcmp(op, "sdf")) {
            const plan::SdfFlags f = plan::plan_sdf_flags(I(0), I(1), I(2), I(3));
            for (int v : {f.list_mode, f.force_rebuild, f.static_stage, f.static_mask, f.moving_box}) out.push_back(v);
        } else if (!strcmp(op, "ok")) {
            out.push_back(plan::stage_ok(I(0), I(1), I(2), I(3), I(4)) ? 1 : 0);
        } else {
            out.insert(out.end(), {(double)plan::skin_small(I(0)), (double)plan::prep_form(I(0), I(1)), (double)plan::bwd2_lds(I(0), I(2))});
        }
    }
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }
    const bool ok = fwrite(out.data(), sizeof(double), out.size(), fo) == out.size();
    return (fclose(fo) == 0 && ok) ? 0 : 2;
}

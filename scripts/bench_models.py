#!/usr/bin/env python3
"""Secondary workloads (BASELINE.json configs[1], configs[2]): IHMR-Baseline B=64 and IHMR-MLP B=128 inference.
Not the driver's bench line (that is bench.py = IHMR-OPT); prints one JSON line per workload.
`baseline --precision fp32|bf16|both`: the encoder precision of IHMR-Baseline (default fp32: the line as before; bf16 / both: one line per
precision with `encoder_precision`, the repetitions and, for bf16, the algorithmic-bytes figure against the HBM peak)."""
import json, os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch

def opt(B, **kw):
    d = dict(isTrain=False, dist=False, process_rank=-1, batchSize=B, inputSize=224, input_nc=3, num_joints=42, total_params_dim=122,
             cam_params_dim=3, pose_params_dim=96, shape_params_dim=20, trans_params_dim=3, model_root="", mean_param_file="mean_mano_params.pkl",
             checkpoints_dir="./checkpoints", strategy="mlp_default")
    d.update(kw); return types.SimpleNamespace(**d)

def timeit(fn, steps, warmup):
    for _ in range(warmup): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / steps

def encoder_algorithmic_bytes(B, res=224):
    """Bytes the bf16 trunk has to move per pass if every activation is written once and read once per consumer and every packed
    weight is read once (bf16: 2 bytes; the image read as fp32, the pooled feature written as fp32) -- from the layer shapes alone."""
    total = B * 3 * res * res * 4 + B * res * res * 4 * 2 * 2            # image in, NHWC4 bf16 staging written + read
    H = res // 2
    total += 7 * 7 * 4 * 64 * 2 + B * H * H * 64 * 2 * 2                   # stem weights, stem output written + read by the max-pool
    H //= 2
    cin, act = 64, B * H * H * 64 * 2                                      # the max-pool's output (bytes); written below with its readers
    total += act
    for planes, blocks, stride in [(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]:
        for b in range(blocks):
            st = stride if b == 0 else 1
            Ho = H // st
            x_bytes = B * H * H * cin * 2
            y1, y2, y3 = B * H * H * planes * 2, B * Ho * Ho * planes * 2, B * Ho * Ho * planes * 4 * 2
            total += x_bytes + y1 + cin * planes * 2                       # conv1: read x, write y1, weights
            total += y1 + y2 + 9 * planes * planes * 2                     # conv2
            if b == 0:
                total += x_bytes + y3 + cin * planes * 4 * 2               # downsample: read x, write the residual, weights
            total += y2 + y3 + y3 + planes * planes * 4 * 2                # conv3: read y2, read the residual, write the block's output
            cin, H = planes * 4, Ho
    total += B * H * H * cin * 2 + B * cin * 4                             # avg-pool: read, write fp32
    return total


def bench_baseline(precisions):
    """IHMR-Baseline B = 64 for each precision; with more than one, the timings alternate between the models (after both warmed up)
    five times each, so that clock and temperature drift hit both alike."""
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.synthetic import synthetic_opt_batch
    B, HBM_PEAK = 64, 8.0e12
    models = {p: InterHandModel(opt(B, encoder_precision=p)).eval() for p in precisions}
    m0 = models[precisions[0]]
    fwd = lambda p, s, t: two_hand.forward_from_packed(m0.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
    batch = {k: v.cuda() for k, v in synthetic_opt_batch(B, fwd, seed=1234, with_image=True).items()}
    pend = {p: [] for p in precisions}

    def step_async(p):        # the export of batch i is collected while batch i + 1 runs (get_pred_result_async)
        m = models[p]
        m.set_input(batch); m.test(); pend[p].append(m.get_pred_result_async())
        if len(pend[p]) > 1: pend[p].pop(0).wait()
    reps = {p: dict(step=[], enc=[]) for p in precisions}
    for p in precisions:                                   # warm-up of every model: packing, workspaces, graph capture
        timeit(lambda: step_async(p), 3, 3); timeit(lambda: models[p].encoder(batch["img"]), 3, 3)
    for _ in range(5):
        for p in precisions:
            reps[p]["step"].append(timeit(lambda: step_async(p), 20, 2))
            reps[p]["enc"].append(timeit(lambda: models[p].encoder(batch["img"]), 10, 2))
    out = {}
    for p in precisions:
        dt, enc = float(np.median(reps[p]["step"])), float(np.median(reps[p]["enc"]))
        d = dict(workload="IHMR-Baseline (ResNet-50 + MANO regress) batch=64 inference", encoder_precision=p, images_per_s=B / dt, ms_per_batch=dt * 1e3,
                 encoder_ms_per_batch=enc * 1e3, encoder_ms_per_batch_reps=[round(t * 1e3, 4) for t in reps[p]["enc"]],
                 images_per_s_reps=[round(B / t, 1) for t in reps[p]["step"]], encoder_tflops=8.2e9 * B / enc / 1e12)
        if p == "bf16":
            nbytes = encoder_algorithmic_bytes(B)
            d.update(encoder_algorithmic_bytes=nbytes, encoder_algorithmic_bytes_per_s=nbytes / enc,
                     encoder_frac_of_hbm_peak=nbytes / enc / HBM_PEAK,
                     bound="HBM: algorithmic bytes (bf16 activations written once and read once per consumer + packed weights) over the 8 TB/s peak")
        else:
            d.update(encoder_frac_of_fp32_mfma_peak=8.2e9 * B / enc / 157.3e12)
        out[p] = d
    if len(precisions) > 1:
        f, b = reps["fp32"], reps["bf16"]
        for p in precisions:
            out[p]["bf16_slowest_faster_than_fp32_fastest"] = dict(encoder=max(b["enc"]) < min(f["enc"]), step=max(b["step"]) < min(f["step"]))
            out[p]["encoder_time_ratio_bf16_over_fp32"] = out["bf16"]["encoder_ms_per_batch"] / out["fp32"]["encoder_ms_per_batch"]
    for p in precisions:
        print(json.dumps(out[p]))


def main():
    from ihmr_amd import two_hand
    from ihmr_amd.baseline_model import InterHandModel
    from ihmr_amd.mlp_model import MLPModel
    from ihmr_amd.strategies import make_mlp_strategy
    from ihmr_amd.synthetic import synthetic_opt_batch
    argv = sys.argv[1:]
    precision = "fp32"                                     # --precision fp32|bf16|both (baseline only; fp32 = the output as before)
    if "--precision" in argv:
        i = argv.index("--precision")
        precision = argv[i + 1]
        del argv[i:i + 2]
        if precision not in ("fp32", "bf16", "both"):
            raise SystemExit("--precision fp32|bf16|both")
    which = argv or ["baseline", "mlp", "train"]
    if "baseline" in which and precision != "fp32":
        bench_baseline(["fp32", "bf16"] if precision == "both" else [precision])
    elif "baseline" in which:
        B = 64
        m = InterHandModel(opt(B)); m.eval()
        fwd = lambda p, s, t: two_hand.forward_from_packed(m.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
        batch = {k: v.cuda() for k, v in synthetic_opt_batch(B, fwd, seed=1234, with_image=True).items()}
        def step():
            m.set_input(batch); m.test(); return m.get_pred_result()
        dt_block = timeit(step, 10, 3)
        pend = []
        def step_async():        # the export of batch i is collected while batch i + 1 runs (get_pred_result_async)
            m.set_input(batch); m.test(); pend.append(m.get_pred_result_async())
            if len(pend) > 1: pend.pop(0).wait()
        dt = timeit(step_async, 20, 3)
        # encoder alone
        enc_dt = timeit(lambda: m.encoder(batch["img"]), 10, 3)
        print(json.dumps(dict(workload="IHMR-Baseline (ResNet-50 + MANO regress) batch=64 inference", images_per_s=B / dt, ms_per_batch=dt * 1e3, blocking_export_ms_per_batch=dt_block * 1e3,
                              encoder_ms_per_batch=enc_dt * 1e3, encoder_tflops=8.2e9 * B / enc_dt / 1e12, encoder_frac_of_fp32_mfma_peak=8.2e9 * B / enc_dt / 157.3e12)))
    if "mlp" in which:
        from helpers import seeded_state_dict
        B = 128
        strat = make_mlp_strategy()
        m = MLPModel(opt(B)); m.set_update_info(strat, B)
        for i in range(len(strat)):
            m.add_new_network(i); net = m.sub_network_list[i]; net.load_state_dict(seeded_state_dict(net, 900 + i, last_scale=0.02))
        m.eval()
        fwd = lambda p, s, t: two_hand.forward_from_packed(m.mano_models["right"], p.cuda(), s.cuda(), t.cuda())[2]
        b = synthetic_opt_batch(B, fwd, seed=1234, with_feat=True)
        b["init_hand_trans"] = b["init_hand_trans"][:, 0, :3].contiguous(); b["img"] = torch.zeros(B, 3, 8, 8)
        batch = {k: v.cuda() for k, v in b.items()}
        def step():
            m.set_input(batch); m.test(); return m.get_pred_result()
        dt = timeit(step, 10, 3)
        pend = []
        def step_async():        # the export of batch i is collected while batch i + 1 runs (get_pred_result_async)
            m.set_input(batch); m.test(); pend.append(m.get_pred_result_async())
            if len(pend) > 1: pend.pop(0).wait()
        dta = timeit(step_async, 20, 3)
        print(json.dumps(dict(workload="IHMR-MLP refinement head batch=128 inference (6 stages: 8 MANO+SDF evaluations, 6 MLPs)", images_per_s=B / dta,
                              ms_per_batch=dta * 1e3, blocking_export_ms_per_batch=dt * 1e3, blocking_export_images_per_s=B / dt)))

    if "train" in which:          # the two training steps: python -m ihmr_amd.run_train_mlp / run_train_baseline
        from ihmr_amd import run_train_baseline, run_train_mlp
        log = run_train_mlp.main(["--num_samples", "512", "--batchSize", "128", "--epochs", "10", "--stages", "6"])
        ms = float(np.mean([r["ms_per_step"] for r in log[1:]]))
        print(json.dumps(dict(workload="IHMR-MLP training step batch=128 (mean over stages 1-5)", ms_per_step=ms, samples_per_s=128 / ms * 1e3)))
        log = run_train_baseline.main(["--num_samples", "256", "--batchSize", "64", "--total_epoch", "3"])
        print(json.dumps(dict(workload="IHMR-Baseline training step batch=64 (ResNet-50 train mode + MANO + losses + Adam)",
                              ms_per_step=log[-1]["ms_per_step"], images_per_s=log[-1]["images_per_s"])))


if __name__ == "__main__":
    main()

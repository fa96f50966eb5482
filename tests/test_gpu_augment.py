"""Training-time augmentation on the GPU (ihmr_amd/augment.py, csrc/augment.h) against the reference's own run
(tests/golden/augment.npz, made by tests/golden/make_golden_augment.py) and, step by step, against tests/augment_ref.py:
every uint8 image bit-exact after every step, the float tensor bit-exact, float labels within the golden's stored tolerance."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
from oracle import preprocess_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment.npz")
LABELS = ("joints_2d", "joints_3d", "mano_pose", "mano_betas", "mano_params_weight", "hand_type_array")


def _G():
    from ihmr_amd import augment
    return augment


def _proc(S, bank=None):
    return _G().TrainDataProcessor(types.SimpleNamespace(inputSize=S), bank)


def _noise(rng, n, S):
    return [rng.randint(0, 256, (S, S, 3)).astype(np.uint8) for _ in range(n)]


def _u8(out):
    return out["img_uint8"].cpu().numpy()


def _check_float(out):
    """The float planes are ToTensor + Normalize of the final bytes (torch's own float32 operations)."""
    u8 = out["img_uint8"].cpu()
    want = u8.permute(0, 3, 1, 2).float().div(255).sub_(0.5).div_(0.5)
    assert torch.equal(out["img"].cpu(), want)


# ------------------------------------------------------------------------------------------------------------ golden replay
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _golden_table(g, idx, S, upto):
    """The parameter table of the golden's samples idx with the steps after `upto` switched off (0 flip .. 4 blur)."""
    G = _G()
    p = G.empty_params(len(idx))
    for r, i in enumerate(idx):
        d = g[f"draw{i}"]
        G.set_flip(p, r, d[1])
        if d[2] and upto >= 1:
            G.set_rescale(p, r, S, float(d[3]), int(d[4]), int(d[5]))
        if d[6] and upto >= 2:
            G.set_rotation(p, r, S, float(d[7]))
        if d[8] and upto >= 3:
            G.set_color(p, r, float(d[9]), float(d[10]), float(d[11]), float(d[12]), g[f"order{i}"])
        if d[13] >= 0 and upto >= 4:
            G.set_blur(p, r, int(d[13]))
    return p


@pytest.mark.parametrize("S", [64, 224])
def test_golden_replay(golden, S):
    g = golden
    idx = [i for i in range(int(g["n"])) if int(g[f"draw{i}"][0]) == S]
    assert len(idx) == (12 if S == 64 else 2)
    bank = [g[f"bank{k}"] for k in range(int(g["n_bank"]))]
    proc = _proc(S, bank)
    images = [g[f"img{i}"] for i in idx]
    labels = {k: np.stack([g[f"in_{k}{i}"] for i in idx]) for k in LABELS}
    stages = ("flip", "rescale", "rotate", "color", "blur")
    for upto, stage in enumerate(stages):
        out = proc.apply(images, labels, _golden_table(g, idx, S, upto))
        got = _u8(out)
        for r, i in enumerate(idx):
            want = next(g[f"u8_{s}{i}"] for s in reversed(stages[:upto + 1]) if f"u8_{s}{i}" in g)
            assert np.array_equal(got[r], want), (stage, i, int((got[r] != want).sum()))
        _check_float(out)
    for r, i in enumerate(idx):                                        # the whole chain: labels
        for k in ("joints_2d", "joints_3d", "mano_pose", "hand_trans"):
            ref, tol = g[f"ref_{k}{i}"], float(g[f"tol_{k}{i}"])
            err = float(np.abs(out[k][r].cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max())
            print(f"[augment golden] S={S} sample {i} {k}: max err {err:.3e} tol {tol:.3e}")
            assert err <= tol, (i, k, err, tol)
        for k in ("mano_betas", "mano_params_weight", "hand_type_array", "do_flip"):
            assert np.array_equal(out[k][r].cpu().numpy(), g[f"ref_{k}{i}"]), (i, k)


# ------------------------------------------------------------------------------------------------------- every step alone
def test_rescale_alone():
    G, S, B = _G(), 64, 16
    rng = np.random.RandomState(1)
    imgs = _noise(rng, B, S)
    lo = int(0.6 * S)
    cfg = [(lo, 0, 0), (lo, S - lo - 1, S - lo - 1), (S - 1, 0, 0), (S - 1, 1, 1), (lo, S - lo, S - lo), (S, 0, 0), (S // 2, 5, 9),
           (S // 2, S // 2, 0), (1, 63, 63), (2, 0, 62), (47, 16, 3), (50, 13, 14), (41, 0, 22), (63, 0, 1), (39, 25, 0), (33, 1, 30)]
    p = G.empty_params(B)
    for i, (ns, x, y) in enumerate(cfg[:-1]):
        G.set_rescale(p, i, S, ns / S, x, y, new_size=ns)                       # the last sample passes through
    out = _proc(S).apply(imgs, None, p)
    got = _u8(out)
    for i, (ns, x, y) in enumerate(cfg[:-1]):
        assert np.array_equal(got[i], A.rescale(imgs[i], ns, x, y)), (ns, x, y)
    assert np.array_equal(got[B - 1], imgs[B - 1])
    _check_float(out)
    bad = G.empty_params(1)
    G.set_rescale(bad, 0, S, 0.9, 10, 0, new_size=60)
    with pytest.raises(ValueError):
        _proc(S).apply(imgs[:1], None, bad)


def test_rotation_alone():
    G, S, B = _G(), 64, 16
    rng = np.random.RandomState(2)
    imgs = _noise(rng, B, S)
    angles = [-90, 0, 72] + [18 * k - 90 for k in range(10)] + [33.3, 180.0]
    p = G.empty_params(B)
    for i, a in enumerate(angles):
        G.set_rotation(p, i, S, a)                                             # the last sample passes through
    out = _proc(S).apply(imgs, None, p)
    got = _u8(out)
    for i, a in enumerate(angles):
        assert np.array_equal(got[i], A.rotate(imgs[i], a)), a
    assert np.array_equal(got[B - 1], imgs[B - 1])
    _check_float(out)


def test_colour_alone():
    import itertools
    G, S = _G(), 64
    rng = np.random.RandomState(3)
    orders = list(itertools.permutations(range(4)))
    B = len(orders) + 8
    imgs = _noise(rng, B, S)
    imgs[1][:] = np.array([200, 13, 77], np.uint8)                              # contrast on a constant image
    imgs[2][..., 1] = imgs[2][..., 0]; imgs[2][..., 2] = imgs[2][..., 0]        # saturation on a grey image
    imgs[3][:] = 255
    imgs[4][:] = 0
    p = G.empty_params(B)
    rec = []
    for i in range(B - 1):
        order = orders[i % 24]
        b = (0.9, 1.3)[i % 2] if i < 8 else rng.uniform(0.9, 1.3)
        c, s = rng.uniform(0.8, 1.3), rng.uniform(0.4, 1.6)
        if i == 5:
            c, s = 0.8, 0.4
        if i == 6:
            c, s = 1.3, 1.6
        shift = (-25, 0, 25)[i % 3] if i < 12 else A.hue_shift_byte(rng.uniform(-0.1, 0.1))
        G.set_color(p, i, b, c, s, 0.0, order, hue_shift=shift)
        rec.append((order, b, c, s, shift & 0xFF))
    out = _proc(S).apply(imgs, None, p)
    got = _u8(out)
    for i, (order, b, c, s, shift) in enumerate(rec):
        want = A.color_jitter(imgs[i], order, b, c, s, shift)
        assert np.array_equal(got[i], want), (i, order, int((got[i] != want).sum()))
    assert np.array_equal(got[B - 1], imgs[B - 1])
    _check_float(out)


def test_blur_alone():
    G, S, B = _G(), 64, 16
    rng = np.random.RandomState(4)
    imgs = _noise(rng, B, S)
    k33 = rng.uniform(0, 1, (33, 33)).astype(np.float32)
    k33[rng.uniform(size=k33.shape) < 0.3] = 0
    bank = [np.array([[1.5]], np.float32), (rng.uniform(-0.2, 1, (4, 6)) / 8).astype(np.float32), (k33 / k33.sum()).astype(np.float32),
            np.zeros((5, 3), np.float32), np.full((1, 9), 1 / 9, np.float32), np.full((7, 1), 1 / 7, np.float32)]
    sel = [0, 1, 2, 3, 4, 5, -1, 1, 2, -1, 0, 4, 5, 3, 1, -1]                   # blurred and unblurred samples mixed
    p = G.empty_params(B)
    for i, k in enumerate(sel):
        G.set_blur(p, i, k)
    out = _proc(S, bank).apply(imgs, None, p)
    got = _u8(out)
    for i, k in enumerate(sel):
        want = imgs[i] if k < 0 else A.filter2d(imgs[i], bank[k])
        assert np.array_equal(got[i], want), (i, k, int((got[i] != want).sum()))
    assert (got[3] == 0).all()
    _check_float(out)
    with pytest.raises(ValueError):
        _proc(S, bank).apply(imgs[:1], None, (lambda q: (G.set_blur(q, 0, 6), q)[1])(G.empty_params(1)))


# ------------------------------------------------------------------------------------------------------ whole chain
def _labels(rng, sizes):
    B = len(sizes)
    j2 = np.stack([np.concatenate([rng.uniform(0, [w, h], (42, 2)), rng.randint(0, 2, (42, 1))], 1) for h, w in sizes]).astype(np.float32)
    j3 = np.concatenate([rng.normal(0, 0.1, (B, 42, 3)), rng.randint(0, 2, (B, 42, 1))], 2).astype(np.float32)
    return dict(joints_2d=j2, joints_3d=j3, mano_pose=rng.normal(0, 0.5, (B, 96)).astype(np.float32),
                mano_betas=rng.normal(0, 0.5, (B, 20)).astype(np.float32), mano_params_weight=rng.randint(0, 2, (B, 2)).astype(np.float32),
                hand_type_array=np.array([[1, 1], [1, 0], [0, 1]], np.float32)[rng.randint(0, 3, B)])


def test_every_switch_off_is_the_test_time_preprocessing():
    from ihmr_amd.preprocess import DataProcessor
    S = 64
    rng = np.random.RandomState(5)
    sizes = [(64, 64), (80, 50), (37, 53), (128, 128), (9, 31), (64, 20)]
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    lab = _labels(rng, sizes)
    proc = _proc(S)
    p = proc.draw(lab["hand_type_array"])
    out = proc.apply(imgs, lab, p)
    ref = DataProcessor(final_size=S)(imgs, joints_2d=lab["joints_2d"], hand_type_array=lab["hand_type_array"], return_uint8=True)
    assert torch.equal(out["img"], ref["img"]) and torch.equal(out["img_uint8"], ref["img_uint8"])
    assert torch.equal(out["joints_2d"], ref["joints_2d"]) and torch.equal(out["do_flip"].cpu(), ref["do_flip"].cpu())
    keep = out["do_flip"].cpu().numpy() == 0                                    # labels untouched (left-only samples are mirrored)
    assert keep.any() and not keep.all()
    for k in ("joints_3d", "mano_pose", "mano_betas", "mano_params_weight", "hand_type_array"):
        assert np.array_equal(out[k].cpu().numpy()[keep], lab[k][keep]), k


def test_ragged_batch_through_the_whole_chain():
    G, S = _G(), 224
    rng = np.random.RandomState(6)
    sizes = [(1, 1), (3, 500), (500, 3), (224, 224), (448, 448), (100, 37), (300, 220), (17, 230)]
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    lab = _labels(rng, sizes)
    bank = G.line_blur_kernels()[:6]
    opt = types.SimpleNamespace(inputSize=S, use_random_flip=True, use_random_rescale=True, use_random_position=True,
                                use_random_rotation=True, use_color_jittering=True, use_motion_blur=True, motion_blur_prob=0.6)
    proc = G.TrainDataProcessor(opt, bank, seed=1)
    p = proc.draw(lab["hand_type_array"])
    out = proc.apply(imgs, lab, p)
    got = _u8(out)
    for i, im in enumerate(imgs):
        r = p[i]
        cur, _ = P.padding_and_resize(im, np.zeros((42, 3), np.float32), S)
        if r["flip"]:
            cur = np.fliplr(cur).copy()
        cur = A.rescale(cur, int(r["new_size"]), int(r["x_pos"]), int(r["y_pos"]))
        cur = A.warp_inverse(cur, r["warp"])
        cur = A.color_jitter(cur, r["order"], r["brightness"], r["contrast"], r["saturation"], int(r["hue_shift"]))
        if r["blur_kernel"] >= 0:
            cur = A.filter2d(cur, bank[int(r["blur_kernel"])])
        assert np.array_equal(got[i], cur), (i, sizes[i], int((got[i] != cur).sum()))
        h, w = sizes[i]
        f64 = A.labels_f64(S, S / h if h > w else S / w, lab["joints_2d"][i], lab["joints_3d"][i], lab["mano_pose"][i], lab["mano_betas"][i],
                           lab["mano_params_weight"][i], lab["hand_type_array"][i], bool(r["flip"]), True, float(r["scale"]),
                           int(r["x_pos"]), int(r["y_pos"]), True, float(r["angle"]))
        # float32 chain of <= 8 roundings on values <= 2 (normalised joints; the pixel coordinates reach 500 before the ratio): 2e-5;
        # metres for joints_3d / hand_trans: 1e-6.  (The orientation is pinned by the golden, on well-conditioned inputs.)
        for k, tol in (("joints_2d", 2e-5), ("joints_3d", 1e-6), ("hand_trans", 1e-6)):
            assert np.abs(out[k][i].cpu().numpy() - f64[k]).max() <= tol, (i, k)
        assert np.array_equal(out["mano_pose"][i].cpu().numpy()[3:], f64["mano_pose"][3:].astype(np.float32))
    _check_float(out)
    assert out["ori_img_size"].tolist() == [max(s) for s in sizes]


def test_training_loop_with_every_augmentation():
    """run_train_baseline with all six flags: finite loss, and two runs with one --augment_seed give identical losses."""
    from ihmr_amd import run_train_baseline
    argv = ["--num_samples", "8", "--batchSize", "4", "--total_epoch", "1", "--use_random_flip", "--use_random_rescale",
            "--use_random_position", "--use_random_rotation", "--use_color_jittering", "--use_motion_blur", "--motion_blur_prob", "0.5",
            "--augment_seed", "3"]
    a = run_train_baseline.main(argv)
    b = run_train_baseline.main(argv)
    strip = lambda log: [{k: v for k, v in e.items() if k not in ("ms_per_step", "images_per_s")} for e in log]
    assert len(a) == 1 and np.isfinite(a[0]["loss_first"]) and np.isfinite(a[0]["loss_last"])
    assert strip(a) == strip(b)

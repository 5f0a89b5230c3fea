"""Capture g19_segregu_semi_step.npz: three iterations of the reference's own
run_training_seg_stack_regulization_semi (utils/trainer.py:1654-1901) on CPU
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segregu_semi.py <reference checkout>
    ... make_golden_segregu_semi.py <reference checkout> --scan     (the seed scan, no file)

In the manner of make_golden_segsemi.py (g15) and make_golden_segregu.py (g17),
whose helpers are imported: the reference's modules come from its checkout
(nothing is copied), weights from seeded numpy generators, the soft D labels
replace make_D_label(random=True)'s draw, run_testing_seg_regulization is
stubbed to record the iteration's gradients, exp_dir is a temporary directory.
B = 2 + 2 clouds of N = 256 points, PointNetSeg_regulization(50) +
StackDiscNet(256, 50, 16), BCELoss, CrossEntropyLoss twice (+ ignore_index=255
for the term), MSELoss, ImagePool(0).  GT soft labels from U(0.7, 1.0), as
g16 / g17 (BCELoss refuses a target above 1).

semi_start = 1 and three iterations: iteration 2 is the first with the term.
Both Adams run at lr = 0, so iteration 2 starts from the seeded weights (g15's
docstring).  The run is made in float32 and in float64 and stored from the
float64 run.

The weights are g17's recipe (torch's default bounds, fstn.fc3 x 0.5) with the
generator's non-T-Net WEIGHTS (not biases) x G_GAIN and D's biases D_BIAS N(0, 1)
from default_rng(d_seed + 1) in named_parameters() order: seeded weights alone do
not separate the points for D (g15's docstring).  The threshold is
pick_threshold's (g15) on iteration 2's no-GT D_out in float64.

StackDiscNet's out / (out + 1) compresses D's spread (D_out spans about 0.89 ..
0.96 here), so g15's absolute margin 1e-3 TH is out of reach.  In its place:
the smallest |D_out - TH| over iteration 2's no-GT rows must be at least 100
times the largest |D_out(float32 run) - D_out(float64 run)| on those rows.

On the reference alone this script ASSERTS
  - every D output BCELoss saw is inside [0, 1],
  - the kept share at iteration 2 is within [0.25, 0.75],
  - the float32 run's semi_gt (and K) equal the float64 run's,
  - the threshold margin above (both numbers are printed),
  - every kept row's top-two logit gap is >= 1e-4 of its max - min,
  - the semi term carries >= 10 % of every generator tensor's gradient norm at
    iteration 2 (lambda_semi is chosen for it),
  - g17's regulariser-share condition on fstn.fc3.bias's gradient (> 0.05 both
    ways, iteration 2).

Seeds: G_SEED 15..26 x D_SEED {151, 161} were scanned (--scan prints, per pair,
the margin ratio and the top-two gap); the pick is recorded at the constants.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import pointnet_np as onp  # noqa: E402
from make_golden_segregu import FSTN_FC3_SCALE, summarize  # noqa: E402
from make_golden_segsemi import pick_threshold  # noqa: E402
from make_golden_segstack import stackdisc_spec  # noqa: E402
from segregu_ref import mse_reg, segregu_spec  # noqa: E402

B, N, NCLS, NSHAPES, ITERS = 2, 256, 50, 16, 3
# The scan's pick: (20, 151) has the widest threshold margin of the 24 pairs
# (1.28e-4 = 1467 x the f32 - f64 difference; kept share 0.49) and a top-two gap
# of 5.8e-2 of the range.  (20, 161) has the largest ratio (1714) at a margin of
# 9.1e-5; another f32 implementation's own rounding is what the margin must
# cover, so the absolute margin decided.
G_SEED, D_SEED, DATA_SEED = 20, 151, 192
G_GAIN, D_BIAS = 3.0, 0.2
SEMI_START = 1
# lambda_semi as g15 (the kept rows are confident under the gain: loss_semi is
# small against loss_seg), and lambda_regu large for the same reason: T is within
# 0.07 of I, so at g17's 10 the regulariser's part of fstn.fc3.bias's gradient
# is 2.3e-4 of the whole; at 2e4 it is a share the comparison cannot miss
LAMBDA_SEG, LAMBDA_ADV, LAMBDA_DISC_SHAPE, LAMBDA_REGU, LAMBDA_SEMI, LR = 1.0, 1.0, 0.5, 2e4, 1000.0, 0.0
LOSSES = ("loss_seg", "loss_adv", "loss_regu", "loss_semi", "loss_D", "loss_D_shape")


def make_data(data_seed=DATA_SEED):
    """Per iteration: GT batch (pts, cls one-hot, seg), no-GT batch (pts, cls),
    soft labels for the GT and the no-GT rows."""
    rng = np.random.default_rng(data_seed)
    its = []
    for _ in range(ITERS):
        d = {}
        for k in ("gt", "ng"):
            d["pts_" + k] = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
            c = np.zeros((B, 1, 16), np.float32)
            c[np.arange(B), 0, rng.integers(0, 16, B)] = 1.0
            d["cls_" + k] = c
        d["seg"] = rng.integers(0, NCLS, (B, N)).astype(np.int64)
        d["soft_gt"] = rng.uniform(0.7, 1.0, (B, N, 1)).astype(np.float32)
        d["soft_ng"] = rng.uniform(0.0, 0.305, (B, N, 1)).astype(np.float32)
        its.append(d)
    return its


def make_weights(g_seed=G_SEED, d_seed=D_SEED):
    """(generator state, D state): the seeded float32 weights both sides load."""
    Gp = onp.make_params(segregu_spec(NCLS), seed=g_seed)
    for k in ("fstn.fc3.weight", "fstn.fc3.bias"):
        Gp[k] = (Gp[k] * np.float32(FSTN_FC3_SCALE)).astype(np.float32)
    for k in Gp:
        if k.endswith("weight") and not k.startswith(("stn.", "fstn.")):
            Gp[k] = (np.float32(G_GAIN) * Gp[k]).astype(np.float32)
    Dp = onp.make_params(stackdisc_spec(), seed=d_seed, init="xavier")
    rng = np.random.default_rng(d_seed + 1)
    for k in Dp:  # named_parameters() order: conv1.weight, conv1.bias, ...
        if k.endswith("bias"):
            Dp[k] = (D_BIAS * rng.standard_normal(Dp[k].shape)).astype(np.float32)
    return Gp, Dp


def build(torch, PointNetSeg_regulization, StackDiscNet, dtype, g_seed=G_SEED, d_seed=D_SEED):
    Gp, Dp = make_weights(g_seed, d_seed)
    model = PointNetSeg_regulization(NCLS)
    assert list(model.state_dict()) == list(Gp)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    model_D = StackDiscNet(N, NCLS, NSHAPES)
    assert [n for n, _ in model_D.named_parameters()] == list(Dp)
    model_D.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    return model.to(dtype), model_D.to(dtype)


def nogt_d_out(torch, model, model_D, d, dtype):
    """(D_out (B N,), logits (B N, NCLS)) of one iteration's no-GT batch."""
    with torch.no_grad():
        pred = model(torch.from_numpy(d["pts_ng"]).to(dtype), torch.from_numpy(d["cls_ng"]).to(dtype))[0]
        out = model_D(torch.log_softmax(pred, dim=1))[1]
    return out.double().numpy().reshape(-1), pred.double().numpy().transpose(0, 2, 1).reshape(B * N, NCLS)


def conditions(d64, d32, logits, th):
    """(kept share, smallest |D_out - TH|, largest f32 - f64 difference, the
    smallest top-two gap of a kept row over its range)."""
    keep = ~(d64 <= th)
    top = np.sort(logits[keep], axis=1)
    gap = ((top[:, -1] - top[:, -2]) / (top[:, -1] - top[:, 0])).min() if keep.any() else 0.0
    return keep.mean(), np.abs(d64 - th).min(), np.abs(d32 - d64).max(), gap


def scan(mods):
    torch, _, G, D = mods[:4]
    data = make_data()
    for g_seed in range(15, 27):
        for d_seed in (151, 161):
            res = []
            for dtype in (torch.float64, torch.float32):
                m, d = build(torch, G, D, dtype, g_seed, d_seed)
                res.append(nogt_d_out(torch, m, d, data[2], dtype))
            th, _ = pick_threshold(res[0][0])
            share, margin, diff, gap = conditions(res[0][0], res[1][0], res[0][1], th)
            ok = 0.0 <= res[0][0].min() and res[0][0].max() <= 1.0
            print(f"G {g_seed} D {d_seed}: D_out {res[0][0].min():.4f}..{res[0][0].max():.4f} "
                  f"{'ok' if ok else 'OUTSIDE [0, 1]'} TH {th:.6f} kept {share:.3f} margin {margin:.2e} "
                  f"f32-f64 {diff:.2e} ratio {margin / diff:.0f} top-two gap {gap:.2e}")


def main(ref_root, do_scan=False):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_root)
    import torch
    import torch.nn as nn
    from models.pointnet import PointNetSeg_regulization
    from models.discriminator import StackDiscNet
    import utils.trainer as rtrainer
    from utils.image_pool import ImagePool

    torch.set_num_threads(min(8, os.cpu_count() or 1))
    mods = (torch, nn, PointNetSeg_regulization, StackDiscNet, rtrainer, ImagePool)
    if do_scan:
        return scan(mods)
    data = make_data()
    m64, d64 = build(torch, PointNetSeg_regulization, StackDiscNet, torch.float64)
    th, gap = pick_threshold(nogt_d_out(torch, m64, d64, data[2], torch.float64)[0])
    print(f"semi_TH = {th!r}: the widest gap {gap:.3e} ({gap / th:.2e} relative)")

    out32, snaps32 = capture(*mods, torch.float32, data, th)
    out, snaps = capture(*mods, torch.float64, data, th)
    # the conditions on iteration 2's inputs
    d_out = out["it2.d_out_nogt"].astype(np.float64).reshape(-1)
    d_out32 = out32["it2.d_out_nogt"].astype(np.float64).reshape(-1)
    logits = out["it2.pred_ng"].astype(np.float64).transpose(0, 2, 1).reshape(B * N, NCLS)
    share, margin, diff, rel_gap = conditions(d_out, d_out32, logits, th)
    keep = ~(d_out <= th)
    print(f"kept {int(keep.sum())} of {keep.size} ({share:.3f}), D_out in {d_out.min():.4f}..{d_out.max():.4f}")
    assert 0.25 <= share <= 0.75, share
    print(f"smallest |D_out - TH| = {margin:.3e} ({margin / th:.2e} TH); largest |D_out(f32 run) - "
          f"D_out(f64 run)| = {diff:.3e}; ratio {margin / diff:.0f}")
    assert margin >= 100.0 * diff, (margin, diff)
    print(f"smallest top-two logit gap of a kept row / its range = {rel_gap:.3e}")
    assert rel_gap >= 1e-4, rel_gap
    assert int(out["K"]) == int(keep.sum())
    assert np.array_equal(out["semi_gt"] == 255, ~keep.reshape(B, N))
    assert np.array_equal(out32["semi_gt"], out["semi_gt"]) and int(out32["K"]) == int(out["K"])
    # the term's share of iteration 2's generator gradients: its own gradient, by
    # autograd on the float64 modules, against the run's total
    m64.zero_grad()
    pred = m64(torch.from_numpy(data[2]["pts_ng"]).double(), torch.from_numpy(data[2]["cls_ng"]).double())[0]
    (LAMBDA_SEMI * nn.CrossEntropyLoss(ignore_index=255)(pred, torch.from_numpy(out["semi_gt"]))).backward()
    shares = {n: float(p.grad.norm() / snaps[2][("G", n)].norm()) for n, p in m64.named_parameters()}
    print("the semi term's share of the gradient norms:", {n: round(s, 3) for n, s in shares.items()})
    assert min(shares.values()) >= 0.1, shares
    # g17's condition: the regulariser's share of fstn.fc3.bias's gradient (= the
    # sum over the 2 B clouds of dL/dT) and the rest of it, iteration 2
    T = np.concatenate([out.pop("it2.trans_gt"), out.pop("it2.trans_ng")])
    _, greg = mse_reg(T, B0=B, scale=LAMBDA_REGU)
    gb = snaps[2][("G", "fstn.fc3.bias")].numpy().reshape(-1)
    rshare = np.linalg.norm(greg.sum(0).reshape(-1)) / np.linalg.norm(gb)
    rest = np.linalg.norm(gb - greg.sum(0).reshape(-1)) / np.linalg.norm(gb)
    print(f"regulariser's share of fstn.fc3.bias's gradient: {rshare:.3e} (the rest: {rest:.3f}) "
          f"(max |T - I| = {np.abs(T - np.eye(128)[None]).max():.3f})")
    assert rshare > 0.05 and rest > 0.05
    # the float32 run's gradients against the float64 run's, for the record
    for it in (0, 2):
        worst = (0.0, "")
        for (w, n), g in snaps[it].items():
            a, r = snaps32[it][(w, n)].double().numpy().reshape(-1), g.numpy().reshape(-1)
            worst = max(worst, (float(np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-300)), f"{w}.{n}"))
            if w == "G":
                summarize(f"it{it}.grad{w}.{n}", g.numpy(), out)
            else:
                out[f"it{it}.grad{w}.{n}"] = g.numpy().astype(np.float32)
        print(f"reference f32 vs f64, it{it}: the largest L2-rel gradient difference {worst[0]:.2e} ({worst[1]})")
    print("losses f32", {k: out32[k].tolist() for k in LOSSES})
    print("losses f64", {k: out[k].tolist() for k in LOSSES})
    out.pop("it2.trans_gt", None)
    print(f"seeds G {G_SEED} D {D_SEED} data {DATA_SEED}: margin / difference {margin / diff:.0f}, "
          f"top-two gap {rel_gap:.2e}")
    path = os.path.join(HERE, "g19_segregu_semi_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def capture(torch, nn, PointNetSeg_regulization, StackDiscNet, rtrainer, ImagePool, dtype, data, th):
    """One run of the reference's run_training_seg_stack_regulization_semi in
    `dtype`: (fixture entries, per-iteration gradients)."""
    model, model_D = build(torch, PointNetSeg_regulization, StackDiscNet, dtype)
    out = {"B": B, "N": N, "iters": ITERS, "g_seed": G_SEED, "d_seed": D_SEED,
           "data_seed": DATA_SEED, "g_gain": G_GAIN, "d_bias": D_BIAS, "lambda_seg": LAMBDA_SEG,
           "lambda_adv": LAMBDA_ADV, "lambda_disc_shape": LAMBDA_DISC_SHAPE,
           "lambda_regu": LAMBDA_REGU, "lambda_semi": LAMBDA_SEMI, "lr": LR,
           "semi_start": SEMI_START, "semi_TH": np.float64(th), "num_shapes": NSHAPES,
           "fstn_fc3_scale": FSTN_FC3_SCALE}
    queue = []
    for d in data:
        queue += [d["soft_gt"].copy(), d["soft_ng"].copy()]
    orig = rtrainer.make_D_label

    def make_D_label(input, value, device, random=False):
        if random:
            lab = torch.from_numpy(queue.pop(0)).to(device, dtype)
            assert lab.shape == input.shape, (lab.shape, input.shape)
            return lab
        return orig(input, value, device, random=False).to(dtype)

    d_outs, preds, trans = [], [], []
    model_D.register_forward_hook(lambda m, i, o: d_outs.append(o[1].detach().clone()))

    def g_hook(m, i, o):  # (a hook's return value would replace the output)
        preds.append(o[0].detach().clone())
        trans.append(o[2].detach().clone())
    model.register_forward_hook(g_hook)
    rec = {"seg": [], "gan": [], "shape": [], "regu": [], "semi": []}
    semi_targets = []

    class Rec(nn.Module):
        def __init__(self, inner, key):
            super().__init__()
            self.inner, self.key = inner, key

        def forward(self, a, b):
            if self.key == "regu":
                b = b.to(a.dtype)  # the loop's torch.eye is float32 in the float64 run too
            r = self.inner(a, b)
            rec[self.key].append(float(r.item()))
            if self.key == "semi":
                semi_targets.append((len(rec["seg"]) - 1, b.detach().clone()))
            return r

    snaps = []

    def run_testing_seg_regulization(**kw):
        """Stands in for the test pass after each iteration: the iteration's
        gradients (p.grad until the next zero_grad)."""
        snaps.append({(w, n): p.grad.detach().clone()
                      for w, m in (("G", model), ("D", model_D)) for n, p in m.named_parameters()})
        return 0.0, 0.0, 0.0, 0.0

    t = lambda a: torch.from_numpy(a).to(dtype) if a.dtype == np.float32 else torch.from_numpy(a)  # noqa: E731
    gt_list = [(t(d["pts_gt"]), t(d["cls_gt"]), t(d["seg"])) for d in data]
    ng_list = [(t(d["pts_ng"]), t(d["cls_ng"])) for d in data]
    before = [p.detach().clone() for m in (model, model_D) for p in m.parameters()]
    optimizer = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999))
    optimizer_D = torch.optim.Adam(model_D.parameters(), lr=LR, betas=(0.9, 0.999))
    args = argparse.Namespace(device=torch.device("cpu"), total_iterations=ITERS,
                              lambda_seg=LAMBDA_SEG, lambda_adv=LAMBDA_ADV,
                              lambda_disc_shape=LAMBDA_DISC_SHAPE, lambda_regu=LAMBDA_REGU,
                              lambda_semi=LAMBDA_SEMI, semi_start=SEMI_START, semi_TH=th,
                              iter_test_epoch=1, exp_dir=tempfile.mkdtemp(prefix="g19_"),
                              tensorboard=False)
    logger = logging.getLogger("golden19")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    orig_test = rtrainer.run_testing_seg_regulization
    rtrainer.make_D_label = make_D_label
    rtrainer.run_testing_seg_regulization = run_testing_seg_regulization
    try:
        rtrainer.run_training_seg_stack_regulization_semi(
            trainloader_gt=gt_list, trainloader_nogt=ng_list,
            trainloader_gt_iter=enumerate(list(gt_list)),
            targetloader_nogt_iter=enumerate(list(ng_list)),
            testloader=None, testdataset=None, model=model, model_D=model_D,
            gan_loss=Rec(nn.BCELoss(), "gan"), seg_loss=Rec(nn.CrossEntropyLoss(), "seg"),
            regu_loss=Rec(nn.MSELoss(), "regu"),
            semi_loss=Rec(nn.CrossEntropyLoss(ignore_index=255), "semi"),
            shape_criterion=Rec(nn.CrossEntropyLoss(), "shape"),
            optimizer=optimizer, optimizer_D=optimizer_D,
            history_pool_gt=ImagePool(0), history_pool_nogt=ImagePool(0),
            train_logger=logger, test_logger=logger, writer=None, args=args)
    finally:
        rtrainer.make_D_label = orig
        rtrainer.run_testing_seg_regulization = orig_test
    assert not queue and len(snaps) == ITERS and len(d_outs) == 4 * ITERS and len(preds) == 2 * ITERS
    for o in d_outs:  # every D output BCELoss saw is inside [0, 1]
        assert float(o.min()) >= 0.0 and float(o.max()) <= 1.0, "D output outside [0, 1]"
    for p, q in zip((p for m in (model, model_D) for p in m.parameters()), before):
        assert torch.equal(p.detach(), q)  # lr = 0: no parameter bit moved
    gan = np.array(rec["gan"]).reshape(ITERS, 3)
    out["loss_seg"] = np.array(rec["seg"])
    out["loss_adv"] = gan[:, 0]
    out["loss_regu"] = np.array(rec["regu"]).reshape(ITERS, 2).sum(1)  # l_gt + l_nogt, unscaled
    out["loss_D"] = 0.5 * gan[:, 1] + 0.5 * gan[:, 2]
    out["loss_D_shape"] = np.array(rec["shape"])  # unscaled, as the log line reports it
    assert [i for i, _ in semi_targets] == [2] and len(rec["semi"]) == 1
    out["loss_semi"] = np.array([0.0, 0.0, rec["semi"][0]])
    semi_gt = semi_targets[0][1].numpy()
    out["semi_gt"] = semi_gt.astype(np.int64)
    out["K"] = np.int64((semi_gt != 255).sum())
    # iteration 2: D's output on the no-GT rows (the generator's pass: D's first
    # forward of the iteration) and the predictions it saw (B x 50 x N)
    out["it2.d_out_nogt"] = d_outs[8].numpy().reshape(B, N)
    out["it2.pred_ng"] = preds[5].numpy()
    out["it2.trans_gt"], out["it2.trans_ng"] = trans[4].double().numpy(), trans[5].double().numpy()
    for i, d in enumerate(data):
        for k in ("cls_gt", "cls_ng", "seg"):
            out[f"it{i}.{k}"] = d[k]
    return out, snaps


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3) or (len(sys.argv) == 3 and sys.argv[2] != "--scan"):
        sys.exit(__doc__)
    main(sys.argv[1], do_scan=len(sys.argv) == 3)

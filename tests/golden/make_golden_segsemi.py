"""Capture g15_segsemi_step.npz: three iterations of the reference's own
run_training_seg_semi (utils/trainer.py:1903-2121) on CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segsemi.py <reference checkout>

In the manner of make_golden_segadv.py (g14): the reference's modules are
imported from its checkout (nothing is copied), weights come from seeded numpy
generators, the soft D labels replace make_D_label(random=True)'s draw,
run_testing_seg is stubbed to record the iteration's gradients, exp_dir is a
temporary directory.  B = 2 + 2 clouds of N = 256 points, PointNetSeg(50) +
PointwiseDiscNet(256, 50), ImagePool(0).

semi_start = 1 and three iterations: iteration 2 is the first with the
semi-supervised term.  Both Adams run at lr = 0: an Adam update with lr = 0
leaves every parameter bit unchanged, so iteration 2 starts from the seeded
weights and its gradients can be compared directly (no parameter drift between
two float32 implementations, the problem g14's docstring describes).

The run is made in float32 and in float64.  Iteration 0's and iteration 2's
gradients are stored from the float64 run (cast to float32, via summarize); the
float32 run's distance from them is printed per tensor for the record.

Seeded weights as g14's do not separate the points: D's output on the no-GT
rows then spans 3.1998..3.2011, and a threshold between two points would sit
at float32 resolution.  So the generator's seeded WEIGHTS (not biases) are
scaled by G_GAIN (stored as g_gain) and D's biases are 0.05 N(0, 1) drawn from
default_rng(d_seed + 1) in named_parameters() order, as
test_gpu_segadv_step._models(d_bias=0.05) does.  The threshold is the midpoint
of the widest gap between neighbouring values of iteration 2's no-GT D_out
(float64, the seeded weights) among those that keep between 25 % and 75 % of
the points.  On the float64 run's iteration 2 this script ASSERTS that
  - the kept share is within [0.25, 0.75],
  - every no-GT point has |D_out - TH| >= 1e-3 TH,
  - every kept row's top-two logit gap is >= 1e-4 of its max - min,
so neither the mask nor a pseudo-label is decided by rounding.
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

from oracle import pointnet_np as onp  # noqa: E402
from make_golden import summarize  # noqa: E402
from make_golden_segadv import pwdisc_spec  # noqa: E402

B, N, NCLS, ITERS = 2, 256, 50, 3
# seeds picked by a scan over G_SEED 15..26 x D_SEED {151, 161}: the pair whose
# threshold margin (1.9e-3 TH) and top-two gap (7e-2 of the range) are widest
G_SEED, D_SEED, DATA_SEED = 26, 151, 152
G_GAIN, D_BIAS = 3.0, 0.05
SEMI_START = 1
# With the gain the kept rows are confident (loss_semi ~1e-3 against loss_seg ~30),
# so lambda_semi is large: the term must carry a share of the generator's gradient
# that the comparison cannot miss (asserted in main: >= 10 % of every tensor's norm)
LAMBDA_SEG, LAMBDA_ADV, LAMBDA_SEMI, LR = 1.0, 1.0, 1000.0, 0.0


def make_data():
    """Per iteration: GT batch (pts, cls one-hot, seg), no-GT batch (pts, cls),
    soft labels for the GT and the no-GT rows."""
    rng = np.random.default_rng(DATA_SEED)
    its = []
    for _ in range(ITERS):
        d = {}
        for k in ("gt", "ng"):
            d["pts_" + k] = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
            c = np.zeros((B, 1, 16), np.float32)
            c[np.arange(B), 0, rng.integers(0, 16, B)] = 1.0
            d["cls_" + k] = c
        d["seg"] = rng.integers(0, NCLS, (B, N)).astype(np.int64)
        d["soft_gt"] = rng.uniform(0.7, 1.05, (B, N)).astype(np.float32)
        d["soft_ng"] = rng.uniform(0.0, 0.305, (B, N)).astype(np.float32)
        its.append(d)
    return its


def make_weights():
    """(generator state, D state): the seeded float32 weights both sides load."""
    Gp = onp.make_params(onp.seg_spec(NCLS), seed=G_SEED)
    for k in Gp:
        if k.endswith("weight"):
            Gp[k] = (np.float32(G_GAIN) * Gp[k]).astype(np.float32)
    Dp = onp.make_params(pwdisc_spec(NCLS), seed=D_SEED, init="xavier")
    rng = np.random.default_rng(D_SEED + 1)
    for k in Dp:  # named_parameters() order: conv1.weight, conv1.bias, ...
        if k.endswith("bias"):
            Dp[k] = (D_BIAS * rng.standard_normal(Dp[k].shape)).astype(np.float32)
    return Gp, Dp


def build(torch, PointNetSeg, PointwiseDiscNet, dtype):
    Gp, Dp = make_weights()
    model = PointNetSeg(NCLS)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    model_D = PointwiseDiscNet(N, NCLS)
    assert [n for n, _ in model_D.named_parameters()] == list(Dp)
    model_D.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    return model.to(dtype), model_D.to(dtype)


def pick_threshold(d_out):
    """The midpoint of the widest gap between neighbouring sorted values among
    the cuts that keep 25 %..75 % of the points."""
    s = np.sort(np.asarray(d_out, np.float64).reshape(-1))
    n = s.size
    best, th = -1.0, None
    for i in range(n - 1):  # cut between s[i] and s[i + 1]: n - 1 - i kept
        kept = (n - 1 - i) / n
        if 0.25 <= kept <= 0.75 and s[i + 1] - s[i] > best:
            best, th = s[i + 1] - s[i], 0.5 * (s[i] + s[i + 1])
    return float(th), float(best)


def main(ref_root):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref_root)
    import torch
    import torch.nn as nn
    from models.pointnet import PointNetSeg
    from models.discriminator import PointwiseDiscNet
    import utils.trainer as rtrainer
    from utils.image_pool import ImagePool

    torch.set_num_threads(min(8, os.cpu_count() or 1))
    data = make_data()
    # the threshold, from iteration 2's no-GT D_out on the seeded weights in float64
    # (lr = 0: the weights the run itself has at iteration 2)
    m64, d64 = build(torch, PointNetSeg, PointwiseDiscNet, torch.float64)
    with torch.no_grad():
        pred = m64(torch.from_numpy(data[2]["pts_ng"]).double(),
                   torch.from_numpy(data[2]["cls_ng"]).double())[0]
        th, gap = pick_threshold(d64(torch.log_softmax(pred, dim=1)).numpy())
    print(f"semi_TH = {th!r}: the widest gap {gap:.3e} ({gap / th:.2e} relative)")

    mods = (torch, nn, PointNetSeg, PointwiseDiscNet, rtrainer, ImagePool)
    out32, snaps32 = capture(*mods, torch.float32, data, th)
    out, snaps = capture(*mods, torch.float64, data, th)
    # the conditions on iteration 2's inputs (float64 run)
    d_out = out["it2.d_out_nogt"].astype(np.float64).reshape(-1)
    logits = out["it2.pred_ng"].astype(np.float64).transpose(0, 2, 1).reshape(B * N, NCLS)
    keep = ~(d_out <= th)
    share = keep.mean()
    print(f"kept {int(keep.sum())} of {keep.size} ({share:.3f}), D_out in "
          f"{d_out.min():.4f}..{d_out.max():.4f}")
    assert 0.25 <= share <= 0.75, share
    margin = np.abs(d_out - th).min() / th
    print(f"smallest |D_out - TH| / TH = {margin:.3e}")
    assert margin >= 1e-3, margin
    top = np.sort(logits[keep], axis=1)
    rel_gap = ((top[:, -1] - top[:, -2]) / (top[:, -1] - top[:, 0])).min()
    print(f"smallest top-two logit gap of a kept row / its range = {rel_gap:.3e}")
    assert rel_gap >= 1e-4, rel_gap
    assert int(out["K"]) == int(keep.sum())
    assert np.array_equal(out["semi_gt"] == 255, ~keep.reshape(B, N))
    assert np.array_equal(out32["semi_gt"], out["semi_gt"]) and int(out32["K"]) == int(out["K"])
    # the term's share of iteration 2's generator gradients: its own gradient, by
    # autograd on the float64 modules, against the run's total
    m64.zero_grad()
    pred = m64(torch.from_numpy(data[2]["pts_ng"]).double(),
               torch.from_numpy(data[2]["cls_ng"]).double())[0]
    (LAMBDA_SEMI * nn.CrossEntropyLoss(ignore_index=255)(pred, torch.from_numpy(out["semi_gt"]))).backward()
    shares = {n: float(p.grad.norm() / snaps[2][("G", n)].norm()) for n, p in m64.named_parameters()}
    print("the semi term's share of the gradient norms:", {n: round(s, 3) for n, s in shares.items()})
    assert min(shares.values()) >= 0.1, shares
    # the float32 run's gradients against the float64 run's, for the record
    for it in (0, 2):
        for (w, n), g in snaps[it].items():
            a, r = snaps32[it][(w, n)].double().numpy().reshape(-1), g.numpy().reshape(-1)
            print(f"reference f32 vs f64, it{it} grad {w}.{n}: max-rel "
                  f"{np.abs(a - r).max() / max(np.abs(r).max(), 1e-300):.2e}, L2-rel "
                  f"{np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-300):.2e}")
            summarize(f"it{it}.grad{w}.{n}", g.numpy(), out)
    print("losses f32", {k: out32[k].tolist() for k in ("loss_seg", "loss_adv", "loss_semi", "loss_D")})
    print("losses f64", {k: out[k].tolist() for k in ("loss_seg", "loss_adv", "loss_semi", "loss_D")})
    # it2.d_out_nogt and it2.pred_ng stay float64: the restatement's loss is held
    # to the run's within 1e-6, closer than float32 logits give on these confident rows
    path = os.path.join(HERE, "g15_segsemi_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def capture(torch, nn, PointNetSeg, PointwiseDiscNet, rtrainer, ImagePool, dtype, data, th):
    """One run of the reference's run_training_seg_semi in `dtype`: (fixture
    entries, per-iteration gradients)."""
    model, model_D = build(torch, PointNetSeg, PointwiseDiscNet, dtype)
    out = {"B": B, "N": N, "iters": ITERS, "g_seed": G_SEED, "d_seed": D_SEED,
           "data_seed": DATA_SEED, "g_gain": G_GAIN, "d_bias": D_BIAS, "lambda_seg": LAMBDA_SEG,
           "lambda_adv": LAMBDA_ADV, "lambda_semi": LAMBDA_SEMI, "lr": LR,
           "semi_start": SEMI_START, "semi_TH": np.float64(th)}
    queue = []
    for d in data:
        queue += [d["soft_gt"].copy(), d["soft_ng"].copy()]
    orig = rtrainer.make_D_label

    def make_D_label(input, value, device, random=False):
        if random:
            lab = torch.from_numpy(queue.pop(0)).to(device, dtype)
            assert lab.shape == input.shape
            return lab
        return orig(input, value, device, random=False).to(dtype)

    d_outs, preds = [], []
    model_D.register_forward_hook(lambda m, i, o: d_outs.append(o.detach().clone()))
    model.register_forward_hook(lambda m, i, o: preds.append(o[0].detach().clone()))
    rec = {"seg": [], "gan": [], "semi": []}
    semi_targets = []

    class Rec(nn.Module):
        def __init__(self, inner, key):
            super().__init__()
            self.inner, self.key = inner, key

        def forward(self, a, b):
            r = self.inner(a, b)
            rec[self.key].append(float(r.item()))
            if self.key == "semi":
                semi_targets.append((len(rec["seg"]) - 1, b.detach().clone()))
            return r

    snaps = []

    def run_testing_seg(**kw):
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
                              lambda_semi=LAMBDA_SEMI, semi_start=SEMI_START, semi_TH=th,
                              iter_test_epoch=1, exp_dir=tempfile.mkdtemp(prefix="g15_"),
                              tensorboard=False)
    logger = logging.getLogger("golden15")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    orig_test = rtrainer.run_testing_seg
    rtrainer.make_D_label = make_D_label
    rtrainer.run_testing_seg = run_testing_seg
    try:
        rtrainer.run_training_seg_semi(
            trainloader_gt=gt_list, trainloader_nogt=ng_list,
            trainloader_gt_iter=enumerate(list(gt_list)),
            targetloader_nogt_iter=enumerate(list(ng_list)),
            testloader=None, testdataset=None, model=model, model_D=model_D,
            gan_loss=Rec(nn.BCEWithLogitsLoss(), "gan"), seg_loss=Rec(nn.CrossEntropyLoss(), "seg"),
            semi_loss=Rec(nn.CrossEntropyLoss(ignore_index=255), "semi"),
            optimizer=optimizer, optimizer_D=optimizer_D,
            history_pool_gt=ImagePool(0), history_pool_nogt=ImagePool(0),
            train_logger=logger, test_logger=logger, writer=None, args=args)
    finally:
        rtrainer.make_D_label = orig
        rtrainer.run_testing_seg = orig_test
    assert not queue and len(snaps) == ITERS and len(d_outs) == 3 * ITERS
    # lr = 0: no parameter bit moved
    for p, q in zip((p for m in (model, model_D) for p in m.parameters()), before):
        assert torch.equal(p.detach(), q)
    gan = np.array(rec["gan"]).reshape(ITERS, 3)
    out["loss_seg"] = np.array(rec["seg"])
    out["loss_adv"] = gan[:, 0]
    out["loss_D"] = 0.5 * gan[:, 1] + 0.5 * gan[:, 2]
    assert [i for i, _ in semi_targets] == [2] and len(rec["semi"]) == 1
    out["loss_semi"] = np.array([0.0, 0.0, rec["semi"][0]])
    semi_gt = semi_targets[0][1].numpy()
    out["semi_gt"] = semi_gt.astype(np.int64)
    out["K"] = np.int64((semi_gt != 255).sum())
    # iteration 2: D's output on the no-GT rows (the generator's pass) and the
    # predictions it saw (B x 50 x N, before the log_softmax)
    out["it2.d_out_nogt"] = d_outs[6].numpy()
    out["it2.pred_ng"] = preds[5].numpy()
    for i, d in enumerate(data):
        for k in ("cls_gt", "cls_ng", "seg"):
            out[f"it{i}.{k}"] = d[k]
    return out, snaps


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

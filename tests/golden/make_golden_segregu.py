"""Capture g17_segregu_step.npz: two iterations of the reference's own
run_training_seg_stack_regulization (utils/trainer.py:1218-1429) on CPU (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segregu.py <reference checkout>

In the manner of make_golden_segstack.py: the reference's modules are imported
from its checkout (nothing is copied), weights come from seeded numpy
generators, the soft D labels replace make_D_label(random=True)'s uniform_
draw, run_testing_seg_regulization is stubbed (it records the iteration's
gradients and the updated parameters) and exp_dir is a temporary directory.
B = 2 + 2 clouds of N = 256 points, PointNetSeg_regulization(50) +
StackDiscNet(256, 50, 16), BCELoss, CrossEntropyLoss twice, MSELoss,
ImagePool(0), two Adams, lambda_disc_shape = 0.5, two iterations.

The GT soft labels are drawn from U(0.7, 1.0), for the reason
make_golden_segstack.py gives (BCELoss refuses a target above 1).

fstn's last layer (fc3) is scaled by FSTN_FC3_SCALE so the feature transform
stays near the identity (max |T - I| is printed), which keeps StackDiscNet's
output inside [0, 1], where BCELoss accepts it: the run asserts that of every
D output.  lambda_regu is chosen so that the regulariser's part of
fstn.fc3.bias's gradient (the sum over clouds of dL/dT) and the rest of it are
of the same size: both shares are printed and asserted above 0.05.

The same run is repeated with both models in float64.  Stored:
  - both iterations' five losses of the float32 run (loss_seg, loss_adv,
    loss_regu, loss_D, loss_D_shape; loss_regu = l_gt + l_nogt unscaled, as
    the log line reports it) and of the float64 run (loss64_*);
  - iteration 0's trans_feat and stn output T3 of both batches from the float64
    run, rounded to float32 (it0.trans_feat64_*, it0.T3_64_*), and the float32
    run's T3;
  - the predictions D saw (it0.pred_*; the float64 run's as it0.pred64_*), the
    recorded data and labels;
  - G's iteration-0 gradients as summarize entries (it0.gradG.*), D's float64
    gradients (it0.grad64D.*), every tensor's float64 two-iteration update
    (it1.upd64<G|D>.*);
  - the reference's state_dict key list and shapes for the generator
    (g_keys, g_shapes: rows padded with 0).
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
import make_golden  # noqa: E402
from make_golden_segstack import stackdisc_spec  # noqa: E402
from segregu_ref import mse_reg, segregu_spec  # noqa: E402

B, N, NCLS, NSHAPES, ITERS = 2, 256, 50, 16, 2
G_SEED, D_SEED, DATA_SEED = 17, 171, 172
LAMBDA_SEG, LAMBDA_ADV, LAMBDA_DISC_SHAPE, LR = 100.0, 100.0, 0.5, 1e-4
LAMBDA_REGU = 10.0
FSTN_FC3_SCALE = 0.5
FULL_LIMIT = 4096  # tensors above this are stored as summaries (the file stays below 1 MiB)


def summarize(prefix, arr, out):
    old = make_golden.FULL_LIMIT
    make_golden.FULL_LIMIT = FULL_LIMIT
    try:
        make_golden.summarize(prefix, arr, out)
    finally:
        make_golden.FULL_LIMIT = old


def make_gen_params():
    """The generator's seeded weights: torch's default bounds, fstn.fc3 scaled."""
    p = onp.make_params(segregu_spec(NCLS), seed=G_SEED)
    for k in ("fstn.fc3.weight", "fstn.fc3.bias"):
        p[k] = (p[k] * np.float32(FSTN_FC3_SCALE)).astype(np.float32)
    return p


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
        d["soft_gt"] = rng.uniform(0.7, 1.0, (B, N, 1)).astype(np.float32)
        d["soft_ng"] = rng.uniform(0.0, 0.305, (B, N, 1)).astype(np.float32)
        its.append(d)
    return its


def main(ref_root):
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
    out, snaps, extra = capture(*mods, torch.float32)
    out64, snaps64, extra64 = capture(*mods, torch.float64)
    from golden_util import adam_update_err
    init = {("G", k): v for k, v in make_gen_params().items()}
    init |= {("D", k): v for k, v in onp.make_params(stackdisc_spec(), seed=D_SEED, init="xavier").items()}
    for (w, kind, n), v in snaps[1].items():
        if kind != "param":
            continue
        p64 = snaps64[1][(w, kind, n)].numpy()
        e, cnt = adam_update_err(v.numpy(), init[(w, n)], p64, init[(w, n)],
                                 snaps64[0][(w, "grad", n)].numpy())
        print(f"reference f32 vs f64, {w}.{n}: {e:.2e} over {cnt}")
        summarize(f"it1.upd64{w}.{n}", p64 - init[(w, n)].astype(np.float64), out)
    for (w, kind, n), v in snaps64[0].items():
        if w == "D" and kind == "grad":
            out[f"it0.grad64D.{n}"] = v.numpy().astype(np.float32)
    for k in ("loss_seg", "loss_adv", "loss_regu", "loss_D", "loss_D_shape"):
        out[k.replace("loss", "loss64")] = out64[k]
    for k in ("gt", "ng"):
        out[f"it0.trans_feat64_{k}"] = extra64["trans_" + k].astype(np.float32)
        out[f"it0.T3_64_{k}"] = extra64["T3_" + k].astype(np.float32)
        out[f"it0.T3_{k}"] = extra["T3_" + k].astype(np.float32)
        out[f"it0.pred64_{k}"] = out64[f"it0.pred_{k}"]
    # the regulariser's share of fstn.fc3.bias's gradient (= the sum over the
    # 2 B clouds of dL/dT), from the float64 run
    T = np.concatenate([extra64["trans_gt"], extra64["trans_ng"]])
    _, greg = mse_reg(T, B0=B, scale=LAMBDA_REGU)
    gb = snaps64[0][("G", "grad", "fstn.fc3.bias")].numpy().reshape(-1)
    share = np.linalg.norm(greg.sum(0).reshape(-1)) / np.linalg.norm(gb)
    rest = np.linalg.norm(gb - greg.sum(0).reshape(-1)) / np.linalg.norm(gb)
    print(f"regulariser's share of fstn.fc3.bias's gradient: {share:.3f} (the rest: {rest:.3f}) "
          f"(max |T - I| = {np.abs(T - np.eye(128)[None]).max():.3f})")
    assert share > 0.05 and rest > 0.05
    sd = extra["state_dict"]
    out["g_keys"] = np.array([k for k, _ in sd])
    out["g_shapes"] = np.array([list(s) + [0] * (3 - len(s)) for _, s in sd], np.int64)
    path = os.path.join(HERE, "g17_segregu_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def capture(torch, nn, PointNetSeg_regulization, StackDiscNet, rtrainer, ImagePool, dtype):
    """One run of the reference's run_training_seg_stack_regulization in `dtype`:
    (fixture entries, per-iteration snapshots, iteration 0's transforms)."""
    Gp = make_gen_params()
    Dp = onp.make_params(stackdisc_spec(), seed=D_SEED, init="xavier")
    model = PointNetSeg_regulization(NCLS)
    state = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert [k for k, _ in state] == list(Gp) and all(tuple(Gp[k].shape) == s for k, s in state)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    model_D = StackDiscNet(N, NCLS, NSHAPES)
    model_D.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    model.to(dtype)
    model_D.to(dtype)
    data = make_data()
    out = {"B": B, "N": N, "iters": ITERS, "g_seed": G_SEED, "d_seed": D_SEED,
           "data_seed": DATA_SEED, "lambda_seg": LAMBDA_SEG, "lambda_adv": LAMBDA_ADV,
           "lambda_disc_shape": LAMBDA_DISC_SHAPE, "lambda_regu": LAMBDA_REGU, "lr": LR,
           "num_shapes": NSHAPES, "fstn_fc3_scale": FSTN_FC3_SCALE}

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

    d_outs, preds, trans, t3 = [], [], [], []
    model_D.register_forward_hook(lambda m, i, o: d_outs.append([t.detach().clone() for t in o]))
    def g_hook(m, i, o):  # (a hook's return value would replace the output)
        preds.append(o[0].detach().clone())
        trans.append(o[2].detach().clone())
    model.register_forward_hook(g_hook)
    model.stn.register_forward_hook(lambda m, i, o: t3.append(o.detach().clone()))
    rec = {"seg": [], "gan": [], "shape": [], "regu": []}

    class Rec(nn.Module):
        def __init__(self, inner, key):
            super().__init__()
            self.inner, self.key = inner, key

        def forward(self, a, b):
            if self.key == "regu":
                b = b.to(a.dtype)  # the loop's torch.eye is float32 in the float64 run too
            r = self.inner(a, b)
            rec[self.key].append(float(r.item()))
            return r

    snaps = []

    def run_testing_seg_regulization(**kw):
        """Stands in for the test pass after each iteration: the iteration's
        gradients (p.grad until the next zero_grad) and the updated parameters."""
        snaps.append({(w, kind, n): (p.grad if kind == "grad" else p).detach().clone()
                      for w, m in (("G", model), ("D", model_D)) for n, p in m.named_parameters()
                      for kind in ("grad", "param")})
        return 0.0, 0.0, 0.0, 0.0

    t = lambda a: torch.from_numpy(a).to(dtype) if a.dtype == np.float32 else torch.from_numpy(a)  # noqa: E731
    gt_list = [(t(d["pts_gt"]), t(d["cls_gt"]), t(d["seg"])) for d in data]
    ng_list = [(t(d["pts_ng"]), t(d["cls_ng"])) for d in data]
    optimizer = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999))
    optimizer_D = torch.optim.Adam(model_D.parameters(), lr=LR, betas=(0.9, 0.999))
    args = argparse.Namespace(device=torch.device("cpu"), total_iterations=ITERS,
                              lambda_seg=LAMBDA_SEG, lambda_adv=LAMBDA_ADV,
                              lambda_disc_shape=LAMBDA_DISC_SHAPE, lambda_regu=LAMBDA_REGU,
                              iter_test_epoch=1, exp_dir=tempfile.mkdtemp(prefix="g17_"),
                              tensorboard=False)
    logger = logging.getLogger("golden17")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    orig_test = rtrainer.run_testing_seg_regulization
    rtrainer.make_D_label = make_D_label
    rtrainer.run_testing_seg_regulization = run_testing_seg_regulization
    try:
        rtrainer.run_training_seg_stack_regulization(
            trainloader_gt=gt_list, trainloader_nogt=ng_list,
            trainloader_gt_iter=enumerate(list(gt_list)),
            targetloader_nogt_iter=enumerate(list(ng_list)),
            testloader=None, testdataset=None, model=model, model_D=model_D,
            gan_loss=Rec(nn.BCELoss(), "gan"), seg_loss=Rec(nn.CrossEntropyLoss(), "seg"),
            regu_loss=Rec(nn.MSELoss(), "regu"),
            shape_criterion=Rec(nn.CrossEntropyLoss(), "shape"),
            optimizer=optimizer, optimizer_D=optimizer_D,
            history_pool_gt=ImagePool(0), history_pool_nogt=ImagePool(0),
            train_logger=logger, test_logger=logger, writer=None, args=args)
    finally:
        rtrainer.make_D_label = orig
        rtrainer.run_testing_seg_regulization = orig_test
    assert not queue and len(snaps) == ITERS and len(d_outs) == 4 * ITERS
    # the condition on the inputs: every D output BCELoss saw is inside [0, 1]
    for o in d_outs:
        assert float(o[1].min()) >= 0.0 and float(o[1].max()) <= 1.0, "D output outside [0, 1]"
    gan = np.array(rec["gan"]).reshape(ITERS, 3)
    out["loss_seg"] = np.array(rec["seg"])
    out["loss_adv"] = gan[:, 0]
    out["loss_regu"] = np.array(rec["regu"]).reshape(ITERS, 2).sum(1)  # l_gt + l_nogt, unscaled
    out["loss_D"] = 0.5 * gan[:, 1] + 0.5 * gan[:, 2]
    out["loss_D_shape"] = np.array(rec["shape"])  # unscaled, as the log line reports it
    out["it0.pred_gt"] = preds[0].float().numpy()
    out["it0.pred_ng"] = preds[1].float().numpy()
    for i, d in enumerate(data):
        for k in ("pts_gt", "pts_ng", "cls_gt", "cls_ng", "seg", "soft_gt", "soft_ng"):
            out[f"it{i}.{k}"] = d[k]
    for (w, kind, n), v in snaps[0].items():
        if w == "G" and kind == "grad":
            summarize(f"it0.{kind}{w}.{n}", v.numpy(), out)
    extra = dict(trans_gt=trans[0].double().numpy(), trans_ng=trans[1].double().numpy(),
                 T3_gt=t3[0].double().numpy(), T3_ng=t3[1].double().numpy(), state_dict=state)
    print(f"{dtype}: losses seg {out['loss_seg']} adv {out['loss_adv']} regu {out['loss_regu']} "
          f"D {out['loss_D']} D_shape {out['loss_D_shape']}; D outputs in "
          f"[{min(float(o[1].min()) for o in d_outs):.4f}, {max(float(o[1].max()) for o in d_outs):.4f}]")
    return out, snaps, extra


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

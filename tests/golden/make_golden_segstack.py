"""Capture g16_segstack_step.npz: two iterations of the reference's own
run_training_seg_stack (utils/trainer.py:1028-1216) on CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segstack.py <reference checkout>

In the manner of make_golden_segadv.py: the reference's modules are imported
from its checkout (nothing is copied), weights come from seeded numpy
generators, the soft D labels replace make_D_label(random=True)'s uniform_
draw, run_testing_seg is stubbed (it records the iteration's gradients and the
updated parameters) and exp_dir is a temporary directory.  B = 2 + 2 clouds of
N = 256 points, PointNetSeg(50) + StackDiscNet(256, 50, 16), BCELoss,
CrossEntropyLoss twice, ImagePool(0), two Adams, lambda_disc_shape = 0.5 (so its
scaling shows): two iterations, so Adam's moments matter.

The GT soft labels are drawn from U(0.7, 1.0) here, not the reference's
U(0.7, 1.05): torch's BCELoss refuses a target above 1 ("all elements of target
should be between 0 and 1"), so the reference's loop cannot run with its own
draw on a current torch.  Labels up to 1.05 are covered by the kernel tests
against the float64 restatement instead.

The same run is repeated with both models in float64.  Stored from it: D's
iteration-0 gradients (it0.grad64D.*, what the float64 restatement is compared
with) and, for every tensor of G and D, the update over both iterations
p_it1 - p_init (it1.upd64<G|D>.*; see make_golden_segadv.py for why the second
update is taken from the float64 run).  D's iteration-0 outputs are stored from
the float32 run (d_out_*; iteration 1's as it1.d_out_*, with both iterations'
predictions of the generator, it<i>.pred_*) and, for the restatement, from the
reference's module in float64 on the recorded predictions (d_out64_*,
s_out64_gt).
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

B, N, NCLS, NSHAPES, ITERS = 2, 256, 50, 16, 2
G_SEED, D_SEED, DATA_SEED = 16, 161, 162
# the lambdas scale the generator's gradients above the 1e-5 floor of the
# Adam-update check (make_golden_segadv.py); Adam itself is scale-free
LAMBDA_SEG, LAMBDA_ADV, LAMBDA_DISC_SHAPE, LR = 100.0, 100.0, 0.5, 1e-4


def stackdisc_spec(input_dim=NCLS, num_shapes=NSHAPES):
    """models/discriminator.py:139-150 (StackDiscNet(input_pts, input_dim, num_shapes))."""
    dims = [(64, input_dim), (64, 64), (64, 64), (128, 64), (num_shapes, 1)]
    s = []
    for i, (o, c) in enumerate(dims, 1):
        s += [(f"conv{i}.weight", (o, c, 1)), (f"conv{i}.bias", (o,))]
    return s


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
    from models.pointnet import PointNetSeg
    from models.discriminator import StackDiscNet
    import utils.trainer as rtrainer
    from utils.image_pool import ImagePool

    torch.set_num_threads(min(8, os.cpu_count() or 1))
    mods = (torch, nn, PointNetSeg, StackDiscNet, rtrainer, ImagePool)
    out, snaps, _ = capture(*mods, torch.float32)
    _, snaps64, _ = capture(*mods, torch.float64)
    sys.path.insert(0, os.path.dirname(HERE))
    from golden_util import adam_update_err
    init = {("G", k): v for k, v in onp.make_params(onp.seg_spec(NCLS), seed=G_SEED).items()}
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
    # D alone in float64 on the float32 run's recorded predictions (iteration 0's
    # weights): what a float64 restatement of D is compared with
    d64 = StackDiscNet(N, NCLS, NSHAPES)
    d64.load_state_dict({n: torch.from_numpy(v.copy()) for (w, n), v in init.items() if w == "D"})
    d64.double()
    with torch.no_grad():
        s_gt, o_gt = d64(torch.softmax(torch.from_numpy(out["it0.pred_gt"]).double(), dim=1))
        _, o_ng = d64(torch.log_softmax(torch.from_numpy(out["it0.pred_ng"]).double(), dim=1))
    # (the shape logits rounded to float32: they are w5 m + b5 of the m behind d_out64_gt)
    out["s_out64_gt"] = s_gt.numpy().astype(np.float32)
    out["d_out64_gt"], out["d_out64_nogt"] = o_gt.numpy(), o_ng.numpy()
    path = os.path.join(HERE, "g16_segstack_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def capture(torch, nn, PointNetSeg, StackDiscNet, rtrainer, ImagePool, dtype):
    """One run of the reference's run_training_seg_stack in `dtype`: (fixture
    entries, per-iteration snapshots, data)."""
    Gp = onp.make_params(onp.seg_spec(NCLS), seed=G_SEED)
    Dp = onp.make_params(stackdisc_spec(), seed=D_SEED, init="xavier")
    model = PointNetSeg(NCLS)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    model_D = StackDiscNet(N, NCLS, NSHAPES)
    model_D.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    model.to(dtype)
    model_D.to(dtype)
    data = make_data()
    out = {"B": B, "N": N, "iters": ITERS, "g_seed": G_SEED, "d_seed": D_SEED,
           "data_seed": DATA_SEED, "lambda_seg": LAMBDA_SEG, "lambda_adv": LAMBDA_ADV,
           "lambda_disc_shape": LAMBDA_DISC_SHAPE, "lr": LR, "num_shapes": NSHAPES}

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

    d_outs, preds, shape_labels = [], [], []
    model_D.register_forward_hook(lambda m, i, o: d_outs.append([t.detach().clone() for t in o]))
    model.register_forward_hook(lambda m, i, o: preds.append(o[0].detach().clone()))
    rec = {"seg": [], "gan": [], "shape": []}

    class Rec(nn.Module):
        def __init__(self, inner, key):
            super().__init__()
            self.inner, self.key = inner, key

        def forward(self, a, b):
            r = self.inner(a, b)
            rec[self.key].append(float(r.item()))
            if self.key == "shape":
                shape_labels.append(b.detach().clone())
            return r

    snaps = []

    def run_testing_seg(**kw):
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
                              lambda_disc_shape=LAMBDA_DISC_SHAPE, iter_test_epoch=1,
                              exp_dir=tempfile.mkdtemp(prefix="g16_"), tensorboard=False)
    logger = logging.getLogger("golden16")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    orig_test = rtrainer.run_testing_seg
    rtrainer.make_D_label = make_D_label
    rtrainer.run_testing_seg = run_testing_seg
    try:
        rtrainer.run_training_seg_stack(
            trainloader_gt=gt_list, trainloader_nogt=ng_list,
            trainloader_gt_iter=enumerate(list(gt_list)),
            targetloader_nogt_iter=enumerate(list(ng_list)),
            testloader=None, testdataset=None, model=model, model_D=model_D,
            gan_loss=Rec(nn.BCELoss(), "gan"), seg_loss=Rec(nn.CrossEntropyLoss(), "seg"),
            shape_criterion=Rec(nn.CrossEntropyLoss(), "shape"),
            optimizer=optimizer, optimizer_D=optimizer_D,
            history_pool_gt=ImagePool(0), history_pool_nogt=ImagePool(0),
            train_logger=logger, test_logger=logger, writer=None, args=args)
    finally:
        rtrainer.make_D_label = orig
        rtrainer.run_testing_seg = orig_test
    assert not queue and len(snaps) == ITERS and len(d_outs) == 4 * ITERS
    gan = np.array(rec["gan"]).reshape(ITERS, 3)
    out["loss_seg"] = np.array(rec["seg"])
    out["loss_adv"] = gan[:, 0]
    out["loss_D"] = 0.5 * gan[:, 1] + 0.5 * gan[:, 2]
    out["loss_D_shape"] = np.array(rec["shape"])  # unscaled, as the log line reports it
    # iteration 0's D outputs (B x N x 1): the no-GT rows (the generator's pass),
    # the GT rows; and the shape labels make_shape_label formed (B x N)
    out["d_out_nogt"] = d_outs[0][1].float().numpy()
    out["d_out_gt"] = d_outs[1][1].float().numpy()
    out["it1.d_out_nogt"] = d_outs[4][1].float().numpy()
    out["it1.d_out_gt"] = d_outs[5][1].float().numpy()
    out["it0.shape_label"] = shape_labels[0].numpy().astype(np.int64)
    # ... and the generator's predictions D saw (B x 50 x N each, before the
    # softmax / log_softmax), so D can be checked on its own
    for i in range(ITERS):
        out[f"it{i}.pred_gt"] = preds[2 * i].float().numpy()
        out[f"it{i}.pred_ng"] = preds[2 * i + 1].float().numpy()
    for i, d in enumerate(data):
        for k in ("cls_gt", "cls_ng", "seg", "soft_gt", "soft_ng"):
            out[f"it{i}.{k}"] = d[k]
    for (w, kind, n), v in snaps[0].items():
        # iteration 0's gradients of G (as g14; its parameters after both iterations
        # are it1.upd64G); D's gradients come from the float64 run
        if w == "G" and kind == "grad":
            summarize(f"it0.{kind}{w}.{n}", v.numpy(), out)
    return out, snaps, data


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

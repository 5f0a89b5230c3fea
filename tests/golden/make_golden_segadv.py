"""Capture g14_segadv_step.npz: two iterations of the reference's own
run_training_seg (utils/trainer.py:849-1026) on CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segadv.py <reference checkout>

In the manner of make_golden.py: the reference's modules are imported from its
checkout (nothing is copied), weights come from seeded numpy generators (only
seeds are stored for the generator), the soft D labels replace
make_D_label(random=True)'s uniform_ draw, run_testing_seg is stubbed (it
records the iteration's gradients and the updated parameters; iteration 0's
gradients are kept) and exp_dir is a temporary directory.  B = 2 + 2 clouds of
N = 256 points, PointNetSeg(50) + PointwiseDiscNet(256, 50), ImagePool(0), two
Adams: two iterations, so Adam's moments matter.

The same run is repeated with both models in float64.  The second Adam update
is linear in the second gradient, so the float32 run's parameters after
iteration 1 carry that gradient's float32 rounding (up to 5e-2 of the update on
the generator's late layers, printed here per tensor): iteration 1's parameters
are therefore taken from the float64 run, stored as the two-iteration update
p_it1 - p_init in float32 (it1.upd64<G|D>.<name>; p_init is the seeded float32
weights on both sides, so the difference keeps 24 bits of the update itself).
D's iteration-0 outputs are stored from the float32 run (d_out_*) and, for the
float64 restatement, from the reference's module in float64 on the recorded
predictions (d_out64_*).
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

B, N, NCLS, ITERS = 2, 256, 50, 2
G_SEED, D_SEED, DATA_SEED = 14, 141, 142
# the lambdas scale the generator's gradients (about 1e-6 at 1.0 on these untrained
# weights) above the 1e-5 floor of the Adam-update check; Adam itself is scale-free
LAMBDA_SEG, LAMBDA_ADV, LR = 100.0, 100.0, 1e-4


def pwdisc_spec(input_dim=NCLS):
    """models/discriminator.py:53-61 (PointwiseDiscNet(input_pts, input_dim))."""
    dims = [(64, input_dim), (64, 64), (64, 64), (128, 64)]
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
        d["soft_gt"] = rng.uniform(0.7, 1.05, (B, N)).astype(np.float32)
        d["soft_ng"] = rng.uniform(0.0, 0.305, (B, N)).astype(np.float32)
        its.append(d)
    return its


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
    f32 = capture(torch, nn, PointNetSeg, PointwiseDiscNet, rtrainer, ImagePool, torch.float32)
    f64 = capture(torch, nn, PointNetSeg, PointwiseDiscNet, rtrainer, ImagePool, torch.float64)
    out, snaps, data = f32
    # Iteration 1's parameters from the float64 run, as the update over both
    # iterations; the float32 run's distance from it is printed for the record.
    sys.path.insert(0, os.path.dirname(HERE))
    from golden_util import adam_update_err
    init = {("G", k): v for k, v in onp.make_params(onp.seg_spec(NCLS), seed=G_SEED).items()}
    init |= {("D", k): v for k, v in onp.make_params(pwdisc_spec(), seed=D_SEED, init="xavier").items()}
    for (w, kind, n), v in snaps[1].items():
        if kind != "param":
            continue
        p64 = f64[1][1][(w, kind, n)].numpy()
        e, cnt = adam_update_err(v.numpy(), init[(w, n)], p64, init[(w, n)],
                                 f64[1][0][(w, "grad", n)].numpy())
        print(f"reference f32 vs f64, {w}.{n}: {e:.2e} over {cnt}")
        summarize(f"it1.upd64{w}.{n}", p64 - init[(w, n)].astype(np.float64), out)
    # D alone in float64 on the float32 run's recorded predictions (iteration 0's
    # weights): what a float64 restatement of D is compared with
    d64 = PointwiseDiscNet(N, NCLS)
    d64.load_state_dict({n: torch.from_numpy(v.copy()) for (w, n), v in init.items() if w == "D"})
    d64.double()
    with torch.no_grad():
        out["d_out64_gt"] = d64(torch.softmax(torch.from_numpy(out["it0.pred_gt"]).double(), dim=1)).numpy()
        out["d_out64_nogt"] = d64(torch.log_softmax(torch.from_numpy(out["it0.pred_ng"]).double(), dim=1)).numpy()
    path = os.path.join(HERE, "g14_segadv_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def capture(torch, nn, PointNetSeg, PointwiseDiscNet, rtrainer, ImagePool, dtype):
    """One run of the reference's run_training_seg in `dtype`: (fixture entries,
    per-iteration snapshots, data)."""
    Gp = onp.make_params(onp.seg_spec(NCLS), seed=G_SEED)
    Dp = onp.make_params(pwdisc_spec(), seed=D_SEED, init="xavier")
    model = PointNetSeg(NCLS)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    model_D = PointwiseDiscNet(N, NCLS)
    model_D.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    model.to(dtype)
    model_D.to(dtype)
    data = make_data()
    out = {"B": B, "N": N, "iters": ITERS, "g_seed": G_SEED, "d_seed": D_SEED,
           "data_seed": DATA_SEED, "lambda_seg": LAMBDA_SEG, "lambda_adv": LAMBDA_ADV, "lr": LR}

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
    rec = {"seg": [], "gan": []}

    class Rec(nn.Module):
        def __init__(self, inner, key):
            super().__init__()
            self.inner, self.key = inner, key

        def forward(self, a, b):
            r = self.inner(a, b)
            rec[self.key].append(float(r.item()))
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
                              lambda_seg=LAMBDA_SEG, lambda_adv=LAMBDA_ADV, iter_test_epoch=1,
                              exp_dir=tempfile.mkdtemp(prefix="g14_"), tensorboard=False)
    logger = logging.getLogger("golden14")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    orig_test = rtrainer.run_testing_seg
    rtrainer.make_D_label = make_D_label
    rtrainer.run_testing_seg = run_testing_seg
    try:
        rtrainer.run_training_seg(
            trainloader_gt=gt_list, trainloader_nogt=ng_list,
            trainloader_gt_iter=enumerate(list(gt_list)),
            targetloader_nogt_iter=enumerate(list(ng_list)),
            testloader=None, testdataset=None, model=model, model_D=model_D,
            gan_loss=Rec(nn.BCEWithLogitsLoss(), "gan"), seg_loss=Rec(nn.CrossEntropyLoss(), "seg"),
            optimizer=optimizer, optimizer_D=optimizer_D,
            history_pool_gt=ImagePool(0), history_pool_nogt=ImagePool(0),
            train_logger=logger, test_logger=logger, writer=None, args=args)
    finally:
        rtrainer.make_D_label = orig
        rtrainer.run_testing_seg = orig_test
    assert not queue and len(snaps) == ITERS and len(d_outs) == 3 * ITERS
    gan = np.array(rec["gan"]).reshape(ITERS, 3)
    out["loss_seg"] = np.array(rec["seg"])
    out["loss_adv"] = gan[:, 0]
    out["loss_D"] = 0.5 * gan[:, 1] + 0.5 * gan[:, 2]
    # iteration 0's D outputs: the no-GT rows (the generator's pass), the GT rows
    out["d_out_nogt"] = d_outs[0].float().numpy()
    out["d_out_gt"] = d_outs[1].float().numpy()
    # ... and the generator's predictions D saw (B x 50 x N each, before the
    # softmax / log_softmax), so D can be checked on its own
    out["it0.pred_gt"] = preds[0].float().numpy()
    out["it0.pred_ng"] = preds[1].float().numpy()
    for i, d in enumerate(data):
        for k in ("cls_gt", "cls_ng", "seg", "soft_gt", "soft_ng"):
            out[f"it{i}.{k}"] = d[k]
    for i, s in enumerate(snaps):
        for (w, kind, n), v in s.items():
            if i > 0:
                continue  # iteration 0's gradients and parameters; iteration 1: main()
            summarize(f"it{i}.{kind}{w}.{n}", v.numpy(), out)
    return out, snaps, data


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

"""Capture g18_segdual_step.npz: two iterations of the reference's own
run_training_seg_dual (utils/trainer.py:2123-2382) on CPU (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segdual.py <reference checkout>

In the manner of make_golden_segstack.py: the reference's modules are imported
from its checkout (nothing is copied), weights come from seeded numpy
generators (the three D nets xavier-initialised), the soft D labels replace
make_D_label(random=True)'s uniform_ draw (the reference's own ranges, U(0.7,
1.05) and U(0, 0.305): BCE-with-logits takes targets above 1), run_testing_seg
is stubbed (it records the iteration's gradients and the updated parameters)
and exp_dir is a temporary directory.  B = 2 + 2 clouds of N = 256 points,
input_pts = 256, PointNetSeg(50) + BaseDiscNet(256, 50, 256) + ShapeDiscNet(256,
16) + PointDiscNet(256, 256), BCEWithLogitsLoss, CrossEntropyLoss twice,
ImagePool(0), Adam for G and two plain SGDs.

Three runs:
  f32    the whole loop in float32: predictions, D outputs, losses and G's
         iteration-0 gradients (it0.gradG.*);
  f64    the whole loop in float64: G's update over both iterations
         (it1.upd64G.*, see make_golden_segadv.py) ;
  d64    the reference's loop again in float64 with a stand-in generator that
         returns the f32 run's recorded predictions, so the three D nets see
         exactly those inputs: D outputs, losses, gradients and updates in
         float64 (d64.*; d64.it<i>.grad<net>.* and d64.it<i>.upd<net>.* = p_it<i> -
         p_init after each iteration), what a float64 restatement of the D side and the
         modules on recorded predictions are compared with.

lr_D_point, lr_D_shape and lambda_disc_shape are chosen so that the reference's
quirks show far above tolerance; the capture prints
  - how much the shape logits of iteration 0 change when the trunk of before
    optimizer_D_point.step() is used instead of the updated one, and
  - how much the point head's second update lr (g0 + g1) differs from lr g1,
both relative to the quantity's largest entry.  Large tensors are stored
through `summarize`.
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
import make_golden  # noqa: E402
from make_golden import summarize  # noqa: E402

B, N, NCLS, NSHAPES, ITERS = 2, 256, 50, 16, 2
G_SEED, S_SEED, H_SEED, P_SEED, DATA_SEED = 18, 181, 182, 183, 184
LAMBDA_SEG, LAMBDA_ADV, LR = 100.0, 100.0, 1e-4
LR_D_POINT, LR_D_SHAPE, LAMBDA_DISC_SHAPE = 0.5, 0.25, 2.0
NETS = ("S", "H", "P")  # shared trunk, shape head, point head


def dual_specs(input_dim=NCLS, num_shapes=NSHAPES):
    """models/discriminator.py:82-137: the state_dict entries of BaseDiscNet(
    input_pts, input_dim, 256), ShapeDiscNet(256, num_shapes), PointDiscNet(256,
    input_pts), conv4 of the trunk (registered, never used) included."""
    def convs(dims, names):
        s = []
        for n, (o, c) in zip(names, dims):
            s += [(f"{n}.weight", (o, c, 1)), (f"{n}.bias", (o,))]
        return s
    return {
        "S": convs([(64, input_dim), (64, 64), (256, 64), (256, 256)],
                   ["conv1", "conv2", "conv3", "conv4"]),
        "H": convs([(512, 256)], ["conv"]) + [("fc1.weight", (64, 512)), ("fc1.bias", (64,)),
                                              ("fc2.weight", (num_shapes, 64)),
                                              ("fc2.bias", (num_shapes,))],
        "P": convs([(256, 256), (128, 256), (128, 128)], ["conv1", "conv2", "conv3"]),
    }


def dual_params():
    sp = dual_specs()
    return {k: onp.make_params(sp[k], seed=s, init="xavier")
            for k, s in (("S", S_SEED), ("H", H_SEED), ("P", P_SEED))}


def make_data():
    """Per iteration: GT batch (pts, cls one-hot, seg), no-GT batch (pts, cls),
    soft labels for the GT and the no-GT rows (B x N / input_pts rows of
    input_pts = N: the shape of PointDiscNet's output)."""
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
    from models.discriminator import BaseDiscNet, PointDiscNet, ShapeDiscNet
    import utils.trainer as rtrainer
    from utils.image_pool import ImagePool

    torch.set_num_threads(min(8, os.cpu_count() or 1))
    # four nets' gradients and updates over two iterations: tensors above 4096
    # elements go through summarize's samples, so the fixture stays under 1 MiB
    make_golden.FULL_LIMIT = 4096
    mods = (torch, nn, PointNetSeg, (BaseDiscNet, ShapeDiscNet, PointDiscNet), rtrainer, ImagePool)
    out, snaps, rec32 = capture(*mods, torch.float32)
    _, snaps64, _ = capture(*mods, torch.float64)
    preds = [torch.from_numpy(out[f"it{i}.pred_{k}"]).double()
             for i in range(ITERS) for k in ("gt", "ng")]
    _, snapsd, recd = capture(*mods, torch.float64, replay=preds)

    Dp = dual_params()
    init = {("G", k): v for k, v in onp.make_params(onp.seg_spec(NCLS), seed=G_SEED).items()}
    for w in NETS:
        init |= {(w, k): v for k, v in Dp[w].items()}
    for (w, kind, n), v in snaps64[1].items():
        if w == "G" and kind == "param":
            summarize(f"it1.upd64G.{n}", v.numpy() - init[(w, n)].astype(np.float64), out)
    for i in range(ITERS):
        for (w, kind, n), v in snaps[i].items():
            if w == "G":
                if i == 0 and kind == "grad":
                    summarize(f"it0.gradG.{n}", v.numpy(), out)
                continue
            a = snapsd[i][(w, kind, n)].numpy()
            if kind == "param":
                summarize(f"d64.it{i}.upd{w}.{n}", a - init[(w, n)].astype(np.float64), out)
            else:
                summarize(f"d64.it{i}.grad{w}.{n}", a, out)
    for k, v in recd.items():
        out["d64." + k] = v
    for w in NETS:
        out[f"keys{w}"] = np.array([f"{n}:{'x'.join(map(str, v.shape))}" for n, v in Dp[w].items()])

    # the two quirks, as the capture sees them (d64 run)
    S0 = BaseDiscNet(N, NCLS, 256).double()
    S0.load_state_dict({k: torch.from_numpy(v.copy()).double() for k, v in Dp["S"].items()})
    H0 = ShapeDiscNet(256, NSHAPES).double()
    H0.load_state_dict({k: torch.from_numpy(v.copy()).double() for k, v in Dp["H"].items()})
    with torch.no_grad():
        old = H0(S0(torch.softmax(preds[0], dim=1))).numpy()
    new = recd["it0.shape_logits"]
    print("shape logits, old trunk vs updated trunk: %.3e of their largest entry"
          % (np.abs(old - new).max() / np.abs(new).max()))
    for n in ("conv1.weight", "conv3.weight"):
        p0 = snapsd[0][("P", "param", n)].numpy()
        p1 = snapsd[1][("P", "param", n)].numpy()
        a1 = snapsd[1][("P", "grad", n)].numpy()   # A_P = g0 + g1
        g1 = a1 - snapsd[0][("P", "grad", n)].numpy()
        upd = p1 - p0
        print(f"point head {n}: update vs -lr (g0 + g1) %.3e, vs -lr g1 %.3e of its largest entry"
              % (np.abs(upd + LR_D_POINT * a1).max() / np.abs(upd).max(),
                 np.abs(upd + LR_D_POINT * g1).max() / np.abs(upd).max()))
    for k in ("loss_seg", "loss_adv", "loss_D_point", "loss_D_shape"):
        print(k, out[k], out["d64." + k])
    path = os.path.join(HERE, "g18_segdual_step.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def capture(torch, nn, PointNetSeg, DNets, rtrainer, ImagePool, dtype, replay=None):
    """One run of the reference's run_training_seg_dual in `dtype`: (fixture
    entries, per-iteration snapshots, the D-side record).  replay: the
    generator's outputs to hand out instead of running PointNetSeg."""
    Gp = onp.make_params(onp.seg_spec(NCLS), seed=G_SEED)
    Dp = dual_params()
    if replay is None:
        model = PointNetSeg(NCLS)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    else:
        queue_pred = list(replay)

        class Replay(nn.Module):
            def __init__(self):
                super().__init__()
                self.w = nn.Parameter(torch.zeros(1))

            def forward(self, pts, cls):
                return queue_pred.pop(0) + 0 * self.w, None
        model = Replay()
    BaseDiscNet, ShapeDiscNet, PointDiscNet = DNets
    shared, shape, point = BaseDiscNet(N, NCLS, 256), ShapeDiscNet(256, NSHAPES), PointDiscNet(256, N)
    for m, k in ((shared, "S"), (shape, "H"), (point, "P")):
        m.load_state_dict({n: torch.from_numpy(v.copy()) for n, v in Dp[k].items()})
        m.to(dtype)
    model.to(dtype)
    data = make_data()
    out = {"B": B, "N": N, "iters": ITERS, "g_seed": G_SEED, "s_seed": S_SEED, "h_seed": H_SEED,
           "p_seed": P_SEED, "data_seed": DATA_SEED, "lambda_seg": LAMBDA_SEG,
           "lambda_adv": LAMBDA_ADV, "lambda_disc_shape": LAMBDA_DISC_SHAPE, "lr": LR,
           "lr_D_point": LR_D_POINT, "lr_D_shape": LR_D_SHAPE, "num_shapes": NSHAPES}

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

    p_outs, s_outs, preds = [], [], []
    point.register_forward_hook(lambda m, i, o: p_outs.append(o.detach().clone()))
    shape.register_forward_hook(lambda m, i, o: s_outs.append(o.detach().clone()))
    model.register_forward_hook(lambda m, i, o: preds.append(o[0].detach().clone()))
    rec = {"seg": [], "gan": [], "shape": []}

    class Rec(nn.Module):
        def __init__(self, inner, key):
            super().__init__()
            self.inner, self.key = inner, key

        def forward(self, a, b):
            r = self.inner(a, b)
            rec[self.key].append(float(r.item()))
            return r

    snaps = []
    named = (("G", model), ("S", shared), ("H", shape), ("P", point))

    def run_testing_seg(**kw):
        """Stands in for the test pass after each iteration: the iteration's
        gradients (p.grad as the loop leaves it; None, the trunk's unused conv4,
        as zeros) and the updated parameters."""
        snaps.append({(w, kind, n): ((torch.zeros_like(p) if p.grad is None else p.grad)
                                     if kind == "grad" else p).detach().clone()
                      for w, m in named for n, p in m.named_parameters()
                      for kind in ("grad", "param")})
        return 0.0, 0.0, 0.0, 0.0

    t = lambda a: torch.from_numpy(a).to(dtype) if a.dtype == np.float32 else torch.from_numpy(a)  # noqa: E731
    gt_list = [(t(d["pts_gt"]), t(d["cls_gt"]), t(d["seg"])) for d in data]
    ng_list = [(t(d["pts_ng"]), t(d["cls_ng"])) for d in data]
    optimizer = torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999))
    optimizer_D_shape = torch.optim.SGD(list(shape.parameters()) + list(shared.parameters()),
                                        lr=LR_D_SHAPE)
    optimizer_D_point = torch.optim.SGD(list(point.parameters()) + list(shared.parameters()),
                                        lr=LR_D_POINT)
    args = argparse.Namespace(device=torch.device("cpu"), total_iterations=ITERS,
                              lambda_seg=LAMBDA_SEG, lambda_adv=LAMBDA_ADV,
                              lambda_disc_shape=LAMBDA_DISC_SHAPE, iter_test_epoch=1,
                              exp_dir=tempfile.mkdtemp(prefix="g18_"), tensorboard=False)
    logger = logging.getLogger("golden18")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    orig_test = rtrainer.run_testing_seg
    rtrainer.make_D_label = make_D_label
    rtrainer.run_testing_seg = run_testing_seg
    try:
        rtrainer.run_training_seg_dual(
            trainloader_gt=gt_list, trainloader_nogt=ng_list,
            trainloader_gt_iter=enumerate(list(gt_list)),
            targetloader_nogt_iter=enumerate(list(ng_list)),
            testloader=None, testdataset=None, model=model, sharedDisc=shared, shapeDisc=shape,
            pointDisc=point, gan_point_loss=Rec(nn.BCEWithLogitsLoss(), "gan"),
            gan_shape_loss=Rec(nn.CrossEntropyLoss(), "shape"),
            seg_loss=Rec(nn.CrossEntropyLoss(), "seg"), optimizer=optimizer,
            optimizer_D_shape=optimizer_D_shape, optimizer_D_point=optimizer_D_point,
            history_pool_gt=ImagePool(0), history_pool_nogt=ImagePool(0),
            train_logger=logger, test_logger=logger, writer=None, args=args)
    finally:
        rtrainer.make_D_label = orig
        rtrainer.run_testing_seg = orig_test
    assert not queue and len(snaps) == ITERS and len(p_outs) == 3 * ITERS and len(s_outs) == ITERS
    gan = np.array(rec["gan"]).reshape(ITERS, 3)
    r = {"loss_seg": np.array(rec["seg"]), "loss_adv": gan[:, 0],
         "loss_D_point": 0.5 * gan[:, 1] + 0.5 * gan[:, 2],
         "loss_D_shape": np.array(rec["shape"])}  # unscaled, as the log line reports it
    for i in range(ITERS):
        # PointDiscNet's outputs: on the no-GT rows with D frozen (the generator's
        # term), on the GT rows, on the no-GT rows again; ShapeDiscNet's logits
        r[f"it{i}.point_nogt"] = p_outs[3 * i].numpy()
        r[f"it{i}.point_gt"] = p_outs[3 * i + 1].numpy()
        r[f"it{i}.shape_logits"] = s_outs[i].numpy()
    out.update(r)
    for i in range(ITERS):
        out[f"it{i}.pred_gt"] = preds[2 * i].float().numpy()
        out[f"it{i}.pred_ng"] = preds[2 * i + 1].float().numpy()
    for i, d in enumerate(data):
        for k in ("pts_gt", "pts_ng", "cls_gt", "cls_ng", "seg", "soft_gt", "soft_ng"):
            out[f"it{i}.{k}"] = d[k]
    return out, snaps, r


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

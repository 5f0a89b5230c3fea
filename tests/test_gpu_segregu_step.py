"""SegStackReguTrainStep and run_training_seg_stack_regulization on the device:
against the reference's two iterations (g17), graph replay against eager, the
fused step against the autograd body, and the trainer's fused and eager paths."""
import argparse
import copy
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

from golden_util import adam_update_err, check_tensor_l2, load
from oracle import pointnet_np as onp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segregu import make_data, make_gen_params  # noqa: E402
from make_golden_segstack import stackdisc_spec  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _models(N, d_seed=171, fc3_seed=None):
    """g17's seeded generator (fstn.fc3 scaled: T near I) and a StackDiscNet."""
    from adversarial_learning_on_pointclouds_amd import PointNetSeg_regulization, StackDiscNet
    G = make_gen_params()
    Dp = onp.make_params(stackdisc_spec(), seed=d_seed, init="xavier")
    m = PointNetSeg_regulization(50)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    d = StackDiscNet(N, 50, 16)
    d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    return m.to(DEV), d.to(DEV), G, Dp


def _fx_ref(fx, prefix, arr):
    """(the fixture's values, the same elements of arr): full or fixed samples."""
    flat = np.asarray(arr).reshape(-1)
    if prefix in fx:
        return np.asarray(fx[prefix]).reshape(-1), flat
    return np.asarray(fx[prefix + ".val"]), flat[fx[prefix + ".idx"]]


LOSSES = ("loss_seg", "loss_adv", "loss_regu", "loss_D", "loss_D_shape")


def test_step_vs_reference_g17():
    """The reference's two iterations with its soft labels: the five losses
    within 1e-3 in both; G's iteration-0 gradients at relative L2 2e-3; every
    tensor's update over both iterations against the reference's float64 run
    (it1.upd64*) by the Adam-update check at 1e-3."""
    from adversarial_learning_on_pointclouds_amd import SegStackReguTrainStep
    fx = load("g17_segregu_step.npz")
    B, N = int(fx["B"]), int(fx["N"])
    m, d, G0, D0 = _models(N, int(fx["d_seed"]))
    lr = float(fx["lr"])
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    opt_d = torch.optim.Adam(d.parameters(), lr=lr, betas=(0.9, 0.999))
    step = SegStackReguTrainStep(m, d, opt, opt_d, lambda_seg=float(fx["lambda_seg"]),
                                 lambda_adv=float(fx["lambda_adv"]),
                                 lambda_disc_shape=float(fx["lambda_disc_shape"]),
                                 lambda_regu=float(fx["lambda_regu"]))
    init = {("G", k): v for k, v in G0.items()} | {("D", k): v for k, v in D0.items()}
    g0 = {}
    for it, dd in enumerate(make_data()):
        for k in ("pts_gt", "pts_ng", "seg", "soft_gt"):
            assert np.array_equal(dd[k], fx[f"it{it}.{k}"])
        losses = step(_t(dd["pts_gt"]), _t(dd["cls_gt"]), _t(dd["seg"], torch.int64),
                      _t(dd["pts_ng"]), _t(dd["cls_ng"]), soft_gt=_t(dd["soft_gt"]),
                      soft_nogt=_t(dd["soft_ng"])).cpu().numpy()
        want = [float(fx[k][it]) for k in LOSSES]
        print(f"iteration {it}: losses {losses.tolist()} reference {want}")
        assert losses.shape == (5,) and np.max(np.abs(losses - np.array(want))) <= 1e-3
        assert step.logged() == losses.tolist()
        assert int(step.bad_rows.item()) == 0
        if it == 0:
            for name, p in m.named_parameters():
                e = check_tensor_l2(fx, "it0.gradG." + name, p.grad.cpu().numpy(), tol=2e-3)
                print(f"G.{name}: gradient relative L2 {e:.2e}")
            for w, mod in (("G", m), ("D", d)):
                for name, p in mod.named_parameters():
                    g0[(w, name)] = p.grad.cpu().numpy().copy()
    checked, bad = 0, []
    for w, mod in (("G", m), ("D", d)):
        for name, p in mod.named_parameters():
            new = p.detach().cpu().numpy()
            key = f"it1.upd64{w}.{name}"
            r_upd, a_new = _fx_ref(fx, key, new)
            a_init = _fx_ref(fx, key, init[(w, name)])[1]
            # selected by the reference's iteration-0 gradients (G's are stored at the
            # update's own sample indices, D's in full: sampled here)
            gsel = _fx_ref(fx, f"it0.gradG.{name}", new)[0] if w == "G" else \
                _fx_ref(fx, key, fx[f"it0.grad64D.{name}"])[1]
            e, n = adam_update_err(a_new, a_init, r_upd.astype(np.float64), np.zeros(len(r_upd)),
                                   gsel.astype(np.float64))
            print(f"{w}.{name}: two-iteration update rel err {e:.2e} over {n} elements")
            if n == 0 or e > 1e-3:
                bad.append(f"{w}.{name}: Adam update rel err {e:.3e} over {n} elements (tol 0.001)")
            checked += 1
    assert not bad, "\n".join(bad)
    assert checked == 54
    assert int(step.step_count.item()) == 2 and int(step.step_count_D.item()) == 2


def _inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    pts, pts_ng = (_t(rng.uniform(-1, 1, (B, N, 3))) for _ in range(2))
    cls, cls_ng = (_t(np.eye(16, dtype=np.float32)[rng.integers(0, 16, B)][:, None, :]) for _ in range(2))
    seg = _t(rng.integers(0, 50, (B, N)), torch.int64)
    return rng, pts, cls, seg, pts_ng, cls_ng


def test_graph_replay_equals_eager_bitwise():
    """One captured graph replayed twice against two eager calls from the same
    initial state (device-drawn labels)."""
    from adversarial_learning_on_pointclouds_amd import SegStackReguTrainStep
    B, N = 2, 128
    _, pts, cls, seg, pts_ng, cls_ng = _inputs(B, N, 9)
    res = []
    for graph in (False, True):
        m, d, _, _ = _models(N)
        step = SegStackReguTrainStep(m, d, lr=1e-3, lr_D=1e-3, lambda_adv=0.5, lambda_disc_shape=0.5,
                                     lambda_regu=10.0, seed=77)
        g = step.capture_on(pts, cls, seg, pts_ng, cls_ng) if graph else None
        ls = []
        for _ in range(2):
            if graph:
                g.replay()
            else:
                step(pts, cls, seg, pts_ng, cls_ng)
            ls.append(step.losses.clone())
        torch.cuda.synchronize()
        res.append((torch.stack(ls), step.param.clone(), step.d_param.clone(),
                    int(step.step_count.item()), int(step.step_count_D.item()),
                    int(step.bad_rows.item())))
    (la, pa, da, sa, sda, ba), (lb, pb, db, sb, sdb, bb) = res
    assert sa == sb == 2 and sda == sdb == 2 and ba == bb == 0
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(da, db)
    assert la.shape == (2, 5) and float(la[0, 2]) > 0 and not torch.equal(la[0], la[1])


class _SoftBCE(torch.nn.Module):
    """binary_cross_entropy (mean) by hand: not BCELoss by type, so the trainer
    takes the autograd body."""

    def forward(self, x, y):
        return -(y * torch.clamp(torch.log(x), min=-100)
                 + (1 - y) * torch.clamp(torch.log1p(-x), min=-100)).mean()


def _replay_labels(monkeypatch, soft):
    """trainer.make_D_label(random=True) hands out the given labels in order."""
    from adversarial_learning_on_pointclouds_amd import trainer
    orig = trainer.make_D_label
    q = list(soft)

    def make(input, value, device, random=False):
        if random:
            return q.pop(0).reshape(input.shape).to(device)
        return orig(input=input, value=value, device=device, random=False)
    monkeypatch.setattr(trainer, "make_D_label", make)
    return q


def test_step_vs_autograd_body(monkeypatch):
    """One iteration: the fused step and the eager _seg_adv_body (autograd over
    the modules, torch's losses and Adams) agree on the five losses at 1e-5."""
    from adversarial_learning_on_pointclouds_amd import SegStackReguTrainStep, trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    B, N = 2, 128
    m, d, _, _ = _models(N)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    rng, pts, cls, seg, pts_ng, cls_ng = _inputs(B, N, N)
    soft = [_t(rng.uniform(0.7, 1.0, (B, N))), _t(rng.uniform(0, 0.305, (B, N)))]
    lam_seg, lam_adv, lam_shape, lam_regu, lr = 1.0, 0.7, 0.5, 10.0, 1e-3
    mk = lambda mod: torch.optim.Adam(mod.parameters(), lr=lr)  # noqa: E731
    step = SegStackReguTrainStep(m, d, mk(m), mk(d), lambda_seg=lam_seg, lambda_adv=lam_adv,
                                 lambda_disc_shape=lam_shape, lambda_regu=lam_regu)
    losses = step(pts, cls, seg, pts_ng, cls_ng, soft_gt=soft[0], soft_nogt=soft[1]).tolist()
    q = _replay_labels(monkeypatch, soft)
    args = argparse.Namespace(device=DEV, lambda_seg=lam_seg, lambda_adv=lam_adv,
                              lambda_disc_shape=lam_shape, lambda_regu=lam_regu)
    want = trainer._seg_adv_body(m2, d2, mk(m2), mk(d2), torch.nn.BCELoss(),
                                 torch.nn.CrossEntropyLoss(), ImagePool(0), ImagePool(0), pts, cls,
                                 seg, pts_ng, cls_ng, args,
                                 shape_criterion=torch.nn.CrossEntropyLoss(),
                                 regu_loss=torch.nn.MSELoss())
    print("fused", losses, "autograd", want)
    assert not q and len(want) == 5
    assert np.max(np.abs(np.array(losses) - np.array(want))) <= 1e-5


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


PAT = re.compile(r"^iter = +\d+/ +\d+ loss_seg = \d+\.\d{3} loss_adv = \d+\.\d{3} "
                 r"loss_regu = \d+\.\d{3} loss_D = \d+\.\d{3} loss_D_shape = \d+\.\d{3} $")


def _batches(rng, sizes, N):
    gt, ng = [], []
    for b in sizes:
        one = lambda: torch.from_numpy(np.eye(16, dtype=np.float32)[rng.integers(0, 16, b)][:, None, :])  # noqa: E731
        gt.append((torch.from_numpy(rng.uniform(-1, 1, (b, N, 3)).astype(np.float32)), one(),
                   torch.from_numpy(rng.integers(0, 50, (b, N)))))
        ng.append((torch.from_numpy(rng.uniform(-1, 1, (b, N, 3)).astype(np.float32)), one()))
    return gt, ng


@pytest.mark.parametrize("ragged", [False, True])
def test_run_training_seg_stack_regulization(tmp_path, monkeypatch, ragged):
    """Over list loaders: a five-number log line per iteration in the
    reference's format, the fused step for equal batches and the eager body for
    a ragged one, the reference's checkpoint names, and the module test pass
    over the 3-tuple model."""
    from adversarial_learning_on_pointclouds_amd import seg, trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    N = 128
    rng = np.random.default_rng(4)
    orig = trainer.make_D_label

    def make(input, value, device, random=False):  # labels BCELoss accepts (<= 1)
        if random and value == 1:
            return torch.empty(input.shape, device=device).uniform_(0.7, 1.0)
        return orig(input=input, value=value, device=device, random=random)
    monkeypatch.setattr(trainer, "make_D_label", make)
    made, calls = [], []
    init0, call0 = seg.SegStackReguTrainStep.__init__, seg.SegStackReguTrainStep.__call__

    def init(self, *a, **k):
        made.append(self)
        init0(self, *a, **k)

    def call(self, *a, **k):
        calls.append(a[0].shape[0])
        return call0(self, *a, **k)
    monkeypatch.setattr(seg.SegStackReguTrainStep, "__init__", init)
    monkeypatch.setattr(seg.SegStackReguTrainStep, "__call__", call)
    sizes_gt = [2, 1] if ragged else [2, 2]
    gt, _ = _batches(rng, sizes_gt, N)
    _, ng = _batches(rng, [2, 2], N)
    m, d, _, _ = _models(N)
    exp = tmp_path / "exp"
    exp.mkdir()
    args = argparse.Namespace(device=DEV, total_iterations=2, lambda_seg=1.0, lambda_adv=0.5,
                              lambda_disc_shape=0.5, lambda_regu=10.0, iter_test_epoch=2,
                              exp_dir=str(exp), tensorboard=False, input_pts=N, seed=21,
                              native_eval=False)
    log, tlog = _Log(), _Log()
    trainer.run_training_seg_stack_regulization(
        gt, ng, enumerate(list(gt)), enumerate(list(ng)), [gt[0]], [0] * 2, m, d,
        torch.nn.BCELoss(), torch.nn.CrossEntropyLoss(), torch.nn.MSELoss(),
        torch.nn.CrossEntropyLoss(), torch.optim.Adam(m.parameters(), lr=1e-3),
        torch.optim.Adam(d.parameters(), lr=1e-3), ImagePool(0), ImagePool(0), log, tlog, None, args)
    lines = [s for s in log.lines if s.startswith("iter")]
    print(lines)
    assert len(lines) == 2 and all(PAT.match(s) for s in lines), lines
    assert all(len(re.findall(r"= (\d+\.\d{3})", s)) == 5 for s in lines)
    assert len(made) == 1 and calls == ([2] if ragged else [2, 2])
    # (the one test batch leaves most categories empty: no category mean, so no best_cat_iou)
    for name in ("model_train_epoch_0.pth", "modelD_train_epoch_0.pth", "model_train_best.pth",
                 "modelD_train_best_all_iou.pth"):
        assert (exp / name).exists(), name
    assert any(s.startswith("Test accuracy") for s in tlog.lines)
    sd = torch.load(exp / "model_train_epoch_0.pth", weights_only=True)
    assert list(sd) == list(make_gen_params())
    assert all(torch.isfinite(p).all() for p in list(m.parameters()) + list(d.parameters()))

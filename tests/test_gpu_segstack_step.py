"""SegStackTrainStep, StackDiscNet and run_training_seg_stack on the device:
against the reference's two iterations (g16), graph replay against eager, the
trainer's fused path against the autograd body, the bad_rows error, the
fall-backs, and the module's forward / backward against the restatement."""
import argparse
import copy
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

import stackdisc_ref as ref
from golden_util import (adam_update_err, assert_adam_update_close, assert_grad_close,
                         check_tensor_l2, load, rel_err)
from oracle import pointnet_np as onp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segstack import make_data, stackdisc_spec  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _models(g_seed, d_seed, N, ncls=50, d_bias=0.0):
    from adversarial_learning_on_pointclouds_amd import PointNetSeg, StackDiscNet
    G = onp.make_params(onp.seg_spec(ncls), seed=g_seed)
    Dp = onp.make_params(stackdisc_spec(ncls), seed=d_seed, init="xavier")
    m = PointNetSeg(ncls)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    d = StackDiscNet(N, ncls, 16)
    d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    if d_bias:
        rng = np.random.default_rng(d_seed + 1)
        for name, p in d.named_parameters():
            if name.endswith("bias"):
                p.data.copy_(torch.from_numpy((d_bias * rng.standard_normal(p.shape)).astype(np.float32)))
    return m.to(DEV), d.to(DEV), G, Dp


def _fx_ref(fx, prefix, arr):
    """(the fixture's values, the same elements of arr): full or fixed samples."""
    flat = np.asarray(arr).reshape(-1)
    if prefix in fx:
        return np.asarray(fx[prefix]).reshape(-1), flat
    return np.asarray(fx[prefix + ".val"]), flat[fx[prefix + ".idx"]]


def _adam_replay(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update number t in float64 (in place on p, m, v)."""
    m *= b1
    m += (1 - b1) * g
    v *= b2
    v += (1 - b2) * g * g
    p -= lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)


def test_step_vs_reference_g16():
    """The reference's two iterations with explicit labels, as
    test_gpu_segadv_step.py holds g14: the four losses within 1e-3; iteration
    0's gradients (D's ten against the float64 run's by assert_grad_close, G's
    by the relative L2 2e-3 of test_seg_step_golden_g8); each iteration's update
    against a float64 replay of torch's Adam on the step's own gradients; and
    the update over both iterations against the reference's float64 run
    (it1.upd64*), both by the Adam-update check at 1e-3."""
    from adversarial_learning_on_pointclouds_amd import SegStackTrainStep
    fx = load("g16_segstack_step.npz")
    B, N = int(fx["B"]), int(fx["N"])
    m, d, G0, D0 = _models(int(fx["g_seed"]), int(fx["d_seed"]), N)
    lr = float(fx["lr"])
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    opt_d = torch.optim.Adam(d.parameters(), lr=lr, betas=(0.9, 0.999))
    step = SegStackTrainStep(m, d, opt, opt_d, lambda_seg=float(fx["lambda_seg"]),
                             lambda_adv=float(fx["lambda_adv"]),
                             lambda_disc_shape=float(fx["lambda_disc_shape"]))
    data = make_data()
    init = {("G", k): v for k, v in G0.items()} | {("D", k): v for k, v in D0.items()}
    old = dict(init)
    rep = {k: (v.astype(np.float64).copy(), np.zeros(v.shape), np.zeros(v.shape))
           for k, v in init.items()}
    checked, bad = 0, []
    for it, dd in enumerate(data):
        assert np.array_equal(dd["seg"], fx[f"it{it}.seg"])
        losses = step(_t(dd["pts_gt"]), _t(dd["cls_gt"]), _t(dd["seg"], torch.int64),
                      _t(dd["pts_ng"]), _t(dd["cls_ng"]), soft_gt=_t(dd["soft_gt"]),
                      soft_nogt=_t(dd["soft_ng"])).cpu().numpy()
        want = [float(fx[k][it]) for k in ("loss_seg", "loss_adv", "loss_D", "loss_D_shape")]
        print(f"iteration {it}: losses {losses.tolist()} reference {want}")
        assert np.max(np.abs(losses - np.array(want))) <= 1e-3
        assert int(step.bad_rows.item()) == 0
        if it == 0:
            for name, p in d.named_parameters():
                assert_grad_close(p.grad.cpu().numpy(), fx["it0.grad64D." + name], "D." + name)
            for name, p in m.named_parameters():
                check_tensor_l2(fx, "it0.gradG." + name, p.grad.cpu().numpy(), tol=2e-3)
        for w, mod in (("G", m), ("D", d)):
            for name, p in mod.named_parameters():
                new = p.detach().cpu().numpy()
                g_own = p.grad.cpu().numpy().astype(np.float64)
                tag = f"it{it}.{w}.{name}"
                rp, rm, rv = rep[(w, name)]
                _adam_replay(rp, rm, rv, g_own, it + 1, lr)
                assert_adam_update_close(new, old[(w, name)], rp, old[(w, name)], g_own, tag + " replay")
                if it == 1:
                    a_new = _fx_ref(fx, f"it1.upd64{w}.{name}", new)[1]
                    a_init = _fx_ref(fx, f"it1.upd64{w}.{name}", init[(w, name)])[1]
                    r_upd = _fx_ref(fx, f"it1.upd64{w}.{name}", new)[0].astype(np.float64)
                    # selected by iteration 0's gradients: the reference's where stored
                    # (G), the step's own, held to the float64 run's above (D)
                    gsel = _fx_ref(fx, f"it0.gradG.{name}", new)[0] if w == "G" else \
                        _fx_ref(fx, f"it0.grad64D.{name}", new)[0]
                    e, n = adam_update_err(a_new, a_init, r_upd, np.zeros_like(r_upd),
                                           gsel.astype(np.float64))
                    print(f"{tag}: two-iteration update rel err {e:.2e} over {n} elements")
                    if n == 0 or e > 1e-3:
                        bad.append(f"{tag}: Adam update rel err {e:.3e} over {n} elements (tol 0.001)")
                    checked += 1
                old[(w, name)] = new.copy()
    assert not bad, "\n".join(bad)
    assert checked == 30
    assert int(step.step_count.item()) == 2 and int(step.step_count_D.item()) == 2


def _inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    pts, pts_ng = (_t(rng.uniform(-1, 1, (B, N, 3))) for _ in range(2))
    cls, cls_ng = (_t(np.eye(16, dtype=np.float32)[rng.integers(0, 16, B)][:, None, :]) for _ in range(2))
    seg = _t(rng.integers(0, 50, (B, N)), torch.int64)
    return rng, pts, cls, seg, pts_ng, cls_ng


class _SoftBCE(torch.nn.Module):
    """torch's binary_cross_entropy (mean) by hand, without its refusal of a
    target above 1: the reference draws labels up to 1.05.  Not BCELoss by type,
    so the trainer takes the autograd body."""

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


@pytest.mark.parametrize("B,N", [(2, 128), (3, 200)])
def test_step_vs_autograd_body(B, N, monkeypatch):
    """One step against the reference's body through autograd over the modules
    (StackDiscNet's own autograd path), torch CE and two torch Adams, labels up
    to 1.05."""
    from adversarial_learning_on_pointclouds_amd import SegStackTrainStep, trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    m, d, _, _ = _models(31 + N, 32 + N, N, d_bias=0.05)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    rng, pts, cls, seg, pts_ng, cls_ng = _inputs(B, N, N)
    soft = [_t(rng.uniform(0.7, 1.05, (B, N))), _t(rng.uniform(0, 0.305, (B, N)))]
    lam_seg, lam_adv, lam_shape, lr = 1.0, 0.7, 0.5, 1e-3
    mk = lambda mod: torch.optim.Adam(mod.parameters(), lr=lr)  # noqa: E731
    step = SegStackTrainStep(m, d, mk(m), mk(d), lambda_seg=lam_seg, lambda_adv=lam_adv,
                             lambda_disc_shape=lam_shape)
    p_old = [p.detach().clone() for mod in (m, d) for p in mod.parameters()]
    losses = step(pts, cls, seg, pts_ng, cls_ng, soft_gt=soft[0], soft_nogt=soft[1]).tolist()
    _replay_labels(monkeypatch, soft)
    args = argparse.Namespace(device=DEV, lambda_seg=lam_seg, lambda_adv=lam_adv,
                              lambda_disc_shape=lam_shape)
    want = trainer._seg_adv_body(m2, d2, mk(m2), mk(d2), _SoftBCE(), torch.nn.CrossEntropyLoss(),
                                 ImagePool(0), ImagePool(0), pts, cls, seg, pts_ng, cls_ng, args,
                                 shape_criterion=torch.nn.CrossEntropyLoss())
    print("fused", losses, "autograd", want)
    assert np.max(np.abs(np.array(losses) - np.array(want))) <= 1e-5
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, q, o in zip(names, ps, ps2, p_old):
        assert_grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), name)
        assert_adam_update_close(p.detach().cpu().numpy(), o.cpu().numpy(), q.detach().cpu().numpy(),
                                 o.cpu().numpy(), q.grad.cpu().numpy(), name)


def test_graph_replay_equals_eager_bitwise():
    """Three steps with device-drawn labels: one captured graph replayed against
    eager calls (the shape labels are formed inside the captured stream)."""
    from adversarial_learning_on_pointclouds_amd import SegStackTrainStep
    B, N = 2, 128
    _, pts, cls, seg, pts_ng, cls_ng = _inputs(B, N, 9)
    res = []
    for graph in (False, True):
        m, d, _, _ = _models(5, 6, N)
        step = SegStackTrainStep(m, d, lr=1e-3, lr_D=1e-3, lambda_adv=0.5, lambda_disc_shape=0.5,
                                 seed=77)
        g = step.capture_on(pts, cls, seg, pts_ng, cls_ng) if graph else None
        ls = []
        for _ in range(3):
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
    assert sa == sb == 3 and sda == sdb == 3 and ba == bb == 0
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(da, db)
    assert not torch.equal(la[0, 2], la[1, 2])  # loss_D moves: labels and parameters change


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


class _PlainAdam(torch.optim.Adam):
    """Adam by another type: run_training_seg_stack then takes the autograd body."""


def _device_labels(seed, steps, M):
    """The labels the fused step draws at the given step counts: k_pwd_fwd's for
    (seed, step, row) (tests/test_gpu_stackdisc.py holds the two equal)."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    ps = [torch.zeros(s, device=DEV) for s in ((64, 50, 1), (64,), (64, 64, 1), (64,), (64, 64, 1),
                                               (64,), (128, 64, 1), (128,))]
    out = []
    for s in steps:
        soft = torch.zeros(2 * M, device=DEV)
        D.pwdisc_forward(torch.zeros(2 * M, 50, device=DEV), 50, M, M, 1, 2, ps,
                         torch.empty(2 * M, device=DEV),
                         torch.empty(2 * M, device=DEV, dtype=torch.int32),
                         D.pwdisc_workspace(2 * M, DEV), losses=torch.zeros(4, device=DEV),
                         soft_out=soft, seed=seed, dout_d=torch.empty(2 * M, device=DEV),
                         step_count=torch.tensor([s], device=DEV, dtype=torch.int32))
        out += [soft[:M].clone(), soft[M:].clone()]
    return out


def _run_trainer(tmp_path, m, d, opt_cls, gan_loss, batches_gt, batches_ng, iters, tag, pool=0,
                 device=DEV):
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    exp = tmp_path / tag
    exp.mkdir()
    args = argparse.Namespace(device=device, total_iterations=iters, lambda_seg=1.0, lambda_adv=0.5,
                              lambda_disc_shape=0.5, iter_test_epoch=10 ** 9, exp_dir=str(exp),
                              tensorboard=False, input_pts=batches_gt[0][0].shape[1], seed=21,
                              native_eval=False)
    log = _Log()
    trainer.run_training_seg_stack(
        batches_gt, batches_ng, enumerate(list(batches_gt)), enumerate(list(batches_ng)),
        [batches_gt[0]], [0] * batches_gt[0][0].shape[0], m, d, gan_loss,
        torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(),
        opt_cls(m.parameters(), lr=1e-3), opt_cls(d.parameters(), lr=1e-3),
        ImagePool(pool), ImagePool(pool), log, logging.getLogger("segstack_test"), None, args)
    return log, exp


def _batches(rng, sizes, N):
    gt, ng = [], []
    for b in sizes:
        one = lambda: torch.from_numpy(np.eye(16, dtype=np.float32)[rng.integers(0, 16, b)][:, None, :])  # noqa: E731
        gt.append((torch.from_numpy(rng.uniform(-1, 1, (b, N, 3)).astype(np.float32)), one(),
                   torch.from_numpy(rng.integers(0, 50, (b, N)))))
        ng.append((torch.from_numpy(rng.uniform(-1, 1, (b, N, 3)).astype(np.float32)), one()))
    return gt, ng


PAT = re.compile(r"^iter = +\d+/ +\d+ loss_seg = \d+\.\d{3} loss_adv = \d+\.\d{3} loss_D = \d+\.\d{3} "
                 r"loss_D_shape = \d+\.\d{3} $")


def _spy_steps(monkeypatch):
    """Counts the SegStackTrainStep objects the trainer builds."""
    from adversarial_learning_on_pointclouds_amd import seg
    made = []
    orig = seg.SegStackTrainStep.__init__

    def init(self, *a, **k):
        made.append(self)
        orig(self, *a, **k)
    monkeypatch.setattr(seg.SegStackTrainStep, "__init__", init)
    return made


def test_run_training_seg_stack_fused_vs_eager(tmp_path, monkeypatch):
    """One iteration over in-memory loaders: the fused path's log line has the
    reference's format and its checkpoints their names, and its losses and
    parameters match the autograd body's, run with the labels the fused step
    drew."""
    N, B = 128, 2
    gt, ng = _batches(np.random.default_rng(3), [B], N)
    m, d, _, _ = _models(41, 42, N)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    p0 = [p.detach().cpu().numpy().copy() for mod in (m, d) for p in mod.parameters()]
    made = _spy_steps(monkeypatch)
    log, exp = _run_trainer(tmp_path, m, d, torch.optim.Adam, torch.nn.BCELoss(), gt, ng, 1, "fused")
    assert len(made) == 1
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == 1 and PAT.match(lines[0]), lines
    for name in ("model_train_epoch_0.pth", "modelD_train_epoch_0.pth", "model_train_best.pth",
                 "modelD_train_best.pth"):
        assert (exp / name).exists(), name
    q = _replay_labels(monkeypatch, _device_labels(21, [0], B * N))
    log2, _ = _run_trainer(tmp_path, m2, d2, torch.optim.Adam, _SoftBCE(), gt, ng, 1, "eager")
    assert not q and len(made) == 1
    lines2 = [s for s in log2.lines if s.startswith("iter")]
    print(lines, lines2)
    num = lambda ls: np.array([[float(v) for v in re.findall(r"= (\d+\.\d{3})", s)] for s in ls])  # noqa: E731
    assert num(lines).shape == (1, 4) and np.max(np.abs(num(lines) - num(lines2))) <= 2e-3
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, r, o in zip(names, ps, ps2, p0):
        assert_adam_update_close(p.detach().cpu().numpy(), o, r.detach().cpu().numpy(), o,
                                 r.grad.cpu().numpy(), name)


def test_run_training_seg_stack_raises_on_bad_rows(tmp_path):
    """conv5's bias at -5: D's output is about 1.8, where BCELoss raises; the
    fused loop raises the same error when it reads the iteration's losses."""
    N, B = 128, 2
    gt, ng = _batches(np.random.default_rng(5), [B], N)
    m, d, _, _ = _models(45, 46, N)
    with torch.no_grad():
        d.conv5.bias.fill_(-5.0)
    with pytest.raises(RuntimeError, match="all elements of input should be between 0 and 1"):
        _run_trainer(tmp_path, m, d, torch.optim.Adam, torch.nn.BCELoss(), gt, ng, 1, "bad")


@pytest.mark.parametrize("why", ["adam", "gan_loss", "pool", "ragged"])
def test_unfusable_configurations_fall_back(tmp_path, monkeypatch, why):
    """Another optimizer type, another gan_loss, a history pool, and batches of
    different shapes run the autograd body: no fused step is built (or, for the
    ragged batch, only the even iterations use it), and training proceeds."""
    from adversarial_learning_on_pointclouds_amd import trainer
    N = 128
    rng = np.random.default_rng(4)
    orig = trainer.make_D_label

    def make(input, value, device, random=False):  # labels BCELoss accepts (<= 1)
        if random and value == 1:
            return torch.empty(input.shape, device=device).uniform_(0.7, 1.0)
        return orig(input=input, value=value, device=device, random=random)
    monkeypatch.setattr(trainer, "make_D_label", make)
    made = _spy_steps(monkeypatch)
    m, d, _, _ = _models(43, 44, N)
    sizes_gt = [2, 1] if why == "ragged" else [2]
    gt, _ = _batches(rng, sizes_gt, N)
    _, ng = _batches(rng, [2] * len(sizes_gt), N)
    log, _ = _run_trainer(tmp_path, m, d, _PlainAdam if why == "adam" else torch.optim.Adam,
                          _SoftBCE() if why == "gan_loss" else torch.nn.BCELoss(), gt, ng,
                          len(sizes_gt), why, pool=3 if why == "pool" else 0)
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == len(sizes_gt) and all(PAT.match(s) for s in lines), lines
    assert len(made) == (1 if why == "ragged" else 0)
    assert all(torch.isfinite(p).all() for p in list(m.parameters()) + list(d.parameters()))


def test_module_forward_backward_vs_restatement():
    """StackDiscNet.forward over the kernels on a permuted view of point-major
    storage: both outputs against the restatement, and the gradients of a loss
    that uses both (so conv5 and the four fused layers all receive one) against
    the restatement's chain on the same weights, input included."""
    from adversarial_learning_on_pointclouds_amd import StackDiscNet
    torch.manual_seed(3)
    B, N, C, S = 3, 200, 50, 16
    m = StackDiscNet(N, C, S).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.05)
    pm = (2 * torch.randn(B, N, C, device=DEV)).requires_grad_(True)
    s_out, d_out = m(torch.log_softmax(pm, dim=2).permute(0, 2, 1))
    assert s_out.shape == (B, S, N) and d_out.shape == (B, N, 1)
    ws = torch.randn(B, S, N, device=DEV)
    wd = torch.randn(B, N, 1, device=DEV)
    ((s_out * ws).sum() + (d_out * wd).sum()).backward()
    params = [p.detach().cpu().numpy() for p in m.parameters()]
    lg = pm.detach().cpu().numpy().reshape(B * N, C).astype(np.float64)
    x0 = ref.transform(lg, ref.LOG_SOFTMAX)
    mm, _, _, _ = ref.forward(x0, params)
    Sr, out, d, p = ref.head(mm, params)
    assert rel_err(s_out.detach().permute(0, 2, 1).reshape(B * N, S).cpu().numpy(), Sr) <= 1e-5
    assert rel_err(d_out.detach().reshape(-1).cpu().numpy(), d) <= 1e-5
    # dL/dS = ws + wd dd/dout p; dL/dm = dS . w5
    wsr = ws.permute(0, 2, 1).reshape(B * N, S).cpu().numpy().astype(np.float64)
    wdr = wd.reshape(-1).cpu().numpy().astype(np.float64)
    dS = wsr + (wdr / (out + 1.0) ** 2)[:, None] * p
    w5 = params[8].reshape(-1).astype(np.float64)
    dm = dS @ w5
    grads, dx0 = ref.backward(x0, params, dm)
    grads += [(dS.T @ mm).reshape(params[8].shape), dS.sum(axis=0)]
    for (name, q), g in zip(m.named_parameters(), grads):
        assert_grad_close(q.grad.cpu().numpy(), g, name)
    assert_grad_close(pm.grad.cpu().numpy().reshape(B * N, C),
                      ref.transform_bwd(x0, dx0, ref.LOG_SOFTMAX), "input")

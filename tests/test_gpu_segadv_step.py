"""SegAdvTrainStep and run_training_seg on the device: against the reference's
two iterations (g14), against the autograd body over the same modules, graph
replay against eager, and the trainer's fused / eager paths."""
import argparse
import copy
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

from golden_util import (adam_update_err, assert_adam_update_close, assert_grad_close,
                         check_tensor_l2, load)
from oracle import pointnet_np as onp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segadv import make_data, pwdisc_spec  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _models(g_seed, d_seed, N, ncls=50, d_bias=0.0):
    from adversarial_learning_on_pointclouds_amd import PointNetSeg, PointwiseDiscNet
    G = onp.make_params(onp.seg_spec(ncls), seed=g_seed)
    Dp = onp.make_params(pwdisc_spec(ncls), seed=d_seed, init="xavier")
    m = PointNetSeg(ncls)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    d = PointwiseDiscNet(N, ncls)
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


def test_step_vs_reference_g14():
    """The reference's two iterations with explicit labels: losses within 1e-3;
    iteration 0's gradients (D: assert_grad_close, G: the relative L2 2e-3 of
    test_seg_step_golden_g8); the parameters after each iteration by the Adam
    update check.

    Iteration 0: assert_adam_update_close against the reference's parameters,
    elements selected by the reference's gradients (the first update is
    ~lr sign(g): insensitive to the gradient's rounding).

    Iteration 1, two checks.  (a) The update itself: every tensor against a
    float64 replay of torch's Adam (t = 2, the moments of iteration 0) on the
    step's own gradients.  (b) Against the reference: the update over both
    iterations, (p_it1 - p_init), against that of the reference's
    run_training_seg run in float64 (it1.upd64*), selected by iteration 0's
    gradients as the check does by default.  The second update is linear in the
    second gradient (up to 0.74 lr / |g0| per unit of it), so the float32
    rounding of that gradient shows in it: the reference's own float32 run is
    off its float64 run by up to 5.4e-2 in this very check (G.conv4.weight
    3.6e-2, G.conv5.weight 5.4e-2, D below 1e-5), which is why the float64 run
    is the one stored.  Both by assert_adam_update_close at its 1e-3.  Measured
    for (b) on an MI355X: at most 1.1e-5 (G.conv4.weight), D at most 6.2e-6."""
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep
    fx = load("g14_segadv_step.npz")
    B, N = int(fx["B"]), int(fx["N"])
    m, d, G0, D0 = _models(int(fx["g_seed"]), int(fx["d_seed"]), N)
    lr = float(fx["lr"])
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(0.9, 0.999))
    opt_d = torch.optim.Adam(d.parameters(), lr=lr, betas=(0.9, 0.999))
    step = SegAdvTrainStep(m, d, opt, opt_d, lambda_seg=float(fx["lambda_seg"]),
                           lambda_adv=float(fx["lambda_adv"]))
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
        ref = [float(fx["loss_seg"][it]), float(fx["loss_adv"][it]), float(fx["loss_D"][it])]
        print(f"iteration {it}: losses {losses.tolist()} reference {ref}")
        assert np.max(np.abs(losses - np.array(ref))) <= 1e-3
        if it == 0:
            for name, p in d.named_parameters():
                assert_grad_close(p.grad.cpu().numpy(), fx["it0.gradD." + name], "D." + name)
            for name, p in m.named_parameters():
                check_tensor_l2(fx, "it0.gradG." + name, p.grad.cpu().numpy(), tol=2e-3)
        for w, mod in (("G", m), ("D", d)):
            for name, p in mod.named_parameters():
                new = p.detach().cpu().numpy()
                g_own = p.grad.cpu().numpy().astype(np.float64)
                tag = f"it{it}.{w}.{name}"
                # (a) this iteration's update against the float64 replay on the step's gradients
                rp, rm, rv = rep[(w, name)]
                _adam_replay(rp, rm, rv, g_own, it + 1, lr)
                assert_adam_update_close(new, old[(w, name)], rp, old[(w, name)], g_own, tag + " replay")
                # (b) against the reference's parameters
                key = f"it{it}.param{w}.{name}"
                a_new = _fx_ref(fx, f"it0.param{w}.{name}", new)[1]
                a_init = _fx_ref(fx, f"it0.param{w}.{name}", init[(w, name)])[1]  # both sides start from the seeds
                gr0 = _fx_ref(fx, f"it0.grad{w}.{name}", new)[0].astype(np.float64)
                if it == 0:
                    r_new = _fx_ref(fx, key, new)[0]
                    e, n = adam_update_err(a_new, a_init, r_new, a_init, gr0)
                    print(f"{tag}: update rel err {e:.2e} over {n} elements")
                else:
                    r_upd = _fx_ref(fx, f"it1.upd64{w}.{name}", new)[0].astype(np.float64)
                    e, n = adam_update_err(a_new, a_init, r_upd, np.zeros_like(r_upd), gr0)
                    print(f"{tag}: two-iteration update rel err {e:.2e} over {n} elements")
                # assert_adam_update_close's two conditions, every tensor reported at once
                if n == 0 or e > 1e-3:
                    bad.append(f"{tag}: Adam update rel err {e:.3e} over {n} elements (tol 0.001)")
                checked += 1
                old[(w, name)] = new.copy()
    assert not bad, "\n".join(bad)
    assert checked == 56
    assert int(step.step_count.item()) == 2 and int(step.step_count_D.item()) == 2


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
    """One step against the reference's body through autograd over the modules,
    torch CE / BCE and two torch Adams."""
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep, trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    m, d, _, _ = _models(31 + N, 32 + N, N, d_bias=0.05)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    rng = np.random.default_rng(N)
    pts, pts_ng = (_t(rng.uniform(-1, 1, (B, N, 3))) for _ in range(2))
    cls, cls_ng = (_t(np.eye(16, dtype=np.float32)[rng.integers(0, 16, B)][:, None, :]) for _ in range(2))
    seg = _t(rng.integers(0, 50, (B, N)), torch.int64)
    soft = [_t(rng.uniform(0.7, 1.05, (B, N))), _t(rng.uniform(0, 0.305, (B, N)))]
    lam_seg, lam_adv, lr = 1.0, 0.7, 1e-3
    mk = lambda mod: torch.optim.Adam(mod.parameters(), lr=lr)  # noqa: E731
    step = SegAdvTrainStep(m, d, mk(m), mk(d), lambda_seg=lam_seg, lambda_adv=lam_adv)
    p_old = [p.detach().clone() for mod in (m, d) for p in mod.parameters()]
    losses = step(pts, cls, seg, pts_ng, cls_ng, soft_gt=soft[0], soft_nogt=soft[1]).tolist()
    _replay_labels(monkeypatch, soft)
    args = argparse.Namespace(device=DEV, lambda_seg=lam_seg, lambda_adv=lam_adv)
    ref = trainer._seg_adv_body(m2, d2, mk(m2), mk(d2), torch.nn.BCEWithLogitsLoss(),
                                torch.nn.CrossEntropyLoss(), ImagePool(0), ImagePool(0), pts, cls,
                                seg, pts_ng, cls_ng, args)
    print("fused", losses, "autograd", ref)
    assert np.max(np.abs(np.array(losses) - np.array(ref))) <= 1e-5
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, q, o in zip(names, ps, ps2, p_old):
        assert_grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), name)
        assert_adam_update_close(p.detach().cpu().numpy(), o.cpu().numpy(), q.detach().cpu().numpy(),
                                 o.cpu().numpy(), q.grad.cpu().numpy(), name)


def test_graph_replay_equals_eager_bitwise():
    """Three steps with device-drawn labels: one captured graph replayed against
    eager calls (fresh labels on every replay: the step counter keys them)."""
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep
    B, N = 2, 128
    rng = np.random.default_rng(9)
    pts, pts_ng = (_t(rng.uniform(-1, 1, (B, N, 3))) for _ in range(2))
    cls, cls_ng = (_t(np.eye(16, dtype=np.float32)[rng.integers(0, 16, B)][:, None, :]) for _ in range(2))
    seg = _t(rng.integers(0, 50, (B, N)), torch.int64)
    res = []
    for graph in (False, True):
        m, d, _, _ = _models(5, 6, N)
        step = SegAdvTrainStep(m, d, lr=1e-3, lr_D=1e-3, lambda_adv=0.5, seed=77)
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
                    int(step.step_count.item()), int(step.step_count_D.item())))
    (la, pa, da, sa, sda), (lb, pb, db, sb, sdb) = res
    assert sa == sb == 3 and sda == sdb == 3
    assert torch.equal(la, lb) and torch.equal(pa, pb) and torch.equal(da, db)
    assert not torch.equal(la[0, 2], la[1, 2])  # loss_D moves: labels and parameters change


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


class _PlainAdam(torch.optim.Adam):
    """Adam by another type: run_training_seg then takes the autograd body."""


def _device_labels(seed, steps, M):
    """The labels SegAdvTrainStep draws at the given step counts (they depend on
    (seed, step, row) only)."""
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


def _run_trainer(tmp_path, m, d, opt_cls, batches_gt, batches_ng, iters, tag):
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    exp = tmp_path / tag
    exp.mkdir()
    args = argparse.Namespace(device=DEV, total_iterations=iters, lambda_seg=1.0, lambda_adv=0.5,
                              iter_test_epoch=10 ** 9, exp_dir=str(exp), tensorboard=False,
                              input_pts=batches_gt[0][0].shape[1], seed=21, native_eval=False)
    log = _Log()
    trainer.run_training_seg(
        batches_gt, batches_ng, enumerate(list(batches_gt)), enumerate(list(batches_ng)),
        [batches_gt[0]], [0] * batches_gt[0][0].shape[0], m, d, torch.nn.BCEWithLogitsLoss(),
        torch.nn.CrossEntropyLoss(), opt_cls(m.parameters(), lr=1e-3), opt_cls(d.parameters(), lr=1e-3),
        ImagePool(0), ImagePool(0), log, logging.getLogger("segadv_test"), None, args)
    return log, exp


def _batches(rng, sizes, N):
    gt, ng = [], []
    for b in sizes:
        one = lambda: torch.from_numpy(np.eye(16, dtype=np.float32)[rng.integers(0, 16, b)][:, None, :])  # noqa: E731
        gt.append((torch.from_numpy(rng.uniform(-1, 1, (b, N, 3)).astype(np.float32)), one(),
                   torch.from_numpy(rng.integers(0, 50, (b, N)))))
        ng.append((torch.from_numpy(rng.uniform(-1, 1, (b, N, 3)).astype(np.float32)), one()))
    return gt, ng


def test_run_training_seg_fused_vs_eager(tmp_path, monkeypatch):
    """Three iterations over in-memory loaders: the fused path's log lines have
    the reference's format, and its parameters match the eager body's (run with
    the labels the fused step drew) within the Adam-update check."""
    N, B = 128, 2
    gt, ng = _batches(np.random.default_rng(3), [B, B, B], N)
    m, d, _, _ = _models(41, 42, N)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    p0 = [p.detach().cpu().numpy().copy() for mod in (m, d) for p in mod.parameters()]
    log, exp = _run_trainer(tmp_path, m, d, torch.optim.Adam, gt, ng, 3, "fused")
    pat = re.compile(r"^iter = +\d+/ +3 loss_seg = \d+\.\d{3} loss_adv = \d+\.\d{3} loss_D = \d+\.\d{3} $")
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == 3 and all(pat.match(s) for s in lines), lines
    assert (exp / "model_train_epoch_0.pth").exists() and (exp / "modelD_train_best.pth").exists()
    q = _replay_labels(monkeypatch, _device_labels(21, [0, 1, 2], B * N))
    log2, _ = _run_trainer(tmp_path, m2, d2, _PlainAdam, gt, ng, 3, "eager")
    assert not q
    lines2 = [s for s in log2.lines if s.startswith("iter")]
    print(lines, lines2)
    num = lambda ls: np.array([[float(v) for v in re.findall(r"= (\d+\.\d{3})", s)] for s in ls])  # noqa: E731
    assert np.max(np.abs(num(lines) - num(lines2))) <= 2e-3
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, r, o in zip(names, ps, ps2, p0):
        assert_adam_update_close(p.detach().cpu().numpy(), o, r.detach().cpu().numpy(), o,
                                 r.grad.cpu().numpy(), name)


def test_run_training_seg_ragged_batch(tmp_path):
    """A ragged last batch (GT and no-GT shapes differ) goes through the eager
    body, and training continues on the fused path."""
    N = 128
    rng = np.random.default_rng(4)
    gt, _ = _batches(rng, [2, 2, 1], N)
    _, ng = _batches(rng, [2, 2, 2], N)
    m, d, _, _ = _models(43, 44, N)
    log, _ = _run_trainer(tmp_path, m, d, torch.optim.Adam, gt, ng, 5, "ragged")
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == 5
    vals = np.array([[float(v) for v in re.findall(r"= (\d+\.\d{3})", s)] for s in lines])
    assert vals.shape == (5, 3) and np.all(np.isfinite(vals))
    assert all(torch.isfinite(p).all() for p in list(m.parameters()) + list(d.parameters()))

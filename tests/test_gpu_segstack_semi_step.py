"""SegStackTrainStep / SegStackReguTrainStep with semi=True and the two stacked
semi-supervised loops on the device: against the reference's own run (g19),
against the autograd body over the same modules, a threshold nothing passes,
graph replay against eager, and the trainers' fused / eager paths."""
import argparse
import copy
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import (assert_adam_update_close, assert_grad_close, check_tensor_l2, load)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segregu_semi import make_data, make_weights  # noqa: E402
from make_golden_segsemi import pick_threshold  # noqa: E402
from test_gpu_segregu_step import _models as _regu_seeded  # noqa: E402
from test_gpu_segstack_step import (_batches, _device_labels, _inputs, _Log, _models,  # noqa: E402
                                    _replay_labels, _SoftBCE, _t)

pytestmark = pytest.mark.gpu

DEV = "cuda"
# Seeded generators do not separate D's outputs on the points (g15, g19).  At a
# gain of 3 the kept rows are so confident that loss_semi is 1e-5, below what a
# 1e-5 bound or a log line's three decimals can see; at 2.5 the no-GT D outputs
# still spread over 0.76..0.78 with gaps near 1e-4 and loss_semi is about 0.4.
GAIN = 2.5
REGU = dict(lambda_disc_shape=0.5, lambda_regu=10.0)


def _models_for(regu, N, g_seed, d_seed):
    """Seeded models with the generator's non-T-Net weights times GAIN and D's
    biases 0.05 N(0, 1)."""
    if regu:
        m, d, _, _ = _regu_seeded(N, d_seed)
        rng = np.random.default_rng(d_seed + 1)
        with torch.no_grad():
            for name, p in d.named_parameters():
                if name.endswith("bias"):
                    p.copy_(torch.from_numpy((0.05 * rng.standard_normal(p.shape)).astype(np.float32)))
    else:
        m, d, _, _ = _models(g_seed, d_seed, N, d_bias=0.05)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("weight") and not name.startswith(("stn.", "fstn.")):
                p.mul_(GAIN)
    return m, d


def _step_class(regu):
    from adversarial_learning_on_pointclouds_amd import SegStackReguTrainStep, SegStackTrainStep
    return (SegStackReguTrainStep, REGU) if regu else (SegStackTrainStep, dict(lambda_disc_shape=0.5))


def _eager_d_out(m, d, pts_ng, cls_ng):
    with torch.no_grad():
        return d(F.log_softmax(m(pts_ng, cls_ng)[0], dim=1))[1].cpu().numpy().reshape(-1)


def _threshold(d_out):
    th, gap = pick_threshold(d_out)
    th = float(np.float32(th))
    print(f"D_out {d_out.min():.5f}..{d_out.max():.5f}, threshold {th:.7f} in a gap of {gap:.2e}, "
          f"smallest |D_out - TH| {np.abs(d_out - th).min():.2e}")
    return th


LOSSES = ("loss_seg", "loss_adv", "loss_regu", "loss_semi", "loss_D", "loss_D_shape")


def test_step_vs_reference_g19():
    """Iterations 0 (semi=False) and 2 (semi=True) of the reference's
    run_training_seg_stack_regulization_semi at lr 0: the six losses within
    1e-3, K and the pseudo-labels exactly, G's gradients at relative L2 2e-3 and
    D's by assert_grad_close, against the reference's float64 run."""
    from adversarial_learning_on_pointclouds_amd import (PointNetSeg_regulization,
                                                         SegStackReguTrainStep, StackDiscNet)
    fx = load("g19_segregu_semi_step.npz")
    B, N = int(fx["B"]), int(fx["N"])
    Gp, Dp = make_weights()
    m, d = PointNetSeg_regulization(50), StackDiscNet(N, 50, int(fx["num_shapes"]))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    m, d = m.to(DEV), d.to(DEV)
    lr = float(fx["lr"])
    assert lr == 0.0
    step = SegStackReguTrainStep(m, d, torch.optim.Adam(m.parameters(), lr=lr),
                                 torch.optim.Adam(d.parameters(), lr=lr),
                                 lambda_seg=float(fx["lambda_seg"]), lambda_adv=float(fx["lambda_adv"]),
                                 lambda_disc_shape=float(fx["lambda_disc_shape"]),
                                 lambda_regu=float(fx["lambda_regu"]),
                                 lambda_semi=float(fx["lambda_semi"]), semi_th=float(fx["semi_TH"]),
                                 keep_activations=True)
    data = make_data()
    for it in (0, 2):
        dd = data[it]
        for k in ("cls_gt", "cls_ng", "seg"):
            assert np.array_equal(dd[k], fx[f"it{it}.{k}"])
        step(_t(dd["pts_gt"]), _t(dd["cls_gt"]), _t(dd["seg"], torch.int64), _t(dd["pts_ng"]),
             _t(dd["cls_ng"]), soft_gt=_t(dd["soft_gt"]), soft_nogt=_t(dd["soft_ng"]),
             semi=it > int(fx["semi_start"]))
        losses = step.losses_semi.cpu().numpy()
        ref = np.array([fx[k][it] for k in LOSSES])
        print(f"iteration {it}: losses {losses.tolist()} reference {ref.tolist()}")
        assert losses.shape == (6,) and np.max(np.abs(losses - ref)) <= 1e-3
        assert torch.equal(step.losses.cpu(), torch.from_numpy(losses[[0, 1, 2, 4, 5]]))
        assert int(step.bad_rows.item()) == 0
        if it == 2:
            assert int(step.kept.item()) == int(fx["K"])
            assert np.array_equal(step.semi_labels.cpu().numpy().reshape(B, N), fx["semi_gt"])
            d_ref = fx["it2.d_out_nogt"].reshape(-1)
            d_own = step.d_out[B * N:].cpu().numpy()
            print(f"D_out on the no-GT rows: max diff {np.max(np.abs(d_own - d_ref)):.2e}, smallest "
                  f"|D_out - TH| {np.abs(d_ref - float(fx['semi_TH'])).min():.2e}")
        else:
            assert int(step.kept.item()) == 0 and step.semi_labels is None and losses[3] == 0.0
        for name, p in d.named_parameters():
            e = assert_grad_close(p.grad.cpu().numpy(), fx[f"it{it}.gradD.{name}"], "D." + name)
            print(f"it{it} D.{name}: max-rel {e[0]:.2e} L2-rel {e[1]:.2e}")
        for name, p in m.named_parameters():
            e = check_tensor_l2(fx, f"it{it}.gradG.{name}", p.grad.cpu().numpy(), tol=2e-3)
            print(f"it{it} G.{name}: relative L2 {e:.2e}")
    for mod, ref in ((m, Gp), (d, Dp)):  # lr 0: not a bit moved
        for name, p in mod.named_parameters():
            assert np.array_equal(p.detach().cpu().numpy(), ref[name])


@pytest.mark.parametrize("regu", [False, True], ids=["stack", "regu"])
@pytest.mark.parametrize("B,N", [(2, 128), (3, 200)])
def test_step_vs_autograd_body(B, N, regu, monkeypatch):
    """One semi=True step of either class against the reference's body through
    autograd over the modules (torch's losses, two torch Adams), replayed labels,
    the threshold in the widest gap of that run's own eager D_out: every loss
    within 1e-5, loss_semi > 0, K equal, the gradients and the Adam updates."""
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    m, d = _models_for(regu, N, 51 + N, 52 + N)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    rng, pts, cls, seg, pts_ng, cls_ng = _inputs(B, N, N + 1)
    soft = [_t(rng.uniform(0.7, 1.0, (B, N))), _t(rng.uniform(0, 0.305, (B, N)))]
    d_out = _eager_d_out(m2, d2, pts_ng, cls_ng)
    th = _threshold(d_out)
    lam_seg, lam_adv, lam_semi, lr = 1.0, 0.7, 10.0, 1e-3
    mk = lambda mod: torch.optim.Adam(mod.parameters(), lr=lr)  # noqa: E731
    Step, extra = _step_class(regu)
    step = Step(m, d, mk(m), mk(d), lambda_seg=lam_seg, lambda_adv=lam_adv, lambda_semi=lam_semi,
                semi_th=th, **extra)
    p_old = [p.detach().clone() for mod in (m, d) for p in mod.parameters()]
    step(pts, cls, seg, pts_ng, cls_ng, soft_gt=soft[0], soft_nogt=soft[1], semi=True)
    losses = step.losses_semi.tolist()
    q = _replay_labels(monkeypatch, soft)
    args = argparse.Namespace(device=DEV, lambda_seg=lam_seg, lambda_adv=lam_adv,
                              lambda_semi=lam_semi, semi_TH=th, **extra)
    ref = trainer._seg_adv_body(m2, d2, mk(m2), mk(d2), torch.nn.BCELoss(),
                                torch.nn.CrossEntropyLoss(), ImagePool(0), ImagePool(0), pts, cls,
                                seg, pts_ng, cls_ng, args,
                                semi_loss=torch.nn.CrossEntropyLoss(ignore_index=255), semi=True,
                                shape_criterion=torch.nn.CrossEntropyLoss(),
                                regu_loss=torch.nn.MSELoss() if regu else None)
    K = int((d_out > th).sum())
    print("fused", losses, "autograd", ref, "kept", int(step.kept.item()), "of", B * N)
    i_semi = 3 if regu else 2
    assert not q and len(ref) == len(losses) == (6 if regu else 5)
    assert int(step.kept.item()) == K and 0 < K < B * N
    assert ref[i_semi] > 0 and losses[i_semi] > 0
    assert np.max(np.abs(np.array(losses) - np.array(ref))) <= 1e-5
    assert step.logged(True) == losses and len(step.logged()) == len(losses) - 1
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, r, o in zip(names, ps, ps2, p_old):
        assert_grad_close(p.grad.cpu().numpy(), r.grad.cpu().numpy(), name)
        assert_adam_update_close(p.detach().cpu().numpy(), o.cpu().numpy(), r.detach().cpu().numpy(),
                                 o.cpu().numpy(), r.grad.cpu().numpy(), name)


@pytest.mark.parametrize("regu", [False, True], ids=["stack", "regu"])
def test_threshold_above_every_output_is_a_plain_step(regu):
    """semi=True with nothing kept: parameters, gradients and `losses` bitwise
    those of a semi=False step, loss_semi 0 and K 0; and a semi=False step after
    a semi=True one reports 0 / 0 again.  N = 100: this D takes any point count."""
    B, N = 2, 100
    rng, *batch = _inputs(B, N, 11)
    soft = dict(soft_gt=_t(rng.uniform(0.7, 1.0, (B, N))), soft_nogt=_t(rng.uniform(0, 0.305, (B, N))))
    Step, extra = _step_class(regu)
    i_semi = 3 if regu else 2
    res = []
    for semi in (False, True):
        m, d = _models_for(regu, 128, 71, 72)
        step = Step(m, d, lr=1e-3, lr_D=1e-3, lambda_adv=0.5, lambda_semi=10.0, semi_th=2.0, **extra)
        step(*batch, semi=semi, **soft)
        res.append((step.losses.clone(), step.losses_semi.clone(), int(step.kept.item()),
                    step.param.clone(), step.d_param.clone(), step.grad.clone(), step.d_grad.clone()))
    (l0, ls0, k0, p0, d0, g0, dg0), (l1, ls1, k1, p1, d1, g1, dg1) = res
    assert torch.equal(l0, l1) and torch.equal(p0, p1) and torch.equal(d0, d1)
    assert torch.equal(g0, g1) and torch.equal(dg0, dg1)
    assert k0 == k1 == 0 and float(ls0[i_semi]) == float(ls1[i_semi]) == 0.0 and torch.equal(ls0, ls1)
    # the term on (everything kept), then off: loss_semi and K return to 0
    step.semi_th = -1.0
    step(*batch, semi=True, **soft)
    assert int(step.kept.item()) == B * N and float(step.losses_semi[i_semi]) > 0
    step(*batch, semi=False, **soft)
    assert int(step.kept.item()) == 0 and float(step.losses_semi[i_semi]) == 0.0


@pytest.mark.parametrize("regu", [False, True], ids=["stack", "regu"])
def test_graph_replay_equals_eager_bitwise(regu):
    """A step without the term, then two with it, device-drawn labels: one
    captured graph per `semi` value replayed against eager calls."""
    B, N = 2, 128
    _, *batch = _inputs(B, N, 9)
    m, d = _models_for(regu, N, 61, 62)
    th = _threshold(_eager_d_out(m, d, batch[3], batch[4]))
    Step, extra = _step_class(regu)
    i_semi = 3 if regu else 2
    res = []
    for graph in (False, True):
        m, d = _models_for(regu, N, 61, 62)
        # small steps: the kept set should not turn over within the three updates
        step = Step(m, d, lr=1e-6, lr_D=1e-6, lambda_adv=0.5, lambda_semi=10.0, semi_th=th, seed=77,
                    **extra)
        graphs = {}  # captured at first use: a capture's warm-up leaves its own loss_semi and K
        ls, ks = [], []
        for semi in (False, True, True):
            if graph:
                if semi not in graphs:
                    graphs[semi] = step.capture_on(*batch, semi=semi)
                graphs[semi].replay()
            else:
                step(*batch, semi=semi)
            ls.append(step.losses_semi.clone())
            ks.append(step.kept.clone())
        torch.cuda.synchronize()
        res.append((torch.stack(ls), torch.stack(ks), step.param.clone(), step.d_param.clone(),
                    int(step.step_count.item()), int(step.step_count_D.item())))
    (la, ka, pa, da, sa, sda), (lb, kb, pb, db, sb, sdb) = res
    print("kept", ka.tolist(), "loss_semi", la[:, i_semi].tolist())
    assert sa == sb == 3 and sda == sdb == 3
    assert torch.equal(la, lb) and torch.equal(ka, kb) and torch.equal(pa, pb) and torch.equal(da, db)
    assert int(ka[0]) == 0 and float(la[0, i_semi]) == 0.0
    assert 0 < int(ka[1]) < B * N and int(ka[2]) > 0 and bool((la[1:, i_semi] > 0).all())
    assert not torch.equal(la[1], la[2])  # the parameters move


PATS = {
    False: re.compile(r"^iter = +\d+/ +4 loss_seg = \d+\.\d{3} loss_adv = \d+\.\d{3} "
                      r"loss_semi = \d+\.\d{3} loss_D = \d+\.\d{3} loss_D_shape = \d+\.\d{3} $"),
    True: re.compile(r"^iter = +\d+/ +4 loss_seg = \d+\.\d{3} loss_adv = \d+\.\d{3} "
                     r"loss_regu = \d+\.\d{3} loss_semi = \d+\.\d{3} loss_D = \d+\.\d{3} "
                     r"loss_D_shape = \d+\.\d{3} $"),
}


def _values(lines):
    return np.array([[float(v) for v in re.findall(r"= (\d+\.\d{3})", s)] for s in lines])


def _run_trainer(tmp_path, regu, m, d, gan_loss, gt, ng, th, tag):
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    exp = tmp_path / tag
    exp.mkdir()
    N = gt[0][0].shape[1]
    args = argparse.Namespace(device=DEV, total_iterations=4, lambda_seg=1.0, lambda_adv=0.5,
                              lambda_semi=10.0, semi_start=1, semi_TH=th, iter_test_epoch=10 ** 9,
                              exp_dir=str(exp), tensorboard=False, input_pts=N, seed=21,
                              native_eval=False, **REGU)
    log = _Log()
    # the test pass: one cloud of every category, so the category mean IoU is a number
    rng = np.random.default_rng(1)
    test_batch = (torch.from_numpy(rng.uniform(-1, 1, (16, N, 3)).astype(np.float32)),
                  torch.from_numpy(np.eye(16, dtype=np.float32)[:, None, :]),
                  torch.from_numpy(rng.integers(0, 50, (16, N))))
    # lr 0: every iteration starts from the seeded weights, so one threshold sits in
    # a gap of D's outputs for the whole run (the updates are test_step_vs_autograd_body's)
    opts = (torch.optim.Adam(m.parameters(), lr=0.0), torch.optim.Adam(d.parameters(), lr=0.0))
    common = (gt, ng, enumerate(list(gt)), enumerate(list(ng)), [test_batch], [0] * 16, m, d,
              gan_loss, torch.nn.CrossEntropyLoss())
    tail = (torch.nn.CrossEntropyLoss(ignore_index=255), torch.nn.CrossEntropyLoss(), *opts,
            ImagePool(0), ImagePool(0), log, logging.getLogger("segstack_semi_test"), None, args)
    if regu:
        ret = trainer.run_training_seg_stack_regulization_semi(*common, torch.nn.MSELoss(), *tail)
    else:
        ret = trainer.run_training_seg_stack_semi(*common, *tail)
    assert len(ret) == 3
    return log, exp


@pytest.mark.parametrize("regu", [False, True], ids=["stack", "regu"])
def test_loops_fused_vs_eager(tmp_path, monkeypatch, regu):
    """Four iterations with semi_start = 1 and a ragged last batch (one GT cloud,
    so iteration 3 runs the eager body with the term on): the fused steps ran
    without the term in iterations 0-1 and with it in iteration 2; the log lines
    have the loop's field order, iterations 0-1 log 0.000 for the term and 2-3
    more; the checkpoints are the reference's (by accuracy included); and every
    logged value is the eager run's (the autograd body throughout, with the
    labels the fused steps drew) within 2e-3."""
    from adversarial_learning_on_pointclouds_amd import trainer
    N, B = 128, 2
    rng = np.random.default_rng(13)
    gt, _ = _batches(rng, [B, B, B, 1], N)
    _, ng = _batches(rng, [B] * 4, N)
    m, d = _models_for(regu, N, 81, 82)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    th = _threshold(np.concatenate([_eager_d_out(m, d, ng[i][0].to(DEV), ng[i][1].to(DEV))
                                    for i in (2, 3)]))
    ragged = [torch.from_numpy(rng.uniform(0.7, 1.0, N).astype(np.float32)),
              torch.from_numpy(rng.uniform(0.0, 0.305, B * N).astype(np.float32))]
    Step, _ = _step_class(regu)
    calls, call0 = [], Step.__call__

    def call(self, *a, **k):
        calls.append(bool(k.get("semi", False)))
        return call0(self, *a, **k)
    monkeypatch.setattr(Step, "__call__", call)
    body, eager = trainer._seg_adv_body, []
    monkeypatch.setattr(trainer, "_seg_adv_body",
                        lambda *a, **k: eager.append((a[8].shape[0], k["semi"])) or body(*a, **k))
    q = _replay_labels(monkeypatch, ragged)
    log, exp = _run_trainer(tmp_path, regu, m, d, torch.nn.BCELoss(), gt, ng, th, "fused")
    assert not q and calls == [False, False, True] and eager == [(1, True)]
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == 4 and all(PATS[regu].match(s) for s in lines), lines
    vals = _values(lines)
    i_semi = 3 if regu else 2
    assert vals.shape == (4, 6 if regu else 5)
    assert np.all(vals[:2, i_semi] == 0.0) and np.all(vals[2:, i_semi] > 0.0)
    names = sorted(os.listdir(exp))
    assert names == sorted(f"{w}_train_{t}.pth" for w in ("model", "modelD")
                           for t in ("epoch_0", "best", "best_cat_iou", "best_all_iou")), names
    eager.clear()
    q = _replay_labels(monkeypatch, _device_labels(21, range(3), B * N) + ragged)
    log2, _ = _run_trainer(tmp_path, regu, m2, d2, _SoftBCE(), gt, ng, th, "eager")
    assert not q and eager == [(2, False), (2, False), (2, True), (1, True)] and len(calls) == 3
    lines2 = [s for s in log2.lines if s.startswith("iter")]
    print(lines, lines2, "threshold", th)
    assert all(PATS[regu].match(s) for s in lines2)
    assert np.max(np.abs(vals - _values(lines2))) <= 2e-3

"""SegAdvTrainStep(semi=True) and run_training_seg_semi on the device: against
the reference's own run (g15), against the autograd body over the same modules,
graph replay against eager, a threshold nothing passes, and the trainer's fused
/ eager paths."""
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

from golden_util import (adam_update_err, assert_adam_update_close, assert_grad_close,
                         check_tensor_l2, grad_err, load)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segsemi import make_data, make_weights, pick_threshold  # noqa: E402
from test_gpu_segadv_step import (_batches, _device_labels, _Log, _models, _PlainAdam,  # noqa: E402
                                  _replay_labels, _t)

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAIN = 3.0  # as g15: seeded generators do not separate D's outputs on the points


def _gained(g_seed, d_seed, N):
    """Seeded models whose D outputs are spread over the points: the generator's
    weights (not biases) times GAIN, D's biases 0.05 N(0, 1)."""
    m, d, _, _ = _models(g_seed, d_seed, N, d_bias=0.05)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("weight"):
                p.mul_(GAIN)
    return m, d


def _eager_d_out(m, d, pts_ng, cls_ng):
    with torch.no_grad():
        return d(F.log_softmax(m(pts_ng, cls_ng)[0], dim=1)).cpu().numpy()


def _cloud_batch(rng, B, N):
    pts, pts_ng = (_t(rng.uniform(-1, 1, (B, N, 3))) for _ in range(2))
    cls, cls_ng = (_t(np.eye(16, dtype=np.float32)[rng.integers(0, 16, B)][:, None, :]) for _ in range(2))
    return pts, cls, _t(rng.integers(0, 50, (B, N)), torch.int64), pts_ng, cls_ng


def test_step_vs_reference_g15():
    """Iterations 0 (semi=False) and 2 (semi=True) of the reference's
    run_training_seg_semi at lr 0, so both start from the seeded weights: the
    four losses within 1e-3, pseudo-labels and K exactly, D's gradients by
    assert_grad_close and the generator's by the relative L2 2e-3 of g8 / g14,
    against the reference's float64 run."""
    from adversarial_learning_on_pointclouds_amd import PointNetSeg, PointwiseDiscNet, SegAdvTrainStep
    fx = load("g15_segsemi_step.npz")
    B, N = int(fx["B"]), int(fx["N"])
    Gp, Dp = make_weights()
    m, d = PointNetSeg(50), PointwiseDiscNet(N, 50)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Gp.items()})
    d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    m, d = m.to(DEV), d.to(DEV)
    lr = float(fx["lr"])
    assert lr == 0.0
    step = SegAdvTrainStep(m, d, torch.optim.Adam(m.parameters(), lr=lr),
                           torch.optim.Adam(d.parameters(), lr=lr),
                           lambda_seg=float(fx["lambda_seg"]), lambda_adv=float(fx["lambda_adv"]),
                           lambda_semi=float(fx["lambda_semi"]), semi_th=float(fx["semi_TH"]),
                           keep_activations=True)
    data = make_data()
    for it in (0, 2):
        dd = data[it]
        assert np.array_equal(dd["seg"], fx[f"it{it}.seg"])
        assert np.array_equal(dd["cls_ng"], fx[f"it{it}.cls_ng"])
        step(_t(dd["pts_gt"]), _t(dd["cls_gt"]), _t(dd["seg"], torch.int64), _t(dd["pts_ng"]),
             _t(dd["cls_ng"]), soft_gt=_t(dd["soft_gt"]), soft_nogt=_t(dd["soft_ng"]),
             semi=it > int(fx["semi_start"]))
        losses = step.losses_semi.cpu().numpy()
        ref = np.array([fx[k][it] for k in ("loss_seg", "loss_adv", "loss_semi", "loss_D")])
        print(f"iteration {it}: losses {losses.tolist()} reference {ref.tolist()}")
        assert np.max(np.abs(losses - ref)) <= 1e-3
        assert torch.equal(step.losses.cpu(), torch.from_numpy(losses[[0, 1, 3]]))
        if it == 2:
            assert int(step.kept.item()) == int(fx["K"])
            assert np.array_equal(step.semi_labels.cpu().numpy().reshape(B, N), fx["semi_gt"])
            d_ref = fx["it2.d_out_nogt"].reshape(-1)
            d_own = step.d_out[B * N:].cpu().numpy()
            print(f"D_out on the no-GT rows: max rel diff {np.max(np.abs(d_own - d_ref) / d_ref):.2e}")
        else:
            assert int(step.kept.item()) == 0 and step.semi_labels is None
        for name, p in d.named_parameters():
            e = assert_grad_close(p.grad.cpu().numpy(), fx[f"it{it}.gradD.{name}"], "D." + name)
            print(f"it{it} D.{name}: max-rel {e[0]:.2e} L2-rel {e[1]:.2e}")
        for name, p in m.named_parameters():
            e = check_tensor_l2(fx, f"it{it}.gradG.{name}", p.grad.cpu().numpy(), tol=2e-3)
            print(f"it{it} G.{name}: relative L2 {e:.2e}")
    for mod, ref in ((m, Gp), (d, Dp)):  # lr 0: not a bit moved
        for name, p in mod.named_parameters():
            assert np.array_equal(p.detach().cpu().numpy(), ref[name])


@pytest.mark.parametrize("B,N", [(2, 128), (3, 200)])
def test_step_vs_autograd_body(B, N, monkeypatch):
    """One semi=True step against the reference's body through autograd over the
    modules (torch CE / BCE, two torch Adams), the threshold in the widest gap
    of that run's own eager D_out."""
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep, trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    m, d = _gained(51 + N, 52 + N, N)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    rng = np.random.default_rng(N + 1)
    pts, cls, seg, pts_ng, cls_ng = _cloud_batch(rng, B, N)
    soft = [_t(rng.uniform(0.7, 1.05, (B, N))), _t(rng.uniform(0, 0.305, (B, N)))]
    d_out = _eager_d_out(m2, d2, pts_ng, cls_ng)
    th, gap = pick_threshold(d_out)
    print(f"D_out {d_out.min():.4f}..{d_out.max():.4f}, threshold {th:.5f} in a gap of {gap:.2e}")
    lam_seg, lam_adv, lam_semi, lr = 1.0, 0.7, 1000.0, 1e-3
    mk = lambda mod: torch.optim.Adam(mod.parameters(), lr=lr)  # noqa: E731
    step = SegAdvTrainStep(m, d, mk(m), mk(d), lambda_seg=lam_seg, lambda_adv=lam_adv,
                           lambda_semi=lam_semi, semi_th=th)
    p_old = [p.detach().clone() for mod in (m, d) for p in mod.parameters()]
    step(pts, cls, seg, pts_ng, cls_ng, soft_gt=soft[0], soft_nogt=soft[1], semi=True)
    losses = step.losses_semi.tolist()
    _replay_labels(monkeypatch, soft)
    args = argparse.Namespace(device=DEV, lambda_seg=lam_seg, lambda_adv=lam_adv,
                              lambda_semi=lam_semi, semi_TH=th)
    ref = trainer._seg_adv_body(m2, d2, mk(m2), mk(d2), torch.nn.BCEWithLogitsLoss(),
                                torch.nn.CrossEntropyLoss(), ImagePool(0), ImagePool(0), pts, cls,
                                seg, pts_ng, cls_ng, args,
                                semi_loss=torch.nn.CrossEntropyLoss(ignore_index=255), semi=True)
    K = int((d_out > th).sum())
    print("fused", losses, "autograd", ref, "kept", int(step.kept.item()), "of", B * N)
    assert int(step.kept.item()) == K and 0 < K < B * N
    assert ref[2] > 0 and np.max(np.abs(np.array(losses) - np.array(ref))) <= 1e-5
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, q, o in zip(names, ps, ps2, p_old):
        print(name, "max-rel %.2e L2-rel %.2e" % grad_err(p.grad.cpu().numpy(), q.grad.cpu().numpy()))
    for name, p, q, o in zip(names, ps, ps2, p_old):
        assert_grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), name)
        assert_adam_update_close(p.detach().cpu().numpy(), o.cpu().numpy(), q.detach().cpu().numpy(),
                                 o.cpu().numpy(), q.grad.cpu().numpy(), name)


def test_semi_needs_input_pts_equal_n():
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep
    B, N = 2, 128
    m, d, _, _ = _models(5, 6, 64)  # rows of 64 points: fine without the term
    step = SegAdvTrainStep(m, d, lr=1e-3, lr_D=1e-3)
    batch = _cloud_batch(np.random.default_rng(0), B, N)
    step(*batch)
    with pytest.raises(ValueError, match="input_pts"):
        step(*batch, semi=True)


def test_graph_replay_equals_eager_bitwise():
    """Three semi=True steps with device-drawn labels: one captured graph
    replayed against eager calls."""
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep
    B, N = 2, 128
    batch = _cloud_batch(np.random.default_rng(9), B, N)
    m, d = _gained(61, 62, N)
    th, _ = pick_threshold(_eager_d_out(m, d, batch[3], batch[4]))
    res = []
    for graph in (False, True):
        m, d = _gained(61, 62, N)
        # small steps: D's outputs (~35 here) move by their whole spread in one update at 1e-4
        step = SegAdvTrainStep(m, d, lr=1e-6, lr_D=1e-6, lambda_adv=0.5, lambda_semi=1000.0,
                               semi_th=th, seed=77)
        g = step.capture_on(*batch, semi=True) if graph else None
        ls, ks = [], []
        for _ in range(3):
            if graph:
                g.replay()
            else:
                step(*batch, semi=True)
            ls.append(step.losses_semi.clone())
            ks.append(step.kept.clone())
        torch.cuda.synchronize()
        res.append((torch.stack(ls), torch.stack(ks), step.param.clone(), step.d_param.clone(),
                    int(step.step_count.item()), int(step.step_count_D.item())))
    (la, ka, pa, da, sa, sda), (lb, kb, pb, db, sb, sdb) = res
    print("kept", ka.tolist(), "loss_semi", la[:, 2].tolist())
    assert sa == sb == 3 and sda == sdb == 3
    assert torch.equal(la, lb) and torch.equal(ka, kb) and torch.equal(pa, pb) and torch.equal(da, db)
    assert 0 < int(ka[0]) < B * N and bool((ka > 0).all()) and bool((la[:, 2] > 0).all())
    assert not torch.equal(la[0], la[1])  # the parameters move


def test_threshold_above_every_output_is_a_plain_step():
    """semi=True with nothing kept: parameters and `losses` bitwise those of a
    semi=False step, loss_semi 0 and K 0; and a semi=False step after a
    semi=True one reports 0 again."""
    from adversarial_learning_on_pointclouds_amd import SegAdvTrainStep
    B, N = 2, 128
    rng = np.random.default_rng(11)
    batch = _cloud_batch(rng, B, N)
    soft = dict(soft_gt=_t(rng.uniform(0.7, 1.05, (B, N))), soft_nogt=_t(rng.uniform(0, 0.305, (B, N))))
    res = []
    for semi in (False, True):
        m, d = _gained(71, 72, N)
        step = SegAdvTrainStep(m, d, lr=1e-3, lr_D=1e-3, lambda_adv=0.5, lambda_semi=1000.0,
                               semi_th=1e30)
        step(*batch, semi=semi, **soft)
        res.append((step.losses.clone(), step.losses_semi.clone(), int(step.kept.item()),
                    step.param.clone(), step.d_param.clone(), step.grad.clone()))
    (l0, ls0, k0, p0, d0, g0), (l1, ls1, k1, p1, d1, g1) = res
    assert torch.equal(l0, l1) and torch.equal(p0, p1) and torch.equal(d0, d1) and torch.equal(g0, g1)
    assert k0 == k1 == 0 and float(ls0[2]) == float(ls1[2]) == 0.0 and torch.equal(ls0, ls1)
    # the term on (everything kept), then off: loss_semi and K return to 0
    step.semi_th = -1.0
    step(*batch, semi=True, **soft)
    assert int(step.kept.item()) == B * N and float(step.losses_semi[2]) > 0
    step(*batch, semi=False, **soft)
    assert int(step.kept.item()) == 0 and float(step.losses_semi[2]) == 0.0


class _CountingCE(torch.nn.CrossEntropyLoss):
    """CrossEntropyLoss(ignore_index=255) by another type, counting its calls."""

    def __init__(self):
        super().__init__(ignore_index=255)
        self.calls = 0

    def forward(self, a, b):
        self.calls += 1
        return super().forward(a, b)


def _run_trainer(tmp_path, m, d, opt_cls, semi_loss, batches_gt, batches_ng, iters, th, tag):
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    exp = tmp_path / tag
    exp.mkdir()
    N = batches_gt[0][0].shape[1]
    # The lambdas keep their ratios of the step tests above, times 100: the generator's
    # gradients at lambda_seg 1 reach down to Adam's eps = 1e-8 (about 1e-6 is typical on
    # seeded weights, g14), where lr g / (|g| + eps) follows the gradient's rounding and
    # not its sign; Adam is otherwise scale-free and the logged losses are unscaled.
    args = argparse.Namespace(device=DEV, total_iterations=iters, lambda_seg=100.0, lambda_adv=50.0,
                              lambda_semi=1e5, semi_start=2, semi_TH=th,
                              iter_test_epoch=10 ** 9, exp_dir=str(exp), tensorboard=False,
                              input_pts=N, seed=21, native_eval=False)
    log = _Log()
    # the test pass: one cloud of every category, so the category mean IoU is a number
    rng = np.random.default_rng(1)
    test_batch = (torch.from_numpy(rng.uniform(-1, 1, (16, N, 3)).astype(np.float32)),
                  torch.from_numpy(np.eye(16, dtype=np.float32)[:, None, :]),
                  torch.from_numpy(rng.integers(0, 50, (16, N))))
    ret = trainer.run_training_seg_semi(
        batches_gt, batches_ng, enumerate(list(batches_gt)), enumerate(list(batches_ng)),
        [test_batch], [0] * 16, m, d, torch.nn.BCEWithLogitsLoss(),
        torch.nn.CrossEntropyLoss(), semi_loss, opt_cls(m.parameters(), lr=1e-4),
        opt_cls(d.parameters(), lr=1e-4), ImagePool(0), ImagePool(0), log,
        logging.getLogger("segsemi_test"), None, args)
    assert len(ret) == 3
    return log, exp


PAT = re.compile(r"^iter = +\d+/ +5 loss_seg = \d+\.\d{3} loss_adv = \d+\.\d{3} "
                 r"loss semi = \d+\.\d{3} loss_D = \d+\.\d{3}$")


def _values(lines):
    return np.array([[float(v) for v in re.findall(r"= (\d+\.\d{3})", s)] for s in lines])


def _trainer_threshold(m, d, ng, i):
    return pick_threshold(_eager_d_out(m, d, ng[i][0].to(DEV), ng[i][1].to(DEV)))[0]


def test_run_training_seg_semi_fused_vs_eager(tmp_path, monkeypatch):
    """Five iterations with semi_start = 2 over in-memory loaders: the log lines
    have the reference's format ('loss semi', no trailing space), iterations 0-2
    log 0.000 for the term, the checkpoints are the reference's (none by
    accuracy), and the parameters match the eager body's (run with the labels
    the fused step drew) within the Adam-update check.  Measured on an MI355X
    over the five updates: the generator at most 5.9e-4 (conv6.weight), D at
    most 7.5e-6."""
    N, B = 128, 2
    gt, ng = _batches(np.random.default_rng(13), [B] * 5, N)
    m, d = _gained(81, 82, N)
    # The threshold: D's outputs move by their whole spread within an update or
    # two at this lr, so it is placed in the widest gap of D's outputs on
    # iteration 3's batch AFTER iterations 0-2, from an eager run of those three
    # (no term yet) on copies, with the labels the fused run will draw.
    m3, d3 = copy.deepcopy(m), copy.deepcopy(d)
    q = _replay_labels(monkeypatch, _device_labels(21, range(3), B * N))
    _run_trainer(tmp_path, m3, d3, _PlainAdam, torch.nn.CrossEntropyLoss(ignore_index=255), gt, ng,
                 3, 1e30, "warmup")
    assert not q
    th = _trainer_threshold(m3, d3, ng, 3)
    m2, d2 = copy.deepcopy(m), copy.deepcopy(d)
    p0 = [p.detach().cpu().numpy().copy() for mod in (m, d) for p in mod.parameters()]
    log, exp = _run_trainer(tmp_path, m, d, torch.optim.Adam,
                            torch.nn.CrossEntropyLoss(ignore_index=255), gt, ng, 5, th, "fused")
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == 5 and all(PAT.match(s) for s in lines), lines
    vals = _values(lines)
    assert vals.shape == (5, 4) and np.all(vals[:3, 2] == 0.0)
    names = sorted(os.listdir(exp))
    assert names == sorted(f"{w}_train_{t}.pth" for w in ("model", "modelD")
                           for t in ("epoch_0", "best_cat_iou", "best_all_iou")), names
    assert not (exp / "model_train_best.pth").exists()
    q = _replay_labels(monkeypatch, _device_labels(21, range(5), B * N))
    counting = _CountingCE()
    log2, _ = _run_trainer(tmp_path, m2, d2, _PlainAdam, counting, gt, ng, 5, th, "eager")
    # iteration 3 keeps a part of its points; iteration 4 may keep any number, none included
    assert not q and 1 <= counting.calls <= 2
    lines2 = [s for s in log2.lines if s.startswith("iter")]
    print(lines, lines2, "threshold", th, "semi_loss calls", counting.calls)
    assert all(PAT.match(s) for s in lines2)
    assert np.max(np.abs(vals - _values(lines2))) <= 2e-3
    names = [f"{w}.{n}" for w, mod in (("G", m), ("D", d)) for n, _ in mod.named_parameters()]
    ps = [p for mod in (m, d) for p in mod.parameters()]
    ps2 = [p for mod in (m2, d2) for p in mod.parameters()]
    for name, p, r, o in zip(names, ps, ps2, p0):
        e, n = adam_update_err(p.detach().cpu().numpy(), o, r.detach().cpu().numpy(), o,
                               r.grad.cpu().numpy())
        print(f"{name}: Adam update rel err {e:.2e} over {n} elements")
    for name, p, r, o in zip(names, ps, ps2, p0):
        assert_adam_update_close(p.detach().cpu().numpy(), o, r.detach().cpu().numpy(), o,
                                 r.grad.cpu().numpy(), name)


def test_run_training_seg_semi_ragged_batch(tmp_path, monkeypatch):
    """A ragged batch in the middle (iteration 3, with the term on) goes through
    the eager body, and training continues on the fused path."""
    N = 128
    rng = np.random.default_rng(14)
    gt, _ = _batches(rng, [2, 2, 2, 1, 2], N)
    _, ng = _batches(rng, [2, 2, 2, 2, 2], N)
    m, d = _gained(83, 84, N)
    # threshold 0: every point with a positive D output is kept, wherever training moves them
    from adversarial_learning_on_pointclouds_amd import trainer
    body, eager = trainer._seg_adv_body, []
    monkeypatch.setattr(trainer, "_seg_adv_body",
                        lambda *a, **k: eager.append((a[8].shape[0], k["semi"])) or body(*a, **k))
    log, _ = _run_trainer(tmp_path, m, d, torch.optim.Adam,
                          torch.nn.CrossEntropyLoss(ignore_index=255), gt, ng, 5, 0.0, "ragged")
    assert eager == [(1, True)]  # the one-cloud GT batch of iteration 3, with the term on
    lines = [s for s in log.lines if s.startswith("iter")]
    assert len(lines) == 5 and all(PAT.match(s) for s in lines), lines
    vals = _values(lines)
    assert vals.shape == (5, 4) and np.all(np.isfinite(vals)) and np.all(vals[:3, 2] == 0.0)
    assert all(torch.isfinite(p).all() for p in list(m.parameters()) + list(d.parameters()))

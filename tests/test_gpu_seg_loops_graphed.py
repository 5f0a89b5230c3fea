"""The seven adversarial segmentation loops (run_training_seg, _seg_semi,
_seg_stack, _seg_stack_semi, _seg_stack_regulization, _seg_stack_regulization_
semi, _seg_dual) fed by a (GT, no-GT) pair of ShapeNet DeviceCloudLoaders: each
full iteration is one HIP graph replay (trainer._SegPairIteration: the packed
gather, the fused step, the loss line into the device ring) and the run is
bitwise the eager loop's (args.use_graph = False: the same loaders iterated,
the step called eagerly).  The fixture split: 4 GT / 3 no-GT clouds, B = 2, 48
points, 7 iterations, the test pass stubbed out.  MI355X only."""
import argparse
import os

import numpy as np
import pytest
import torch

import adversarial_learning_on_pointclouds_amd as pc
from adversarial_learning_on_pointclouds_amd import dataset as D
from adversarial_learning_on_pointclouds_amd import trainer
from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool

pytestmark = pytest.mark.gpu
H5 = os.path.join(os.path.dirname(__file__), "golden", "h5")
DEV = "cuda"
N, B, ITERS = 48, 2, 7
GT_ROWS = np.array([0, 2, 5, 6])
LOOPS = ["seg", "seg_semi", "stack", "stack_semi", "regu", "regu_semi", "dual"]


def _list(tmp_path, names):
    p = tmp_path / "files.txt"
    if not p.exists():
        p.write_text("".join(os.path.join(H5, n) + "\n" for n in names))
    return str(p)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, s):
        self.lines.append(s)


def _xavier_zero_bias(*nets):
    """Seeded weights with zero biases: the stacked D's output starts inside
    [0, 1] (its logsumexp over 16 shape logits is then at least log 16 + the
    mean logit) and stays there for the few updates of a test."""
    with torch.no_grad():
        for net in nets:
            for name, p in net.named_parameters():
                if name.endswith("bias"):
                    p.zero_()
                elif p.dim() > 1:
                    torch.nn.init.xavier_uniform_(p)


def _loaders(tmp_path, drop_last, b_nogt=B):
    lst = _list(tmp_path, ["shapenet_latest.h5"])
    gt = D.DeviceCloudLoader(D.ShapeNetDatasetGT(GT_ROWS, lst, num_classes=16, num_pts=N), B,
                             shuffle=True, seed=1, drop_last=drop_last)
    ng = D.DeviceCloudLoader(D.ShapeNetDataset_noGT(GT_ROWS, lst, num_classes=16, num_pts=N),
                             b_nogt, shuffle=True, seed=2, drop_last=drop_last)
    assert (gt.n, ng.n) == (4, 3)
    return gt, ng


def _full_iterations(gt, ng, iters=ITERS):
    """How many of the iterations find both batches full (each loader wraps on
    its own)."""
    def sizes(ld):
        return [min(ld.B, ld.n - k * ld.B) for k in range(len(ld))]
    sg, sn = sizes(gt), sizes(ng)
    return sum(sg[i % len(sg)] == gt.B and sn[i % len(sn)] == ng.B for i in range(iters))


def _soft_labels_at_most_one(monkeypatch):
    """The autograd body's soft labels for BCELoss, at most 1 (drawn from the
    same generator in every run)."""
    orig = trainer.make_D_label

    def make(input, value, device, random=False):
        if random and value == 1:
            return torch.empty(input.shape, device=device).uniform_(0.7, 1.0)
        return orig(input=input, value=value, device=device, random=random)
    monkeypatch.setattr(trainer, "make_D_label", make)


def _stub_testing(monkeypatch, on_pass=None):
    passes = []

    def testing(dataloader, dataset, model, criterion, logger, test_iter, writer, args):
        passes.append(test_iter)
        if on_pass is not None:
            on_pass(len(passes))
        return 0.0, 0.0, 0.0, 0.0
    monkeypatch.setattr(trainer, "run_testing_seg", testing)
    monkeypatch.setattr(trainer, "run_testing_seg_regulization", testing)
    return passes


def _halve_lr(k, opt, Ds):
    if k == 1:
        opt.param_groups[0]["lr"] *= 0.5


def _run(tmp_path, monkeypatch, loop, use_graph, drop_last=True, iters=ITERS, on_pass=None,
         loaders=None, prepare=None, tag="", replays=None, **args_kw):
    """One run of `loop` from seeded models and loaders: (parameters of G and of
    every D, the optimizers' step counts, the loss lines, the replays' semi
    flags).  on_pass(k, G's optimizer, Ds) runs inside the k-th (stubbed) test
    pass; prepare(G, Ds, gt, ng) before the optimizers are built."""
    torch.manual_seed(0)
    exp = tmp_path / f"{loop}_{int(use_graph)}_{int(drop_last)}{tag}"
    exp.mkdir()
    gt, ng = loaders or _loaders(tmp_path, drop_last)
    stack, semi, regu = loop != "seg" and loop != "seg_semi" and loop != "dual", \
        loop.endswith("semi"), loop.startswith("regu")
    G = (pc.PointNetSeg_regulization(50) if regu else pc.PointNetSeg(50)).to(DEV)
    if loop == "dual":
        Ds = [pc.BaseDiscNet(N, 50, 256), pc.ShapeDiscNet(256, 16), pc.PointDiscNet(256, N)]
    else:
        Ds = [pc.StackDiscNet(N, 50, 16) if stack else pc.PointwiseDiscNet(N, 50)]
    Ds = [d.to(DEV) for d in Ds]
    _xavier_zero_bias(*Ds)
    if prepare is not None:
        prepare(G, Ds, gt, ng)
    opt = torch.optim.Adam(G.parameters(), lr=1e-3)
    if loop == "dual":
        S, H, P = Ds
        opts = [opt, torch.optim.SGD(list(H.parameters()) + list(S.parameters()), lr=1e-3),
                torch.optim.SGD(list(P.parameters()) + list(S.parameters()), lr=2e-3)]
    else:
        opts = [opt, torch.optim.Adam(Ds[0].parameters(), lr=1e-3)]
    args = argparse.Namespace(device=DEV, total_iterations=iters, lambda_seg=1.0, lambda_adv=0.5,
                              lambda_disc_shape=0.5, lambda_regu=0.001, lambda_semi=1.0,
                              semi_start=2, semi_TH=-1e9, iter_test_epoch=4, exp_dir=str(exp),
                              tensorboard=False, input_pts=N, seed=21, use_graph=use_graph)
    vars(args).update(args_kw)
    _soft_labels_at_most_one(monkeypatch)
    _stub_testing(monkeypatch, None if on_pass is None else (lambda k: on_pass(k, opt, Ds)))
    replays = [] if replays is None else replays
    orig = getattr(trainer, "_SegPairIteration", None)
    if orig is not None:
        replay0 = orig.replay

        def spy(self, semi=False):
            replays.append(bool(semi))
            return replay0(self, semi)
        monkeypatch.setattr(orig, "replay", spy)
    log = _Log()
    ce, ce255 = torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss(ignore_index=255)
    head = (gt, ng, enumerate(gt), enumerate(ng), [None], [0] * B, G)
    tail = (ImagePool(0), ImagePool(0), log, log, None, args)
    bce, bcel = torch.nn.BCELoss(), torch.nn.BCEWithLogitsLoss()
    try:
        if loop == "dual":
            trainer.run_training_seg_dual(*head, *Ds, bcel, ce, ce, *opts, *tail)
        elif loop == "seg":
            trainer.run_training_seg(*head, Ds[0], bcel, ce, *opts, *tail)
        elif loop == "seg_semi":
            trainer.run_training_seg_semi(*head, Ds[0], bcel, ce, ce255, *opts, *tail)
        elif loop == "stack":
            trainer.run_training_seg_stack(*head, Ds[0], bce, ce, ce, *opts, *tail)
        elif loop == "stack_semi":
            trainer.run_training_seg_stack_semi(*head, Ds[0], bce, ce, ce255, ce, *opts, *tail)
        elif loop == "regu":
            trainer.run_training_seg_stack_regulization(*head, Ds[0], bce, ce, torch.nn.MSELoss(),
                                                        ce, *opts, *tail)
        else:
            trainer.run_training_seg_stack_regulization_semi(
                *head, Ds[0], bce, ce, torch.nn.MSELoss(), ce255, ce, *opts, *tail)
    finally:
        if orig is not None:
            monkeypatch.setattr(orig, "replay", replay0)
    params = [torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()
              for net in [G] + Ds]
    steps = [sorted(float(st["step"]) for st in o.state.values() if "step" in st) for o in opts]
    return params, steps, [s for s in log.lines if s.startswith("iter")], replays


def _assert_same_run(a, b, iters=ITERS):
    pa, sa, la, _ = a
    pb, sb, lb, _ = b
    for k, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), \
            f"net {k}: max |diff| {(x - y).abs().max().item():.3e}"
    assert sa == sb and sa[0] and all(t == iters for t in sa[0])
    print("\n".join(la))
    assert la == lb and len(la) == iters
    assert [int(s.split("/")[0].split("=")[1]) for s in la] == list(range(iters))


@pytest.mark.parametrize("drop_last", [True, False], ids=["drop_last", "ragged"])
@pytest.mark.parametrize("loop", LOOPS)
def test_graphed_loop_equals_eager(tmp_path, monkeypatch, loop, drop_last):
    """Full iterations are graph replays (none with use_graph=False); the
    parameters of G and of every D are bitwise the eager run's, the optimizers'
    step counts and the loss lines equal, one line per iteration in order.
    With drop_last=False the no-GT loader's second batch is ragged: iterations
    1, 3, 5 run the autograd body between the replays.  The semi loops replay
    both graphs (semi_start = 2: without the term up to iteration 2, with it
    after) and, with semi_TH far below every D output, log a non-zero
    loss_semi."""
    a = _run(tmp_path, monkeypatch, loop, True, drop_last)
    b = _run(tmp_path, monkeypatch, loop, False, drop_last)
    full = _full_iterations(*_loaders(tmp_path, drop_last))
    assert full == (ITERS if drop_last else 4)
    assert len(a[3]) == full and len(b[3]) == 0
    _assert_same_run(a, b)
    if loop.endswith("semi"):
        assert set(a[3]) == {False, True}
        key = "loss semi = " if loop == "seg_semi" else "loss_semi = "
        semi = [float(s.split(key)[1].split()[0]) for s in a[2]]
        assert all(v == 0.0 for v in semi[:3]) and all(v > 0.0 for v in semi[3:]), semi


@pytest.mark.parametrize("loop", ["seg", "stack_semi", "dual"])
def test_lr_change_recaptures(tmp_path, monkeypatch, loop):
    """The generator's lr halved at the first test pass (after iteration 0):
    the graphs are dropped and recaptured with the new value, and the run still
    equals the eager one, which re-reads the optimizers every iteration."""
    captures = []
    cap0 = trainer._SegPairIteration._capture

    def cap(self, semi):
        captures.append(bool(semi))
        return cap0(self, semi)
    monkeypatch.setattr(trainer._SegPairIteration, "_capture", cap)
    a = _run(tmp_path, monkeypatch, loop, True, on_pass=_halve_lr)
    ncap = len(captures)
    b = _run(tmp_path, monkeypatch, loop, False, on_pass=_halve_lr)
    assert len(captures) == ncap  # the eager run captures nothing
    # iteration 0's graph, then again after the change (and the semi graph later)
    assert captures[:2] == [False, False] and ncap == (3 if loop.endswith("semi") else 2)
    assert len(a[3]) == ITERS
    _assert_same_run(a, b)
    c = _run(tmp_path, monkeypatch, loop, True, tag="_const")
    assert not torch.equal(a[0][0], c[0][0])  # the change mattered


def test_stack_loop_raises_on_bad_rows(tmp_path, monkeypatch):
    """conv5's bias at -5: D's output is about 1.8, where BCELoss raises.  The
    graph-fed loop raises the same error when the ring is drained (here before
    the test pass that follows iteration 0), naming the iteration."""
    def prepare(G, Ds, gt, ng):
        with torch.no_grad():
            Ds[0].conv5.bias.fill_(-5.0)
    with pytest.raises(RuntimeError, match="all elements of input should be between 0 and 1.*"
                                           "iteration 0"):
        _run(tmp_path, monkeypatch, "stack", True, prepare=prepare)


def test_stack_loop_raises_late_but_within_half_a_ring(tmp_path, monkeypatch):
    """The one test pass (after iteration 0) sets the bias, so iteration 1 is
    the first bad one, and nothing drains the ring before the end of the 45
    iterations.  The stacked loops' ring waits for each half's copy where it is
    queued (every 32 iterations), so the error, naming iteration 1, is raised
    inside iteration 31: 30 iterations after the bad one, within the 32 the
    loop promises, and not at the final drain."""
    def on_pass(k, opt, Ds):
        with torch.no_grad():
            Ds[0].conv5.bias.fill_(-5.0)
    replays = []
    with pytest.raises(RuntimeError, match="between 0 and 1.*iteration 1"):
        _run(tmp_path, monkeypatch, "stack", True, iters=45, on_pass=on_pass, tag="_late",
             replays=replays, iter_test_epoch=10 ** 9)
    assert 2 <= len(replays) <= 1 + 32


def test_labels_outside_16_are_refused_before_any_capture(tmp_path, monkeypatch):
    captures = []
    monkeypatch.setattr(trainer._SegPairIteration, "_capture",
                        lambda self, semi: captures.append(semi))

    def prepare(G, Ds, gt, ng):
        ng.labels[1] = 16
    with pytest.raises(IndexError, match=r"\[0, 16\)"):
        _run(tmp_path, monkeypatch, "seg", True, prepare=prepare)
    assert not captures


def test_different_batch_sizes_fall_back(tmp_path, monkeypatch):
    """GT batches of 2, no-GT batches of 1: not the graph-fed path; the loop
    runs today's (the loaders iterated, the autograd body on unequal shapes)."""
    loaders = _loaders(tmp_path, True, b_nogt=1)
    _, steps, lines, replays = _run(tmp_path, monkeypatch, "seg", True, iters=3, loaders=loaders)
    assert replays == [] and len(lines) == 3 and steps[0] and all(t == 3 for t in steps[0])

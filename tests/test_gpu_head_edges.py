"""Teacher-forced edge-batch tests of the fused step's head and discriminator
tail (csrc/tail.hip and the fused-launch side of csrc/linear.hip: adv_head_part
and cls_step of csrc/capi.hip), through part 3 of pcadv_adv_step /
pcadv_cls_step on given pooled features.

Every array the step stores is read back through
pcadv_adv_step_workspace_layout and every link of the chain is held, element by
element, to its float64 restatement applied to the kernel's OWN stored inputs of
that link (tests/head_ref.py, which states the bounds; its checker is tested on
the CPU by tests/test_head_ref.py).  Each activation mask a backward link needs
is the sign of a stored activation, so the bounds are rigorous at every batch
size; the batch sizes (tests/head_cases.py) sit on the row-block, chain and
weight-gradient switches.  Gradients, workspace, logits and losses start as a
NaN sentinel: what the step should write it must have written, and part 3 must
leave the generator's conv1..conv4 gradients alone.

Each test prints its worst error / bound ratio per link (profiles/
head_edges_margins.txt collects them).  MI355X only."""
import ctypes

import numpy as np
import pytest
import torch

import head_cases as cases
import head_ref as ref
from oracle import pointnet_np as onp

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 16
SENT = 0x7FC0BEEF  # a quiet NaN no kernel produces
LOSS_TOL = 1e-6


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _fill(t):
    t.view(torch.int32).fill_(SENT)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def nets():
    import adversarial_learning_on_pointclouds_amd as pc
    G, D = cases.params()
    m, d = pc.PointNetCls(k=40), pc.DeepConvDiscNet(40, 1)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in D.items()})
    return m.to(DEV), d.to(DEV)


@pytest.fixture(scope="module")
def adv_step(nets):
    from adversarial_learning_on_pointclouds_amd.step import AdvTrainStep
    return AdvTrainStep(nets[0], nets[1], cases.MAX_B, N, seed=11)


@pytest.fixture(scope="module")
def cls_step(nets):
    import adversarial_learning_on_pointclouds_amd as pc
    from adversarial_learning_on_pointclouds_amd.step import ClsTrainStep
    G, _ = cases.params()
    m = pc.PointNetCls(k=40)  # its own module: a step binds its model's parameters
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    return ClsTrainStep(m.to(DEV), cases.MAX_B, N, seed=11)


def _workspace_arrays(step, B, rows):
    """The step's stored arrays by name, through the layout accessor."""
    from adversarial_learning_on_pointclouds_amd import _lib
    lay = _lib.StepWsLayout()
    _lib.check(step.lib.pcadv_adv_step_workspace_layout(B, N, ctypes.byref(lay)), "layout")
    assert lay.total == step.lib.pcadv_adv_step_workspace_bytes(B, N)
    ws = step.workspace[:lay.total].cpu().numpy()
    return {nm: np.frombuffer(ws, np.float32, int(np.prod(shape)), getattr(lay, nm)).reshape(shape)
            for nm, shape in rows.items()}


def _by_name(flat, layout, spec):
    flat = flat.cpu().numpy()
    return {k: flat[layout[k]:layout[k] + int(np.prod(s))].reshape(s) for k, s in spec
            if k in layout}


def _sentinels(step, A, flat_g, flat_d, nlosses):
    """Part 3 leaves conv1..conv4's gradients alone and writes everything else."""
    from adversarial_learning_on_pointclouds_amd._lib import D_NUMEL, G_LAYOUT, G_NUMEL
    fc1 = G_LAYOUT["fc1.weight"]
    g = _bits(flat_g.cpu().numpy())
    assert (g[:fc1] == SENT).all(), "part 3 wrote into the conv1..conv4 gradients"
    assert not (g[fc1:G_NUMEL] == SENT).any(), "a generator head gradient was not written"
    if flat_d is not None:
        assert not (_bits(flat_d.cpu().numpy())[:D_NUMEL] == SENT).any(), "a D gradient was not written"
    assert not (_bits(A["dgmax"]) == SENT).any(), "a feat_dgmax element was not written"
    assert not (_bits(A["losses"][:nlosses]) == SENT).any(), "a loss was not written"


def run_adv(step, B, inp, semi=False, semi_th=None, drawn=False, count=0):
    """One part-3 call of pcadv_adv_step as AdvFtTrainStep.__call__ drives it.
    Returns (A, gG, gD, hp)."""
    from adversarial_learning_on_pointclouds_amd._lib import D_LAYOUT, G_LAYOUT, check, stream_ptr
    C, R = 2 * B, 3 * B
    step.hp["semi_th"] = cases.HP["semi_th"] if semi_th is None else float(semi_th)
    step.step_count.fill_(count)
    pts = torch.zeros(B, N, 3, device=DEV)
    labels = _t(inp["labels"], torch.int64)
    masks = soft = None
    if not drawn:
        masks = (_t(inp["mask"][:B]), _t(inp["mask"][B:]))
        soft = (_t(inp["soft_gt"]), _t(inp["soft_nogt"]))
    a = step._args(pts, labels, pts, masks, soft, False, semi, part=3)
    a.gather, a.ngather = None, 0
    a.epi_counters, a.epi_ncounters, a.epi_ring = None, 0, None
    gmax = _t(inp["gmax"])
    dgmax = torch.empty(C, 1024, device=DEV)
    a.feat_gmax, a.feat_dgmax = gmax.data_ptr(), dgmax.data_ptr()
    for t in (step.grad_flat, step.workspace, dgmax, step.logits, step.losses):
        _fill(t)
    check(step.lib.pcadv_adv_step(ctypes.byref(a), stream_ptr()), "pcadv_adv_step (part 3)")
    torch.cuda.synchronize()
    A = _workspace_arrays(step, B, dict(
        h1=(C, 512), h2=(C, 256), dlogits=(C, 40), dh2=(C, 256), dh1=(C, 512), din=(R, 40),
        d1=(R, 512), d2=(R, 256), d3=(R, 256), dd3=(R, 256), dd2=(R, 256), dd1=(R, 512),
        z4=(C, 64), z5=(C, 64), a4=(C, 64), mask=(C, 256), dout=(R,)))
    A.update(gmax=inp["gmax"], labels=inp["labels"], dgmax=dgmax.cpu().numpy(),
             logits=step.logits[:C].cpu().numpy(), losses=step.losses.cpu().numpy())
    if not drawn:
        A.update(soft_gt=inp["soft_gt"], soft_nogt=inp["soft_nogt"])
        assert np.array_equal(A["mask"], inp["mask"])
    gG = _by_name(step.g_grad, G_LAYOUT, onp.cls_spec(40))
    gD = _by_name(step.d_grad, D_LAYOUT, onp.disc_spec(40, 1))
    _sentinels(step, A, step.g_grad, step.d_grad, 4)
    hp = dict(step.hp, B=B, semi=semi)
    return A, gG, gD, hp


def _report(rep, tag):
    for line in rep.lines(tag):
        print(line)
    assert not rep.failures(), (tag, rep.failures(), rep.notes)


@pytest.mark.parametrize("B", cases.ADV_B)
def test_adv_head_links(adv_step, B):
    """Every link of the adversarial step's head, explicit masks and soft
    labels, at the batch sizes of tests/head_cases.py."""
    G, D = cases.params()
    A, gG, gD, hp = run_adv(adv_step, B, cases.adv_inputs(B, adv_step.hp["p"]))
    _report(ref.check_adv_step(A, G, D, gG, gD, hp), f"adv B={B}")


@pytest.mark.parametrize("B", cases.SEMI_B)
@pytest.mark.parametrize("th", ["median", "above"])
def test_adv_head_links_semi(adv_step, B, th):
    """semi: the threshold at the median of the float64 reference's D logits of
    the no-GT rows, and one above all of them (nothing kept: losses[4] =
    losses[5] = 0 and no pseudo-label term in dlogits)."""
    G, D = cases.params()
    inp = cases.adv_inputs(B, adv_step.hp["p"])
    dref = ref.chain_adv_fwd(inp, G, D, dict(cases.HP, B=B, p=adv_step.hp["p"]))["dout"][2 * B:]
    semi_th = float(np.median(dref)) if th == "median" else float(dref.max()) + 1.0
    A, gG, gD, hp = run_adv(adv_step, B, inp, semi=True, semi_th=semi_th)
    assert not (_bits(A["losses"][4:6]) == SENT).any()
    kept = int((A["dout"][2 * B:] > np.float32(semi_th)).sum())
    if th == "above":
        assert kept == 0 and A["losses"][4] == 0 and A["losses"][5] == 0
    else:
        assert 0 < kept < B
    _report(ref.check_adv_step(A, G, D, gG, gD, hp), f"adv-semi-{th} B={B}")


@pytest.mark.parametrize("B", cases.DRAWN_B)
def test_adv_head_device_drawn(adv_step, B):
    """No masks or soft labels given: the stored mask is {0, 1} at the keep
    rate, a function of (seed, step count) alone; every link that does not need
    the drawn labels holds with that mask; the D losses lie between the BCE
    means at the ends of their label ranges (the BCE is monotone in the label)."""
    G, D = cases.params()
    p = adv_step.hp["p"]
    inp = cases.adv_inputs(B, p)
    A, gG, gD, hp = run_adv(adv_step, B, inp, drawn=True, count=3)
    mask = A["mask"].copy()
    assert np.isin(mask, (0.0, 1.0)).all()
    n = mask.size
    assert abs(mask.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)
    _report(ref.check_adv_step(A, G, D, gG, gD, hp, y_known=False), f"adv-drawn B={B}")
    dout = A["dout"].astype(np.float64)
    for k, rows, (lo, hi) in ((2, slice(0, B), (0.7, 1.05)), (3, slice(B, 2 * B), (0.0, 0.305))):
        ends = [0.5 * ref.bce(dout[rows], y).mean() for y in (lo, hi)]
        v = float(A["losses"][k])
        assert min(ends) - LOSS_TOL * max(1, abs(v)) <= v <= max(ends) + LOSS_TOL * max(1, abs(v))
    A2 = run_adv(adv_step, B, inp, drawn=True, count=3)[0]
    assert np.array_equal(_bits(A2["mask"]), _bits(mask))
    assert np.array_equal(_bits(A2["losses"][:4]), _bits(A["losses"][:4]))
    A3 = run_adv(adv_step, B, inp, drawn=True, count=4)[0]
    assert not np.array_equal(A3["mask"], mask)


def test_adv_head_two_ranks(adv_step):
    """rng_world = 2 at per-rank B = 3 on the two halves of a global batch of 6,
    all device-drawn, same seed and count: the ranks' stored masks are bitwise
    the global run's rows, the mean of their losses the global run's."""
    Bg, Br = 6, 3
    inp = cases.adv_inputs(Bg, adv_step.hp["p"])
    Ag = run_adv(adv_step, Bg, inp, drawn=True, count=5)[0]
    gmask, glosses = Ag["mask"].copy(), Ag["losses"][:4].astype(np.float64)
    losses = []
    try:
        for r in range(2):
            gt, ng = slice(r * Br, (r + 1) * Br), slice(Bg + r * Br, Bg + (r + 1) * Br)
            sub = dict(gmax=np.concatenate([inp["gmax"][gt], inp["gmax"][ng]]), labels=inp["labels"][gt])
            adv_step.set_rng_rank(r, 2)
            A = run_adv(adv_step, Br, sub, drawn=True, count=5)[0]
            assert np.array_equal(_bits(A["mask"]), _bits(np.concatenate([gmask[gt], gmask[ng]]))), r
            losses.append(A["losses"][:4].astype(np.float64))
    finally:
        adv_step.set_rng_rank(0, 1)
    mean = np.mean(losses, axis=0)
    assert (np.abs(mean - glosses) <= LOSS_TOL * np.maximum(1.0, np.abs(glosses))).all(), (mean, glosses)


@pytest.mark.parametrize("B", cases.CLS_B)
def test_cls_head_links(cls_step, B):
    """Every link of the cls step's head (k_cls_head, fc3's gradient and the CE
    mean riding in fc2's backward launch)."""
    from adversarial_learning_on_pointclouds_amd._lib import G_LAYOUT, check, stream_ptr
    step = cls_step
    G, _ = cases.params()
    inp = cases.cls_inputs(B, step.hp["p"])
    pts = torch.zeros(B, N, 3, device=DEV)
    labels, mask = _t(inp["labels"], torch.int64), _t(inp["mask"])  # alive through the call
    a = step._args(pts, labels, mask, False)
    a.part = 3
    a.gather, a.ngather = None, 0
    a.epi_counters, a.epi_ncounters, a.epi_ring = None, 0, None
    gmax = _t(inp["gmax"])
    dgmax = torch.empty(B, 1024, device=DEV)
    a.feat_gmax, a.feat_dgmax = gmax.data_ptr(), dgmax.data_ptr()
    for t in (step.g_grad, step.workspace, dgmax, step.logits, step.losses):
        _fill(t)
    check(step.lib.pcadv_cls_step(ctypes.byref(a), stream_ptr()), "pcadv_cls_step (part 3)")
    torch.cuda.synchronize()
    A = _workspace_arrays(step, B, dict(h1=(B, 512), h2=(B, 256), dlogits=(B, 40), dh2=(B, 256),
                                        dh1=(B, 512), mask=(B, 256), rowloss=(B,)))
    A.update(gmax=inp["gmax"], labels=inp["labels"], dgmax=dgmax.cpu().numpy(),
             logits=step.logits[:B].cpu().numpy(), losses=step.losses.cpu().numpy())
    assert np.array_equal(A["mask"], inp["mask"])
    _sentinels(step, A, step.g_grad, None, 1)
    gG = _by_name(step.g_grad, G_LAYOUT, onp.cls_spec(40))
    _report(ref.check_cls_step(A, G, gG, dict(step.hp, B=B)), f"cls B={B}")

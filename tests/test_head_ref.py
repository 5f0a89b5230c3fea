"""CPU checks of tests/head_ref.py, what tests/test_gpu_head_edges.py holds the
fused step's head and discriminator tail to: the float64 links chained end to
end against the oracle's float32 functions and against torch autograd in
float64, the checker on a float32 emulation of the chain (it passes) and on
five mutations of it (each is caught), and the either-branch cap on every
case's inputs."""
import numpy as np
import pytest
import torch

import head_cases as cases
import head_ref as ref
from oracle import pointnet_np as onp

P = 0.3  # PointNetCls's dropout
F32 = np.float32


def _hp(B, **kw):
    return dict(cases.HP, B=B, p=P, **kw)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _emulate_adv(B, semi=False, semi_th=None):
    """The chain in float32 numpy: the oracle's activations (head_fwd,
    log_softmax, disc_forward), then the losses and the backward in float32."""
    G, D = cases.params()
    hp = _hp(B, semi=semi)
    if semi_th is not None:
        hp["semi_th"] = semi_th
    inp = cases.adv_inputs(B, P)
    logits, (h1, h2, _) = onp.head_fwd(inp["gmax"], G, inp["mask"], P)
    lsm = onp.log_softmax(logits)
    din = np.concatenate([lsm, lsm[B:]])
    # the adversarial rows as copies of their twins: a BLAS product need not
    # repeat a row's sum bit for bit at another row, the kernels' tiles do
    out, acts = onp.disc_forward(D, din[:2 * B])
    out, *acts = [np.concatenate([a, a[B:]]) for a in [out] + acts]
    A = dict(inp, h1=h1, h2=h2, logits=logits, din=din, d1=acts[1], d2=acts[2], d3=acts[3],
             a4=acts[4], a5=acts[5], dout=out[:, 0])
    A, gG, gD = ref.chain_adv_bwd(A, G, D, hp, F32)
    return A, gG, gD, hp


@pytest.mark.parametrize("B", [3, 8])
def test_chain_matches_the_oracle(B):
    """The float64 chain against the oracle's float32 functions, 1e-5 of each
    array's largest entry: head_fwd, log_softmax, disc_forward, the CE and BCE
    values, disc_backward on both of D's passes and adv_step's loss algebra."""
    G, D = cases.params()
    hp = _hp(B)
    inp = cases.adv_inputs(B, P)
    A, gG, gD = ref.chain_adv_bwd(ref.chain_adv_fwd(inp, G, D, hp), G, D, hp)
    logits, (h1, h2, scale) = onp.head_fwd(inp["gmax"], G, inp["mask"], P)
    lsm = onp.log_softmax(logits)
    d_gt, acts_gt = onp.disc_forward(D, lsm[:B])
    d_ng, acts_ng = onp.disc_forward(D, lsm[B:])
    for nm, o in (("h1", h1), ("h2", h2), ("logits", logits)):
        assert _rel(A[nm], o) < 1e-5, nm
    assert _rel(A["dout"], np.concatenate([d_gt, d_ng, d_ng])[:, 0]) < 1e-5
    l_ce, dce = onp.cross_entropy(logits[:B], inp["labels"])
    l_adv, dadv = onp.bce_with_logits(d_ng, np.ones_like(d_ng))
    lD1, d1 = onp.bce_with_logits(d_gt, inp["soft_gt"][:, None])
    lD2, d2 = onp.bce_with_logits(d_ng, inp["soft_nogt"][:, None])
    assert np.allclose(A["losses"][:4], [l_ce, l_adv, 0.5 * lD1, 0.5 * lD2], rtol=1e-5, atol=0)
    g1, _ = onp.disc_backward(D, acts_gt, F32(0.5) * d1, need_input=False)
    g2, _ = onp.disc_backward(D, acts_ng, F32(0.5) * d2, need_input=False)
    for k in D:
        assert _rel(gD[k], g1[k] + g2[k]) < 1e-5, k
    _, dlsm = onp.disc_backward(D, acts_ng, F32(hp["lambda_adv"]) * dadv, need_params=False)
    dlog = np.concatenate([F32(hp["lambda_cls"]) * dce, onp.log_softmax_bwd(lsm[B:], dlsm)])
    assert _rel(A["dlogits"], dlog) < 1e-5
    cache = dict(pts=np.zeros((2 * B, 1, 3), F32), x1=np.zeros((2 * B, 1, 64), F32),
                 x2=np.zeros((2 * B, 1, 64), F32), x3=np.zeros((2 * B, 1, 128), F32),
                 gmax=inp["gmax"], am=np.zeros((2 * B, 1024), np.int64), head=(h1, h2, scale))
    og = onp.cls_backward(G, cache, dlog)
    for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"):
        assert _rel(gG[k], og[k]) < 1e-5, k
    assert _rel(A["dgmax"], og["_dglobal"]) < 1e-5


@pytest.mark.parametrize("semi", [False, True])
def test_chain_matches_autograd_f64(semi):
    """The float64 chain against torch autograd in float64, 1e-10 relative."""
    B = 6
    G, D = cases.params()
    inp = cases.adv_inputs(B, P)
    hp = _hp(B, semi=semi)
    fwd = ref.chain_adv_fwd(inp, G, D, hp)
    hp["semi_th"] = float(np.median(fwd["dout"][2 * B:]))
    A, gG, gD = ref.chain_adv_bwd(fwd, G, D, hp)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    Gt = {k: t(v).reshape(v.shape[0], -1).requires_grad_() if v.ndim > 1 else t(v).requires_grad_()
          for k, v in G.items() if k.startswith("fc")}
    Dt = {k: t(v).reshape(v.shape[0], -1).requires_grad_() if v.ndim > 1 else t(v).requires_grad_()
          for k, v in D.items()}
    gmax = t(inp["gmax"]).requires_grad_()
    kp = ref.keep_of(P)
    h1 = torch.relu(gmax @ Gt["fc1.weight"].T + Gt["fc1.bias"])
    h2 = torch.relu((h1 @ Gt["fc2.weight"].T + Gt["fc2.bias"]) * (t(inp["mask"]) * kp))
    logits = h2 @ Gt["fc3.weight"].T + Gt["fc3.bias"]
    lsm = torch.log_softmax(logits, 1)

    def disc(x):
        for i in range(1, 6):
            x = torch.nn.functional.leaky_relu(x @ Dt[f"conv{i}.weight"].T + Dt[f"conv{i}.bias"], 0.2)
        return x @ Dt["fc.weight"].T + Dt["fc.bias"]
    bcel = torch.nn.functional.binary_cross_entropy_with_logits
    y = torch.tensor(inp["labels"])
    d_adv = disc(lsm[B:])
    l_ce = torch.nn.functional.cross_entropy(logits[:B], y)
    l_adv = bcel(d_adv, torch.ones_like(d_adv))
    loss_g = hp["lambda_cls"] * l_ce + hp["lambda_adv"] * l_adv
    want = [l_ce.item(), l_adv.item()]
    if semi:
        keep = d_adv[:, 0].detach() > hp["semi_th"]
        assert 0 < int(keep.sum()) < B
        tgt = torch.where(keep, logits[B:].argmax(1), torch.full((B,), 255))
        l_semi = torch.nn.functional.cross_entropy(logits[B:], tgt, ignore_index=255)
        loss_g = loss_g + hp["lambda_semi"] * l_semi
    gnames = list(Gt)
    gg = torch.autograd.grad(loss_g, [Gt[k] for k in gnames] + [gmax], retain_graph=True)
    d_gt, d_ng = disc(lsm[:B].detach()), disc(lsm[B:].detach())
    lD1, lD2 = 0.5 * bcel(d_gt, t(inp["soft_gt"])[:, None]), 0.5 * bcel(d_ng, t(inp["soft_nogt"])[:, None])
    dnames = list(Dt)
    dg = torch.autograd.grad(lD1 + lD2, [Dt[k] for k in dnames])
    want += [lD1.item(), lD2.item()]
    assert np.allclose(A["losses"][:4], want, rtol=1e-10, atol=0)
    if semi:
        assert abs(A["losses"][4] - l_semi.item()) < 1e-10 * l_semi.item()
        assert A["losses"][5] == F32(int(keep.sum())) / F32(B)
    for k, g in zip(gnames, gg):
        assert _rel(gG[k], g.numpy().reshape(gG[k].shape)) < 1e-10, k
    assert _rel(A["dgmax"], gg[-1].numpy()) < 1e-10
    for k, g in zip(dnames, dg):
        assert _rel(np.asarray(gD[k]).reshape(g.shape), g.numpy()) < 1e-10, k


def test_cls_chain_matches_autograd_f64():
    B = 5
    G, _ = cases.params()
    inp = cases.cls_inputs(B, P)
    hp = _hp(B, lambda_cls=0.7)
    A, gG = ref.chain_cls(inp, G, hp)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    Gt = {k: t(v).requires_grad_() for k, v in G.items() if k.startswith("fc")}
    gmax = t(inp["gmax"]).requires_grad_()
    h1 = torch.relu(gmax @ Gt["fc1.weight"].T + Gt["fc1.bias"])
    h2 = torch.relu((h1 @ Gt["fc2.weight"].T + Gt["fc2.bias"]) * (t(inp["mask"]) * ref.keep_of(P)))
    ce = torch.nn.functional.cross_entropy(h2 @ Gt["fc3.weight"].T + Gt["fc3.bias"],
                                           torch.tensor(inp["labels"]))
    names = list(Gt)
    gg = torch.autograd.grad(0.7 * ce, [Gt[k] for k in names] + [gmax])
    assert abs(A["losses"][0] - ce.item()) < 1e-10 * ce.item()
    for k, g in zip(names, gg):
        assert _rel(gG[k], g.numpy()) < 1e-10, k
    assert _rel(A["dgmax"], gg[-1].numpy()) < 1e-10


# ---- the checker on itself ---------------------------------------------------

@pytest.mark.parametrize("B,semi", [(3, False), (8, False), (33, False), (6, True)])
def test_checker_passes_the_f32_emulation(B, semi):
    G, D = cases.params()
    th = None
    if semi:
        th = float(np.median(ref.chain_adv_fwd(cases.adv_inputs(B, P), G, D, _hp(B))["dout"][2 * B:]))
    A, gG, gD, hp = _emulate_adv(B, semi, th)
    rep = ref.check_adv_step(A, G, D, gG, gD, hp)
    assert not rep.failures(), rep.failures()
    assert len(rep.ratio) > 40


def test_checker_passes_the_f32_cls_emulation():
    G, _ = cases.params()
    for B in (1, 17):
        hp = _hp(B)
        A, gG = ref.chain_cls(cases.cls_inputs(B, P), G, hp, F32)
        rep = ref.check_cls_step(A, G, gG, hp)
        assert not rep.failures(), rep.failures()


def _mut_dd2_row(A, gG, gD, B):
    A["dd2"] = A["dd2"].copy()
    A["dd2"][2 * B + 1] = 0
    return "dd2"


def _mut_d1_shift(A, gG, gD, B):
    A["d1"] = A["d1"].copy()
    A["d1"][2 * B:] = np.roll(A["d1"][2 * B:], 1, axis=0)
    return "dup.d1"


def _mut_dh2_keep(A, gG, gD, B):
    A["dh2"] = A["dh2"].copy()
    A["dh2"][:, 32:48] /= F32(ref.keep_of(P))
    return "dh2"


def _mut_fc3_extra_row(A, gG, gD, B):
    # one 16 x 16 tile of fc3's weight gradient with row 0's term added twice
    gG["fc3.weight"] = gG["fc3.weight"].copy()
    gG["fc3.weight"][16:32, 64:80] += np.outer(A["dlogits"][0, 16:32], A["h2"][0, 64:80])
    return "g.fc3.weight"


def _mut_z5_slope(A, gG, gD, B):
    G, D = cases.params()
    _, _, pre, epre = ref.a5_of(A["a4"], D)
    A["z5"] = A["z5"].copy()
    r, c = np.unravel_index(np.argmax(np.where(np.abs(A["z5"]) > 0, pre - epre, -np.inf)), pre.shape)
    assert pre[r, c] > 100 * epre[r, c]
    A["z5"][r, c] *= F32(0.2)
    return "z5"


@pytest.mark.parametrize("mutate", [_mut_dd2_row, _mut_d1_shift, _mut_dh2_keep, _mut_fc3_extra_row,
                                    _mut_z5_slope])
def test_checker_catches(mutate):
    B = 8
    G, D = cases.params()
    A, gG, gD, hp = _emulate_adv(B)
    link = mutate(A, gG, gD, B)
    bad = ref.check_adv_step(A, G, D, gG, gD, hp).failures()
    assert link in bad, (link, bad)


# ---- the either-branch cap -----------------------------------------------------

@pytest.mark.parametrize("B", cases.ADV_B)
def test_either_branch_cap(B):
    """At most 2 % of a case's z5 units may have a conv5 pre-activation within
    its own bound of zero, in the float64 reference alone."""
    G, D = cases.params()
    fwd = ref.chain_adv_fwd(cases.adv_inputs(B, P), G, D, _hp(B))
    share = ref.either_branch(fwd["a4"][:2 * B].astype(F32), D).mean()
    assert share <= ref.EITHER_CAP, share

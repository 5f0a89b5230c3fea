"""The fused PointwiseDiscNet kernels (csrc/pwdisc.hip) against the numpy f64
restatement tests/pwdisc_ref.py: forward, argmax channel, BCE terms, backward
(weight, bias and input gradients), dead rows, ties, repeatability, labels."""
import functools

import numpy as np
import pytest
import torch

import pwdisc_ref as ref
from golden_util import assert_grad_close, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0

# (GT rows, no-GT rows, ncls, row stride, max workgroups): one row, a tile less
# one + one, two full tiles, a ragged tile that straddles the ranges, several
# tiles per persistent workgroup (16 tiles on 3 workgroups), narrow inputs, a
# padded row stride
SHAPES = [(1, 0, 50, 50, 0), (0, 1, 50, 50, 0), (63, 1, 50, 50, 0), (64, 64, 50, 50, 0),
          (65, 200, 50, 50, 0), (300, 700, 50, 50, 3), (65, 200, 16, 16, 0), (65, 200, 3, 3, 0),
          (65, 200, 50, 56, 2)]


def _xavier(rng, o, k):
    return (rng.standard_normal((o, k, 1)) * np.sqrt(2.0 / (o + k))).astype(np.float32)


def make_params(rng, ncls, bias_std=0.0):
    """init_type "xavier" of the reference (utils/model_utils.py:27-58)."""
    p = []
    for o, k in ((64, ncls), (64, 64), (64, 64), (128, 64)):
        p += [_xavier(rng, o, k), (rng.standard_normal(o) * bias_std).astype(np.float32)]
    return p


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _logits_buf(lg, ld):
    buf = torch.full((lg.shape[0], ld), SENTINEL, device=DEV)
    buf[:, :lg.shape[1]] = _t(lg)
    return buf


def run_kernels(lg, params, n0, n1, t0, t1, ld, maxwg, soft0=None, soft1=None, lambda_adv=0.37,
                dout_d=None, dout_adv=None, seed=0, step=None):
    """Forward (+ losses) and backward on the device; numpy results."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    M, ncls = n0 + n1, lg.shape[1]
    buf = _logits_buf(lg, ld)
    ps = [_t(p) for p in params]
    out = torch.empty(M, device=DEV)
    argc = torch.empty(M, device=DEV, dtype=torch.int32)
    ws = D.pwdisc_workspace(M, DEV, maxwg)
    losses = torch.zeros(4, device=DEV)
    dd = torch.zeros(M, device=DEV)
    da = torch.zeros(n1, device=DEV)
    so = torch.zeros(M, device=DEV)
    D.pwdisc_forward(buf, ncls, n0, n1, t0, t1, ps, out, argc, ws, losses=losses,
                     soft0=None if soft0 is None else _t(soft0),
                     soft1=None if soft1 is None else _t(soft1), soft_out=so, seed=seed,
                     step_count=step, dout_d=dd, dout_adv=da, max_workgroups=maxwg)
    if dout_d is not None:
        dd = _t(dout_d)
    if dout_adv is not None:
        da = _t(dout_adv)
    grads = [torch.full_like(p, SENTINEL) for p in ps]
    dl = torch.full((M, ld), SENTINEL, device=DEV)
    xs = torch.full((3, M, 64), SENTINEL, device=DEV)
    D.pwdisc_backward(buf, ncls, n0, n1, t0, t1, ps, out, argc, ws, dd, grads, dout_adv=da,
                      lambda_adv=lambda_adv, dlogits=dl, max_workgroups=maxwg, x_out=xs)
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0  # the ticket is left zero
    return dict(out=out.cpu().numpy(), argc=argc.cpu().numpy().astype(np.int64),
                losses=losses.cpu().numpy(), dout_d=dd.cpu().numpy(), dout_adv=da.cpu().numpy(),
                soft=so.cpu().numpy(), grads=[g.cpu().numpy() for g in grads],
                dlogits=dl.cpu().numpy(), xs=xs.cpu().numpy())


@functools.lru_cache(maxsize=None)
def case(shape):
    """One shape's inputs, device results and f64 forward, shared by the tests."""
    n0, n1, ncls, ld, maxwg = shape
    rng = np.random.default_rng(1000 + 7 * n0 + n1 + 31 * ncls + ld)
    lg = (2.0 * rng.standard_normal((n0 + n1, ncls))).astype(np.float32)
    params = make_params(rng, ncls)
    soft0 = rng.uniform(0.7, 1.05, n0).astype(np.float32)
    soft1 = rng.uniform(0.0, 0.305, n1).astype(np.float32)
    lam = 0.37
    k = run_kernels(lg, params, n0, n1, ref.SOFTMAX, ref.LOG_SOFTMAX, ld, maxwg, soft0, soft1, lam)
    x0 = np.concatenate([ref.transform(lg[:n0], ref.SOFTMAX), ref.transform(lg[n0:], ref.LOG_SOFTMAX)])
    out, argc, acts, y4 = ref.forward(x0, params)
    return dict(lg=lg, params=params, soft0=soft0, soft1=soft1, lam=lam, k=k, x0=x0, out=out,
                argc=argc, y4=y4, acts=acts)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_vs_f64(shape):
    c = case(shape)
    k = c["k"]
    e = rel_err(k["out"], c["out"])
    assert e <= 1e-5, e
    gap = ref.top2_gap(c["y4"])
    dead = c["out"] <= 0
    sel = (gap >= 1e-5) | dead
    print(f"shape {shape}: out rel err {e:.2e}, rows left out {int((~sel).sum())} of {len(sel)}, "
          f"smallest gap {gap.min():.2e}")
    assert (~sel).mean() <= 0.005
    assert np.array_equal(k["argc"][sel], c["argc"][sel])


@pytest.mark.parametrize("shape", SHAPES)
def test_losses_explicit_labels(shape):
    """The three BCE terms and their derivatives, on the kernel's own outputs."""
    c = case(shape)
    k = c["k"]
    n0, n1 = shape[:2]
    adv, ld_, dd, da = ref.losses(k["out"], n0, n1, c["soft0"], c["soft1"])
    assert abs(k["losses"][0] - adv) <= 1e-6, (k["losses"], adv)
    assert abs(k["losses"][1] - ld_) <= 1e-6, (k["losses"], ld_)
    assert abs(k["losses"][1] - (np.float32(k["losses"][2]) + np.float32(k["losses"][3]))) <= 1e-7
    assert_grad_close(k["dout_d"], dd, "dout_d")
    if n1:
        assert_grad_close(k["dout_adv"], da, "dout_adv")
    assert np.array_equal(k["soft"], np.concatenate([c["soft0"], c["soft1"]]))


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_vs_f64_same_activations(shape):
    """Weight, bias and input gradients against the f64 backward on the kernel's
    own argmax channel, live flags and ReLU masks: the signs of the x1..x3 the
    backward recomputed, which it writes out for this test and which must
    themselves be the f64 activations within the forward's bound."""
    c = case(shape)
    k = c["k"]
    n0, n1, ncls, ld, _ = shape
    live = k["out"] > 0
    masks = [x > 0 for x in k["xs"]]
    for i, x in enumerate(k["xs"]):
        assert rel_err(x, c["acts"][i + 1]) <= 1e-5, f"recomputed x{i + 1}"
    flips = sum(int((m != (a > 0)).sum()) for m, a in zip(masks, c["acts"][1:]))
    print(f"shape {shape}: ReLU masks that differ from the f64 ones: {flips}")
    grads, _ = ref.backward(c["x0"], c["params"], k["dout_d"], argc=k["argc"], masks=masks, live=live)
    names = [f"conv{i // 2 + 1}.{'weight' if i % 2 == 0 else 'bias'}" for i in range(8)]
    for g, r, nm in zip(k["grads"], grads, names):
        assert_grad_close(g, r, nm)
    dl = k["dlogits"]
    assert np.all(dl[:n0] == SENTINEL)       # GT rows: not touched
    assert np.all(dl[:, ncls:] == SENTINEL)  # nor the padding of the row stride
    if n1:
        d = np.zeros(n0 + n1)
        d[n0:] = c["lam"] * k["dout_adv"].astype(np.float64)
        _, dx0 = ref.backward(c["x0"], c["params"], d, argc=k["argc"], masks=masks, live=live)
        dref = ref.transform_bwd(c["x0"][n0:], dx0[n0:], ref.LOG_SOFTMAX)
        assert_grad_close(dl[n0:, :ncls], dref, "dlogits")


def test_single_row_dout():
    """dout_adv non-zero on one row: only that row's input gradient is non-zero."""
    c = case((65, 200, 50, 50, 0))
    n0, n1 = 65, 200
    da = np.zeros(n1, np.float32)
    da[77] = 0.5
    k = run_kernels(c["lg"], c["params"], n0, n1, ref.SOFTMAX, ref.LOG_SOFTMAX, 50, 0, c["soft0"],
                    c["soft1"], lambda_adv=2.0, dout_adv=da)
    dl = k["dlogits"][n0:]
    assert k["out"][n0 + 77] > 0
    others = np.delete(dl, 77, axis=0)
    assert np.all(others == 0)
    d = np.zeros(n0 + n1)
    d[n0 + 77] = 1.0
    _, dx0 = ref.backward(c["x0"], c["params"], d, argc=k["argc"], masks=[x > 0 for x in k["xs"]],
                          live=k["out"] > 0)
    dref = ref.transform_bwd(c["x0"][n0:], dx0[n0:], ref.LOG_SOFTMAX)
    assert_grad_close(dl[77], dref[77], "dlogits row")


def test_exact_ties_first_index():
    rng = np.random.default_rng(5)
    n0, n1 = 100, 157
    lg = (2.0 * rng.standard_normal((n0 + n1, 50))).astype(np.float32)
    params = make_params(rng, 50)
    params[6][77] = params[6][5]
    params[7][77] = params[7][5] = 1.0  # a bias that lets the pair win on most rows
    k = run_kernels(lg, params, n0, n1, ref.SOFTMAX, ref.LOG_SOFTMAX, 50, 0,
                    np.full(n0, 0.9, np.float32), np.full(n1, 0.1, np.float32))
    print("rows won by the tied pair:", int((k["argc"] == 5).sum()), "of", n0 + n1)
    assert (k["argc"] == 5).sum() > (n0 + n1) // 4
    assert not (k["argc"] == 77).any()
    x0 = np.concatenate([ref.transform(lg[:n0], ref.SOFTMAX), ref.transform(lg[n0:], ref.LOG_SOFTMAX)])
    _, argc, _, y4 = ref.forward(x0, params)
    sel = ref.top2_gap(np.delete(y4, 77, axis=1)) >= 1e-5
    assert np.array_equal(k["argc"][sel], argc[sel])


def test_dead_rows_contribute_nothing():
    """conv4's bias at -100: rows with small inputs have every channel dead."""
    rng = np.random.default_rng(11)
    nl, nd = 100, 70
    live = (300.0 * rng.standard_normal((nl, 50))).astype(np.float32)
    dead = rng.standard_normal((nd, 50)).astype(np.float32)
    params = make_params(rng, 50)
    params[7][:] = -100.0
    dd = rng.standard_normal(nl + nd).astype(np.float32)
    da = rng.standard_normal(nl + nd).astype(np.float32)
    a = run_kernels(live, params, 0, nl, ref.NONE, ref.NONE, 50, 0, None, np.zeros(nl, np.float32),
                    dout_d=dd[:nl], dout_adv=da[:nl])
    b = run_kernels(np.concatenate([live, dead]), params, 0, nl + nd, ref.NONE, ref.NONE, 50, 0,
                    None, np.zeros(nl + nd, np.float32), dout_d=dd, dout_adv=da)
    assert (a["out"] > 0).sum() > nl // 2
    assert np.all(b["out"][nl:] == 0) and np.all(b["argc"][nl:] == 0)
    assert np.array_equal(a["out"], b["out"][:nl])
    assert np.array_equal(a["dlogits"], b["dlogits"][:nl])  # bitwise
    assert np.all(b["dlogits"][nl:] == 0)
    for ga, gb, i in zip(a["grads"], b["grads"], range(8)):
        assert_grad_close(gb, ga, f"grad {i}")
    # every row dead: all gradients exactly zero
    z = run_kernels(dead, params, 0, nd, ref.NONE, ref.NONE, 50, 0, None, np.zeros(nd, np.float32),
                    dout_d=dd[:nd], dout_adv=da[:nd])
    assert np.all(z["out"] == 0) and np.all(z["argc"] == 0)
    assert all(np.all(g == 0) for g in z["grads"]) and np.all(z["dlogits"] == 0)


def test_repeatable_bitwise():
    c = case((300, 700, 50, 50, 3))
    k2 = run_kernels(c["lg"], c["params"], 300, 700, ref.SOFTMAX, ref.LOG_SOFTMAX, 50, 3,
                     c["soft0"], c["soft1"], c["lam"])
    k = c["k"]
    for name in ("out", "argc", "losses", "dout_d", "dout_adv", "dlogits"):
        assert np.array_equal(k[name], k2[name]), name
    for g, g2 in zip(k["grads"], k2["grads"]):
        assert np.array_equal(g, g2)


def test_device_drawn_labels():
    c = case((65, 200, 50, 50, 0))
    n0, n1 = 65, 200
    step = torch.tensor([3], device=DEV, dtype=torch.int32)
    draw = lambda: run_kernels(c["lg"], c["params"], n0, n1, ref.SOFTMAX, ref.LOG_SOFTMAX, 50, 0,  # noqa: E731
                               seed=99, step=step)
    a = draw()
    b = draw()
    step += 1
    d = draw()
    s0, s1 = a["soft"][:n0], a["soft"][n0:]
    assert np.all(s0 >= np.float32(0.7)) and np.all(s0.astype(np.float64) < 1.05)
    assert np.all(s1 >= 0) and np.all(s1.astype(np.float64) < 0.305)
    assert s0.std() > 0.05 and s1.std() > 0.05 and len(np.unique(a["soft"])) > 250
    assert np.array_equal(a["soft"], b["soft"]) and np.array_equal(a["losses"], b["losses"])
    assert not np.array_equal(a["soft"], d["soft"])
    adv, ld_, dd, _ = ref.losses(a["out"], n0, n1, s0, s1)
    assert abs(a["losses"][0] - adv) <= 1e-6 and abs(a["losses"][1] - ld_) <= 1e-6
    assert_grad_close(a["dout_d"], dd, "dout_d")


def test_module_autograd():
    """PointwiseDiscNet.forward over the kernels: values and gradients against
    the same layers in torch (f64), on a permuted view of point-major storage."""
    from adversarial_learning_on_pointclouds_amd import PointwiseDiscNet
    torch.manual_seed(3)
    B, N, C = 3, 200, 50
    m = PointwiseDiscNet(N, C).to(DEV)
    pm = (2 * torch.randn(B, N, C, device=DEV)).requires_grad_(True)
    out = m(torch.log_softmax(pm, dim=2).permute(0, 2, 1))
    assert out.shape == (B, N)
    w = torch.randn(B, N, device=DEV)
    (out * w).sum().backward()
    import copy
    m64 = copy.deepcopy(m).double()
    p64 = pm.detach().double().requires_grad_(True)
    h = torch.log_softmax(p64, dim=2).permute(0, 2, 1)
    for conv in (m64.conv1, m64.conv2, m64.conv3, m64.conv4):
        h = torch.relu(torch.nn.functional.conv1d(h, conv.weight, conv.bias))
    o64 = h.max(dim=1)[0]
    (o64 * w.double()).sum().backward()
    assert rel_err(out.detach().cpu().numpy(), o64.detach().cpu().numpy()) <= 1e-5
    assert_grad_close(pm.grad.cpu().numpy(), p64.grad.cpu().numpy(), "input")
    for (n, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()):
        assert_grad_close(p.grad.cpu().numpy(), q.grad.cpu().numpy(), n)


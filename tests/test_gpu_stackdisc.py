"""The fused StackDiscNet kernels (csrc/pwdisc.hip: k_stk_fwd and the LeakyReLU
backward) against the numpy f64 restatement tests/stackdisc_ref.py: forward,
arg-max channel, the BCE / shape terms with their derivatives and conv5's
gradients, the backward on the kernel's own masks, all-negative rows, ties, a
pre-activation of exactly 0, large shape logits, the BCE clamps, rows outside
[0, 1], repeatability, device-drawn labels."""
import functools

import numpy as np
import pytest
import torch

import stackdisc_cases as cases
import stackdisc_ref as ref
from golden_util import assert_grad_close, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0
NAMES = [f"conv{i // 2 + 1}.{'weight' if i % 2 == 0 else 'bias'}" for i in range(10)]


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def run_kernels(c, shape, lambda_adv=cases.LAMBDA_ADV, lam=cases.LAMBDA_SHAPE, drawn=None,
                params=None, ws=None):
    """Forward (+ losses) and backward on the device; numpy results.  drawn =
    (seed, step tensor): device-drawn labels instead of the case's."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    n0, n1, ncls, ld, maxwg, ppc = shape
    M = n0 + n1
    params = c["params"] if params is None else params
    S = params[9].size
    buf = torch.full((M, ld), SENTINEL, device=DEV)
    buf[:, :ncls] = _t(c["lg"])
    ps = [_t(p) for p in params]
    m, d_out = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    argc = torch.empty(M, device=DEV, dtype=torch.int32)
    sl = torch.empty(M, S, device=DEV)
    ws = D.stackdisc_workspace(M, DEV, maxwg) if ws is None else ws
    losses = torch.full((5,), SENTINEL, device=DEV)
    dd, da, so = torch.zeros(M, device=DEV), torch.zeros(n1, device=DEV), torch.zeros(M, device=DEV)
    bad = torch.full((1,), -7, device=DEV, dtype=torch.int32)
    grads = [torch.full_like(p, SENTINEL) for p in ps]
    soft = dict(soft0=_t(c["soft0"]), soft1=_t(c["soft1"])) if drawn is None else \
        dict(seed=drawn[0], step_count=drawn[1])
    t0, t1 = c.get("t0", ref.SOFTMAX), c.get("t1", ref.LOG_SOFTMAX)
    D.stackdisc_forward(buf, ncls, n0, n1, t0, t1, ps, m, argc, d_out, ws,
                        shape_logits=sl, losses=losses, shape_label=_t(c["labels"], torch.int32),
                        pts_per_cloud=ppc, lambda_disc_shape=lam, soft_out=so, dm_d=dd, dm_adv=da,
                        grads5=grads[8:10], bad_rows=bad, max_workgroups=maxwg, **soft)
    dl = torch.full((M, ld), SENTINEL, device=DEV)
    xs = torch.full((3, M, 64), SENTINEL, device=DEV)
    D.stackdisc_backward(buf, ncls, n0, n1, t0, t1, ps, m, argc, ws, dd,
                         grads, dm_adv=da, lambda_adv=lambda_adv, dlogits=dl, max_workgroups=maxwg,
                         x_out=xs)
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0  # the ticket is left zero
    return dict(m=m.cpu().numpy(), argc=argc.cpu().numpy().astype(np.int64),
                d_out=d_out.cpu().numpy(), S=sl.cpu().numpy(), losses=losses.cpu().numpy(),
                dm_d=dd.cpu().numpy(), dm_adv=da.cpu().numpy(), soft=so.cpu().numpy(),
                bad=int(bad.item()), grads=[g.cpu().numpy() for g in grads],
                dlogits=dl.cpu().numpy(), xs=xs.cpu().numpy())


@functools.lru_cache(maxsize=None)
def case(cs):
    """One case's inputs, device results and f64 forward, shared by the tests."""
    shape, S = cs
    c = cases.make_inputs(shape, S)
    c["k"] = run_kernels(c, shape)
    c["m"], c["argc"], c["acts"], c["y4"] = ref.forward(c["x0"], c["params"])
    return c


def check_forward(c, k, left_out_cap=0.005, what=""):
    S, _, d, _ = ref.head(c["m"], c["params"])
    for name, a, r in (("m", k["m"], c["m"]), ("S", k["S"], S), ("d_out", k["d_out"], d)):
        e = rel_err(a, r)
        assert e <= 1e-5, (what, name, e)
    gap = ref.top2_gap(c["y4"])
    sel = gap >= 1e-5
    assert (~sel).mean() <= left_out_cap
    assert np.array_equal(k["argc"][sel], c["argc"][sel])
    return sel


def check_losses(c, k, shape, lam=cases.LAMBDA_SHAPE, params=None, at_d_out=False,
                 relative=False):
    """The five terms, dm_d / dm_adv and conv5's gradients on the kernel's own m
    (at_d_out: and its own d_out, where a clamp makes a term discontinuous).
    The losses are held to the absolute 1e-6 of test_gpu_pwdisc.py.  relative:
    1e-6 of max(1, |value|) instead, for the cases whose terms are far above 1
    (an f32 ulp at 100 is 7.6e-6, so no f32 result can meet 1e-6 there)."""
    n0, n1, _, _, _, ppc = shape
    params = c["params"] if params is None else params
    r = ref.losses(k["m"], params, n0, n1, c["soft0"], c["soft1"], c["labels"], ppc, lam,
                   d_out=k["d_out"] if at_d_out else None)
    want = [r["loss_adv"], r["loss_D"], r["d_gt"], r["d_nogt"], r["loss_D_shape"]]
    print("losses", k["losses"].tolist(), "f64", want)
    for got, w in zip(k["losses"], want):
        assert abs(got - w) <= 1e-6 * (max(1.0, abs(w)) if relative else 1.0), (k["losses"], want)
    assert_grad_close(k["dm_d"], r["dm_d"], "dm_d")
    if n1:
        assert_grad_close(k["dm_adv"], r["dm_adv"], "dm_adv")
    assert_grad_close(k["grads"][8], r["dw5"], "conv5.weight")
    assert_grad_close(k["grads"][9], r["db5"], "conv5.bias")
    return r


def check_backward(c, k, shape, lambda_adv=cases.LAMBDA_ADV, params=None):
    """conv1..conv4's gradients and the no-GT dlogits against the f64 backward
    on the kernel's own arg-max channel and masks (the signs of the x1..x3 it
    recomputed and of m), those x themselves within the forward's bound."""
    n0, n1, ncls, ld, _, _ = shape
    params = c["params"] if params is None else params
    acts = ref.forward(c["x0"], params)[2]
    masks = [x > 0 for x in k["xs"]]
    for i, x in enumerate(k["xs"]):
        assert rel_err(x, acts[i + 1]) <= 1e-5, f"recomputed x{i + 1}"
    top = k["m"] > 0
    grads, _ = ref.backward(c["x0"], params, k["dm_d"], argc=k["argc"], masks=masks, top=top)
    for g, r, nm in zip(k["grads"][:8], grads, NAMES):
        assert_grad_close(g, r, nm)
    dl = k["dlogits"]
    assert np.all(dl[:n0] == SENTINEL)       # GT rows: not touched
    assert np.all(dl[:, ncls:] == SENTINEL)  # nor the padding of the row stride
    if n1:
        d = np.zeros(n0 + n1)
        d[n0:] = lambda_adv * k["dm_adv"].astype(np.float64)
        _, dx0 = ref.backward(c["x0"], params, d, argc=k["argc"], masks=masks, top=top)
        assert_grad_close(dl[n0:, :ncls],
                          ref.transform_bwd(c["x0"][n0:], dx0[n0:], c.get("t1", ref.LOG_SOFTMAX)),
                          "dlogits")
    return grads


@pytest.mark.parametrize("cs", cases.CASES)
def test_forward_vs_f64(cs):
    c = case(cs)
    sel = check_forward(c, c["k"])
    print(f"{cs}: rows left out {int((~sel).sum())} of {len(sel)}")
    assert c["k"]["bad"] == 0


@pytest.mark.parametrize("cs", cases.CASES)
def test_losses_and_derivatives(cs):
    """Labels up to 1.05 (one exactly), on the kernel's own m."""
    c = case(cs)
    check_losses(c, c["k"], cs[0])
    assert np.array_equal(c["k"]["soft"], np.concatenate([c["soft0"], c["soft1"]]))
    assert abs(c["k"]["losses"][1] - (np.float32(c["k"]["losses"][2]) + np.float32(c["k"]["losses"][3]))) <= 1e-7


@pytest.mark.parametrize("cs", cases.CASES)
def test_backward_vs_f64_same_activations(cs):
    c = case(cs)
    check_backward(c, c["k"], cs[0])


def test_device_drawn_labels_are_pwdiscs():
    """The labels drawn on the device are k_pwd_fwd's for the same seed, step and
    rows, bitwise, and the terms formed on them are the restatement's."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    cs = ((65, 200, 50, 50, 0, 13), 16)
    c = case(cs)
    n0, n1 = 65, 200
    step = torch.tensor([3], device=DEV, dtype=torch.int32)
    a = run_kernels(c, cs[0], drawn=(99, step))
    b = run_kernels(c, cs[0], drawn=(99, step))
    ps = [torch.zeros(s, device=DEV) for s in ((64, 50, 1), (64,), (64, 64, 1), (64,), (64, 64, 1),
                                               (64,), (128, 64, 1), (128,))]
    soft = torch.zeros(n0 + n1, device=DEV)
    D.pwdisc_forward(torch.zeros(n0 + n1, 50, device=DEV), 50, n0, n1, 1, 2, ps,
                     torch.empty(n0 + n1, device=DEV),
                     torch.empty(n0 + n1, device=DEV, dtype=torch.int32),
                     D.pwdisc_workspace(n0 + n1, DEV), losses=torch.zeros(4, device=DEV),
                     soft_out=soft, seed=99, dout_d=torch.empty(n0 + n1, device=DEV), step_count=step)
    assert np.array_equal(a["soft"], soft.cpu().numpy())
    assert np.array_equal(a["soft"], b["soft"]) and np.array_equal(a["losses"], b["losses"])
    step += 1
    d = run_kernels(c, cs[0], drawn=(99, step))
    assert not np.array_equal(a["soft"], d["soft"])
    s0, s1 = a["soft"][:n0], a["soft"][n0:]
    assert np.all(s0 >= np.float32(0.7)) and np.all(s0.astype(np.float64) < 1.05) and s0.max() > 1.0
    assert np.all(s1 >= 0) and np.all(s1.astype(np.float64) < 0.305)
    check_losses(dict(c, soft0=s0, soft1=s1), a, cs[0])


def test_all_negative_rows_are_scaled_not_dropped():
    """conv4's bias at -3 on every channel: every m < 0, and the gradients are
    0.2 times the unit chain's (the f64 backward with top = False), not zero.
    The rows enter D as they are here (no transform): log_softmax rows' inputs
    of -5 .. -10 drive some channels of conv4 above 3, and after a softmax the
    channels are so close that more rows than the arg-max rule allows tie."""
    shape = (65, 200, 50, 50, 0, 13)
    c = dict(cases.make_inputs(shape), t0=ref.NONE, t1=ref.NONE)
    c["x0"] = c["lg"].astype(np.float64)
    c["params"] = [p.copy() for p in c["params"]]
    c["params"][7][:] = -3.0
    k = run_kernels(c, shape)
    c["m"], c["argc"], _, c["y4"] = ref.forward(c["x0"], c["params"])
    assert np.all(k["m"] < 0) and np.all(c["m"] < 0)
    check_forward(c, k)
    check_losses(c, k, shape)
    check_backward(c, k, shape)
    assert all(np.abs(g).max() > 0 for g in k["grads"]) and np.abs(k["dlogits"][65:, :50]).max() > 0
    # against the chain without the arg-max channel's own mask: a factor 0.2
    full, _ = ref.backward(c["x0"], c["params"], k["dm_d"], argc=k["argc"],
                           masks=[x > 0 for x in k["xs"]], top=np.ones(265, bool))
    assert_grad_close(5.0 * k["grads"][6], full[6], "conv4.weight x 5")


def test_exact_ties_first_index():
    shape = (100, 157, 50, 50, 0, 10)
    c = dict(cases.make_inputs(shape))
    params = [p.copy() for p in c["params"]]
    params[6][77] = params[6][5]
    params[7][77] = params[7][5] = 1.0  # a bias that lets the pair win on most rows
    c["params"] = params
    k = run_kernels(c, shape)
    print("rows won by the tied pair:", int((k["argc"] == 5).sum()), "of", 257)
    assert (k["argc"] == 5).sum() > 257 // 4
    assert not (k["argc"] == 77).any()
    _, argc, _, y4 = ref.forward(c["x0"], params)
    sel = ref.top2_gap(np.delete(y4, 77, axis=1)) >= 1e-5
    assert np.array_equal(k["argc"][sel], argc[sel])


def test_zero_preactivation_takes_the_leaky_slope():
    """conv2's unit 9 with zero weights and bias: its pre-activation is exactly 0
    on every row, x2 is 0 there, and its mask is 0.2 (y > 0 ? 1 : 0.2), so its
    bias gradient is 0.2 of what a mask of 1 would give, not 0 and not 1."""
    shape = (65, 200, 50, 50, 0, 13)
    c = dict(cases.make_inputs(shape))
    params = [p.copy() for p in c["params"]]
    params[2][9] = 0.0
    params[3][9] = 0.0
    c["params"] = params
    k = run_kernels(c, shape)
    assert np.all(k["xs"][1][:, 9] == 0)
    check_backward(c, k, shape)
    masks = [x > 0 for x in k["xs"]]
    masks[1][:, 9] = True
    one, _ = ref.backward(c["x0"], params, k["dm_d"], argc=k["argc"], masks=masks, top=k["m"] > 0)
    assert abs(one[3][9]) > 0
    assert abs(k["grads"][3][9] / one[3][9] - 0.2) <= 1e-3


def test_large_shape_logits_stay_finite():
    """w5 x 64: |S| in the hundreds.  The logsumexp subtracts the row maximum, so
    everything stays finite and within the forward's bound; the terms are held
    on the kernel's own d_out (1 - d_out is a few 1e-3: its f32 rounding alone
    moves log(1 - d_out) by 1e-5)."""
    shape = (65, 200, 50, 50, 0, 13)
    c = dict(cases.make_inputs(shape))
    params = [p.copy() for p in c["params"]]
    params[8] = params[8] * 64.0
    # larger activations, so that w5 m reaches the hundreds
    params[6] = params[6] * 8.0
    c["params"] = params
    k = run_kernels(c, shape)
    c["m"], c["argc"], _, c["y4"] = ref.forward(c["x0"], params)
    print("largest |S|:", float(np.abs(k["S"]).max()))
    assert np.abs(k["S"]).max() > 100
    for name in ("m", "S", "d_out", "losses", "dm_d", "dm_adv"):
        assert np.all(np.isfinite(k[name])), name
    assert all(np.all(np.isfinite(g)) for g in k["grads"]) and k["bad"] == 0
    check_forward(c, k)
    # loss_D_shape is about 10 and D's no-GT term about 3 here: relative bound
    check_losses(c, k, shape, at_d_out=True, relative=True)
    check_backward(c, k, shape)


@pytest.mark.parametrize("b50,target", [(0.0, 0.0), (1e9, 1.0)])
def test_bce_clamps(b50, target):
    """d_out driven to exactly 0 (out = 0) and to 1 (out + 1 == out in f32)
    through b5, with w5 = 0: log(0) and log(1 - 1) clamp at -100, x (1 - x) at
    1e-12, as torch's binary_cross_entropy does; conv5's gradients carry the
    clamped derivative."""
    shape = (65, 200, 50, 50, 0, 13)
    c = dict(cases.make_inputs(shape))
    params = [p.copy() for p in c["params"]]
    params[8][:] = 0.0
    params[9][:] = -1000.0
    params[9][0] = b50
    c["params"] = params
    k = run_kernels(c, shape)
    assert np.all(np.abs(k["d_out"] - target) <= 1e-7) and np.all(k["d_out"] == target)
    assert k["bad"] == 0
    # the clamped terms are 100 y or 100 (1 - y) and the shape term 1e3 / 1e9: relative bound
    r = check_losses(c, k, shape, at_d_out=True, relative=True)
    # label 1 at x = 0 costs 100; labels below 1 at x = 1 cost (1 - y) 100
    if target == 0.0:
        assert abs(k["losses"][0] - 100.0) <= 1e-4
    else:
        assert k["losses"][0] == 0.0 and k["losses"][3] > 30.0
    assert np.abs(r["db5"]).max() > 0 and np.all(np.isfinite(k["grads"][9]))


def test_rows_outside_unit_interval_are_counted():
    """b5 = -5 on every shape class: out is about -2.2 and d_out about 1.8.  The
    call returns normally, bad_rows is the row count, nothing faults, and the
    next call with in-range weights reports 0."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    shape = (65, 200, 50, 50, 0, 13)
    c = dict(cases.make_inputs(shape))
    bad_params = [p.copy() for p in c["params"]]
    bad_params[9][:] = -5.0
    ws = D.stackdisc_workspace(265, DEV, 0)
    k = run_kernels(c, shape, params=bad_params, ws=ws)
    print("d_out range:", float(k["d_out"].min()), float(k["d_out"].max()))
    assert np.all(k["d_out"] > 1.0) and abs(float(np.median(k["d_out"][:65])) - 1.8) < 0.1
    assert k["bad"] == 265
    c2 = dict(c, m=None)
    c2["m"], c2["argc"], _, c2["y4"] = ref.forward(c["x0"], bad_params)
    c2["params"] = bad_params
    check_forward(c2, k)
    k2 = run_kernels(c, shape, ws=ws)  # the same workspace: ticket and counter are ready
    assert k2["bad"] == 0
    good = case((shape, 16))["k"]
    for name in ("m", "d_out", "losses", "dm_d"):
        assert np.array_equal(k2[name], good[name]), name


def test_repeatable_bitwise():
    cs = ((300, 700, 50, 50, 3, 50), 16)
    c = case(cs)
    k2 = run_kernels(c, cs[0])
    k = c["k"]
    for name in ("m", "argc", "d_out", "S", "losses", "dm_d", "dm_adv", "dlogits"):
        assert np.array_equal(k[name], k2[name]), name
    for g, g2 in zip(k["grads"], k2["grads"]):
        assert np.array_equal(g, g2)
    assert k["bad"] == 0 and k2["bad"] == 0

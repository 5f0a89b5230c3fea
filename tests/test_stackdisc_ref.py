"""CPU checks of the StackDiscNet work: the numpy f64 restatement
(tests/stackdisc_ref.py) against the reference capture g16 and against finite
differences, make_shape_label, load_models("disc_stack"), the module's
state_dict and host-side validation, and the arg-max rule of the GPU shapes."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import stackdisc_cases as cases
import stackdisc_ref as ref
from golden_util import adam_update_err, assert_grad_close, load
from oracle import pointnet_np as onp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segstack import stackdisc_spec  # noqa: E402

SPEC = stackdisc_spec()


def _rows(pred):
    B, C, N = pred.shape
    return pred.transpose(0, 2, 1).reshape(B * N, C)


def _row_ce(pred, seg):
    z = _rows(pred).astype(np.float64)
    lse = np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1)) + z.max(axis=1)
    return float((lse - z[np.arange(len(z)), seg.reshape(-1)]).mean())


def _adam(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update number t in float64 (in place)."""
    m *= b1
    m += (1 - b1) * g
    v *= b2
    v += (1 - b2) * g * g
    p -= lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)


def test_ref_matches_g16():
    """Both iterations of the reference's run_training_seg_stack, D on its own
    from the recorded predictions of the generator: D's outputs and the four
    loss values within 1e-3 (iteration 0's outputs also within 1e-12 of the
    reference's module in float64), iteration 0's ten gradients against the
    float64 run's by assert_grad_close, and D's update over both iterations
    (Adam replayed in float64 on the restatement's own gradients) against the
    float64 run's by the Adam-update check at 1e-3."""
    fx = load("g16_segstack_step.npz")
    B, N, S = int(fx["B"]), int(fx["N"]), int(fx["num_shapes"])
    M, lam, lr = B * N, float(fx["lambda_disc_shape"]), float(fx["lr"])
    init = list(onp.make_params(SPEC, seed=int(fx["d_seed"]), init="xavier").values())
    params = [p.astype(np.float64).copy() for p in init]
    mom = [(np.zeros(p.shape), np.zeros(p.shape)) for p in params]
    for it in range(2):
        lg = np.concatenate([_rows(fx[f"it{it}.pred_gt"]), _rows(fx[f"it{it}.pred_ng"])])
        labels = np.argmax(fx[f"it{it}.cls_gt"].reshape(B, 16), axis=1)
        grads, _, r = ref.full_backward(lg, params, M, M, ref.SOFTMAX, ref.LOG_SOFTMAX,
                                        fx[f"it{it}.soft_gt"], fx[f"it{it}.soft_ng"], labels, N, lam)
        pre = "" if it == 0 else "it1."
        e0 = float(np.max(np.abs(r["d_out"][:M] - fx[pre + "d_out_gt"].reshape(-1))))
        e1 = float(np.max(np.abs(r["d_out"][M:] - fx[pre + "d_out_nogt"].reshape(-1))))
        got = [_row_ce(fx[f"it{it}.pred_gt"], fx[f"it{it}.seg"]), r["loss_adv"], r["loss_D"],
               r["loss_D_shape"]]
        want = [float(fx[k][it]) for k in ("loss_seg", "loss_adv", "loss_D", "loss_D_shape")]
        print(f"iteration {it}: D outputs vs the float32 run {e0:.2e} / {e1:.2e}, losses {got} "
              f"reference {want}")
        assert e0 <= 1e-3 and e1 <= 1e-3
        assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-3
        if it == 0:
            assert np.array_equal(np.repeat(labels[:, None], N, axis=1), fx["it0.shape_label"])
            f0 = float(np.max(np.abs(r["d_out"][:M] - fx["d_out64_gt"].reshape(-1))))
            f1 = float(np.max(np.abs(r["d_out"][M:] - fx["d_out64_nogt"].reshape(-1))))
            s_ref = fx["s_out64_gt"].transpose(0, 2, 1).reshape(M, S)
            fs = float(np.max(np.abs(r["S"][:M] - s_ref)))
            print(f"... vs the reference's module in float64: {f0:.2e} / {f1:.2e}, shape logits "
                  f"(stored as float32) {fs:.2e}")
            assert f0 <= 1e-12 and f1 <= 1e-12 and fs <= 1e-6
            for (name, _), g in zip(SPEC, grads):
                assert_grad_close(g, fx["it0.grad64D." + name], name)
            g0 = [g.copy() for g in grads]
        for p, (m, v), g in zip(params, mom, grads):
            _adam(p, m, v, np.asarray(g, np.float64).reshape(p.shape), it + 1, lr)
    for (name, _), p, p0, g in zip(SPEC, params, init, g0):
        e, n = adam_update_err(p, p0, fx["it1.upd64D." + name].astype(np.float64), np.zeros(p0.shape),
                               g)
        print(f"D.{name}: two-iteration update rel err {e:.2e} over {n} elements")
        assert e <= 1e-3, name


def _fd_case(all_negative):
    rng = np.random.default_rng(17 + all_negative)
    n0, n1, ncls, ppc, S = 6, 5, 7, 3, 4
    params = [p.astype(np.float64) for p in cases.make_params(rng, ncls, S, bias_std=0.3)]
    if all_negative:
        params[7] = params[7] - 3.0  # conv4's bias: every channel of every row negative
    lg = 2.0 * rng.standard_normal((n0 + n1, ncls))
    soft0 = rng.uniform(0.7, 1.05, n0)
    soft0[2] = 1.05
    soft1 = rng.uniform(0.0, 0.305, n1)
    labels = rng.integers(0, S, n0 // ppc)
    return n0, n1, ppc, params, lg, soft0, soft1, labels


@pytest.mark.parametrize("all_negative", [False, True])
def test_ref_backward_vs_finite_differences(all_negative):
    """Central differences in float64 on every parameter group (conv1..conv5,
    weights and biases) for loss_D + lambda loss_D_shape, and on the no-GT rows'
    logits for lambda_adv loss_adv; with conv4's bias at -3 every m is negative
    (the 0.2 slope on the arg-max channel itself), and one label is 1.05."""
    n0, n1, ppc, params, lg, soft0, soft1, labels = _fd_case(all_negative)
    lam, lam_adv, h = 0.5, 0.37, 1e-6
    args = (n0, n1, ref.SOFTMAX, ref.LOG_SOFTMAX, soft0, soft1, labels, ppc, lam)
    x0 = np.concatenate([ref.transform(lg[:n0], ref.SOFTMAX), ref.transform(lg[n0:], ref.LOG_SOFTMAX)])
    m = ref.forward(x0, params)[0]
    assert (m < 0).all() if all_negative else (m > 0).any()
    grads, dlg, _ = ref.full_backward(lg, params, *args, lambda_adv=lam_adv)
    rng = np.random.default_rng(3)
    for i, g in enumerate(grads):
        flat = params[i].reshape(-1)
        # the six largest entries (conv4's gradient lives in the few arg-max rows) and six others
        idx = np.unique(np.concatenate([np.argsort(-np.abs(np.asarray(g).reshape(-1)))[:6],
                                        rng.choice(flat.size, min(flat.size, 6), replace=False)]))
        fd = np.zeros(len(idx))
        for j, k in enumerate(idx):
            old = flat[k]
            flat[k] = old + h
            up = ref.total_loss(lg, params, *args)[0]
            flat[k] = old - h
            dn = ref.total_loss(lg, params, *args)[0]
            flat[k] = old
            fd[j] = (up - dn) / (2 * h)
        got = np.asarray(g).reshape(-1)[idx]
        assert np.max(np.abs(got - fd)) <= 1e-6 * max(1.0, float(np.max(np.abs(fd)))), (i, got, fd)
        assert np.max(np.abs(fd)) > 0
    fd = np.zeros_like(lg)
    for r in range(n0 + n1):
        for c in range(lg.shape[1]):
            old = lg[r, c]
            lg[r, c] = old + h
            up = ref.total_loss(lg, params, *args)[1]
            lg[r, c] = old - h
            dn = ref.total_loss(lg, params, *args)[1]
            lg[r, c] = old
            fd[r, c] = lam_adv * (up - dn) / (2 * h)
    assert np.all(fd[:n0] == 0)  # loss_adv does not see the GT rows
    assert np.max(np.abs(dlg - fd[n0:])) <= 1e-6 * max(1.0, float(np.max(np.abs(fd))))


def test_ref_bce_is_torchs():
    """The clamps at -100 and 1e-12, labels above 1, against torch in float64."""
    x = np.array([0.0, 1e-50, 1e-9, 0.3, 0.5, 1 - 1e-9, 1.0])
    for y in (0.0, 0.2, 1.0, 1.05):
        tx = torch.tensor(x, requires_grad=True)
        # binary_cross_entropy refuses a target above 1: the same expression by hand
        l = -(y * torch.clamp(torch.log(tx), min=-100) + (1 - y) * torch.clamp(torch.log1p(-tx), min=-100))
        assert np.allclose(ref.bce(x, y), l.detach().numpy(), rtol=1e-14, atol=0)
        if y <= 1.0:
            t2 = torch.tensor(x, requires_grad=True)
            l2 = torch.nn.functional.binary_cross_entropy(t2, torch.full_like(t2, y), reduction="none")
            assert np.allclose(ref.bce(x, y), l2.detach().numpy(), rtol=1e-14, atol=0)
            l2.sum().backward()
            assert np.allclose(ref.bce_dx(x, y), t2.grad.numpy(), rtol=1e-12, atol=0)


def test_make_shape_label():
    from adversarial_learning_on_pointclouds_amd.utils import make_shape_label
    fx = load("g16_segstack_step.npz")
    cls = torch.from_numpy(fx["it0.cls_gt"])
    lab = make_shape_label(input=cls.squeeze(1), npts=int(fx["N"]))
    assert lab.dtype == torch.int64 and lab.shape == (int(fx["B"]), int(fx["N"]))
    assert np.array_equal(lab.numpy(), fx["it0.shape_label"])


def test_load_models_disc_stack():
    from adversarial_learning_on_pointclouds_amd import StackDiscNet
    from adversarial_learning_on_pointclouds_amd.model_utils import load_models
    torch.manual_seed(0)
    args = argparse.Namespace(input_pts=2048, disc_indim=50, init_disc="xavier")
    m = load_models("disc_stack", torch.device("cpu"), args)
    assert isinstance(m, StackDiscNet) and m.input_pts == 2048 and m.num_shapes == 16
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == SPEC
    fx = load("g16_segstack_step.npz")
    for name, shape in SPEC:
        assert fx["it0.grad64D." + name].shape == shape
    for name, p in m.named_parameters():
        if name.endswith("bias"):
            assert torch.all(p == 0)
        elif p.numel() >= 1024:
            std = float(np.sqrt(2.0 / (p.shape[0] + p.shape[1])))
            assert abs(float(p.detach().std()) - std) < 0.1 * std and abs(float(p.detach().mean())) < 0.1 * std


def test_module_on_cpu():
    """StackDiscNet on the CPU, the way PointwiseDiscNet is usable there: it is
    built, takes the reference's state_dict (g16's seeded weights) and validates
    its input; the forward itself runs on the HIP device only."""
    from adversarial_learning_on_pointclouds_amd import StackDiscNet
    fx = load("g16_segstack_step.npz")
    init = onp.make_params(SPEC, seed=int(fx["d_seed"]), init="xavier")
    m = StackDiscNet(int(fx["N"]), 50, int(fx["num_shapes"]))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in init.items()})
    with pytest.raises(ValueError, match="input_dim"):
        StackDiscNet(2048, 65, 16)
    with pytest.raises(ValueError, match="num_shapes"):
        StackDiscNet(2048, 50, 33)
    with pytest.raises(ValueError, match="input_pts"):
        StackDiscNet(0, 50, 16)
    with pytest.raises(ValueError, match="expected B x 50 x N"):
        m(torch.zeros(2, 49, 256))
    with pytest.raises(TypeError, match="float32"):
        m(torch.zeros(2, 50, 256, dtype=torch.float64))
    with pytest.raises(ValueError, match="HIP device"):
        m(torch.from_numpy(fx["it0.pred_gt"]))  # no CPU fallback


def test_c_abi_refuses_invalid_shapes():
    from adversarial_learning_on_pointclouds_amd import _lib
    lib = _lib.load()
    a = _lib.StackdiscArgs()
    a.ncls, a.n0, a.n1, a.num_shapes = 65, 1, 1, 16
    assert lib.pcadv_stackdisc_forward(a, None) == -1
    assert b"ncls" in lib.pcadv_last_error()
    a.ncls, a.num_shapes = 50, 33
    assert lib.pcadv_stackdisc_forward(a, None) == -1
    assert b"num_shapes" in lib.pcadv_last_error()
    a.num_shapes, a.n0, a.n1 = 16, 0, 0
    assert lib.pcadv_stackdisc_backward(a, None) == -1
    assert b"row counts" in lib.pcadv_last_error()
    a.n1, a.ld = 4, 49
    assert lib.pcadv_stackdisc_forward(a, None) == -1
    assert b"row stride" in lib.pcadv_last_error()
    assert lib.pcadv_stackdisc_workspace_bytes(0, 0) == 0
    assert lib.pcadv_stackdisc_workspace_bytes(65536, 0) >= 256 * 20800 * 4


@pytest.mark.parametrize("case", cases.CASES)
def test_gpu_shapes_argmax_rule(case):
    """The rows the GPU tests leave out of the arg-max comparison (top-2 relative
    gap below 1e-5) are at most 0.5 % at every shape, by the restatement alone."""
    shape, S = case
    c = cases.make_inputs(shape, S)
    y4 = ref.forward(c["x0"], c["params"])[3]
    gap = ref.top2_gap(y4)
    print(f"{case}: rows left out {int((gap < 1e-5).sum())} of {len(gap)}, smallest gap {gap.min():.2e}")
    assert (gap < 1e-5).mean() <= 0.005

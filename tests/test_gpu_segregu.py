"""PointNetSeg_regulization on the device against the reference capture g17:
the module's forward on iteration 0's inputs, the autograd backward of the
generator's loss against the reference's iteration-0 gradients, the state_dict
round trip, the two TypeErrors that keep the generators' steps apart, and the
release of a pass's activations."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import segregu_ref as ref
from golden_util import check_tensor_l2, load, rel_err
from oracle import pointnet_np as onp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segregu import make_gen_params  # noqa: E402
from make_golden_segstack import stackdisc_spec  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _models(fx, precision="fp32"):
    from adversarial_learning_on_pointclouds_amd import PointNetSeg_regulization, StackDiscNet
    G = make_gen_params()
    Dp = onp.make_params(stackdisc_spec(), seed=int(fx["d_seed"]), init="xavier")
    m = PointNetSeg_regulization(50, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    d = StackDiscNet(int(fx["N"]), 50, 16)
    d.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in Dp.items()})
    return m.to(DEV), d.to(DEV), G


@pytest.fixture(scope="module")
def fx():
    return load("g17_segregu_step.npz")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_forward_g17(fx, precision):
    """logits and x_global at 1e-3 (the project's forward bound; x_global against
    the float64 restatement, which test_segregu_ref.py holds to g17), trans_feat
    and T3 at 1e-4.  In the labelled bf16x3 mode conv1..conv3 feed fstn, so
    trans_feat is held to that mode's forward bound, 1e-3; T3 (f32 kernels on the
    points alone) stays at 1e-4."""
    m, _, G = _models(fx, precision)
    for k in ("gt", "ng"):
        pts, cls = fx[f"it0.pts_{k}"], fx[f"it0.cls_{k}"]
        with torch.no_grad():
            logits, xg, tf = m(_t(pts), _t(cls))
            T3 = m.forward_points(_t(pts), _t(cls))[3]
        assert logits.shape == (2, 50, 256) and xg.shape == (2, 2048, 1) and tf.shape == (2, 128, 128)
        r = ref.segregu_forward(G, pts, cls)
        errs = dict(logits=rel_err(logits.cpu().numpy(), fx[f"it0.pred64_{k}"]),
                    x_global=rel_err(xg.cpu().numpy(), r["x_global"]),
                    trans_feat=rel_err(tf.cpu().numpy(), fx[f"it0.trans_feat64_{k}"]),
                    T3=rel_err(T3.cpu().numpy(), fx[f"it0.T3_64_{k}"]))
        print(k, errs)
        assert errs["logits"] <= 1e-3 and errs["x_global"] <= 1e-3
        assert errs["trans_feat"] <= (1e-4 if precision == "fp32" else 1e-3) and errs["T3"] <= 1e-4


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-3), ("bf16x3", 1e-2)])
def test_autograd_backward_g17(fx, precision, tol):
    """The generator's part of the reference's iteration 0 through plain
    autograd over the modules: lambda_seg CE + lambda_adv BCE(D(log_softmax), 1)
    with D frozen + lambda_regu (MSE_gt + MSE_nogt).  Every gradient of G at
    relative L2 2e-3 (the bound test_gpu_segstack_step.py uses for g16; the
    labelled bf16x3 mode at 1e-2, its end-to-end bound in test_gpu_seg.py)."""
    m, d, _ = _models(fx, precision)
    for p in d.parameters():
        p.requires_grad = False
    mse = torch.nn.MSELoss()

    def regu(tf):
        eye = torch.eye(128, device=DEV).unsqueeze(0).repeat(tf.size(0), 1, 1)
        return mse(torch.bmm(tf, tf.transpose(2, 1)), eye)

    pred, _, tf = m(_t(fx["it0.pts_gt"]), _t(fx["it0.cls_gt"]))
    l_seg = torch.nn.CrossEntropyLoss()(pred, _t(fx["it0.seg"], torch.int64))
    pred_ng, _, tf_ng = m(_t(fx["it0.pts_ng"]), _t(fx["it0.cls_ng"]))
    assert tf.requires_grad and tf_ng.requires_grad
    d_out = d(F.log_softmax(pred_ng, dim=1))[1]
    l_adv = torch.nn.BCELoss()(d_out, torch.ones_like(d_out))
    l_gt, l_ng = regu(tf), regu(tf_ng)
    got = [l_seg.item(), l_adv.item(), l_gt.item() + l_ng.item()]
    want = [float(fx[k][0]) for k in ("loss_seg", "loss_adv", "loss_regu")]
    print("losses", got, "reference", want)
    assert np.max(np.abs(np.array(got) - np.array(want))) <= 1e-3
    lam = float(fx["lambda_regu"])
    (float(fx["lambda_seg"]) * l_seg + float(fx["lambda_adv"]) * l_adv + lam * l_gt
     + lam * l_ng).backward()
    n = 0
    for name, p in m.named_parameters():
        e = check_tensor_l2(fx, "it0.gradG." + name, p.grad.cpu().numpy(), tol=tol)
        print(f"{name}: relative L2 {e:.2e}")
        n += 1
    assert n == 44


def test_state_dict_round_trip(fx):
    from adversarial_learning_on_pointclouds_amd import PointNetSeg_regulization
    G = make_gen_params()
    assert list(G) == [str(k) for k in fx["g_keys"]]
    m = PointNetSeg_regulization(50)
    missing = m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m = m.to(DEV)
    sd = m.state_dict()
    assert list(sd) == list(G)
    for k, v in G.items():
        assert tuple(sd[k].shape) == v.shape and np.array_equal(sd[k].cpu().numpy(), v)
    # a step's flat buffers keep the keys and values
    from adversarial_learning_on_pointclouds_amd import SegStackReguTrainStep, StackDiscNet
    SegStackReguTrainStep(m, StackDiscNet(256, 50, 16).to(DEV))
    sd = m.state_dict()
    assert list(sd) == list(G) and all(np.array_equal(sd[k].cpu().numpy(), G[k]) for k in G)


def test_generators_and_steps_do_not_mix():
    from adversarial_learning_on_pointclouds_amd import (PointNetSeg, PointNetSeg_regulization,
                                                         PointwiseDiscNet, SegAdvTrainStep,
                                                         SegStackReguTrainStep, SegStackTrainStep,
                                                         StackDiscNet)
    plain, regu = PointNetSeg(50).to(DEV), PointNetSeg_regulization(50).to(DEV)
    assert not isinstance(regu, PointNetSeg)
    d = StackDiscNet(128, 50, 16).to(DEV)
    with pytest.raises(TypeError):
        SegStackReguTrainStep(plain, d)
    with pytest.raises(TypeError):
        SegStackTrainStep(regu, d)
    with pytest.raises(TypeError):
        SegAdvTrainStep(regu, PointwiseDiscNet(128, 50).to(DEV))


def test_autograd_passes_release_their_activations(fx):
    """Grad-enabled forwards, with and without a backward: once the outputs are
    dropped the node and every activation it saved are freed by reference
    counting alone, so the allocated memory is back at its baseline (the
    parameters' .grad buffers exist from the warm-up pass on)."""
    import gc
    m, _, _ = _models(fx)
    pts, cls = _t(fx["it0.pts_gt"]), _t(fx["it0.cls_gt"])

    def one(backward):
        pred, xg, tf = m(pts, cls)
        if backward:
            (pred.sum() + xg.sum() + tf.sum()).backward()

    one(True)
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    gc.disable()
    try:
        for backward in (True, False, True, False):
            one(backward)
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == base, (backward, torch.cuda.memory_allocated(), base)
    finally:
        gc.enable()

"""The float64 restatement of the stacked semi-supervised iteration
(stack_semi_ref) held to the reference's own run_training_seg_stack_
regulization_semi (g19): losses, K, the pseudo-labels, D's gradients and the
logit gradient's column sum (fc4.bias's gradient), iterations 0 and 2, at the
tolerances test_semi_seg_ref.py uses for g15."""
import functools
import os
import sys

import numpy as np
import pytest

import stack_semi_ref as R
from golden_util import assert_grad_close, load

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_segregu_semi import make_data, make_weights  # noqa: E402

LOSSES = ("loss_seg", "loss_adv", "loss_regu", "loss_semi", "loss_D", "loss_D_shape")


@functools.lru_cache(maxsize=None)
def _iteration(it):
    fx = load("g19_segregu_semi_step.npz")
    Gp, Dp = make_weights()
    d = make_data()[it]
    for k in ("cls_gt", "cls_ng", "seg"):
        assert np.array_equal(d[k], fx[f"it{it}.{k}"])
    r = R.iteration(Gp, list(Dp.values()), d, it > int(fx["semi_start"]), float(fx["semi_TH"]),
                    float(fx["lambda_seg"]), float(fx["lambda_adv"]),
                    float(fx["lambda_disc_shape"]), float(fx["lambda_semi"]))
    return fx, Dp, r


@pytest.mark.parametrize("it", [0, 2])
def test_losses_match_g19(it):
    """Every loss within 1e-6 relative of the float64 run's."""
    fx, _, r = _iteration(it)
    for k in LOSSES:
        ref = float(fx[k][it])
        print(f"iteration {it} {k}: {r[k]!r}, the reference's {ref!r}")
        assert abs(r[k] - ref) <= 1e-6 * abs(ref), k
    assert np.all(fx["loss_semi"][:2] == 0.0)  # iterations 0 and 1: i_iter <= semi_start
    assert (r["loss_semi"] > 0) == (it == 2)


def test_labels_and_k_match_g19():
    fx, _, r = _iteration(2)
    assert np.array_equal(r["semi_gt"], fx["semi_gt"])
    assert r["K"] == int(fx["K"]) and 0 < r["K"] < r["semi_gt"].size
    B, N = int(fx["B"]), int(fx["N"])
    d_ref = fx["it2.d_out_nogt"].astype(np.float64).reshape(-1)
    assert np.abs(r["d_out"][B * N:] - d_ref).max() <= 1e-9
    _, _, r0 = _iteration(0)
    assert r0["K"] == 0 and np.all(r0["semi_gt"] == 255)


def test_fixture_conditions_hold():
    """What the generator asserts on iteration 2's inputs, on what is stored
    (the 100 x margin needs the float32 run and stays with the generator)."""
    fx = load("g19_segregu_semi_step.npz")
    B, N = int(fx["B"]), int(fx["N"])
    d_out = fx["it2.d_out_nogt"].astype(np.float64).reshape(-1)
    logits = fx["it2.pred_ng"].astype(np.float64).transpose(0, 2, 1).reshape(B * N, -1)
    th = float(fx["semi_TH"])
    keep = ~(d_out <= th)
    assert 0.25 <= keep.mean() <= 0.75 and 0.0 <= d_out.min() and d_out.max() <= 1.0
    top = np.sort(logits[keep], axis=1)
    assert ((top[:, -1] - top[:, -2]) / (top[:, -1] - top[:, 0])).min() >= 1e-4
    assert float(fx["lr"]) == 0.0


@pytest.mark.parametrize("it", [0, 2])
def test_gradients_match_g19(it):
    """D's ten gradients, and fc4.bias's (the column sum of the logit gradient:
    seg CE on the GT rows, the adversarial and the semi term on the no-GT rows)."""
    fx, Dp, r = _iteration(it)
    for name, g in zip(Dp, r["gradD"]):
        assert_grad_close(np.asarray(g).reshape(-1), fx[f"it{it}.gradD.{name}"].reshape(-1), name)
    assert_grad_close(r["dlogits"].sum(axis=0), fx[f"it{it}.gradG.fc4.bias"], "fc4.bias")
    if it == 2:  # the semi term is a share of it that the bound would not hide
        _, _, r0 = _iteration(0)
        semi_part = r["dlogits"][r["dlogits"].shape[0] // 2:][r["semi_gt"].reshape(-1) != 255]
        assert np.abs(semi_part).max() > 0 and r0["K"] == 0

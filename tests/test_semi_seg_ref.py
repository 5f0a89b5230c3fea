"""The float64 restatement of run_training_seg_semi's term (semi_seg_ref) held
to the reference's own run (g15) and to a case computed by hand."""
import numpy as np

import semi_seg_ref as R
from golden_util import load


def _g15_inputs(fx):
    B, N = int(fx["B"]), int(fx["N"])
    logits = fx["it2.pred_ng"].astype(np.float64).transpose(0, 2, 1).reshape(B * N, -1)
    return logits, fx["it2.d_out_nogt"].astype(np.float64).reshape(-1)


def test_labels_and_loss_match_g15():
    """Iteration 2 of the reference's run: pseudo-labels (255s included) and K
    exactly, the loss within 1e-6 relative of the float64 run's."""
    fx = load("g15_segsemi_step.npz")
    logits, d_out = _g15_inputs(fx)
    loss, g, lab, K = R.semi_ce(logits, d_out, float(fx["semi_TH"]), float(fx["lambda_semi"]))
    assert np.array_equal(lab, fx["semi_gt"].reshape(-1))
    assert K == int(fx["K"]) and 0 < K < lab.size
    ref = float(fx["loss_semi"][2])
    print(f"loss_semi {loss!r}, the reference's {ref!r}")
    assert abs(loss - ref) <= 1e-6 * ref
    assert np.all(fx["loss_semi"][:2] == 0.0)  # iterations 0 and 1: i_iter <= semi_start
    assert not g[lab == R.IGNORE].any() and np.abs(g[lab != R.IGNORE].sum(axis=1)).max() < 1e-12


def test_fixture_conditions_hold():
    """The conditions the generator asserts on iteration 2's inputs, on what is
    stored: the mask and the labels are not decided by rounding."""
    fx = load("g15_segsemi_step.npz")
    logits, d_out = _g15_inputs(fx)
    th = float(fx["semi_TH"])
    keep = ~(d_out <= th)
    assert 0.25 <= keep.mean() <= 0.75
    assert np.abs(d_out - th).min() >= 1e-3 * th
    top = np.sort(logits[keep], axis=1)
    assert ((top[:, -1] - top[:, -2]) / (top[:, -1] - top[:, 0])).min() >= 1e-4


def test_hand_computed_case():
    """M = 3, ncls = 4: row 0 kept with an exact tie of its maximum (columns 1
    and 3: label 1), row 1 ignored (d_out equal to the threshold), row 2 kept."""
    ln2, ln3 = np.log(2.0), np.log(3.0)
    logits = np.array([[0.0, ln2, 0.0, ln2],      # exp: 1 2 1 2, sum 6
                       [5.0, 1.0, 2.0, 3.0],
                       [ln3, 0.0, 0.0, 0.0]])     # exp: 3 1 1 1, sum 6
    d_out = np.array([0.9, 0.8, 1.5])
    loss, g, lab, K = R.semi_ce(logits, d_out, 0.8, scale=4.0)
    assert lab.tolist() == [1, 255, 0] and K == 2
    # rows 0 and 2: log(6) - log(2) and log(6) - log(3)
    assert abs(loss - 0.5 * (np.log(3.0) + np.log(2.0))) < 1e-15
    want = 4.0 / 2 * np.array([[1 / 6, 2 / 6 - 1, 1 / 6, 2 / 6],
                               [0, 0, 0, 0],
                               [3 / 6 - 1, 1 / 6, 1 / 6, 1 / 6]])
    assert np.abs(g - want).max() < 1e-15
    # nothing kept: no term
    loss, g, lab, K = R.semi_ce(logits, d_out, 1.5, scale=4.0)
    assert loss == 0.0 and K == 0 and not g.any() and lab.tolist() == [255] * 3

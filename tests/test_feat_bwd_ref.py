"""feat_bwd_ref (the float64 reference the GPU edge tests compare with) pinned
against float64 autograd of conv1..conv4 + max over points, on the CPU."""
import numpy as np
import pytest
import torch

from feat_bwd_ref import NAMES, feat_bwd_ref


def _autograd(pts, w, dg):
    """conv1..conv3 with ReLU, conv4 without, max over points; the gradients of
    sum(dg * gmax) -> (grads over NAMES, argmax, x3)."""
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in w]
    w1, b1, w2, b2, w3, b3, w4, b4 = t
    x = torch.tensor(pts, dtype=torch.float64)
    x1 = torch.relu(x @ w1.T + b1)
    x2 = torch.relu(x1 @ w2.T + b2)
    x3 = torch.relu(x2 @ w3.T + b3)
    y = x3 @ w4.T + b4                      # (C, N, 1024)
    gmax, am = y.max(dim=1)
    (torch.tensor(dg, dtype=torch.float64) * gmax).sum().backward()
    g = dict(zip(NAMES, (p.grad.numpy() for p in t)))
    return g, am.numpy(), x3.detach().numpy()


@pytest.mark.parametrize("C,N,seed", [(1, 1, 0), (2, 5, 1), (3, 37, 2)])
def test_reference_equals_float64_autograd(C, N, seed):
    rng = np.random.default_rng(seed)
    shapes = [(64, 3), (64,), (64, 64), (64,), (128, 64), (128,), (1024, 128), (1024,)]
    w = [rng.normal(0, 0.5, s) for s in shapes]
    pts = rng.uniform(-1, 1, (C, N, 3))
    dg = rng.normal(0, 1, (C, 1024))
    ref, am, x3 = _autograd(pts, w, dg)
    if N > 1:
        assert len(np.unique(am)) > 1  # the scatter is not to one point only
    got, bounds, inner = feat_bwd_ref(dg, am, pts, w[0], w[1], w[2], w[3], w[4], w[6], x3)
    for k in NAMES:
        r = ref[k]
        assert got[k].shape == r.shape and np.abs(r).max() > 0, k
        assert np.abs(got[k] - r).max() <= 1e-12 * np.abs(r).max(), k
        # the bound is a bound
        assert (np.abs(got[k]) <= bounds[k] * (1 + 1e-12)).all(), k
    assert all(v > 0 for v in inner.values())


def test_reference_masks_and_duplicate_hits():
    """Two channels on one point add up; x3 <= 0 (0.0 and -0.0 included) blocks
    the point's gradient into conv3 but its values still reach dW4."""
    rng = np.random.default_rng(5)
    C, N = 1, 3
    w1, b1 = rng.integers(-1, 2, (64, 3)), np.ones(64)
    w2, b2 = rng.integers(0, 2, (64, 64)), np.ones(64)
    w3, w4 = rng.integers(-1, 2, (128, 64)), rng.integers(-1, 2, (1024, 128))
    pts = rng.integers(1, 5, (C, N, 3)) / 4.0
    dg = np.zeros((C, 1024))
    dg[0, :4] = [1, 2, -1, 1]
    gidx = np.zeros((C, 1024), np.int64)
    gidx[0, :4] = [1, 1, 2, 2]
    x3 = np.full((C, N, 128), 2.0)
    x3[0, 2, :64], x3[0, 2, 64:] = 0.0, -0.0
    x3[0, 2, 0] = -3.0
    g, _, _ = feat_bwd_ref(dg, gidx, pts, w1, b1, w2, b2, w3, w4, x3)
    dz3 = w4[0] + 2.0 * w4[1]  # point 1 only: point 2 is masked, point 0 has g = 0
    assert np.array_equal(g["db3"], dz3)
    assert np.array_equal(g["dw4"][2], -x3[0, 2]) and np.array_equal(g["dw4"][1], 2 * x3[0, 1])
    assert np.array_equal(g["db4"], dg[0])

"""Pin oracle.regularizer_bwd (and the regulariser's value) to CPU torch
autograd of mean(norm(bmm(T, T^T) - I, dim=(1, 2))) (models/pointnet.py:
345-353), including clouds whose T T^T is exactly I: their norm is 0 and
torch.norm's backward gives them the zero gradient, not 0/0.  CPU only."""
import numpy as np
import torch

from oracle import pointnet_np as onp
from golden_util import grad_err

ORTHO = (0, 1)    # reg_batch's clouds with T T^T == I exactly
GENERIC = (2, 3)


def reg_batch(k=64, seed=5):
    """Four k x k transforms: I, a signed permutation, two generic I + 0.1 normal."""
    rng = np.random.default_rng(seed)
    T = np.zeros((4, k, k), np.float32)
    T[0] = np.eye(k)
    T[1, np.arange(k), rng.permutation(k)] = rng.choice([-1.0, 1.0], k)
    T[2:] = np.eye(k)[None] + 0.1 * rng.normal(size=(2, k, k))
    return T


def torch_regularizer(T, dtype=torch.float64):
    """(value, dT) of the reference's regulariser by CPU autograd."""
    t = torch.from_numpy(T).to(dtype).requires_grad_(True)
    eye = torch.eye(T.shape[1], dtype=dtype)[None]
    reg = torch.mean(torch.norm(torch.bmm(t, t.transpose(2, 1)) - eye, dim=(1, 2)))
    reg.backward()
    return reg.item(), t.grad.numpy()


def test_regularizer_bwd_vs_torch_autograd_with_zero_norm_clouds():
    T = reg_batch()
    reg, ref = torch_regularizer(T)
    # what the f32 autograd of the reference's own expression gives at norm 0
    _, ref32 = torch_regularizer(T, torch.float32)
    got = onp.regularizer_bwd(T)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    for b in ORTHO:
        assert not ref[b].any() and not ref32[b].any()
        assert not got[b].any(), f"cloud {b}: the zero-norm gradient must be exactly 0"
    for b in GENERIC:
        e = grad_err(got[b], ref[b])
        print(f"cloud {b}: max-rel {e[0]:.2e} l2-rel {e[1]:.2e}")
        assert e[0] < 1e-6, (b, e)
    assert abs(onp.feature_transform_regularizer(T) - reg) < 1e-6 * reg

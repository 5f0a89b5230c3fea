"""Float64 numpy restatement of the regularised segmentation generator
(PointNetSeg_regulization, models/pointnet.py:205-259) and of the pieces
csrc/segtnet.hip adds: the per-cloud transform and its backward, and the MSE
orthogonality regulariser of run_training_seg_stack_regulization
(utils/trainer.py:1276-1282,1297-1303) with its gradient.  Parameter specs come
from oracle.pointnet_np; everything here computes in float64.
"""
from __future__ import annotations

import numpy as np

from oracle import pointnet_np as onp

F64 = np.float64


def segregu_spec(num_seg_classes=50):
    """state_dict order of the reference's module: stn, fstn, conv1..6, fc1..4."""
    return onp.stnkd_spec("stn.", 3) + onp.stnkd_spec("fstn.", 128) + onp.seg_spec(num_seg_classes)


def xform_fwd(x, T):
    """y[c, n, j] = sum_i x[c, n, i] T[c, i, j] (torch.bmm)."""
    return np.matmul(np.asarray(x, F64), np.asarray(T, F64))


def xform_bwd(dy, x, T, add=None, relu_x=False):
    """(dT, ddx): dT = x^T dy per cloud; ddx = (dy T^T + add) [x > 0 if relu_x],
    the term the kernel accumulates into dx."""
    dy, x, T = (np.asarray(a, F64) for a in (dy, x, T))
    dT = np.matmul(x.transpose(0, 2, 1), dy)
    ddx = np.matmul(dy, T.transpose(0, 2, 1))
    if add is not None:
        ddx = ddx + np.asarray(add, F64).reshape(ddx.shape)
    if relu_x:
        ddx = ddx * (x > 0)
    return dT, ddx


def mse_reg(T, B0=None, scale=1.0):
    """MSELoss()(T T^T, I) per group (the first B0 clouds, the rest) and
    scale * d(sum of the group losses)/dT.  Returns (loss[2], grad)."""
    T = np.asarray(T, F64)
    C, k, _ = T.shape
    B0 = C if B0 is None else B0
    S = np.matmul(T, T.transpose(0, 2, 1)) - np.eye(k)[None]
    per = (S ** 2).sum((1, 2))
    loss = np.zeros(2)
    grad = np.zeros_like(T)
    for g, (lo, hi) in enumerate(((0, B0), (B0, C))):
        if hi > lo:
            loss[g] = per[lo:hi].sum() / ((hi - lo) * k * k)
            grad[lo:hi] = scale * 4.0 / ((hi - lo) * k * k) * np.matmul(S[lo:hi], T[lo:hi])
    return loss, grad


def _w(p, name):
    w = np.asarray(p[name], F64)
    return w.reshape(w.shape[0], -1)


def _b(p, name):
    return np.asarray(p[name], F64)


def _relu(x):
    return np.maximum(x, 0.0)


def stn_forward(p, x, prefix, k):
    """STN3d / STNkd on point-major x (B, N, k) -> (B, k, k)."""
    h = _relu(x @ _w(p, prefix + "conv1.weight").T + _b(p, prefix + "conv1.bias"))
    h = _relu(h @ _w(p, prefix + "conv2.weight").T + _b(p, prefix + "conv2.bias"))
    h = _relu(h @ _w(p, prefix + "conv3.weight").T + _b(p, prefix + "conv3.bias"))
    g = h.max(1)
    h = _relu(g @ _w(p, prefix + "fc1.weight").T + _b(p, prefix + "fc1.bias"))
    h = _relu(h @ _w(p, prefix + "fc2.weight").T + _b(p, prefix + "fc2.bias"))
    t = h @ _w(p, prefix + "fc3.weight").T + _b(p, prefix + "fc3.bias")
    return t.reshape(-1, k, k) + np.eye(k)[None]


def segregu_forward(p, pts, cls):
    """PointNetSeg_regulization.forward: pts (B, N, 3), cls (B, 1, 16) ->
    dict(logits (B, C, N), x_global (B, 2048, 1), trans_feat (B, 128, 128),
    T3 (B, 3, 3))."""
    pts = np.asarray(pts, F64)
    B, N, _ = pts.shape
    T3 = stn_forward(p, pts, "stn.", 3)
    h = xform_fwd(pts, T3)
    xs = []
    for i in range(1, 4):
        h = _relu(h @ _w(p, f"conv{i}.weight").T + _b(p, f"conv{i}.bias"))
        xs.append(h)
    T = stn_forward(p, xs[2], "fstn.", 128)
    h = xform_fwd(xs[2], T)
    for i in range(4, 7):
        h = _relu(h @ _w(p, f"conv{i}.weight").T + _b(p, f"conv{i}.bias"))
        xs.append(h)
    g = xs[5].max(1)
    cvec = np.asarray(cls, F64).reshape(B, 1, -1)
    feat = np.concatenate(xs[:5] + [np.broadcast_to(g[:, None, :], (B, N, 2048)),
                                    np.broadcast_to(cvec, (B, N, cvec.shape[-1]))], axis=2)
    h = _relu(feat @ _w(p, "fc1.weight").T + _b(p, "fc1.bias"))
    h = _relu(h @ _w(p, "fc2.weight").T + _b(p, "fc2.bias"))
    h = _relu(h @ _w(p, "fc3.weight").T + _b(p, "fc3.bias"))
    out = h @ _w(p, "fc4.weight").T + _b(p, "fc4.bias")
    return dict(logits=out.transpose(0, 2, 1), x_global=g[:, :, None], trans_feat=T, T3=T3)


def log_softmax(x, axis):
    m = x.max(axis, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis, keepdims=True))


def seg_ce(logits, seg):
    """CrossEntropyLoss()(logits (B, C, N), seg (B, N)) in float64."""
    lsm = log_softmax(np.asarray(logits, F64), 1)
    return float(-np.take_along_axis(lsm, seg[:, None, :], 1).mean())

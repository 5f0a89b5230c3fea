"""StackDiscNet (models/discriminator.py:139-175) and the four loss terms of
run_training_seg_stack (utils/trainer.py:1097-1150) restated in numpy float64:
forward, the losses with their derivatives, and the full backward (conv1..conv5
and the input), behind the input transforms of pwdisc_ref.

    x1..x3 = lrelu(conv(.)), y4 = lrelu(conv4(x3)), m = max_c y4 (first index),
    S[s] = w5[s] m + b5[s], out = logsumexp_s S, d_out = out / (out + 1).

As in pwdisc_ref the backward can run on a given arg-max channel and given
masks (the signs of x1..x3 and of m), so the f32 kernels and this restatement
differentiate the same piecewise-linear function."""
import numpy as np

from pwdisc_ref import LOG_SOFTMAX, NONE, SOFTMAX, top2_gap, transform, transform_bwd  # noqa: F401

SLOPE = 0.2


def lrelu(x):
    return np.where(x > 0, x, SLOPE * x)


def _mats(params):
    p = [np.asarray(t, np.float64) for t in params]
    W = [p[2 * i].reshape(p[2 * i].shape[0], -1) for i in range(4)]
    return W, [p[2 * i + 1] for i in range(4)], p[8].reshape(-1), p[9].reshape(-1)


def forward(x0, params):
    """x0 (rows, C), params: the ten tensors in state_dict order.  Returns m
    (rows,), argc (rows,) (the first index on ties), acts [x0, x1, x2, x3] and
    y4 (rows, 128)."""
    W, b, _, _ = _mats(params)
    acts = [np.asarray(x0, np.float64)]
    for i in range(3):
        acts.append(lrelu(acts[-1] @ W[i].T + b[i]))
    y4 = lrelu(acts[3] @ W[3].T + b[3])
    argc = np.argmax(y4, axis=1)
    return y4[np.arange(len(y4)), argc], argc, acts, y4


def head(m, params):
    """conv5 and the custom activation on the per-point scalar m: S (rows,
    num_shapes), out (rows,), d_out (rows,), p = softmax_s S."""
    _, _, w5, b5 = _mats(params)
    S = np.asarray(m, np.float64)[:, None] * w5 + b5
    mx = S.max(axis=1, keepdims=True)
    e = np.exp(S - mx)
    out = mx[:, 0] + np.log(e.sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = out / (out + 1.0)
    return S, out, d, e / e.sum(axis=1, keepdims=True)


def bce(x, y):
    """torch.nn.functional.binary_cross_entropy per element: both logs clamped
    at -100 (x outside [0, 1] is the caller's to exclude)."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lx = np.maximum(np.log(x), -100.0)
        l1 = np.maximum(np.log1p(-x), -100.0)
    return -(y * lx + (1.0 - y) * l1)


def bce_dx(x, y):
    """... and its derivative as torch forms it: (x - y) / max(x (1 - x), 1e-12),
    the 1e-12 a float32 constant in every dtype."""
    x = np.asarray(x, np.float64)
    return (x - y) / np.maximum(x * (1.0 - x), float(np.float32(1e-12)))


def losses(m, params, n0, n1, soft0, soft1, shape_label, pts_per_cloud, lambda_shape, d_out=None):
    """From the per-point m of the rows [GT; no-GT]: a dict with loss_adv,
    loss_D (and its parts d_gt, d_nogt), loss_D_shape (unscaled), dm_d (n0 + n1,)
    = d(loss_D + lambda_shape loss_D_shape)/dm, dm_adv (n1,) = d loss_adv/dm,
    dw5, db5 (of loss_D + lambda_shape loss_D_shape) and dS (rows, S).
    d_out: evaluate the BCE terms at these probabilities instead of the
    restatement's own (the kernel's f32 d_out, where a clamp makes the terms
    discontinuous in it)."""
    _, _, w5, _ = _mats(params)
    m = np.asarray(m, np.float64)
    S, out, d, p = head(m, params)
    x = d if d_out is None else np.asarray(d_out, np.float64)
    dxdo = 1.0 / (out + 1.0) ** 2
    rows = n0 + n1
    y = np.concatenate([np.asarray(soft0, np.float64).reshape(-1)[:n0],
                        np.asarray(soft1, np.float64).reshape(-1)[:n1]])
    cnt = np.concatenate([np.full(n0, max(n0, 1)), np.full(n1, max(n1, 1))]).astype(np.float64)
    l = bce(x, y)
    d_gt = 0.5 * l[:n0].mean() if n0 else 0.0
    d_ng = 0.5 * l[n0:].mean() if n1 else 0.0
    adv = bce(x[n0:], 1.0).mean() if n1 else 0.0
    gd = 0.5 * bce_dx(x, y) * dxdo / cnt
    dS = gd[:, None] * p
    ce = 0.0
    if n0:
        lab = np.repeat(np.asarray(shape_label, np.int64), pts_per_cloud)
        assert len(lab) == n0
        ce = float((out[:n0] - S[np.arange(n0), lab]).mean())
        onehot = np.zeros_like(p[:n0])
        onehot[np.arange(n0), lab] = 1.0
        dS[:n0] += lambda_shape / n0 * (p[:n0] - onehot)
    dm_d = dS @ w5
    dm_adv = bce_dx(x[n0:], 1.0) * dxdo[n0:] * (p[n0:] @ w5) / max(n1, 1)
    assert len(dm_d) == rows
    return dict(loss_adv=float(adv), loss_D=float(d_gt + d_ng), d_gt=float(d_gt), d_nogt=float(d_ng),
                loss_D_shape=ce, dm_d=dm_d, dm_adv=dm_adv, dw5=dS.T @ m, db5=dS.sum(axis=0), dS=dS,
                d_out=d, S=S)


def backward(x0, params, dm, argc=None, masks=None, top=None):
    """Gradients of sum_row dm[row] m[row]: (conv1..conv4's eight gradients in
    state_dict order and shapes, dx0 (rows, C)).  argc / masks (three boolean
    (rows, 64) arrays, x1..x3 > 0) / top (m > 0) default to this restatement's
    own."""
    W, b, _, _ = _mats(params)
    m, a0, acts, _ = forward(x0, params)
    argc = a0 if argc is None else np.asarray(argc)
    masks = [a > 0 for a in acts[1:]] if masks is None else [np.asarray(k, bool) for k in masks]
    top = m > 0 if top is None else np.asarray(top, bool)
    rows = len(m)
    dz = np.zeros((rows, 128))
    dz[np.arange(rows), argc] = np.asarray(dm, np.float64) * np.where(top, 1.0, SLOPE)
    grads = [None] * 8
    for i in range(3, -1, -1):
        grads[2 * i] = (dz.T @ acts[i]).reshape(np.asarray(params[2 * i]).shape)
        grads[2 * i + 1] = dz.sum(axis=0)
        dz = dz @ W[i]
        if i > 0:
            dz = dz * np.where(masks[i - 1], 1.0, SLOPE)
    return grads, dz


def total_loss(lg, params, n0, n1, t0, t1, soft0, soft1, shape_label, ppc, lambda_shape):
    """(loss_D + lambda_shape loss_D_shape, loss_adv) as functions of the logits
    and the parameters (finite differences)."""
    x0 = np.concatenate([transform(lg[:n0], t0), transform(lg[n0:], t1)])
    m = forward(x0, params)[0]
    r = losses(m, params, n0, n1, soft0, soft1, shape_label, ppc, lambda_shape)
    return r["loss_D"] + lambda_shape * r["loss_D_shape"], r["loss_adv"]


def full_backward(lg, params, n0, n1, t0, t1, soft0, soft1, shape_label, ppc, lambda_shape,
                  lambda_adv=1.0):
    """All ten parameter gradients of loss_D + lambda_shape loss_D_shape and the
    no-GT rows' gradient of lambda_adv loss_adv with respect to the logits."""
    x0 = np.concatenate([transform(lg[:n0], t0), transform(lg[n0:], t1)])
    m = forward(x0, params)[0]
    r = losses(m, params, n0, n1, soft0, soft1, shape_label, ppc, lambda_shape)
    grads, _ = backward(x0, params, r["dm_d"])
    grads += [r["dw5"].reshape(np.asarray(params[8]).shape), r["db5"]]
    d = np.zeros(n0 + n1)
    d[n0:] = lambda_adv * r["dm_adv"]
    _, dx0 = backward(x0, params, d)
    return grads, transform_bwd(x0[n0:], dx0[n0:], t1), r

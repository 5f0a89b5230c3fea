"""PointwiseDiscNet (models/discriminator.py:53-79) and the three
BCE-with-logits terms of run_training_seg (utils/trainer.py:916-963) restated
in numpy float64: forward, backward, and the input transforms (softmax /
log_softmax) the trainer puts in front of D.

The backward can run on a given argmax channel and given ReLU masks ("same
activations"): the f32 kernels and this f64 restatement then differentiate the
same piecewise-linear function, and the comparison is not disturbed by a
pre-activation within rounding of zero or by a near-tie of the channel max."""
import numpy as np

NONE, SOFTMAX, LOG_SOFTMAX = 0, 1, 2


def transform(x, kind):
    """x (rows, C) -> D's input."""
    x = np.asarray(x, np.float64)
    if kind == NONE:
        return x
    z = x - x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1, keepdims=True))
    return np.exp(z - lse) if kind == SOFTMAX else z - lse


def transform_bwd(y, dy, kind):
    """Gradient with respect to the logits given y = transform(x) and dL/dy."""
    if kind == NONE:
        return dy
    if kind == SOFTMAX:
        return y * (dy - (dy * y).sum(axis=1, keepdims=True))
    return dy - np.exp(y) * dy.sum(axis=1, keepdims=True)


def _mats(params):
    p = [np.asarray(t, np.float64) for t in params]
    return [p[2 * i].reshape(p[2 * i].shape[0], -1) for i in range(4)], [p[2 * i + 1] for i in range(4)]


def forward(x0, params):
    """x0 (rows, C), params: the eight tensors in state_dict order.  Returns
    out (rows,), argc (rows,) (the first index on ties), acts [x0, x1, x2, x3]
    and y4 (rows, 128)."""
    W, b = _mats(params)
    acts = [np.asarray(x0, np.float64)]
    for i in range(3):
        acts.append(np.maximum(acts[-1] @ W[i].T + b[i], 0.0))
    y4 = np.maximum(acts[3] @ W[3].T + b[3], 0.0)
    argc = np.argmax(y4, axis=1)
    return y4[np.arange(len(y4)), argc], argc, acts, y4


def top2_gap(y4):
    """Relative gap between the largest and the second largest channel."""
    s = np.sort(y4, axis=1)
    return (s[:, -1] - s[:, -2]) / np.maximum(np.abs(s[:, -1]), 1e-300)


def backward(x0, params, dout, argc=None, masks=None, live=None):
    """Gradients of sum_row dout[row] out[row]: (eight parameter gradients in
    state_dict order and shapes, dx0 (rows, C)).  argc / masks (three boolean
    (rows, 64) arrays, x1..x3 > 0) / live (out > 0) default to this
    restatement's own."""
    W, b = _mats(params)
    out, a0, acts, _ = forward(x0, params)
    argc = a0 if argc is None else np.asarray(argc)
    masks = [a > 0 for a in acts[1:]] if masks is None else [np.asarray(m, bool) for m in masks]
    live = out > 0 if live is None else np.asarray(live, bool)
    rows = len(out)
    dz = np.zeros((rows, 128))
    dz[np.arange(rows), argc] = np.asarray(dout, np.float64) * live
    grads = [None] * 8
    for i in range(3, -1, -1):
        grads[2 * i] = (dz.T @ acts[i]).reshape(np.asarray(params[2 * i]).shape)
        grads[2 * i + 1] = dz.sum(axis=0)
        dz = dz @ W[i]
        if i > 0:
            dz = dz * masks[i - 1]
    return grads, dz


def bce_with_logits(z, y):
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def losses(out, n0, n1, soft0, soft1):
    """(loss_adv, loss_D, dout_d (n0 + n1,), dout_adv (n1,)) of D's outputs on
    the rows [GT; no-GT] (trainer.py:924,945-946,960-961)."""
    z0, z1 = np.asarray(out[:n0], np.float64), np.asarray(out[n0:n0 + n1], np.float64)
    y0, y1 = np.asarray(soft0, np.float64), np.asarray(soft1, np.float64)
    adv = bce_with_logits(z1, 1.0).mean() if n1 else 0.0
    dgt = 0.5 * bce_with_logits(z0, y0).mean() if n0 else 0.0
    dng = 0.5 * bce_with_logits(z1, y1).mean() if n1 else 0.0
    dout_d = np.concatenate([0.5 * (sigmoid(z0) - y0) / max(n0, 1),
                             0.5 * (sigmoid(z1) - y1) / max(n1, 1)])
    dout_adv = (sigmoid(z1) - 1.0) / max(n1, 1)
    return adv, dgt + dng, dout_d, dout_adv

"""The semi-supervised term of run_training_seg_semi (utils/trainer.py:1999-2024)
restated in numpy float64, point-major: logits (M, ncls), D's raw per-point
output d_out (M,).

  - a point is ignored where d_out <= semi_th (a value equal to the threshold
    included), kept otherwise;
  - its pseudo-label is argmax(logits) (the first index on ties), 255 where
    ignored;
  - with no point kept there is no term: loss 0, no gradient;
  - otherwise the loss is CrossEntropyLoss(ignore_index=255) against the
    pseudo-labels, the mean over the K kept points of logsumexp(row) - max(row);
  - the labels are data, so the gradient of scale x loss on a kept row is
    scale / K (softmax(row) - onehot(label)) and nothing on an ignored row."""
import numpy as np

IGNORE = 255


def semi_labels(logits, d_out, semi_th):
    """(labels int64 (M,) with 255 where ignored, keep mask, K)."""
    logits = np.asarray(logits, np.float64)
    keep = ~(np.asarray(d_out) <= semi_th)
    lab = np.argmax(logits, axis=1).astype(np.int64)
    lab[~keep] = IGNORE
    return lab, keep, int(keep.sum())


def semi_ce(logits, d_out, semi_th, scale=1.0):
    """(loss, dlogits (M, ncls) = d(scale loss)/dlogits, labels, K), float64."""
    x = np.asarray(logits, np.float64)
    lab, keep, K = semi_labels(x, d_out, semi_th)
    g = np.zeros_like(x)
    if K == 0:
        return 0.0, g, lab, 0
    z = x[keep] - x[keep].max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    loss = float(np.log(s).sum() / K)  # the label's logit is the row's maximum: z there is 0
    p = e / s
    p[np.arange(K), lab[keep]] -= 1.0
    g[keep] = scale / K * p
    return loss, g, lab, K

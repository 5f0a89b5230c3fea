"""One iteration of run_training_seg_stack_regulization_semi (utils/trainer.py:
1680-1833; without the regulariser, run_training_seg_stack_semi's :1457-1586)
restated in numpy float64 by composing the restatements this suite already has:
segregu_ref (the generator's forward, the regulariser), stackdisc_ref (D's
forward, its four terms and every gradient) and semi_seg_ref (the pseudo-label
term on D's (B N,) output, taken on the no-GT rows).

The generator's backward is not restated; what the iteration hands to it is:
dlogits, the gradient of lambda_seg loss_seg + lambda_adv loss_adv +
lambda_semi loss_semi with respect to the 2 B N logit rows [GT; no-GT].  Its
column sum is fc4.bias's gradient, which pins the composition against a
recorded run."""
import numpy as np

import semi_seg_ref
import stackdisc_ref as sd
from segregu_ref import mse_reg, seg_ce, segregu_forward


def _rows(logits):
    """(B, C, N) -> point-major (B N, C)."""
    B, C, N = logits.shape
    return logits.transpose(0, 2, 1).reshape(B * N, C)


def iteration(Gp, Dp, d, semi, semi_th, lambda_seg, lambda_adv, lambda_disc_shape, lambda_semi):
    """Gp: the generator's state (name -> array), Dp: D's ten tensors in
    state_dict order, d: one iteration's batches (pts_gt, cls_gt, seg, pts_ng,
    cls_ng, soft_gt, soft_ng).  Returns a dict: the six losses, K, semi_gt
    ((B, N), 255 where ignored or with the term off), gradD (ten arrays),
    dlogits (2 B N, C), d_out (2 B N,), trans (2 B, 128, 128)."""
    B, N = d["seg"].shape
    M = B * N
    fw = [segregu_forward(Gp, d["pts_" + k], d["cls_" + k]) for k in ("gt", "ng")]
    lg = np.concatenate([_rows(f["logits"]) for f in fw])
    seg = np.asarray(d["seg"]).reshape(-1)
    loss_seg = seg_ce(fw[0]["logits"], np.asarray(d["seg"]))
    trans = np.concatenate([f["trans_feat"] for f in fw])
    regu, _ = mse_reg(trans, B0=B)
    shape_label = np.argmax(np.asarray(d["cls_gt"]).reshape(B, -1), axis=1)
    gradD, dl_adv, r = sd.full_backward(lg, Dp, M, M, sd.SOFTMAX, sd.LOG_SOFTMAX,
                                        np.asarray(d["soft_gt"]).reshape(-1),
                                        np.asarray(d["soft_ng"]).reshape(-1), shape_label, N,
                                        lambda_disc_shape, lambda_adv)
    dlogits = np.zeros_like(lg)
    p = np.exp(sd.transform(lg[:M], sd.LOG_SOFTMAX))
    p[np.arange(M), seg] -= 1.0
    dlogits[:M] = lambda_seg / M * p
    dlogits[M:] = dl_adv
    loss_semi, K, semi_gt = 0.0, 0, np.full(M, semi_seg_ref.IGNORE, np.int64)
    if semi:
        loss_semi, g, semi_gt, K = semi_seg_ref.semi_ce(lg[M:], r["d_out"][M:], semi_th, lambda_semi)
        dlogits[M:] += g
    return dict(loss_seg=loss_seg, loss_adv=r["loss_adv"], loss_regu=float(regu.sum()),
                loss_semi=loss_semi, loss_D=r["loss_D"], loss_D_shape=r["loss_D_shape"], K=K,
                semi_gt=semi_gt.reshape(B, N), gradD=gradD, dlogits=dlogits, d_out=r["d_out"],
                trans=trans)

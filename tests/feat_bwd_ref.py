"""Float64 reference of the PointNetfeat backward (pcadv_feat_bwd), written
from the maths alone, plus the bound that makes an f32 computation of it exact.

Forward (models/pointnet.py:115-130): x1 = relu(conv1(pts)), x2 = relu(conv2(x1)),
x3 = relu(conv3(x2)), gmax[c,o] = max_n (x3[c,n,:] . W4[o,:] + b4[o]), no ReLU
before the max.  Given g = dL/dgmax and gidx = argmax:
  dX3[c,n,:] = sum_{o: gidx[c,o] = n} g[c,o] W4[o,:]
  dZ3 = dX3 * (x3 > 0);  dZ2 = (dZ3 W3) * (x2 > 0);  dZ1 = (dZ2 W2) * (x1 > 0)
  dW4[o,:] = sum_c g[c,o] x3[c, gidx[c,o], :];  db4 = sum_c g
  dW3 = dZ3^T x2, db3 = sum dZ3;  dW2 = dZ2^T x1, db2 = sum dZ2;
  dW1 = dZ1^T pts, db1 = sum dZ1
x3 is an input (the forward's saved activation: only its sign reaches the mask,
its values reach dW4); x1 and x2 are recomputed from the points.

Every quantity also carries its bound sum |a||b|: the same expressions on
absolute values.  Any partial sum of the terms of an entry, in any order and
grouping, is bounded by that entry's bound, so when all terms are multiples of
1/q and q * bound < 2^24 every partial sum is an f32 number: an f32
implementation is then exact whatever its summation order.
"""
import numpy as np

F64 = np.float64
NAMES = ("dw1", "db1", "dw2", "db2", "dw3", "db3", "dw4", "db4")


def _mat(w):
    w = np.asarray(w, F64)
    return w.reshape(w.shape[0], -1)


def feat_bwd_ref(dg, gidx, pts, w1, b1, w2, b2, w3, w4, x3):
    """-> (grads, bounds, inner): grads and bounds are dicts over NAMES (float64
    arrays of the parameters' matrix shapes); inner holds the largest bound of
    every intermediate an implementation has to form (x1, x2, dX3, dX2, dX1:
    the pre-mask products)."""
    dg, pts, x3 = np.asarray(dg, F64), np.asarray(pts, F64), np.asarray(x3, F64)
    gidx = np.asarray(gidx).astype(np.int64)
    w1, w2, w3, w4 = _mat(w1), _mat(w2), _mat(w3), _mat(w4)
    b1, b2 = np.asarray(b1, F64), np.asarray(b2, F64)
    C, N, _ = pts.shape
    O = w4.shape[0]
    assert dg.shape == (C, O) and gidx.shape == (C, O) and x3.shape == (C, N, w4.shape[1])
    assert gidx.min() >= 0 and gidx.max() < N

    x1 = np.maximum(pts @ w1.T + b1, 0.0)
    x2 = np.maximum(x1 @ w2.T + b2, 0.0)
    x1_bound = np.abs(pts) @ np.abs(w1).T + np.abs(b1)
    x2_bound = x1_bound @ np.abs(w2).T + np.abs(b2)

    cc = np.broadcast_to(np.arange(C)[:, None], (C, O))
    dx3 = np.zeros((C, N, w4.shape[1]), F64)
    dx3_bound = np.zeros_like(dx3)
    for c in range(C):  # per cloud: the (O, 128) products stay small
        np.add.at(dx3[c], gidx[c], dg[c][:, None] * w4)
        np.add.at(dx3_bound[c], gidx[c], np.abs(dg[c])[:, None] * np.abs(w4))
    m3, m2, m1 = x3 > 0, x2 > 0, x1 > 0
    dz3, dz3_bound = dx3 * m3, dx3_bound * m3
    dx2, dx2_bound = dz3 @ w3, dz3_bound @ np.abs(w3)
    dz2, dz2_bound = dx2 * m2, dx2_bound * m2
    dx1, dx1_bound = dz2 @ w2, dz2_bound @ np.abs(w2)
    dz1, dz1_bound = dx1 * m1, dx1_bound * m1

    rows = x3[cc, gidx]  # (C, O, 128): the argmax point's activations
    flat = lambda a: a.reshape(C * N, -1)
    grads = dict(
        dw1=flat(dz1).T @ flat(pts), db1=flat(dz1).sum(0),
        dw2=flat(dz2).T @ flat(x1), db2=flat(dz2).sum(0),
        dw3=flat(dz3).T @ flat(x2), db3=flat(dz3).sum(0),
        dw4=np.einsum("co,cok->ok", dg, rows), db4=dg.sum(0))
    bounds = dict(
        dw1=flat(dz1_bound).T @ np.abs(flat(pts)), db1=flat(dz1_bound).sum(0),
        dw2=flat(dz2_bound).T @ flat(x1_bound), db2=flat(dz2_bound).sum(0),
        dw3=flat(dz3_bound).T @ flat(x2_bound), db3=flat(dz3_bound).sum(0),
        dw4=np.einsum("co,cok->ok", np.abs(dg), np.abs(rows)), db4=np.abs(dg).sum(0))
    inner = dict(x1=float(x1_bound.max()), x2=float(x2_bound.max()), dx3=float(dx3_bound.max()),
                 dx2=float(dx2_bound.max()), dx1=float(dx1_bound.max()))
    return grads, bounds, inner

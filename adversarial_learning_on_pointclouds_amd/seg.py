"""PointNetSeg on the pcadv dense point-wise GEMM engine (csrc/gemm.hip).

Mirrors models/pointnet.py:261-317 of the reference: same class name,
constructor argument, forward signature (x: B x N x 3, cls: B x 1 x 16) and
return tuple (logits B x C x N, x_global B x 2048 x 1), same state_dict keys
and shapes, so reference checkpoints load unchanged.  The training loop
run_training_pointnet_seg (utils/trainer.py:310-400) is mirrored in
trainer.py.

Layout: activations are point-major rows (B*N rows).  conv1..conv5 write
their outputs straight into the column blocks of one [B*N][960] buffer, which
is both the next layer's input and the per-point part of fc1's 3024-wide
input (pointnet.py:304-306: [x1..x5 | tile(x_global) | tile(cls)]).  The
tiled parts are the same for every point of a cloud, so they are folded into
a per-cloud bias of fc1 (a B-row GEMM) instead of being materialised.
conv6 + ReLU + max over points never materialises the [B*N][2048] output: a
screened GEMM keeps per-tile candidates and the winner is re-evaluated in f32.

Numerics (precision="fp32", the default, the reference's dtype): every GEMM
multiplies the three-way bf16 splits of its f32 operands as six MFMA products
(hi hi, hi mid, mid hi, hi lo, mid mid, lo hi; f32 accumulate): f32-level
accuracy.  conv6's max is screened with three products and its winner (and
near-tie runner-up) re-evaluated as an exact f32 dot product, so the pooled
values are f32.  precision="bf16x3" (an explicitly labelled speed option,
below fp32): the forward and data-gradient GEMMs take three products of
hi / lo splits (relative error <= ~1.2e-5 of sum|a b| per layer), the forward
staged from bf16 planes its producers write.  Weight gradients (sums over all
B*N points, heavy cancellation) take six products in both modes.
tests/test_gpu_seg.py holds the tolerances.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check, stream_ptr
from .discriminator import (PWD_LOG_SOFTMAX, PWD_SOFTMAX, PointwiseDiscNet, StackDiscNet,
                            pwdisc_backward, pwdisc_forward, pwdisc_workspace, row_semi_apply,
                            stackdisc_backward, stackdisc_forward, stackdisc_workspace)
from .flat import FlatAdam
from .pointnet import STN3d, STNkd
from .step import FusedStep

__all__ = ["PointNetSeg", "PointNetSeg_regulization", "SegTrainStep", "SegAdvTrainStep",
           "SegStackTrainStep", "SegStackReguTrainStep", "seg_cross_entropy", "seg_forward",
           "seg_backward", "segregu_forward", "segregu_backward", "SegDualTrainStep",
           "dualdisc_point", "dualdisc_shape", "sgd_"]

_LOC = 960                       # x1..x5 widths 64 + 128 + 128 + 128 + 512
PRECISIONS = ("fp32", "bf16x3")
# _PLANES, _PAIR and _DEFER are not options: they are the seams through which
# tests/test_gpu_seg.py holds each form bitwise to the older one it replaced.
# bf16x3 mode: the forward's operands as bf16 hi / lo planes written once by
# their producers (pcadv_gemm_bf2; bitwise the f32-staged result); False
# stages f32
_PLANES = True


def _check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision: one of {PRECISIONS}, got {precision!r}")
    return precision
_OFF = [0, 64, 192, 320, 448, 960]
_CONV = [(3, 64), (64, 128), (128, 128), (128, 128), (128, 512), (512, 2048)]


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _pb(t, off=0):  # bf16 tensors: element offsets of 2 bytes
    return ctypes.c_void_p(t.data_ptr() + 2 * off)


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), device=dev, dtype=torch.uint8)


class _Engine:
    """Thin, validated calls into the C ABI (every launch on the current stream)."""

    def __init__(self):
        self.lib = _lib.load()

    def gemm(self, a, lda, b, ldb, c, ldc, M, N, K, *, ta=0, tb=0, cmask=None, ldm=0, bias=None,
             bias_rows=None, rows_per_group=0, relu=False, accumulate=False, precise=False,
             a_off=0, b_off=0, c_off=0, m_off=0, cp=None, ldcp=0, cp_off=0):
        check(self.lib.pcadv_gemm(_p(a, a_off), lda, ta, _p(b, b_off), ldb, tb, _p(c, c_off), ldc,
                                  M, N, K, None if bias is None else _p(bias),
                                  None if bias_rows is None else _p(bias_rows), rows_per_group,
                                  int(relu), int(accumulate),
                                  None if cmask is None else _p(cmask, m_off), ldm, int(precise),
                                  None if cp is None else _pb(cp[0], cp_off),
                                  None if cp is None else _pb(cp[1], cp_off), ldcp, stream_ptr()),
              "pcadv_gemm")

    def gemm_bf2(self, ap, lda, bp, ldb, c, ldc, M, N, K, *, bias=None, bias_rows=None,
                 rows_per_group=0, relu=False, a_off=0, b_off=0, c_off=0, cp=None, ldcp=0,
                 cp_off=0):
        """A, B as (hi, lo) bf16 plane pairs; C f32 (+ its planes)."""
        check(self.lib.pcadv_gemm_bf2(_pb(ap[0], a_off), _pb(ap[1], a_off), lda, _pb(bp[0], b_off),
                                      _pb(bp[1], b_off), ldb, _p(c, c_off), ldc,
                                      None if cp is None else _pb(cp[0], cp_off),
                                      None if cp is None else _pb(cp[1], cp_off), ldcp, M, N, K,
                                      None if bias is None else _p(bias),
                                      None if bias_rows is None else _p(bias_rows),
                                      rows_per_group, int(relu), 0, None, 0, stream_ptr()),
              "pcadv_gemm_bf2")

    def split(self, x, hi, lo):
        """x (rows, cols) f32 contiguous -> hi, lo bf16 of the same shape."""
        r, c = (1, x.numel()) if x.dim() == 1 else (x.shape[0], x.shape[1])
        check(self.lib.pcadv_split_bf2(_p(x), c, r, c, _pb(hi), _pb(lo), c, stream_ptr()),
              "pcadv_split_bf2")

    def gemm_desc(self, a, lda, b, ldb, c, ldc, M, N, K, *, ta=0, tb=0, cmask=None, ldm=0,
                  bias=None, bias_rows=None, rows_per_group=0, relu=False, accumulate=False,
                  precise=False, a_off=0, b_off=0, c_off=0, m_off=0):
        """pcadv_gemm's arguments as a pcadv_gemm_desc (for wgrad(..., pair=))."""
        return _lib.GemmDesc(_p(a, a_off), lda, ta, _p(b, b_off), ldb, tb, _p(c, c_off), ldc, M, N,
                             K, None if bias is None else _p(bias),
                             None if bias_rows is None else _p(bias_rows), rows_per_group,
                             int(relu), int(accumulate), None if cmask is None else _p(cmask, m_off),
                             ldm, int(precise), None, None, 0)

    def gemm_run(self, g):
        """Enqueue a pcadv_gemm_desc as its own launch."""
        check(self.lib.pcadv_gemm(g.a, g.lda, g.ta, g.b, g.ldb, g.tb, g.c, g.ldc, g.M, g.N, g.K,
                                  g.bias, g.bias_rows, g.rows_per_group, g.relu, g.accumulate,
                                  g.cmask, g.ldm, g.precise, g.c_hi, g.c_lo, g.ldcp, stream_ptr()),
              "pcadv_gemm")

    def wgrad(self, dz, ldz, x, ldx, rows, O, K, dw, ldo, *, db=None, gsum=None, rpg=0, dz_off=0,
              x_off=0, dw_off=0, fin=None, pair=None):
        """dw (+ db, gsum) = dz^T x over fixed-order slabs.

        fin: a caller-owned list; the finishing dw (and db) sums are then left to
        finish(fin), which runs all of them in one launch (the workspace rides in
        the list until then).  pair: a pcadv_gemm_desc (an independent data
        gradient) enqueued in the same launch as the slab GEMM.  Nothing is held
        by the library between calls: dropping `fin` abandons the sums."""
        nb = self.lib.pcadv_gemm_wgrad_workspace_bytes(rows, O, K, rpg)
        ws = _ws(nb, dz.device)
        if fin is None and pair is None:
            check(self.lib.pcadv_gemm_wgrad(
                _p(dz, dz_off), ldz, _p(x, x_off), ldx, rows, O, K, _p(dw, dw_off), ldo,
                None if db is None else _p(db), None if gsum is None else _p(gsum), rpg, 0, _p(ws),
                ws.numel(), stream_ptr()), "pcadv_gemm_wgrad")
            return
        d = _lib.WgradDesc(_p(dz, dz_off), ldz, _p(x, x_off), ldx, rows, O, K, _p(dw, dw_off), ldo,
                           None if db is None else _p(db), None if gsum is None else _p(gsum), rpg,
                           0, _p(ws), ws.numel())
        check(self.lib.pcadv_gemm_wgrad_slabs(ctypes.byref(d),
                                              None if pair is None else ctypes.byref(pair),
                                              stream_ptr()), "pcadv_gemm_wgrad_slabs")
        if fin is None:
            check(self.lib.pcadv_wgrad_finish(ctypes.byref(d), 1, stream_ptr()), "pcadv_wgrad_finish")
        else:
            fin.append((d, ws))

    def finish(self, fin):
        """Enqueue the finishing sums of the weight gradients collected in fin
        (one launch); the workspaces are released after it is enqueued (stream
        order keeps them until the launch has read them)."""
        if not fin:
            return
        arr = (_lib.WgradDesc * len(fin))(*[d for d, _ in fin])
        check(self.lib.pcadv_wgrad_finish(arr, len(fin), stream_ptr()), "pcadv_wgrad_finish")
        fin.clear()

    def wgrad_and_gemm(self, fin, wargs, wkw, g):
        """One layer's weight gradient (wgrad(*wargs, **wkw)) and its data gradient
        g (a pcadv_gemm_desc): one paired launch, or two (_PAIR False)."""
        if _PAIR:
            self.wgrad(*wargs, fin=fin, pair=g, **wkw)
        else:
            self.wgrad(*wargs, fin=fin, **wkw)
            self.gemm_run(g)

    def xform_fwd(self, x, ldx, T, y, ldy, C, Npts, k, *, x_off=0):
        """y = x T per cloud (pcadv_cloud_xform_fwd)."""
        check(self.lib.pcadv_cloud_xform_fwd(_p(x, x_off), ldx, _p(T), _p(y), ldy, C, Npts, k,
                                             stream_ptr()), "pcadv_cloud_xform_fwd")

    def xform_bwd(self, dy, lddy, x, ldx, T, C, Npts, k, *, dT=None, accumulate=False, dx=None,
                  lddx=0, add=None, relu_x=False, x_off=0, dx_off=0):
        """dT (+)= x^T dy and / or dx += (dy T^T + add) [x > 0] (pcadv_cloud_xform_bwd)."""
        check(self.lib.pcadv_cloud_xform_bwd(
            _p(dy), lddy, _p(x, x_off), ldx, _p(T), None if dT is None else _p(dT),
            int(accumulate), None if dx is None else _p(dx, dx_off), lddx,
            None if add is None else _p(add), int(relu_x), C, Npts, k, stream_ptr()),
            "pcadv_cloud_xform_bwd")

    def mse_reg(self, T, B0, scale, loss, dT=None, ws=None):
        """loss[0:2] = MSELoss(T T^T, I) of the first B0 clouds and of the rest;
        dT += scale x its gradient (pcadv_tnet_mse_reg).  ws: the call's
        workspace, at least 4 C f32 (the row-block sums of the C clouds, include/
        pcadv.h); a step passes its resident one, else it is allocated here."""
        C, k, _ = T.shape
        if ws is None:
            ws = torch.empty(4 * max(C, 1), device=T.device)
        elif ws.dtype != torch.float32 or ws.numel() < 4 * C:
            raise ValueError(f"mse_reg: workspace of {ws.numel()} elements, needs {4 * C} f32")
        check(self.lib.pcadv_tnet_mse_reg(_p(T), C, B0, k, float(scale), _p(loss),
                                          None if dT is None else _p(dT), _p(ws), stream_ptr()),
              "pcadv_tnet_mse_reg")

    def colsum(self, x, ld, M, N, out, *, ymask=None, ldm=0, x_off=0, m_off=0):
        nb = self.lib.pcadv_colsum_workspace_bytes(M, N)
        ws = _ws(nb, x.device)
        check(self.lib.pcadv_colsum(_p(x, x_off), None if ymask is None else _p(ymask, m_off), ld,
                                    ldm, M, N, _p(out), 0, _p(ws), ws.numel(), stream_ptr()),
              "pcadv_colsum")

    def group_colsum(self, x, ld, M, N, rows_per_group, out, *, ymask=None, ldm=0):
        check(self.lib.pcadv_group_colsum(_p(x), None if ymask is None else _p(ymask), ld, ldm, M,
                                          N, rows_per_group, _p(out), stream_ptr()),
              "pcadv_group_colsum")


_ENGINE = None


# weight gradients' finishing slab sums deferred and run in one launch at the
# end of the backward (False: one launch after each)
_DEFER = True
# each layer's weight and data gradients in one launch (_Engine.pair)
_PAIR = True


def _engine():
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = _Engine()
    return _ENGINE


def _wmat(w):
    return w.reshape(w.shape[0], -1)


def _check_dev(t, name, shape=None, dtype=torch.float32):
    if t.device.type != "cuda":
        raise ValueError(f"{name}: pcadv ops run on the HIP device only (got {t.device})")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def _weight_planes(W, Wf, wplanes=None):
    """(hi, lo) bf16 planes of conv2..conv6 and fc1..fc4, from ``wplanes`` (the
    caller's split of its flat parameter buffer: a list of 20 (hi, lo) pairs in
    state_dict order) or split here."""
    if wplanes is not None:
        return ([None] + [tuple(t.view(W[i].shape) for t in wplanes[2 * i]) for i in range(1, 6)],
                [tuple(t.view(Wf[i].shape) for t in wplanes[12 + 2 * i]) for i in range(4)])
    E = _engine()
    out = []
    for w in W[1:] + Wf:
        hi = torch.empty(w.shape, device=w.device, dtype=torch.bfloat16)
        lo = torch.empty_like(hi)
        E.split(w, hi, lo)
        out.append((hi, lo))
    return [None] + out[:5], out[5:]


def seg_forward(pts, cls, params, wplanes=None, precision="fp32"):
    """PointNetSeg forward (pointnet.py:282-317) on the engine.  Returns a dict
    with logits (B*N, C) point-major, gmax (B, 2048), gidx (B, 2048) and every
    activation the backward needs.  Each layer's epilogue also writes its
    output's bf16 hi / lo planes, which the next layer's GEMM stages as they
    are (no per-tile splitting)."""
    return _forward(pts, cls, params, wplanes, precision)


def segregu_forward(pts, cls, params, wplanes=None, precision="fp32"):
    """PointNetSeg_regulization forward (pointnet.py:226-259) on the engine:
    seg_forward with the two T-Nets spliced in.  params: the 44 parameters in
    state_dict order (stn, fstn, conv1..conv6, fc1..fc4); wplanes likewise.
    The dict also holds T3 (B, 3, 3), trans_feat (B, 128, 128), the
    transformed points and x3 (conv1's and conv4's inputs) and the T-Nets'
    activations.  The T-Nets run on their f32 kernels in both precisions."""
    return _forward(pts, cls, params[_NTN:], None if wplanes is None else wplanes[_NTN:],
                    precision, tn=params[:_NTN])


_NTN = 24  # parameters of stn + fstn, ahead of conv1 in PointNetSeg_regulization's state_dict


def _tnet_forward(x, p, k):
    """STN3d / STNkd (pointnet.py:26-43,59-79) on point-major x (B, N, k) through
    the native point-wise, conv + max and linear ops: T (B, k, k) and the
    activations its backward reads."""
    h1 = ops.pw_fwd(x, p[0], p[1], ops.ACT_RELU)
    h2 = ops.pw_fwd(h1, p[2], p[3], ops.ACT_RELU)
    g, gidx = ops.conv_max_fwd(h2, p[4], p[5], True)
    f1 = ops.linear_fwd(g, p[6], p[7], ops.ACT_RELU)
    f2 = ops.linear_fwd(f1, p[8], p[9], ops.ACT_RELU)
    t = ops.linear_fwd(f2, p[10], p[11], ops.ACT_NONE, add_identity_k=k)
    return t.view(-1, k, k), dict(x=x, h1=h1, h2=h2, g=g, gidx=gidx, f1=f1, f2=f2, t=t, p=list(p))


def _tnet_backward(c, dT, out, need_dx):
    """Gradients of a T-Net's 12 parameters, written into out[0:12], given dL/dT;
    returns dL/dx (B, N, k) when asked."""
    p, k = c["p"], c["x"].shape[2]
    dt = dT.reshape(dT.shape[0], -1)
    df2, _, _ = ops.linear_bwd(dt, c["t"], ops.ACT_NONE, None, 0.0, c["f2"], p[10],
                               dw_out=out[10], db_out=out[11])
    df1, _, _ = ops.linear_bwd(df2, c["f2"], ops.ACT_RELU, None, 0.0, c["f1"], p[8],
                               dw_out=out[8], db_out=out[9])
    dg, _, _ = ops.linear_bwd(df1, c["f1"], ops.ACT_RELU, None, 0.0, c["g"], p[6],
                              dw_out=out[6], db_out=out[7])
    # the ReLU before the max and conv2's own: dz2 comes back masked
    dz2, _, _ = ops.conv_max_bwd(dg, c["gidx"], c["h2"], p[4], gmax_relu=c["g"], dw_out=out[4],
                                 db_out=out[5], dx_relu=True)
    ops.pw_bwd_weight(dz2, None, ops.ACT_NONE, c["h1"], dw_out=out[2], db_out=out[3])
    dh1 = ops.pw_bwd_data(dz2, None, ops.ACT_NONE, _wmat(p[2]), 64)
    ops.pw_bwd_weight(dh1, c["h1"], ops.ACT_RELU, c["x"], dw_out=out[0], db_out=out[1])
    if need_dx:
        return ops.pw_bwd_data(dh1, c["h1"], ops.ACT_RELU, _wmat(p[0]), k)
    return None


def _forward(pts, cls, params, wplanes, precision, tn=None):
    """seg_forward, or with tn (the 24 T-Net parameters) segregu_forward: the
    conv / fc / conv6-max / fc1-split code both share."""
    E = _engine()
    B, N, _ = pts.shape
    M = B * N
    dev = pts.device
    pts = pts.contiguous()
    cvec = cls.reshape(B, -1).contiguous()
    W = [_wmat(params[2 * i]).contiguous() for i in range(6)]
    bc = [params[2 * i + 1].contiguous() for i in range(6)]
    Wf = [params[12 + 2 * i].contiguous() for i in range(4)]
    bf = [params[13 + 2 * i].contiguous() for i in range(4)]
    ncls = Wf[3].shape[0]
    fp32 = _check_precision(precision) == "fp32"
    planes = _PLANES and not fp32  # bf16x3: every forward GEMM staged from bf16 planes
    pf = fp32  # six-product forward GEMMs (staged from f32, split three ways per tile)
    # conv6's screen is three products in both modes (its winners are re-evaluated
    # in exact f32), staged from x5's planes: conv5's epilogue writes them
    c6p = _PLANES
    xloc = torch.empty(M, _LOC, device=dev)
    pl = lambda rows, cols: (torch.empty(rows, cols, device=dev, dtype=torch.bfloat16),  # noqa: E731
                             torch.empty(rows, cols, device=dev, dtype=torch.bfloat16))
    if c6p:
        Wp, Wfp = _weight_planes(W, Wf, wplanes)
    if planes:
        xp = pl(M, _LOC)
        x5p, x5ld, x5off = xp, _LOC, _OFF[4]
    elif c6p:
        x5p, x5ld, x5off = pl(M, 512), 512, 0
    # the input transform (pointnet.py:229-231): conv1 reads p' = pts T3
    pin, tnet = pts, None
    if tn is not None:
        T3, c3 = _tnet_forward(pts, tn[:12], 3)
        pin = torch.empty(M, 3, device=dev)
        E.xform_fwd(pts, 3, T3, pin, 3, B, N, 3)
    # conv1..conv5 + ReLU into the column blocks of xloc
    E.gemm(pin, 3, W[0], 3, xloc, _LOC, M, 64, 3, bias=bc[0], relu=True, c_off=_OFF[0],
           precise=pf, cp=xp if planes else None, ldcp=_LOC, cp_off=_OFF[0])
    for i in range(1, 5):
        K, O = _CONV[i]
        a, lda, a_off, ap = xloc, _LOC, _OFF[i - 1], xp if planes else None
        if i == 3 and tn is not None:
            # the feature transform (pointnet.py:237-239): fstn on a dense copy of x3,
            # conv4 reads x3t = x3 T from its own buffer; xloc keeps x3 for fc1
            x3d = xloc[:, _OFF[2]:_OFF[3]].contiguous().view(B, N, 128)
            T, cf = _tnet_forward(x3d, tn[12:], 128)
            x3t = torch.empty(M, 128, device=dev)
            E.xform_fwd(xloc, _LOC, T, x3t, 128, B, N, 128, x_off=_OFF[2])
            tnet = dict(T3=T3, T=T, c3=c3, cf=cf, pin=pin, x3t=x3t)
            a, lda, a_off = x3t, 128, 0
            if planes:
                ap = pl(M, 128)
                E.split(x3t, *ap)
        if planes:
            E.gemm_bf2(ap, lda, Wp[i], K, xloc, _LOC, M, O, K, bias=bc[i], relu=True,
                       a_off=a_off, c_off=_OFF[i], cp=xp, ldcp=_LOC, cp_off=_OFF[i])
        else:
            last = i == 4 and c6p  # conv5 also writes x5's planes for conv6's screen
            E.gemm(a, lda, W[i], K, xloc, _LOC, M, O, K, bias=bc[i], relu=True,
                   a_off=a_off, c_off=_OFF[i], precise=pf, cp=x5p if last else None,
                   ldcp=x5ld if last else 0)
    # conv6 + ReLU + max over the points of each cloud
    gmax = torch.empty(B, 2048, device=dev)
    gidx = torch.empty(B, 2048, device=dev, dtype=torch.int32)
    nb = E.lib.pcadv_conv_max_x3_workspace_bytes(B, N, 2048)
    ws = _ws(nb, dev)
    if c6p:
        check(E.lib.pcadv_conv_max_bf2(_p(xloc, _OFF[4]), _LOC, _pb(x5p[0], x5off),
                                       _pb(x5p[1], x5off), x5ld, B, N, 512, _p(W[5]),
                                       _pb(Wp[5][0]), _pb(Wp[5][1]), _p(bc[5]), 2048, 1,
                                       _p(gmax), _p(gidx), _p(ws), ws.numel(), stream_ptr()),
              "pcadv_conv_max_bf2")
    else:
        check(E.lib.pcadv_conv_max_x3(_p(xloc, _OFF[4]), _LOC, B, N, 512, _p(W[5]), _p(bc[5]),
                                      2048, 1, _p(gmax), _p(gidx), _p(ws), ws.numel(),
                                      stream_ptr()), "pcadv_conv_max_x3")
    # fc1: per-cloud bias from the tiled global feature and class vector
    W1 = Wf[0]
    cb = torch.empty(B, 256, device=dev)
    E.gemm(gmax, 2048, W1, 3024, cb, 256, B, 256, 2048, bias=bf[0], b_off=960,
           precise=pf)
    E.gemm(cvec, cvec.shape[1], W1, 3024, cb, 256, B, 256, cvec.shape[1], b_off=3008,
           accumulate=True)
    h1 = torch.empty(M, 256, device=dev)
    h2 = torch.empty(M, 256, device=dev)
    h3 = torch.empty(M, 128, device=dev)
    logits = torch.empty(M, ncls, device=dev)
    if planes:
        h1p, h2p, h3p = pl(M, 256), pl(M, 256), pl(M, 128)
        E.gemm_bf2(xp, _LOC, Wfp[0], 3024, h1, 256, M, 256, _LOC, bias_rows=cb,
                   rows_per_group=N, relu=True, cp=h1p, ldcp=256)
        E.gemm_bf2(h1p, 256, Wfp[1], 256, h2, 256, M, 256, 256, bias=bf[1], relu=True, cp=h2p,
                   ldcp=256)
        E.gemm_bf2(h2p, 256, Wfp[2], 256, h3, 128, M, 128, 256, bias=bf[2], relu=True, cp=h3p,
                   ldcp=128)
        E.gemm_bf2(h3p, 128, Wfp[3], 128, logits, ncls, M, ncls, 128, bias=bf[3])
    else:
        E.gemm(xloc, _LOC, W1, 3024, h1, 256, M, 256, _LOC, bias_rows=cb, rows_per_group=N,
               relu=True, precise=pf)
        E.gemm(h1, 256, Wf[1], 256, h2, 256, M, 256, 256, bias=bf[1], relu=True,
               precise=pf)
        E.gemm(h2, 256, Wf[2], 256, h3, 128, M, 128, 256, bias=bf[2], relu=True,
               precise=pf)
        E.gemm(h3, 128, Wf[3], 128, logits, ncls, M, ncls, 128, bias=bf[3], precise=pf)
    return dict(pts=pts, cvec=cvec, xloc=xloc, gmax=gmax, gidx=gidx, h1=h1, h2=h2, h3=h3, W=W,
                Wf=Wf, logits=logits, dims=(B, N, ncls), xp=xp if planes else None,
                precision=precision, x5p=(x5p, x5ld, x5off) if c6p else None,
                W6p=Wp[5] if c6p else None, tnet=tnet)


def seg_backward(fw, dlogits, dgmax_out=None, out=None):
    """Gradients of the 20 parameters (state_dict order) given dL/dlogits
    (B*N, C) (and optionally dL/dgmax), from the activations of seg_forward.
    `out`: optional list of 20 parameter-shaped tensors written in place."""
    return _backward(fw, dlogits, dgmax_out, out)


def segregu_backward(fw, dlogits, dgmax_out=None, out=None, reg=None):
    """Gradients of the 44 parameters (state_dict order) from the activations
    of segregu_forward.  reg(T, dT): called once dT (B, 128, 128) holds the
    transform's own gradient, to add what else reaches trans_feat (the
    orthogonality regulariser, or an upstream gradient), before fstn's
    backward reads it.

    The gradient at x3 has three consumers: fc1 (the concatenated features),
    the transform x3 T and fstn.  fc1's part lands in dloc's x3 block masked
    by its GEMM as before; the other two are summed by pcadv_cloud_xform_bwd
    (fstn's input gradient rides in as `add`) and masked once as they are
    accumulated there."""
    return _backward(fw, dlogits, dgmax_out, out, reg=reg, regu=True)


def _backward(fw, dlogits, dgmax_out, out, reg=None, regu=False):
    E = _engine()
    tn = fw.get("tnet")
    if regu != (tn is not None):
        raise ValueError("the activations are not this generator's forward's")
    o0 = _NTN if regu else 0  # conv1.weight's place in `out`
    if regu and out is None:
        out = [torch.empty_like(q) for q in tn["c3"]["p"] + tn["cf"]["p"]] + [None] * 20
    pts, cvec, xloc, gmax, gidx = fw["pts"], fw["cvec"], fw["xloc"], fw["gmax"], fw["gidx"]
    h1, h2, h3, W, Wf = fw["h1"], fw["h2"], fw["h3"], fw["W"], fw["Wf"]
    B, N, ncls = fw["dims"]
    M = B * N
    dev = xloc.device
    pd = fw.get("precision", "fp32") == "fp32"  # six-product data gradients
    dl = torch.zeros(M, ncls, device=dev) if dlogits is None else dlogits.reshape(M, ncls).contiguous()
    # Every data-gradient GEMM applies the relu' of the layer below in its
    # epilogue (cmask), so each dz is stored masked once and read as is by the
    # weight gradient (which also forms the bias gradient) and the next GEMM.
    def _g(k, like):  # the k-th gradient (state_dict order): caller's buffer or a new one
        if out is not None and out[o0 + k] is not None:
            return out[o0 + k].view(like.shape) if hasattr(like, "shape") else out[o0 + k]
        return torch.empty_like(like) if hasattr(like, "shape") else torch.empty(like, device=dev)
    # the weight gradients' finishing slab sums wait in this local list and run
    # in one launch at the end (E.finish); an exception drops the list and
    # nothing is left behind (the library holds no state between calls)
    fin = [] if _DEFER else None
    # ---- fc4 .. fc2 -------------------------------------------------------
    dW4 = _g(18, Wf[3]); db4 = _g(19, ncls)
    dh3 = torch.empty(M, 128, device=dev)
    E.wgrad_and_gemm(fin, (dl, ncls, h3, 128, M, ncls, 128, dW4, 128), dict(db=db4),
                     E.gemm_desc(dl, ncls, Wf[3], 128, dh3, 128, M, 128, ncls, tb=1, cmask=h3,
                                 ldm=128, precise=pd))
    dW3 = _g(16, Wf[2]); db3 = _g(17, 128)
    dh2 = torch.empty(M, 256, device=dev)
    E.wgrad_and_gemm(fin, (dh3, 128, h2, 256, M, 128, 256, dW3, 256), dict(db=db3),
                     E.gemm_desc(dh3, 128, Wf[2], 256, dh2, 256, M, 256, 128, tb=1, cmask=h2,
                                 ldm=256, precise=pd))
    dW2 = _g(14, Wf[1]); db2 = _g(15, 256)
    dh1 = torch.empty(M, 256, device=dev)
    E.wgrad_and_gemm(fin, (dh2, 256, h1, 256, M, 256, 256, dW2, 256), dict(db=db2),
                     E.gemm_desc(dh2, 256, Wf[1], 256, dh1, 256, M, 256, 256, tb=1, cmask=h1,
                                 ldm=256, precise=pd))
    # ---- fc1: local columns (+ per-cloud sums s1), then the tiled columns --
    W1 = Wf[0]
    dW1 = _g(12, W1); db1 = _g(13, 256)
    s1 = torch.empty(B, 256, device=dev)  # per-cloud sums of dz1
    dloc = torch.empty(M, _LOC, device=dev)
    E.wgrad_and_gemm(fin, (dh1, 256, xloc, _LOC, M, 256, _LOC, dW1, 3024),
                     dict(db=db1, gsum=s1, rpg=N),
                     E.gemm_desc(dh1, 256, W1, 3024, dloc, _LOC, M, _LOC, 256, tb=1, cmask=xloc,
                                 ldm=_LOC, precise=pd))
    # the tiled global and class columns: B per-cloud rows, exact f32, one launch
    check(E.lib.pcadv_wgrad_small(_p(s1), 256, B, 256, _p(gmax), 2048, 2048, _p(dW1, 960),
                                  _p(cvec), cvec.shape[1], cvec.shape[1], _p(dW1, 3008), 3024,
                                  0, stream_ptr()), "pcadv_wgrad_small")
    dg = torch.empty(B, 2048, device=dev)
    E.gemm(s1, 256, W1, 3024, dg, 2048, B, 2048, 256, tb=1, b_off=960, precise=pd)
    if dgmax_out is not None:
        dg += dgmax_out.reshape(B, 2048)
    # ---- conv6 + ReLU + max: the gradient reaches the argmax points -------
    dW6 = _g(10, W[5]); db6 = _g(11, 2048)
    check(E.lib.pcadv_conv_max_x3_bwd(_p(dg), _p(gmax), _p(gidx), _p(xloc, _OFF[4]), _LOC, B,
                                      N, 2048, 512, _p(W[5]), _p(dW6), _p(db6),
                                      _p(dloc, _OFF[4]), _LOC, 1, stream_ptr()),
          "pcadv_conv_max_x3_bwd")
    # ---- conv5 .. conv1 (each layer's output gradient also carries fc1's) --
    dWc = [None] * 6
    dbc = [None] * 6
    dWc[5], dbc[5] = dW6, db6
    for i in range(4, -1, -1):
        K, O = _CONV[i]
        dWc[i] = _g(2 * i, W[i])
        dbc[i] = _g(2 * i + 1, O)
        if i == 3 and regu:
            # conv4 read x3t: its data gradient goes to dx3t (no mask, nothing to add to)
            x3t, T = tn["x3t"], tn["T"]
            dx3t = torch.empty(M, 128, device=dev)
            E.wgrad_and_gemm(fin, (dloc, _LOC, x3t, 128, M, O, K, dWc[i], K),
                             dict(db=dbc[i], dz_off=_OFF[i]),
                             E.gemm_desc(dloc, _LOC, W[i], K, dx3t, 128, M, K, O, tb=1,
                                         precise=pd, a_off=_OFF[i]))
            dT = torch.empty(B, 128, 128, device=dev)
            E.xform_bwd(dx3t, 128, xloc, _LOC, T, B, N, 128, dT=dT, x_off=_OFF[2])
            if reg is not None:
                reg(T, dT)
            dx3f = _tnet_backward(tn["cf"], dT, out[12:24], True)
            E.xform_bwd(dx3t, 128, xloc, _LOC, T, B, N, 128, dx=dloc, lddx=_LOC, add=dx3f,
                        relu_x=True, x_off=_OFF[2], dx_off=_OFF[2])
        elif i > 0:
            E.wgrad_and_gemm(fin, (dloc, _LOC, xloc, _LOC, M, O, K, dWc[i], K),
                             dict(db=dbc[i], dz_off=_OFF[i], x_off=_OFF[i - 1]),
                             E.gemm_desc(dloc, _LOC, W[i], K, dloc, _LOC, M, K, O, tb=1,
                                         cmask=xloc, ldm=_LOC, accumulate=True,
                                         precise=pd, a_off=_OFF[i],
                                         m_off=_OFF[i - 1], c_off=_OFF[i - 1]))
        elif regu:
            # conv1 read p' = pts T3: dp' = dz1 W1, then dT3 and stn's backward
            E.wgrad(dloc, _LOC, tn["pin"], 3, M, O, K, dWc[i], K, db=dbc[i], dz_off=_OFF[i],
                    fin=fin)
            dpin = torch.empty(M, 3, device=dev)
            E.gemm(dloc, _LOC, W[0], 3, dpin, 3, M, 3, 64, tb=1, a_off=_OFF[0], precise=pd)
            dT3 = torch.empty(B, 3, 3, device=dev)
            E.xform_bwd(dpin, 3, pts, 3, tn["T3"], B, N, 3, dT=dT3)
            _tnet_backward(tn["c3"], dT3, out[0:12], False)
        else:
            E.wgrad(dloc, _LOC, pts, 3, M, O, K, dWc[i], K, db=dbc[i], dz_off=_OFF[i], fin=fin)
    # every weight gradient's slab sums (collected above) in one launch
    if fin is not None:
        E.finish(fin)
    grads = []
    for i in range(6):
        grads += [dWc[i].view(O_shape(i)), dbc[i]]
    grads += [dW1, db1, dW2, db2, dW3, db3, dW4, db4]
    if regu:
        grads = [g.view(q.shape) for g, q in zip(out[:_NTN], tn["c3"]["p"] + tn["cf"]["p"])] + grads
    return grads


class SegNetFunction(torch.autograd.Function):
    """PointNetSeg forward and its whole backward as one autograd node.

    Inputs: pts (B, N, 3), cls (B, 1, 16), then the 20 parameters in state_dict
    order.  Outputs: logits point-major (B, N, C), gmax (B, 2048), gidx (B, 2048)
    int32 (argmax over points, non-differentiable)."""

    @staticmethod
    def forward(ctx, precision, pts, cls, *params):
        fw = seg_forward(pts, cls, params, precision=precision)
        ctx.precision = precision
        ctx.save_for_backward(fw["pts"], fw["cvec"], fw["xloc"], fw["gmax"], fw["gidx"], fw["h1"],
                              fw["h2"], fw["h3"], *fw["W"], *fw["Wf"])
        ctx.dims = fw["dims"]
        ctx.mark_non_differentiable(fw["gidx"])
        B, N, ncls = fw["dims"]
        return fw["logits"].view(B, N, ncls), fw["gmax"], fw["gidx"]

    @staticmethod
    def backward(ctx, dlogits, dgmax_out, _dgidx):
        t = ctx.saved_tensors
        fw = dict(pts=t[0], cvec=t[1], xloc=t[2], gmax=t[3], gidx=t[4], h1=t[5], h2=t[6], h3=t[7],
                  W=list(t[8:14]), Wf=list(t[14:18]), dims=ctx.dims, precision=ctx.precision)
        B, N, ncls = ctx.dims
        dl = None if dlogits is None else dlogits.reshape(B * N, ncls)
        return (None, None, None, *seg_backward(fw, dl, dgmax_out))


# what segregu_backward reads of segregu_forward's dict, its "tnet" entry and a
# T-Net's cache (SegReguNetFunction saves and rebuilds them in this order)
_FW_KEYS = ("pts", "cvec", "xloc", "gmax", "gidx", "h1", "h2", "h3")
_TN_KEYS = ("T3", "T", "pin", "x3t")
_TC_KEYS = ("x", "h1", "h2", "g", "gidx", "f1", "f2", "t")


class SegReguNetFunction(torch.autograd.Function):
    """PointNetSeg_regulization forward and its whole backward as one autograd
    node.  Inputs: pts (B, N, 3), cls (B, 1, 16), then the 44 parameters in
    state_dict order.  Outputs: logits point-major (B, N, C), gmax (B, 2048),
    gidx (B, 2048) int32 and T3 (B, 3, 3) (both non-differentiable), trans_feat
    (B, 128, 128) (differentiable: the regulariser's gradient joins the
    transform's own before fstn's backward)."""

    @staticmethod
    def forward(ctx, precision, pts, cls, *params):
        fw = segregu_forward(pts, cls, [p.detach() for p in params], precision=precision)
        tn = fw["tnet"]
        # every tensor the backward reads goes through save_for_backward, flattened
        # (some are outputs: kept on ctx directly they would tie the node to its
        # own outputs and nothing would ever be freed); only metadata stays on ctx
        ctx.save_for_backward(*[fw[n] for n in _FW_KEYS], *fw["W"], *fw["Wf"],
                              *[tn[n] for n in _TN_KEYS],
                              *[t for c in (tn["c3"], tn["cf"])
                                for t in [c[n] for n in _TC_KEYS] + c["p"]])
        ctx.dims, ctx.precision = fw["dims"], precision
        ctx.mark_non_differentiable(fw["gidx"], tn["T3"])
        B, N, ncls = fw["dims"]
        return fw["logits"].view(B, N, ncls), fw["gmax"], fw["gidx"], tn["T3"], tn["T"]

    @staticmethod
    def backward(ctx, dlogits, dgmax_out, _dgidx, _dT3, dtrans):
        t = list(ctx.saved_tensors)
        take = lambda n: [t.pop(0) for _ in range(n)]  # noqa: E731
        fw = dict(zip(_FW_KEYS, take(len(_FW_KEYS))), W=take(6), Wf=take(4), dims=ctx.dims,
                  precision=ctx.precision)
        tn = dict(zip(_TN_KEYS, take(len(_TN_KEYS))))
        for name in ("c3", "cf"):
            tn[name] = dict(zip(_TC_KEYS, take(len(_TC_KEYS))), p=take(12))
        fw["tnet"] = tn
        B, N, ncls = fw["dims"]
        dl = None if dlogits is None else dlogits.reshape(B * N, ncls)
        reg = None if dtrans is None else (lambda T, dT: dT.add_(dtrans))
        return (None, None, None, *segregu_backward(fw, dl, dgmax_out, reg=reg))


def O_shape(i):
    K, O = _CONV[i]
    return (O, K, 1)


def seg_cross_entropy(logits_pm, seg, scale=1.0):
    """CrossEntropyLoss()(pred (B, C, N), seg (B, N)) for point-major logits
    (B, N, C): the mean over all points (pointnet/train_pointnet_seg.py:152,
    utils/trainer.py:344), on the device."""
    return _RowCE.apply(logits_pm, seg, float(scale))


class _RowCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_pm, seg, scale):
        lib = _lib.load()
        B, N, C = logits_pm.shape
        M = B * N
        lg = logits_pm.reshape(M, C).contiguous()
        _check_dev(lg, "logits")
        lab = seg.reshape(M).to(torch.int64).contiguous()
        _check_dev(lab, "seg", dtype=torch.int64)
        loss = torch.empty((), device=lg.device)
        d = torch.empty_like(lg)
        ws = _ws(lib.pcadv_row_ce_workspace_bytes(M), lg.device)
        check(lib.pcadv_row_ce(_p(lg), C, _p(lab), M, C, 1.0, _p(loss), _p(d), _p(ws), ws.numel(),
                               stream_ptr()), "pcadv_row_ce")
        ctx.save_for_backward(d)
        ctx.shape = (B, N, C)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (d,) = ctx.saved_tensors
        return (d * gl).view(ctx.shape), None, None


class PointNetSeg(nn.Module):
    """models/pointnet.py:261-317.  forward(x: B x N x 3, cls: B x 1 x 16) ->
    (logits B x NUM_SEG_CLASSES x N, x_global B x 2048 x 1)."""

    def __init__(self, NUM_SEG_CLASSES, *, precision="fp32"):
        super().__init__()
        self.output_dim = NUM_SEG_CLASSES
        # "fp32" (the reference's dtype) or "bf16x3" (labelled speed option)
        self.precision = _check_precision(precision)
        self.conv1 = nn.Conv1d(3, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 128, 1)
        self.conv4 = nn.Conv1d(128, 128, 1)
        self.conv5 = nn.Conv1d(128, 512, 1)
        self.conv6 = nn.Conv1d(512, 2048, 1)
        self.fc1 = nn.Linear(3024, 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, 128)
        self.fc4 = nn.Linear(128, self.output_dim)

    def forward_points(self, x, cls):
        """Point-major logits (B, N, C), x_global (B, 2048), argmax (B, 2048)."""
        B, N, c3 = x.shape
        if c3 != 3:
            raise ValueError(f"x: expected B x N x 3, got {tuple(x.shape)}")
        if cls.numel() != B * 16:
            raise ValueError(f"cls: expected B x 1 x 16, got {tuple(cls.shape)}")
        _check_dev(x, "x")
        params = [p for _, p in self.named_parameters()]
        return SegNetFunction.apply(self.precision, x.float().contiguous(),
                                    cls.float().reshape(B, 1, 16), *params)

    def forward(self, x, cls):
        logits, g, _ = self.forward_points(x, cls)
        return logits.permute(0, 2, 1), g.unsqueeze(2)


class PointNetSeg_regulization(nn.Module):
    """models/pointnet.py:205-259: PointNetSeg with an STN3d on the points and an
    STNkd(128) on conv3's output.  forward(x: B x N x 3, cls: B x 1 x 16) ->
    (logits B x NUM_SEG_CLASSES x N, x_global B x 2048 x 1, trans_feat B x 128 x
    128).  Not a PointNetSeg by type: the steps written for that generator
    would run this one without its T-Nets.  Under precision="bf16x3" the T-Nets
    and the two transforms stay on their f32 kernels."""

    def __init__(self, NUM_SEG_CLASSES, *, precision="fp32"):
        super().__init__()
        self.output_dim = NUM_SEG_CLASSES
        self.precision = _check_precision(precision)
        self.stn = STN3d()
        self.fstn = STNkd(k=128)
        self.conv1 = nn.Conv1d(3, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 128, 1)
        self.conv4 = nn.Conv1d(128, 128, 1)
        self.conv5 = nn.Conv1d(128, 512, 1)
        self.conv6 = nn.Conv1d(512, 2048, 1)
        self.fc1 = nn.Linear(3024, 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, 128)
        self.fc4 = nn.Linear(128, self.output_dim)

    def forward_points(self, x, cls):
        """Point-major logits (B, N, C), x_global (B, 2048), argmax (B, 2048), the
        input transform T3 (B, 3, 3) and trans_feat (B, 128, 128)."""
        B, N, c3 = x.shape
        if c3 != 3:
            raise ValueError(f"x: expected B x N x 3, got {tuple(x.shape)}")
        if cls.numel() != B * 16:
            raise ValueError(f"cls: expected B x 1 x 16, got {tuple(cls.shape)}")
        _check_dev(x, "x")
        params = [p for _, p in self.named_parameters()]
        return SegReguNetFunction.apply(self.precision, x.float().contiguous(),
                                        cls.float().reshape(B, 1, 16), *params)

    def forward(self, x, cls):
        logits, g, _, _, trans_feat = self.forward_points(x, cls)
        return logits.permute(0, 2, 1), g.unsqueeze(2), trans_feat


class _SegStep(FusedStep):
    """What the two PointNetSeg steps share: lr / betas / eps as attributes (the
    discriminator's with a _D suffix), the generator's flat state (param, grad,
    m, v, grad_views, params, step_count) with the bf16 hi / lo planes of all
    its parameters (one split per step feeds every forward GEMM's weight
    operand), a discriminator's flat state under its own step counter, and one
    pcadv_adam launch per network."""

    def __init__(self, model, optimizers, hyper, device, precision, keep_activations,
                 model_D=None):
        # the model's precision unless given ("fp32" / "bf16x3")
        self.precision = _check_precision(precision or getattr(model, "precision", "fp32"))
        super().__init__(device, optimizers, hyper)
        # keep_activations: hold the last step's forward tensors in self.fw (for
        # inspection / tests); off by default, so a step's per-point activations
        # (hundreds of MB at B=16, N=2048) are released when it returns
        self.keep_activations = bool(keep_activations)
        self.fw = None
        dev, self.model = self.device, model
        G = FlatAdam(model, optimizers[0], dev)
        self.param, self.grad, self.m, self.v = G.param, G.grad, G.m, G.v
        self.grad_views, self.params, self.numel = G.grad_views, G.params, G.numel
        self.step_count = torch.full((1,), G.t0, device=dev, dtype=torch.int32)
        self.wph = torch.empty(G.numel, device=dev, dtype=torch.bfloat16)
        self.wpl = torch.empty(G.numel, device=dev, dtype=torch.bfloat16)
        self.wplanes = [(self.wph[o:o + p.numel()], self.wpl[o:o + p.numel()])
                        for p, o in zip(G.params, G.offsets)]
        self.nets, self.counts = (G,), (self.step_count,)
        if model_D is not None:
            self.model_D = model_D
            D = FlatAdam(model_D, optimizers[1], dev)
            self.d_param, self.d_grad, self.d_m, self.d_v = D.param, D.grad, D.m, D.v
            self.d_grad_views, self.d_params, self.d_numel = D.grad_views, D.params, D.numel
            self.step_count_D = torch.full((1,), D.t0, device=dev, dtype=torch.int32)
            self.nets, self.counts = (G, D), (self.step_count, self.step_count_D)

    def _store_hyper(self, k, lr, betas, eps):
        s = "_D" if k else ""
        setattr(self, "lr" + s, lr)
        setattr(self, "betas" + s, betas)
        setattr(self, "eps" + s, eps)

    def _adam(self, k, lr, betas, eps):
        f = self.nets[k]
        check(self.lib.pcadv_adam(_p(f.param), _p(f.grad), _p(f.m), _p(f.v), f.numel,
                                  _p(self.counts[k]), lr, betas[0], betas[1], eps, stream_ptr()),
              "pcadv_adam")


class SegTrainStep(_SegStep):
    """One iteration of run_training_pointnet_seg (utils/trainer.py:334-349:
    forward, CrossEntropyLoss over every point, (lambda_seg * l).backward(),
    optimizer.step() with Adam) as native launches on one stream, capturable
    into a HIP graph.

    The model's parameters become views of one flat f32 buffer, their .grad
    views of one flat gradient buffer (written in place by the backward), and
    the Adam moments are flat too (handed to a torch Adam's state as views, so
    optimizer.state_dict() stays meaningful); the update is one pcadv_adam
    launch over the whole network."""

    def __init__(self, model, optimizer=None, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 lambda_seg=1.0, device="cuda", keep_activations=False, precision=None):
        super().__init__(model, (optimizer,), [(lr, betas, eps)], device, precision,
                         keep_activations)
        self.lambda_seg = float(lambda_seg)
        self.loss = torch.zeros((), device=self.device)
        self.graph = None

    def __call__(self, pts, cls, seg, apply_adam=True):
        B, N, _ = pts.shape
        _check_dev(pts, "pts")
        if seg.shape != (B, N) or seg.dtype != torch.int64 or not seg.is_contiguous():
            raise ValueError("seg: expected contiguous int64 (B, N)")
        wpl = None
        if _PLANES:  # every weight's planes (fp32 mode reads conv6's only)
            _engine().split(self.param, self.wph, self.wpl)
            wpl = self.wplanes
        fw = seg_forward(pts, cls.float().reshape(B, 1, 16), self.params, wplanes=wpl,
                         precision=self.precision)
        if self.keep_activations:
            self.fw = fw  # the last step's activations (logits, x_global, argmax, ...)
        M, ncls = B * N, fw["dims"][2]
        d = torch.empty(M, ncls, device=self.device)
        ws = _ws(self.lib.pcadv_row_ce_workspace_bytes(M), self.device)
        check(self.lib.pcadv_row_ce(_p(fw["logits"]), ncls, _p(seg), M, ncls, self.lambda_seg,
                                    _p(self.loss), _p(d), _p(ws), ws.numel(), stream_ptr()),
              "pcadv_row_ce")
        seg_backward(fw, d, None, out=self.grad_views)
        if apply_adam:
            self.adam()
        return self.loss

    def adam(self):
        self._adam(0, self.lr, self.betas, self.eps)

    def capture_on(self, pts, cls, seg):
        """A HIP graph of one step reading the given resident buffers (state is
        restored to what it was before the warm-up)."""
        def body():
            self(pts, cls, seg)
        return self._capture(body, body)

    @property
    def losses(self):
        """The loss as a 1-vector (the trainers' loss-ring interface)."""
        return self.loss.view(1)


class _SegDiscStep(_SegStep):
    """What the two adversarial PointNetSeg steps share (SegAdvTrainStep with
    PointwiseDiscNet, SegStackTrainStep with StackDiscNet): one iteration with
    ImagePool(0) and two Adams as native launches on one stream, capturable
    into a HIP graph:

      weight-plane split; seg_forward on the 2B clouds [GT; no-GT] (PointNetSeg
      has no batch statistics: the reference's two forwards); pcadv_row_ce on the
      GT rows (dlogits rows [0, B N), scale lambda_seg); the subclass's _disc:
      the fused D forward on softmax(GT) / log_softmax(no-GT) with its losses
      and their derivatives, and the fused D backward (D's gradients, and the
      no-GT rows of dlogits from lambda_adv loss_adv through the frozen D);
      seg_backward; the two Adam updates.

    Parameters, gradients and Adam moments of G and of D are flat buffers handed
    to the torch modules and optimizers as views.  D always runs in f32;
    `precision` is the generator's.  Soft labels: explicit (soft_gt / soft_nogt,
    one per point) or drawn on the device keyed by (seed, the generator's step
    counter, row), the same draws in both steps for the same seed.

    A subclass names its discriminator class and workspace function, implements
    _disc and `losses`, and keeps its own terms in loss_buf[3:]."""

    _D_NET = _d_workspace = None
    _G_NET = PointNetSeg  # the generator's class

    def __init__(self, model, model_D, optimizer, optimizer_D, lambda_seg, lambda_adv, lr, lr_D,
                 betas, eps, device, precision, seed, keep_activations):
        if not isinstance(model, self._G_NET) or not isinstance(model_D, self._D_NET):
            raise TypeError(f"{type(self).__name__}: expected a {self._G_NET.__name__} and a "
                            f"{self._D_NET.__name__}")
        if model_D.input_dim != model.output_dim:
            raise ValueError(f"model_D takes {model_D.input_dim} channels, the generator predicts "
                             f"{model.output_dim} classes")
        super().__init__(model, (optimizer, optimizer_D), [(lr, betas, eps), (lr_D, betas, eps)],
                         device, precision, keep_activations, model_D)
        self.lambda_seg, self.lambda_adv, self.seed = float(lambda_seg), float(lambda_adv), int(seed)
        # [loss_seg, loss_adv, loss_D, loss_D's GT part, its no-GT part, the subclass's term]
        self.loss_buf = torch.zeros(6, device=self.device)
        self.d_out = None
        self._ws = None

    def __call__(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt=None, soft_nogt=None,
                 apply_adam=True, semi=False):
        self._run(pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt, apply_adam, semi)
        return self.losses

    def _run(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt, apply_adam,
             semi=False):
        """The step's launches and nothing else: what capture_on captures (reading
        `losses` may launch, so it stays with __call__)."""
        B, N, _ = pts_gt.shape
        _check_dev(pts_gt, "pts_gt")
        _check_dev(pts_nogt, "pts_nogt", shape=(B, N, 3))
        if seg.shape != (B, N) or seg.dtype != torch.int64 or not seg.is_contiguous():
            raise ValueError("seg: expected contiguous int64 (B, N)")
        pts = torch.cat([pts_gt, pts_nogt])
        cls = torch.cat([cls_gt.float().reshape(B, 1, 16), cls_nogt.float().reshape(B, 1, 16)])
        self._run_packed(pts, cls, seg, soft_gt, soft_nogt, apply_adam, semi)

    def _run_packed(self, pts, cls, seg, soft_gt=None, soft_nogt=None, apply_adam=True,
                    semi=False):
        """_run on the step's packed input, as dataset.gather_seg_pair writes it:
        pts (2B, N, 3) and cls (2B, 1, 16) f32 with the GT batch in rows [0, B)
        and the no-GT batch in rows [B, 2B), seg (B, N) int64.  _run is the two
        concatenations and this."""
        B, N = seg.shape
        _check_dev(pts, "pts", shape=(2 * B, N, 3))
        _check_dev(cls, "cls", shape=(2 * B, 1, 16))
        if seg.dtype != torch.int64 or not seg.is_contiguous():
            raise ValueError("seg: expected contiguous int64 (B, N)")
        if self.model_D.fills_rows and (B * N) % self.model_D.input_pts:
            raise ValueError(f"{B} x {N} points do not fill rows of model_D.input_pts = "
                             f"{self.model_D.input_pts}")
        if semi and self.model_D.fills_rows and self.model_D.input_pts != N:
            raise ValueError(f"semi=True: model_D.input_pts = {self.model_D.input_pts} is not the "
                             f"clouds' {N} points (the reference's mask indexes (B, N))")
        M = B * N
        wpl = None
        if _PLANES:  # every weight's planes (fp32 mode reads conv6's only)
            _engine().split(self.param, self.wph, self.wpl)
            wpl = self.wplanes
        cls_gt = cls[:B]
        fw = self._g_forward(pts, cls, wpl)
        ncls = fw["dims"][2]
        logits = fw["logits"]
        d = torch.empty(2 * M, ncls, device=self.device)
        ws = _ws(self.lib.pcadv_row_ce_workspace_bytes(M), self.device)
        check(self.lib.pcadv_row_ce(_p(logits), ncls, _p(seg), M, ncls, self.lambda_seg,
                                    _p(self.loss_buf), _p(d), _p(ws), ws.numel(), stream_ptr()),
              "pcadv_row_ce")
        if self._ws is None or self._ws[0] != M:
            self._ws = (M, self._d_workspace(2 * M, self.device))
        d_out = self._disc(logits, ncls, M, N, cls_gt, d, self._ws[1],
                           None if soft_gt is None else soft_gt.reshape(M),
                           None if soft_nogt is None else soft_nogt.reshape(M), semi)
        self._g_backward(fw, d)
        if self.keep_activations:
            self.fw, self.d_out = fw, d_out
        if apply_adam:
            self.adam()

    def _disc(self, logits, ncls, M, N, cls_gt, d, dws, soft0, soft1, semi):
        """D's fused forward and backward on logits' 2M rows: loss_buf[1:] and D's
        gradients written, the no-GT rows of d filled.  Returns D's output."""
        raise NotImplementedError

    def _g_forward(self, pts, cls, wpl):
        """The generator's forward on the 2B clouds [GT; no-GT]."""
        return seg_forward(pts, cls, self.params, wplanes=wpl, precision=self.precision)

    def _g_backward(self, fw, d):
        """The generator's backward from dlogits into the flat gradient views."""
        seg_backward(fw, d, None, out=self.grad_views)

    def adam(self):
        """optimizer.step() and optimizer_D.step() (trainer.py:965-966, 1152-1153)."""
        self._adam(0, self.lr, self.betas, self.eps)
        self._adam(1, self.lr_D, self.betas_D, self.eps_D)

    def capture_on(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt=None, soft_nogt=None,
                   semi=False):
        """One HIP graph of a step reading the given resident buffers: a single
        stream, no parallel branches (state is restored to what it was before
        the warm-up).  `semi` is baked into the graph."""
        def body():
            self._run(pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt, True, semi)
        return self._capture(body, body)

    def logged(self, with_semi=False):
        """The last step's losses in the order of its loop's log line, as floats
        (the loops' one host read per iteration).  The stacked step raises here
        what BCELoss raises in the eager body."""
        return (self.losses_semi if with_semi else self.losses).tolist()


class SegAdvTrainStep(_SegDiscStep):
    """One iteration of run_training_seg (utils/trainer.py:873-966) with
    PointNetSeg + PointwiseDiscNet; the launches are _SegDiscStep's, with the
    fused D forward on softmax(GT) / log_softmax(no-GT) (trainer.py:901,914)
    giving loss_adv, loss_D and their derivatives.

    The no-GT rows feed the adversarial term and D's own term from one forward
    (D is frozen in the first and its input detached in the second, so the three
    reference forwards compute the same values).

    semi=True adds run_training_seg_semi's term (utils/trainer.py:1999-2024):
    after the D backward, pcadv_row_semi_ce on the no-GT rows adds lambda_semi
    times the cross entropy of the points whose D output is above semi_th
    against their own argmax to those rows of dlogits (D receives nothing from
    it).  It needs model_D.input_pts == N, as the reference's mask does.  The
    term's loss and the number of kept points are `losses_semi[2]` and `kept`;
    `losses` stays [loss_seg, loss_adv, loss_D].  A captured graph has `semi`
    baked in: capture one graph per value."""

    _D_NET, _d_workspace = PointwiseDiscNet, staticmethod(pwdisc_workspace)

    def __init__(self, model, model_D, optimizer=None, optimizer_D=None, lambda_seg=1.0,
                 lambda_adv=0.01, lr=1e-4, lr_D=1e-4, betas=(0.9, 0.999), eps=1e-8, device="cuda",
                 precision=None, seed=0, keep_activations=False, lambda_semi=1.0, semi_th=0.8):
        super().__init__(model, model_D, optimizer, optimizer_D, lambda_seg, lambda_adv, lr, lr_D,
                         betas, eps, device, precision, seed, keep_activations)
        self.lambda_semi, self.semi_th = float(lambda_semi), float(semi_th)
        self.kept_buf = torch.zeros(1, device=self.device, dtype=torch.int32)  # loss_buf[5]: semi
        self._semi_idx = torch.tensor([0, 1, 5, 2], device=self.device)  # the semi log line's order
        self.semi_labels = None
        self._semi_stale = False

    def _disc(self, logits, ncls, M, N, cls_gt, d, dws, soft0, soft1, semi):
        out = torch.empty(2 * M, device=self.device)
        argc = torch.empty(2 * M, device=self.device, dtype=torch.int32)
        dout_d = torch.empty(2 * M, device=self.device)
        dout_adv = torch.empty(M, device=self.device)
        pwdisc_forward(logits, ncls, M, M, PWD_SOFTMAX, PWD_LOG_SOFTMAX, self.d_params, out, argc,
                       dws, losses=self.loss_buf[1:5], soft0=soft0, soft1=soft1, seed=self.seed,
                       step_count=self.step_count, dout_d=dout_d, dout_adv=dout_adv)
        pwdisc_backward(logits, ncls, M, M, PWD_SOFTMAX, PWD_LOG_SOFTMAX, self.d_params, out, argc,
                        dws, dout_d, self.d_grad_views, dout_adv=dout_adv,
                        lambda_adv=self.lambda_adv, dlogits=d)
        labels = None
        if semi:
            if self.keep_activations:
                labels = torch.empty(M, device=self.device, dtype=torch.int32)
            sws = _ws(self.lib.pcadv_row_semi_ce_workspace_bytes(M), self.device)
            check(self.lib.pcadv_row_semi_ce(_p(logits, M * ncls), ncls, _p(out, M), M, ncls,
                                             self.semi_th, self.lambda_semi, _p(d, M * ncls), ncls,
                                             None if labels is None else _p(labels),
                                             _p(self.loss_buf, 5), _p(self.kept_buf), _p(sws),
                                             sws.numel(), stream_ptr()),
                  "pcadv_row_semi_ce")
            self._semi_stale = True
        elif self._semi_stale:
            # the first step without the term after one with it: loss_semi and K
            # back to 0 (a step that never ran the term launches nothing for it)
            self.loss_buf[5:].zero_()
            self.kept_buf.zero_()
            self._semi_stale = False
        if self.keep_activations:
            self.semi_labels = labels
        return out

    @property
    def losses(self):
        """[loss_seg, loss_adv, loss_D] (the trainers' loss-ring interface)."""
        return self.loss_buf[:3]

    @property
    def losses_semi(self):
        """[loss_seg, loss_adv, loss_semi, loss_D] of the last step (loss_semi is
        0 for a step without the term, or with no point kept)."""
        return self.loss_buf.index_select(0, self._semi_idx)

    @property
    def kept(self):
        """The number of no-GT points the last step's semi term kept (device
        int32; 0 for a step without the term)."""
        return self.kept_buf[0]


class SegStackTrainStep(_SegDiscStep):
    """One iteration of run_training_seg_stack (utils/trainer.py:1053-1153) with
    PointNetSeg + StackDiscNet; the launches are _SegDiscStep's, where _disc is:

      the shape labels (argmax of cls_gt, one per GT cloud) on the device; the
      fused stacked D forward on softmax(GT) / log_softmax(no-GT)
      (trainer.py:1082,1095) with loss_adv, loss_D, loss_D_shape, their
      derivatives with respect to the per-point channel max, conv5's gradients
      and the bad_rows counter; the fused D backward (conv1..conv4's gradients
      of loss_D + lambda_disc_shape loss_D_shape, and the no-GT rows of dlogits).

    One D forward serves each half.  With ImagePool(0) the reference's two
    forwards of D on the GT predictions (trainer.py:1117 for the shape term,
    :1127 for the pooled BCE term) see the same detached input and the same
    weights, and so do its two on the no-GT predictions (:1097 with D frozen
    for the generator's term, :1141 for D's own): D has no batch statistics and
    no dropout, so each pair computes the same values, and the gradients the
    reference accumulates over three backward calls are the sum formed here.

    `losses` is [loss_seg, loss_adv, loss_D, loss_D_shape] (the reference's log
    line; loss_D_shape unscaled).  `bad_rows` (device int32) counts the points
    whose D output left [0, 1] in the last step: torch's BCELoss raises there,
    a captured graph cannot, so the caller checks the counter when it reads the
    losses (`logged` does).

    semi=True adds run_training_seg_stack_semi's term (utils/trainer.py:
    1516-1537): lambda_semi times the cross entropy of the no-GT points whose D
    output is above semi_th against their own argmax.  The D forward counts the
    kept points and sums their losses in its own launch
    (pcadv_stackdisc_forward_semi), the D backward writes the no-GT rows of
    dlogits, and pcadv_row_semi_apply adds the term's gradient to them with the
    count read on the device (D receives nothing from it).  Any point count is
    allowed: this D does not use input_pts.  `losses_semi` is [loss_seg,
    loss_adv, loss_semi, loss_D, loss_D_shape], `kept` the number of kept points
    and, under keep_activations, `semi_labels` the pseudo-labels (255 where
    ignored); `losses` is as above.  A captured graph has `semi` baked in:
    capture one graph per value."""

    _D_NET, _d_workspace = StackDiscNet, staticmethod(stackdisc_workspace)
    _SEMI = 9  # loss_buf[9]: loss_semi (6..8 are the regularised step's)

    def __init__(self, model, model_D, optimizer=None, optimizer_D=None, lambda_seg=1.0,
                 lambda_adv=0.01, lambda_disc_shape=1.0, lr=1e-4, lr_D=1e-4, betas=(0.9, 0.999),
                 eps=1e-8, device="cuda", precision=None, seed=0, keep_activations=False,
                 lambda_semi=1.0, semi_th=0.8):
        if isinstance(model_D, StackDiscNet) and model_D.num_shapes < 16:
            raise ValueError(f"model_D has {model_D.num_shapes} shape classes, cls is 16 wide")
        super().__init__(model, model_D, optimizer, optimizer_D, lambda_seg, lambda_adv, lr, lr_D,
                         betas, eps, device, precision, seed, keep_activations)
        self.lambda_disc_shape = float(lambda_disc_shape)
        self.lambda_semi, self.semi_th = float(lambda_semi), float(semi_th)
        self.loss_buf = torch.zeros(10, device=self.device)
        self.bad_buf = torch.zeros(1, device=self.device, dtype=torch.int32)  # loss_buf[5]: shape
        self.kept_buf = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._loss_idx = torch.tensor([0, 1, 2, 5], device=self.device)  # the log line's order
        self._semi_idx = torch.tensor([0, 1, self._SEMI, 2, 5], device=self.device)
        self.semi_labels = None
        self._semi_stale = False

    def _disc(self, logits, ncls, M, N, cls_gt, d, dws, soft0, soft1, semi):
        # make_shape_label (utils/utils.py:33-38): one label per GT cloud
        shape_label = torch.argmax(cls_gt.reshape(M // N, 16), dim=1).to(torch.int32)
        m = torch.empty(2 * M, device=self.device)
        d_out = torch.empty(2 * M, device=self.device)
        argc = torch.empty(2 * M, device=self.device, dtype=torch.int32)
        dm_d = torch.empty(2 * M, device=self.device)
        dm_adv = torch.empty(M, device=self.device)
        scan = dict(semi_th=self.semi_th, loss_semi=self.loss_buf[self._SEMI:self._SEMI + 1],
                    kept=self.kept_buf) if semi else {}
        stackdisc_forward(logits, ncls, M, M, PWD_SOFTMAX, PWD_LOG_SOFTMAX, self.d_params, m, argc,
                          d_out, dws, losses=self.loss_buf[1:6], shape_label=shape_label,
                          pts_per_cloud=N, lambda_disc_shape=self.lambda_disc_shape, soft0=soft0,
                          soft1=soft1, seed=self.seed, step_count=self.step_count, dm_d=dm_d,
                          dm_adv=dm_adv, grads5=self.d_grad_views[8:10], bad_rows=self.bad_buf,
                          **scan)
        stackdisc_backward(logits, ncls, M, M, PWD_SOFTMAX, PWD_LOG_SOFTMAX, self.d_params, m,
                           argc, dws, dm_d, self.d_grad_views, dm_adv=dm_adv,
                           lambda_adv=self.lambda_adv, dlogits=d)
        labels = None
        if semi:
            if self.keep_activations:
                labels = torch.empty(M, device=self.device, dtype=torch.int32)
            self._semi_grad(logits[M:], ncls, d_out[M:], d[M:], labels)
            self._semi_stale = True
        elif self._semi_stale:
            # the first step without the term after one with it: loss_semi and K
            # back to 0 (a step that never ran the term launches nothing for it)
            self.loss_buf[self._SEMI].zero_()
            self.kept_buf.zero_()
            self._semi_stale = False
        if self.keep_activations:
            self.semi_labels = labels
        return d_out

    def _semi_grad(self, logits, ncls, d_out, d, labels):
        """The semi term's gradient on the no-GT rows, after the forward's scan
        left K in kept_buf and the backward wrote those rows of d."""
        row_semi_apply(logits, ncls, d_out, self.semi_th, self.lambda_semi, self.kept_buf, d,
                       labels)

    @property
    def losses(self):
        """[loss_seg, loss_adv, loss_D, loss_D_shape], the order of the reference's
        log line (one gather from the loss buffer by a resident index: a new
        tensor on every read)."""
        return self.loss_buf.index_select(0, self._loss_idx)

    @property
    def losses_semi(self):
        """`losses` with loss_semi (0 for a step without the term, or with no
        point kept) before loss_D: the order of the semi loops' log lines."""
        return self.loss_buf.index_select(0, self._semi_idx)

    @property
    def kept(self):
        """The number of no-GT points the last step's semi term kept (device
        int32; 0 for a step without the term)."""
        return self.kept_buf[0]

    @property
    def bad_rows(self):
        """The number of points whose D output was outside [0, 1] in the last
        step (device int32)."""
        return self.bad_buf[0]

    def capture_on(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt=None, soft_nogt=None,
                   semi=False):
        """_SegDiscStep.capture_on.  Reading `losses` launches its gather, so that
        stays outside the graph."""
        return super().capture_on(pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt,
                                  semi)

    def logged(self, with_semi=False):
        vals = (self.losses_semi if with_semi else self.losses).tolist()
        if int(self.bad_rows.item()) > 0:
            raise RuntimeError("all elements of input should be between 0 and 1")
        return vals


class SegStackReguTrainStep(SegStackTrainStep):
    """One iteration of run_training_seg_stack_regulization (utils/trainer.py:
    1244-1363) with PointNetSeg_regulization + StackDiscNet: SegStackTrainStep's
    launches, with the regularised generator's forward and backward in their
    places.  Inside the backward, once the feature transform's own gradient is
    formed, pcadv_tnet_mse_reg adds lambda_regu times the gradient of
    MSELoss(T T^T, I) of each batch (the 2B clouds as the groups (B, B):
    trainer.py:1276-1282,1297-1303,1316-1318) and writes the two losses.

    `losses` is [loss_seg, loss_adv, loss_regu, loss_D, loss_D_shape], the
    order of the reference's log line; loss_regu = l_gt + l_nogt, unscaled.
    bad_rows, logged() and capture_on are the stack step's, and so is semi=True
    (run_training_seg_stack_regulization_semi, utils/trainer.py:1747-1775):
    `losses_semi` is [loss_seg, loss_adv, loss_regu, loss_semi, loss_D,
    loss_D_shape]."""

    _G_NET = PointNetSeg_regulization

    def __init__(self, model, model_D, optimizer=None, optimizer_D=None, lambda_seg=1.0,
                 lambda_adv=0.01, lambda_disc_shape=1.0, lambda_regu=0.001, lr=1e-4, lr_D=1e-4,
                 betas=(0.9, 0.999), eps=1e-8, device="cuda", precision=None, seed=0,
                 keep_activations=False, lambda_semi=1.0, semi_th=0.8):
        super().__init__(model, model_D, optimizer, optimizer_D, lambda_seg, lambda_adv,
                         lambda_disc_shape, lr, lr_D, betas, eps, device, precision, seed,
                         keep_activations, lambda_semi, semi_th)
        self.lambda_regu = float(lambda_regu)
        # loss_buf[6:8]: the two batches' regulariser losses, [8]: their sum
        self._loss_idx = torch.tensor([0, 1, 8, 2, 5], device=self.device)
        self._semi_idx = torch.tensor([0, 1, 8, self._SEMI, 2, 5], device=self.device)
        self._regu_ws = None  # pcadv_tnet_mse_reg's 4 x (2B) floats, kept between steps

    def _g_forward(self, pts, cls, wpl):
        return segregu_forward(pts, cls, self.params, wplanes=wpl, precision=self.precision)

    def _g_backward(self, fw, d):
        def reg(T, dT):
            if self._regu_ws is None or self._regu_ws.numel() < 4 * T.shape[0]:
                self._regu_ws = torch.empty(4 * T.shape[0], device=self.device)
            _engine().mse_reg(T, T.shape[0] // 2, self.lambda_regu, self.loss_buf[6:8], dT,
                              ws=self._regu_ws)
            torch.add(self.loss_buf[6], self.loss_buf[7], out=self.loss_buf[8])
        segregu_backward(fw, d, None, out=self.grad_views, reg=reg)


# ---------------------------------------------------------------------------
# The dual discriminator of run_training_seg_dual (utils/trainer.py:2123-2382):
# BaseDiscNet + PointDiscNet + ShapeDiscNet on the dense engine.  Every layer
# is pcadv_gemm (six products, no activation) followed by pcadv_lrelu_fwd in
# place; every data gradient pcadv_gemm (tb = 1) followed by pcadv_lrelu_bwd on
# the activation below; every weight gradient pcadv_gemm_wgrad (csrc/
# dualdisc.hip has the rest: the input transform, the point head's tail, SGD).
# ---------------------------------------------------------------------------

def _lrelu(E, y):
    check(E.lib.pcadv_lrelu_fwd(_p(y), y.numel(), stream_ptr()), "pcadv_lrelu_fwd")


def _lrelu_bwd(E, d, y, y_off=0):
    check(E.lib.pcadv_lrelu_bwd(_p(d), _p(y, y_off), d.numel(), stream_ptr()), "pcadv_lrelu_bwd")


def _dual_layer(E, x, w, b, rows):
    """lrelu(x w^T + b) of the first `rows` rows of x; w a Conv1d weight [O][K](, 1)."""
    O, K = w.shape[0], w.shape[1]
    y = torch.empty(rows, O, device=x.device)
    if rows:
        E.gemm(x, K, w, K, y, O, rows, O, K, bias=b, precise=True)
        _lrelu(E, y)
    return y


def _dual_dgrad(E, dz, w, rows, y_below, y_off=0):
    """dz W of `rows` rows, times the LeakyReLU slope of the layer below's
    output y_below (from element y_off on; None: the net's input, no slope)."""
    O, K = w.shape[0], w.shape[1]
    dx = torch.empty(rows, K, device=dz.device)
    E.gemm(dz, O, w, K, dx, K, rows, K, O, tb=1, precise=True)
    if y_below is not None:
        _lrelu_bwd(E, dx, y_below, y_off)
    return dx


def _dual_wgrad(E, dz, x, rows, w, dw, db, accumulate):
    O, K = w.shape[0], w.shape[1]
    nb = E.lib.pcadv_gemm_wgrad_workspace_bytes(rows, O, K, 0)
    ws = _ws(nb, dz.device)
    check(E.lib.pcadv_gemm_wgrad(_p(dz), O, _p(x), K, rows, O, K, _p(dw), K, _p(db), None, 0,
                                 int(accumulate), _p(ws), ws.numel(), stream_ptr()),
          "pcadv_gemm_wgrad")


def _dual_params(ps, n, name):
    if len(ps) < n:
        raise ValueError(f"{name}: expected at least {n} tensors (weights and biases)")
    for t in ps[:n]:
        _check_dev(t, name)
        if not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous tensors")
    return list(ps[:n])


def dualdisc_point(logits, ncls, n0, n1, t0, t1, sp, pp, *, losses=None, soft0=None, soft1=None,
                   soft_out=None, seed=0, step_count=None, lambda_adv=1.0, grads_s=None,
                   grads_p=None, dlogits=None, max_workgroups=0):
    """PointDiscNet(BaseDiscNet(.)) on the n0 + n1 point-major rows of `logits`
    (row stride logits.stride(0); rows [0, n0) through transform t0, the rest
    through t1), on the current stream.  sp: the trunk's conv1..conv3 weights and
    biases (6 tensors, state_dict order), pp: the point head's.

    Returns a dict: x0 (the transformed rows), acts (x0 and the six layers'
    outputs), out (per row the max over the head's channels), argc (its
    channel, the first on ties).  With `losses` (4 floats) also the BCE terms
    and their derivatives as pcadv_pwdisc_forward defines them (dout_d,
    dout_adv in the dict; labels soft0 / soft1 or device-drawn by (seed,
    *step_count, row)); then grads_s / grads_p (six parameter-shaped tensors
    each) receive the gradients of loss_D_point (overwritten), and rows
    [n0, n0 + n1) of dlogits (point-major like logits) the gradient of
    lambda_adv loss_adv through the frozen nets; its other rows are untouched."""
    E = _engine()
    dev = logits.device
    R = n0 + n1
    if logits.dim() != 2 or logits.shape[0] != R or logits.shape[1] < ncls \
            or logits.stride(1) != 1 or R < 1:
        raise ValueError(f"logits: expected point-major ({R}, >= {ncls}) rows, "
                         f"got {tuple(logits.shape)} with strides {logits.stride()}")
    _check_dev(logits, "logits")
    sp, pp = _dual_params(sp, 6, "trunk parameters"), _dual_params(pp, 6, "point-head parameters")
    if sp[0].shape[1] != ncls or pp[0].shape[1] != sp[4].shape[0] or pp[4].shape[0] % 4:
        raise ValueError("dualdisc_point: the nets' widths do not chain from the logits' classes")
    ld = max(logits.stride(0), ncls)
    x0 = torch.empty(R, ncls, device=dev)
    check(E.lib.pcadv_dual_input(_p(logits), ld, ncls, n0, n1, int(t0), int(t1), _p(x0),
                                 stream_ptr()), "pcadv_dual_input")
    W = [sp[0], sp[2], sp[4], pp[0], pp[2], pp[4]]
    Bs = [sp[1], sp[3], sp[5], pp[1], pp[3], pp[5]]
    acts = [x0]
    for w, b in zip(W, Bs):
        acts.append(_dual_layer(E, acts[-1], w, b, R))
    y = acts[-1]
    C = y.shape[1]
    res = dict(x0=x0, acts=acts, out=torch.empty(R, device=dev),
               argc=torch.empty(R, device=dev, dtype=torch.int32))
    a = _lib.DualTailArgs()
    a.y, a.C, a.n0, a.n1 = y.data_ptr(), C, n0, n1
    a.out, a.argc = res["out"].data_ptr(), res["argc"].data_ptr()
    a.max_workgroups = int(max_workgroups)
    keep = []
    if losses is not None:
        if losses.numel() != 4 or losses.dtype != torch.float32 or not losses.is_contiguous():
            raise ValueError("losses: expected 4 contiguous float32")
        for t, n, nm in ((soft0, n0, "soft0"), (soft1, n1, "soft1"), (soft_out, R, "soft_out")):
            if t is not None:
                _check_dev(t, nm)
                if t.numel() != n or not t.is_contiguous():
                    raise ValueError(f"{nm}: expected {n} contiguous float32")
        res["dout_d"] = torch.empty(R, device=dev)
        res["dout_adv"] = torch.empty(max(n1, 1), device=dev)
        dz_d = torch.empty(R, C, device=dev) if grads_s is not None else None
        want_dx = dlogits is not None and n1 > 0
        dz_adv = torch.empty(n1, C, device=dev) if want_dx else None
        ws = _ws(E.lib.pcadv_dual_point_tail_workspace_bytes(R), dev)
        keep += [dz_d, dz_adv, ws]
        a.losses = losses.data_ptr()
        a.soft0 = None if soft0 is None else soft0.data_ptr()
        a.soft1 = None if soft1 is None else soft1.data_ptr()
        a.soft_out = None if soft_out is None else soft_out.data_ptr()
        a.rng_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.step_count = None if step_count is None else step_count.data_ptr()
        a.dout_d, a.dout_adv = res["dout_d"].data_ptr(), res["dout_adv"].data_ptr()
        a.lambda_adv = float(lambda_adv)
        a.dz_d = None if dz_d is None else dz_d.data_ptr()
        a.dz_adv = None if dz_adv is None else dz_adv.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    check(E.lib.pcadv_dual_point_tail(ctypes.byref(a), stream_ptr()), "pcadv_dual_point_tail")
    if losses is None:
        return res
    if grads_s is not None:
        G = list(grads_s[:6]) + list(grads_p[:6])
        for g, p in zip(G, sp + pp):
            _check_dev(g, "D gradient")
            if g.numel() != p.numel() or not g.is_contiguous():
                raise ValueError("D gradients: expected parameter-shaped contiguous tensors")
        dz = dz_d
        for i in range(5, -1, -1):
            _dual_wgrad(E, dz, acts[i], R, W[i], G[2 * i], G[2 * i + 1], False)
            if i:
                dz = _dual_dgrad(E, dz, W[i], R, acts[i])
    if want_dx:
        if dlogits.dim() != 2 or dlogits.shape[0] != R or dlogits.shape[1] < ncls \
                or dlogits.stride(1) != 1 or dlogits.dtype != torch.float32 \
                or dlogits.device.type != "cuda":
            raise ValueError("dlogits: expected point-major float32 rows like logits")
        dz = dz_adv
        for i in range(5, -1, -1):
            dz = _dual_dgrad(E, dz, W[i], n1, acts[i] if i else None, n0 * acts[i].shape[1])
        ldd = max(dlogits.stride(0), ncls)
        check(E.lib.pcadv_dual_input_bwd(_p(x0, n0 * ncls), _p(dz), ncls, n1, int(t1),
                                         _p(dlogits, n0 * ldd), ldd, stream_ptr()),
              "pcadv_dual_input_bwd")
    return res


def dualdisc_shape(x0, C, N, sp, hp, labels, scale, loss, grads_s, grads_h):
    """ShapeDiscNet(BaseDiscNet(.)) and CrossEntropyLoss on C clouds of N points
    whose transformed rows x0 (C N, ncls) are given, forward and backward, on
    the current stream.  sp as in dualdisc_point; hp: the shape head's conv,
    fc1, fc2 weights and biases; labels (C,) int64; loss: one float, the
    unscaled mean cross entropy.  The gradients of scale x loss: grads_h (six
    tensors) overwritten, grads_s (six tensors) ADDED to (the reference does not
    clear the trunk's .grad between its two D terms).  Returns a dict: acts (x0
    and the trunk's outputs), gmax / gidx (the conv's max over the points
    before the LeakyReLU, which is increasing and so keeps the winner, and its
    point, the first on ties), logits (C, num_shapes)."""
    E = _engine()
    dev = x0.device
    M = C * N
    sp, hp = _dual_params(sp, 6, "trunk parameters"), _dual_params(hp, 6, "shape-head parameters")
    _check_dev(x0, "x0", shape=(M, sp[0].shape[1]))
    _check_dev(labels, "labels", shape=(C,), dtype=torch.int64)
    W = [sp[0], sp[2], sp[4]]
    acts = [x0.contiguous()]
    for i, w in enumerate(W):
        acts.append(_dual_layer(E, acts[-1], w, sp[2 * i + 1], M))
    h3 = acts[-1]
    K, O = h3.shape[1], hp[0].shape[0]
    if hp[0].shape[1] != K or K % 32 or K > 512:
        raise ValueError(f"dualdisc_shape: trunk width {K} (a multiple of 32 up to 512) against "
                         f"the head's {hp[0].shape[1]}")
    gmax = torch.empty(C, O, device=dev)
    gidx = torch.empty(C, O, device=dev, dtype=torch.int32)
    ws = _ws(E.lib.pcadv_conv_max_x3_workspace_bytes(C, N, O), dev)
    check(E.lib.pcadv_conv_max_x3(_p(h3), K, C, N, K, _p(hp[0]), _p(hp[1]), O, 0, _p(gmax),
                                  _p(gidx), _p(ws), ws.numel(), stream_ptr()), "pcadv_conv_max_x3")
    pooled = gmax.clone()
    _lrelu(E, pooled)
    f1 = ops.linear_fwd(pooled, hp[2], hp[3], ops.ACT_LRELU)
    s = ops.linear_fwd(f1, hp[4], hp[5], ops.ACT_NONE)
    S = s.shape[1]
    ds = torch.empty_like(s)
    cws = _ws(E.lib.pcadv_row_ce_workspace_bytes(C), dev)
    check(E.lib.pcadv_row_ce(_p(s), S, _p(labels), C, S, float(scale), _p(loss), _p(ds), _p(cws),
                             cws.numel(), stream_ptr()), "pcadv_row_ce")
    df1, _, _ = ops.linear_bwd(ds, s, ops.ACT_NONE, None, 0.0, f1, hp[4], dw_out=grads_h[4],
                               db_out=grads_h[5])
    dpool, _, _ = ops.linear_bwd(df1, f1, ops.ACT_LRELU, None, 0.0, pooled, hp[2],
                                 dw_out=grads_h[2], db_out=grads_h[3])
    _lrelu_bwd(E, dpool, pooled)
    # pcadv_conv_max_x3_bwd masks by [gmax > 0] (the ReLU before conv6's max); the
    # LeakyReLU's slope is already in dpool, so every channel passes
    ones = torch.ones(C, O, device=dev)
    dh3 = torch.zeros(M, K, device=dev)
    check(E.lib.pcadv_conv_max_x3_bwd(_p(dpool), _p(ones), _p(gidx), _p(h3), K, C, N, O, K,
                                      _p(hp[0]), _p(grads_h[0]), _p(grads_h[1]), _p(dh3), K, 0,
                                      stream_ptr()), "pcadv_conv_max_x3_bwd")
    _lrelu_bwd(E, dh3, h3)
    dz = dh3
    for i in range(2, -1, -1):
        _dual_wgrad(E, dz, acts[i], M, W[i], grads_s[2 * i], grads_s[2 * i + 1], True)
        if i:
            dz = _dual_dgrad(E, dz, W[i], M, acts[i])
    return dict(acts=acts, gmax=gmax, gidx=gidx, pooled=pooled, logits=s, dh3=dh3)


def sgd_(param, grad, lr, acc=None):
    """pcadv_sgd on flat float32 tensors: param -= lr grad, or with acc (a
    running gradient sum) acc += grad; param -= lr acc."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (acc, "acc")):
        if t is None:
            continue
        _check_dev(t, nm)
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"sgd: {nm} has {t.numel()} elements, expected {n} contiguous")
    check(_engine().lib.pcadv_sgd(_p(param), _p(grad), None if acc is None else _p(acc), n,
                                  float(lr), stream_ptr()), "pcadv_sgd")


def _plain_sgd_lr(opt, nets, what):
    """The learning rate of a torch.optim.SGD the fused dual step can stand in
    for: one param group over exactly `nets`' parameters, no momentum,
    dampening, weight decay, nesterov or maximize."""
    if type(opt) is not torch.optim.SGD or len(opt.param_groups) != 1:
        raise ValueError(f"{what}: expected a torch.optim.SGD with one param group")
    g = opt.param_groups[0]
    if g.get("momentum", 0) or g.get("dampening", 0) or g.get("weight_decay", 0) \
            or g.get("nesterov") or g.get("maximize"):
        raise ValueError(f"{what}: plain SGD only (no momentum, dampening, weight decay, nesterov "
                         "or maximize)")
    want = {id(p) for net in nets for p in net.parameters()}
    if {id(p) for p in g["params"]} != want or len(g["params"]) != len(want):
        raise ValueError(f"{what}: its parameters are not exactly its head's and the trunk's")
    return float(g["lr"])


class SegDualTrainStep(_SegStep):
    """One iteration of run_training_seg_dual (utils/trainer.py:2151-2286) with
    PointNetSeg + BaseDiscNet / ShapeDiscNet / PointDiscNet, ImagePool(0), G's
    Adam and the two plain SGDs that both own the trunk, as native launches on
    one stream, capturable into one HIP graph (no parallel branches):

      weight-plane split; seg_forward on the 2B clouds [GT; no-GT]; pcadv_row_ce
      on the GT rows; the point phase (dualdisc_point) on [softmax(GT);
      log_softmax(no-GT)]: loss_adv, loss_D_point, the trunk's and the point
      head's gradients of loss_D_point and the no-GT rows of dlogits from
      lambda_adv loss_adv; seg_backward; G's Adam; optimizer_D_point.step() as
      two pcadv_sgd launches; the shape phase (dualdisc_shape) on the GT rows
      through the UPDATED trunk, its trunk gradients added to the point phase's;
      optimizer_D_shape.step() as two more.

    The reference runs D three times in the point phase (frozen on the no-GT
    rows for G's term, then on each detached half for its own): D has no batch
    statistics or dropout and G's Adam does not touch it, so one forward serves
    all three.  G's Adam is placed after G's backward; the reference steps it
    before D's terms, which read detached predictions: the same values.

    The reference never clears PointDiscNet's gradients (optimizer_D_point.
    zero_grad() is not called in its loop), so its SGD steps by the running sum
    A_P of every iteration's gradient.  That sum lives in the point head's flat
    .grad buffer (pcadv_sgd's accumulator form), so an eager iteration continues
    it; the trunk's .grad holds g_S^P + g_S^H and the shape head's g_H after a
    step, conv4's (never used by forward) zeros.  The three nets' parameters and
    gradients are flat buffers handed to the modules as views.  D always runs in
    f32; `precision` is the generator's.  `losses` is [loss_seg, loss_adv,
    loss_D_point, loss_D_shape] (loss_D_shape unscaled)."""

    def __init__(self, model, sharedDisc, shapeDisc, pointDisc, optimizer=None,
                 optimizer_D_shape=None, optimizer_D_point=None, lambda_seg=1.0, lambda_adv=0.01,
                 lambda_disc_shape=1.0, lr=1e-4, lr_D_shape=1e-4, lr_D_point=1e-4,
                 betas=(0.9, 0.999), eps=1e-8, device="cuda", precision=None, seed=0,
                 keep_activations=False):
        from .discriminator import BaseDiscNet, PointDiscNet, ShapeDiscNet
        if not (isinstance(model, PointNetSeg) and isinstance(sharedDisc, BaseDiscNet)
                and isinstance(shapeDisc, ShapeDiscNet) and isinstance(pointDisc, PointDiscNet)):
            raise TypeError("SegDualTrainStep: expected a PointNetSeg, a BaseDiscNet, a "
                            "ShapeDiscNet and a PointDiscNet")
        if sharedDisc.input_dim != model.output_dim:
            raise ValueError(f"sharedDisc takes {sharedDisc.input_dim} channels, the generator "
                             f"predicts {model.output_dim} classes")
        if not (sharedDisc.output_dim == shapeDisc.shared_output_dim
                == pointDisc.shared_output_dim == 256) or shapeDisc.interm_dim != 512:
            raise ValueError("SegDualTrainStep: a 256-wide trunk and a 512-wide shape conv")
        if shapeDisc.num_shapes < 16:
            raise ValueError(f"shapeDisc has {shapeDisc.num_shapes} shape classes, cls is 16 wide")
        self._d_opts = (optimizer_D_shape, optimizer_D_point)
        self._d_nets = (sharedDisc, shapeDisc, pointDisc)
        self.lr_D_shape, self.lr_D_point = float(lr_D_shape), float(lr_D_point)
        super().__init__(model, (optimizer,), [(lr, betas, eps)], device, precision,
                         keep_activations)
        dev = self.device
        self.sharedDisc, self.shapeDisc, self.pointDisc = sharedDisc, shapeDisc, pointDisc
        # FlatAdam without an optimizer: flat parameters and gradients as views
        self.S, self.H, self.P = (FlatAdam(m, None, dev) for m in self._d_nets)
        # this iteration's point-head gradient; P.grad is the running sum A_P
        self.gp = torch.zeros(self.P.numel, device=dev)
        self.gp_views = list(self.P.views(self.gp).values())
        self.lambda_seg, self.lambda_adv = float(lambda_seg), float(lambda_adv)
        self.lambda_disc_shape, self.seed = float(lambda_disc_shape), int(seed)
        # [loss_seg, loss_adv, loss_D_point, its GT part, its no-GT part, loss_D_shape]
        self.loss_buf = torch.zeros(6, device=dev)
        self._loss_idx = torch.tensor([0, 1, 2, 5], device=dev)
        self.d_out = self.act = None

    def sync_hyper(self):
        super().sync_hyper()
        shared, shape, point = self._d_nets
        if self._d_opts[0] is not None:
            self.lr_D_shape = _plain_sgd_lr(self._d_opts[0], (shape, shared), "optimizer_D_shape")
        if self._d_opts[1] is not None:
            self.lr_D_point = _plain_sgd_lr(self._d_opts[1], (point, shared), "optimizer_D_point")

    def graph_state(self):
        """The base's list and what else a warm-up changes: the three D nets'
        parameters and the running sum A_P."""
        return super().graph_state() + [self.S.param, self.H.param, self.P.param, self.P.grad]

    def after_eager(self):
        """The base's hand-over for G; the D nets' .grad go back to their flat
        views (a fresh tensor's values copied in, None as zeros).  The point
        head's were accumulated in place by the eager iterations, so A_P
        carries on."""
        super().after_eager()
        for f in (self.S, self.H, self.P):
            for p, gv in zip(f.params, f.grad_views):
                if p.grad is None:
                    gv.zero_()
                elif p.grad.data_ptr() != gv.data_ptr():
                    gv.copy_(p.grad)
                p.grad = gv

    def __call__(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt=None, soft_nogt=None,
                 apply_adam=True):
        self._run(pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt, apply_adam)
        return self.losses

    def _run(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt, apply_adam):
        """The step's launches and nothing else: what capture_on captures.
        apply_adam False: the gradients only (no Adam, no SGD; the shape phase
        then sees the trunk as it was, and A_P still takes this gradient)."""
        B, N, _ = pts_gt.shape
        _check_dev(pts_gt, "pts_gt")
        _check_dev(pts_nogt, "pts_nogt", shape=(B, N, 3))
        if seg.shape != (B, N) or seg.dtype != torch.int64 or not seg.is_contiguous():
            raise ValueError("seg: expected contiguous int64 (B, N)")
        pts = torch.cat([pts_gt, pts_nogt])
        cls = torch.cat([cls_gt.float().reshape(B, 1, 16), cls_nogt.float().reshape(B, 1, 16)])
        self._run_packed(pts, cls, seg, soft_gt, soft_nogt, apply_adam)

    def _run_packed(self, pts, cls, seg, soft_gt=None, soft_nogt=None, apply_adam=True):
        """_run on the step's packed input, as dataset.gather_seg_pair writes it:
        pts (2B, N, 3) and cls (2B, 1, 16) f32 with the GT batch in rows [0, B)
        and the no-GT batch in rows [B, 2B), seg (B, N) int64.  _run is the two
        concatenations and this."""
        B, N = seg.shape
        _check_dev(pts, "pts", shape=(2 * B, N, 3))
        _check_dev(cls, "cls", shape=(2 * B, 1, 16))
        if seg.dtype != torch.int64 or not seg.is_contiguous():
            raise ValueError("seg: expected contiguous int64 (B, N)")
        if (B * N) % int(self.pointDisc.input_pts):
            raise ValueError(f"{B} x {N} points do not fill rows of pointDisc.input_pts = "
                             f"{self.pointDisc.input_pts}")
        M = B * N
        wpl = None
        if _PLANES:
            _engine().split(self.param, self.wph, self.wpl)
            wpl = self.wplanes
        cls_gt = cls[:B]
        fw = seg_forward(pts, cls, self.params, wplanes=wpl, precision=self.precision)
        ncls = fw["dims"][2]
        logits = fw["logits"]
        d = torch.empty(2 * M, ncls, device=self.device)
        ws = _ws(self.lib.pcadv_row_ce_workspace_bytes(M), self.device)
        check(self.lib.pcadv_row_ce(_p(logits), ncls, _p(seg), M, ncls, self.lambda_seg,
                                    _p(self.loss_buf), _p(d), _p(ws), ws.numel(), stream_ptr()),
              "pcadv_row_ce")
        S, H, P = self.S, self.H, self.P
        act = dualdisc_point(logits, ncls, M, M, PWD_SOFTMAX, PWD_LOG_SOFTMAX, S.params[:6],
                             P.params, losses=self.loss_buf[1:5],
                             soft0=None if soft_gt is None else soft_gt.reshape(M),
                             soft1=None if soft_nogt is None else soft_nogt.reshape(M),
                             seed=self.seed, step_count=self.step_count,
                             lambda_adv=self.lambda_adv, grads_s=S.grad_views[:6],
                             grads_p=self.gp_views, dlogits=d)
        seg_backward(fw, d, None, out=self.grad_views)
        if apply_adam:
            self._adam(0, self.lr, self.betas, self.eps)
            # optimizer_D_point.step(): the head by its running sum, the trunk by g_S^P
            sgd_(P.param, self.gp, self.lr_D_point, acc=P.grad)
            sgd_(S.param, S.grad, self.lr_D_point)
        else:
            P.grad += self.gp
        labels = torch.argmax(cls_gt.reshape(B, 16), dim=1)
        x0_gt = act["x0"][:M]
        sh = dualdisc_shape(x0_gt, B, N, S.params[:6], H.params, labels, self.lambda_disc_shape,
                            self.loss_buf[5:6], S.grad_views[:6], H.grad_views)
        if apply_adam:
            # optimizer_D_shape.step(): the trunk by g_S^P + g_S^H
            sgd_(H.param, H.grad, self.lr_D_shape)
            sgd_(S.param, S.grad, self.lr_D_shape)
        if self.keep_activations:
            self.fw, self.d_out, self.act = fw, act["out"], dict(point=act, shape=sh)

    def adam(self):
        raise NotImplementedError("SegDualTrainStep: the updates are interleaved with the two D "
                                  "phases (the shape phase reads the updated trunk); call the step")

    def capture_on(self, pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt=None, soft_nogt=None):
        """One HIP graph of a step reading the given resident buffers: a single
        stream, no parallel branches (state, A_P included, is restored to what
        it was before the warm-up)."""
        def body():
            self._run(pts_gt, cls_gt, seg, pts_nogt, cls_nogt, soft_gt, soft_nogt, True)
        return self._capture(body, body)

    @property
    def losses(self):
        """[loss_seg, loss_adv, loss_D_point, loss_D_shape], the order of the
        reference's log line (a gather by a resident index: a new tensor)."""
        return self.loss_buf.index_select(0, self._loss_idx)

    def logged(self, with_semi=False):
        return self.losses.tolist()

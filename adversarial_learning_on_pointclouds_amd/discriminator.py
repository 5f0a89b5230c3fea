"""Drop-in discriminators of models/discriminator.py, same state_dicts as the
reference.

DeepConvDiscNet (:30-51), backed by the pcadv linear kernels: five 1x1 Conv1d
layers on B x C x 1 with LeakyReLU(0.2), then Linear(64, output_dim).

PointwiseDiscNet (:53-79), the per-point discriminator of run_training_seg
(utils/trainer.py:849-1026): conv1..conv4 + ReLU and the max over the 128
channels, one logit per point, fused in csrc/pwdisc.hip (pwdisc_forward /
pwdisc_backward below are the thin calls into it).

StackDiscNet (:139-175), the stacked shape discriminator of
run_training_seg_stack (utils/trainer.py:1028-1216): the same four layers with
LeakyReLU(0.2), the max over the 128 channels, conv5 = Conv1d(1, num_shapes, 1)
on that one value per point (the shape logits) and disc_out = lse / (lse + 1)
with lse their logsumexp; stackdisc_forward / stackdisc_backward call the fused
kernels (csrc/pwdisc.hip, the k_stk_fwd part).

BaseDiscNet, ShapeDiscNet and PointDiscNet (:82-137), the dual discriminator of
run_training_seg_dual (utils/trainer.py:2123-2382): a shared trunk (50 -> 64 ->
64 -> 256, LeakyReLU(0.2)), a per-point head (256 -> 256 -> 128 -> 128 and the
max over the 128 channels) and a shape head (256 -> 512, the max over the
points, 512 -> 64 -> num_shapes).  Their forward is plain torch on whatever
device the module is on; the training iteration's native path is
seg.SegDualTrainStep (the dense GEMM engine and csrc/dualdisc.hip)."""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import PWD_LOG_SOFTMAX, PWD_NONE, PWD_SOFTMAX, check, stream_ptr
from ._lib import ptr as _vp
from .ops import ACT_LRELU, ACT_NONE, LinearFunction

__all__ = ["DeepConvDiscNet", "PointwiseDiscNet", "pwdisc_forward", "pwdisc_backward",
           "pwdisc_workspace", "PWD_NONE", "PWD_SOFTMAX", "PWD_LOG_SOFTMAX", "StackDiscNet",
           "stackdisc_forward", "stackdisc_backward", "stackdisc_workspace", "row_semi_apply",
           "BaseDiscNet",
           "ShapeDiscNet", "PointDiscNet"]

PWD_MAX_DIM = 64  # input channels the fused kernels take (the MFMA's padded K)
STACK_MAX_SHAPES = 32  # shape classes the fused stacked discriminator takes


class DeepConvDiscNet(nn.Module):
    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.conv1 = nn.Conv1d(input_dim, 512, 1)
        self.conv2 = nn.Conv1d(512, 256, 1)
        self.conv3 = nn.Conv1d(256, 256, 1)
        self.conv4 = nn.Conv1d(256, 64, 1)
        self.conv5 = nn.Conv1d(64, 64, 1)
        self.fc = nn.Linear(64, output_dim)
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def forward(self, x):
        h = x.contiguous()
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5):
            h = LinearFunction.apply(h, conv.weight, conv.bias, ACT_LRELU, None, 0.0)
        return LinearFunction.apply(h, self.fc.weight, self.fc.bias, ACT_NONE, None, 0.0)


def _f32(t, name, numel=None):
    if t.device.type != "cuda":
        raise ValueError(f"{name}: pcadv ops run on the HIP device only (got {t.device})")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} elements, got {t.numel()}")
    return t


def _i32(t, name, numel):
    if t.dtype != torch.int32 or t.numel() != numel or t.device.type != "cuda" \
            or not t.is_contiguous():
        raise TypeError(f"{name}: expected {numel} contiguous int32 on the HIP device")
    return t


# The two fused discriminators share their host path: one builder for the
# common prefix of the two args structs, one backward and one workspace body.
# What differs per net: the struct, the lengths of the parameters after conv1's
# weight, and the struct's names for the per-row output and its two gradients.
_PWD = ("pwdisc", _lib.PwdiscArgs, ("out", "dout_d", "dout_adv"))
_STK = ("stackdisc", _lib.StackdiscArgs, ("m", "dm_d", "dm_adv"))
_CONV_SIZES = (64, 4096, 64, 4096, 64, 8192, 128)  # conv1's bias .. conv4's bias


def _workspace(net, rows, device, max_workgroups, zero):
    n = getattr(_lib.load(), f"pcadv_{net[0]}_workspace_bytes")(int(rows), int(max_workgroups))
    return (torch.zeros if zero else torch.empty)(max(int(n), 256), device=device,
                                                  dtype=torch.uint8)


def pwdisc_workspace(rows, device, max_workgroups=0, zero=True):
    """The workspace the forward and the backward of `rows` points share.  Only a
    forward with losses needs it zeroed (its ticket); the backward writes its
    slabs before it reads them, and a forward without losses takes ws=None."""
    return _workspace(_PWD, rows, device, max_workgroups, zero)


def stackdisc_workspace(rows, device, max_workgroups=0, zero=True):
    """The workspace the stacked discriminator's forward and backward of `rows`
    points share (zeroed once for the forward's ticket, as pwdisc_workspace)."""
    return _workspace(_STK, rows, device, max_workgroups, zero)


def _args(net, logits, ncls, n0, n1, t0, t1, params, out, argc, ws, max_workgroups):
    """The args struct of `net` with everything the two structs share filled in:
    logits, the row counts and transforms, conv1..'s parameters, the per-row
    output, argc, max_workgroups and the workspace."""
    _, struct, (out_name, _, _) = net
    rows = n0 + n1
    if logits.dim() != 2 or logits.shape[0] != rows or logits.shape[1] < ncls \
            or logits.stride(1) != 1:
        raise ValueError(f"logits: expected point-major ({rows}, >= {ncls}) rows, "
                         f"got {tuple(logits.shape)} with strides {logits.stride()}")
    if logits.device.type != "cuda" or logits.dtype != torch.float32:
        raise TypeError("logits: expected torch.float32 on the HIP device")
    if not 2 <= ncls <= PWD_MAX_DIM:
        raise ValueError(f"ncls: the fused discriminator takes 2..{PWD_MAX_DIM} channels, got {ncls}")
    sizes = (64 * ncls,) + _CONV_SIZES
    a = struct()
    if net is _STK:
        if len(params) != 10:
            raise ValueError("params: expected conv1..conv5's weights and biases (10 tensors)")
        a.num_shapes = S = params[9].numel()
        if not 2 <= S <= STACK_MAX_SHAPES:
            raise ValueError(f"num_shapes: the fused discriminator takes 2..{STACK_MAX_SHAPES}, got {S}")
        sizes += (S, S)
    for i, (p, n) in enumerate(zip(params, sizes)):
        (a.b if i % 2 else a.w)[i // 2] = _f32(p, f"D parameter {i}", n).data_ptr()
    a.logits, a.ld = _vp(logits), logits.stride(0) if rows > 1 else max(logits.stride(0), ncls)
    a.ncls, a.n0, a.n1, a.t0, a.t1 = ncls, n0, n1, int(t0), int(t1)
    setattr(a, out_name, _vp(_f32(out, out_name, rows)))
    a.argc = _vp(_i32(argc, "argc", rows))
    a.max_workgroups = int(max_workgroups)
    if ws is not None:
        a.workspace, a.workspace_bytes = _vp(ws), ws.numel()
    return a


def _backward(net, logits, ncls, n0, n1, t0, t1, params, out, argc, ws, d_d, grads, d_adv,
              lambda_adv, dlogits, max_workgroups, x_out):
    name, _, (_, d_name, adv_name) = net
    a = _args(net, logits, ncls, n0, n1, t0, t1, params, out, argc, ws, max_workgroups)
    setattr(a, d_name, _vp(_f32(d_d, d_name, n0 + n1)))
    setattr(a, adv_name, _vp(None if d_adv is None else _f32(d_adv, adv_name, n1)))
    a.lambda_adv = float(lambda_adv)
    for i, (g, p) in enumerate(zip(grads[:8], params[:8])):
        (a.db if i % 2 else a.dw)[i // 2] = _f32(g, f"D gradient {i}", p.numel()).data_ptr()
    if x_out is not None:
        a.x_out = _vp(_f32(x_out, "x_out", 3 * (n0 + n1) * 64))
    if dlogits is not None:
        if dlogits.dim() != 2 or dlogits.shape[0] != n0 + n1 or dlogits.shape[1] < ncls \
                or dlogits.stride(1) != 1 or dlogits.dtype != torch.float32 \
                or dlogits.device.type != "cuda":
            raise ValueError("dlogits: expected point-major float32 rows like logits")
        a.dlogits, a.ldd = _vp(dlogits), max(dlogits.stride(0), ncls)
    entry = f"pcadv_{name}_backward"
    check(getattr(_lib.load(), entry)(ctypes.byref(a), stream_ptr()), entry)


def pwdisc_forward(logits, ncls, n0, n1, t0, t1, params, out, argc, ws, *, losses=None,
                   soft0=None, soft1=None, soft_out=None, seed=0, step_count=None, dout_d=None,
                   dout_adv=None, max_workgroups=0):
    """pcadv_pwdisc_forward on the current stream (include/pcadv.h): out, argc
    and, with `losses` (4 floats), the BCE terms with dout_d / dout_adv."""
    a = _args(_PWD, logits, ncls, n0, n1, t0, t1, params, out, argc, ws, max_workgroups)
    if losses is not None:
        a.losses = _vp(_f32(losses, "losses", 4))
        a.soft0 = _vp(None if soft0 is None else _f32(soft0, "soft0", n0))
        a.soft1 = _vp(None if soft1 is None else _f32(soft1, "soft1", n1))
        a.soft_out = _vp(None if soft_out is None else _f32(soft_out, "soft_out", n0 + n1))
        a.rng_seed = int(seed)
        a.step_count = _vp(step_count)
        a.dout_d = _vp(_f32(dout_d, "dout_d", n0 + n1))
        a.dout_adv = _vp(None if dout_adv is None else _f32(dout_adv, "dout_adv", n1))
    check(_lib.load().pcadv_pwdisc_forward(ctypes.byref(a), stream_ptr()), "pcadv_pwdisc_forward")


def pwdisc_backward(logits, ncls, n0, n1, t0, t1, params, out, argc, ws, dout_d, grads, *,
                    dout_adv=None, lambda_adv=1.0, dlogits=None, max_workgroups=0, x_out=None):
    """pcadv_pwdisc_backward on the current stream: `grads` (eight
    parameter-shaped tensors, state_dict order) are written, and rows
    [n0, n0 + n1) of `dlogits` when it and dout_adv are given.  x_out
    (3, n0 + n1, 64), optional, receives the recomputed x1..x3."""
    _backward(_PWD, logits, ncls, n0, n1, t0, t1, params, out, argc, ws, dout_d, grads, dout_adv,
              lambda_adv, dlogits, max_workgroups, x_out)


def stackdisc_forward(logits, ncls, n0, n1, t0, t1, params, m, argc, d_out, ws, *,
                      shape_logits=None, losses=None, shape_label=None, pts_per_cloud=0,
                      lambda_disc_shape=1.0, soft0=None, soft1=None, soft_out=None, seed=0,
                      step_count=None, dm_d=None, dm_adv=None, grads5=None, bad_rows=None,
                      max_workgroups=0, semi_th=None, loss_semi=None, kept=None):
    """pcadv_stackdisc_forward on the current stream (include/pcadv.h): m, argc,
    d_out, optionally shape_logits (rows, num_shapes), and, with `losses` (5
    floats), the BCE and shape terms with dm_d / dm_adv, conv5's gradients
    grads5 = (dw5, db5) and the int32 bad_rows counter.

    With semi_th, pcadv_stackdisc_forward_semi instead: the same outputs, and the
    semi-supervised term's scan of the no-GT rows in the same launch: loss_semi
    (1 float) and kept (1 int32, the number of rows with d_out above semi_th).
    It needs `losses`."""
    if semi_th is not None and losses is None:
        raise ValueError("semi_th: the scan runs with the loss terms, `losses` is required")
    a = _args(_STK, logits, ncls, n0, n1, t0, t1, params, m, argc, ws, max_workgroups)
    S = a.num_shapes
    a.d_out = _vp(_f32(d_out, "d_out", n0 + n1))
    if shape_logits is not None:
        a.shape_logits = _vp(_f32(shape_logits, "shape_logits", (n0 + n1) * S))
    if losses is not None:
        a.losses = _vp(_f32(losses, "losses", 5))
        if n0:
            if pts_per_cloud < 1 or n0 % pts_per_cloud:
                raise ValueError(f"pts_per_cloud = {pts_per_cloud} does not divide the {n0} GT rows")
            a.shape_label = _vp(_i32(shape_label, "shape_label", n0 // pts_per_cloud))
            a.pts_per_cloud = int(pts_per_cloud)
        a.lambda_disc_shape = float(lambda_disc_shape)
        a.soft0 = _vp(None if soft0 is None else _f32(soft0, "soft0", n0))
        a.soft1 = _vp(None if soft1 is None else _f32(soft1, "soft1", n1))
        a.soft_out = _vp(None if soft_out is None else _f32(soft_out, "soft_out", n0 + n1))
        a.rng_seed = int(seed)
        a.step_count = _vp(step_count)
        a.dm_d = _vp(_f32(dm_d, "dm_d", n0 + n1))
        a.dm_adv = _vp(None if dm_adv is None else _f32(dm_adv, "dm_adv", n1))
        a.dw[4] = _f32(grads5[0], "conv5's weight gradient", S).data_ptr()
        a.db[4] = _f32(grads5[1], "conv5's bias gradient", S).data_ptr()
        a.bad_rows = _vp(_i32(bad_rows, "bad_rows", 1))
    if semi_th is not None:
        sm = _lib.StackdiscSemi(float(semi_th), _vp(_f32(loss_semi, "loss_semi", 1)),
                                _vp(_i32(kept, "kept", 1)))
        check(_lib.load().pcadv_stackdisc_forward_semi(ctypes.byref(a), ctypes.byref(sm),
                                                       stream_ptr()),
              "pcadv_stackdisc_forward_semi")
        return
    check(_lib.load().pcadv_stackdisc_forward(ctypes.byref(a), stream_ptr()),
          "pcadv_stackdisc_forward")


def row_semi_apply(logits, ncls, d_out, semi_th, scale, kept, dlogits, labels_out=None):
    """pcadv_row_semi_apply on the current stream (include/pcadv.h): with K =
    kept[0] > 0 (device int32), scale / K (softmax - onehot(argmax)) is ADDED to
    the rows of dlogits whose d_out is above semi_th.  logits and dlogits are
    point-major (M, >= ncls) rows, d_out (M,); labels_out (M int32, optional)
    receives every row's pseudo-label, 255 where ignored."""
    M = d_out.numel()
    for t, name in ((logits, "logits"), (dlogits, "dlogits")):
        if t.dim() != 2 or t.shape[0] != M or t.shape[1] < ncls or t.stride(1) != 1 \
                or t.dtype != torch.float32 or t.device.type != "cuda":
            raise ValueError(f"{name}: expected point-major float32 ({M}, >= {ncls}) rows on the "
                             "HIP device")
    check(_lib.load().pcadv_row_semi_apply(
        _vp(logits), max(logits.stride(0), ncls), _vp(_f32(d_out, "d_out", M)), M, ncls,
        float(semi_th), float(scale), _vp(_i32(kept, "kept", 1)), _vp(dlogits),
        max(dlogits.stride(0), ncls), None if labels_out is None else
        _vp(_i32(labels_out, "labels_out", M)), stream_ptr()), "pcadv_row_semi_apply")


def stackdisc_backward(logits, ncls, n0, n1, t0, t1, params, m, argc, ws, dm_d, grads, *,
                       dm_adv=None, lambda_adv=1.0, dlogits=None, max_workgroups=0, x_out=None):
    """pcadv_stackdisc_backward on the current stream: the first eight of
    `grads` (conv1..conv4, state_dict order) are written, and rows
    [n0, n0 + n1) of `dlogits` when it and dm_adv are given.  x_out
    (3, n0 + n1, 64), optional, receives the recomputed x1..x3."""
    _backward(_STK, logits, ncls, n0, n1, t0, t1, params, m, argc, ws, dm_d, grads, dm_adv,
              lambda_adv, dlogits, max_workgroups, x_out)


def _point_major(x):
    """x (B, C, N) as point-major rows (B * N, ld) without a copy when it is a
    permuted view of point-major storage (what PointNetSeg.forward returns)."""
    B, C, N = x.shape
    xt = x.permute(0, 2, 1)  # (B, N, C)
    if not xt.is_contiguous():
        xt = xt.contiguous()
    return xt.reshape(B * N, C)


def _autograd_backward(net, ctx, dout):
    """The backward of both autograd nodes: the fused backward scaled per row by
    the incoming gradient.  Returns (dx, conv1..conv4's gradients)."""
    rows, out, argc, *ps = ctx.saved_tensors
    B, C, N = ctx.dims
    M = B * N
    d = dout.reshape(M).contiguous().float()
    grads = [torch.empty_like(p) for p in ps[:8]]
    need_dx = ctx.needs_input_grad[0]
    dl = torch.empty(M, C, device=rows.device) if need_dx else None
    ws = _workspace(net, M, rows.device, 0, zero=False)
    _backward(net, rows, C, 0, M, PWD_NONE, PWD_NONE, ps, out, argc, ws, d, grads,
              d if need_dx else None, 1.0, dl, 0, None)
    dx = dl.view(B, N, C).permute(0, 2, 1) if need_dx else None
    return (dx, *grads)


class _PointwiseDisc(torch.autograd.Function):
    """x (B, C, N) -> (B * N,) logits: the fused forward, and the fused backward
    scaled per row by the incoming gradient."""

    @staticmethod
    def forward(ctx, x, *params):
        B, C, N = x.shape
        rows = _point_major(x.detach())
        M = B * N
        out = torch.empty(M, device=x.device)
        argc = torch.empty(M, device=x.device, dtype=torch.int32)
        ps = [p.detach().contiguous() for p in params]
        pwdisc_forward(rows, C, 0, M, PWD_NONE, PWD_NONE, ps, out, argc, None)
        ctx.save_for_backward(rows, out, argc, *ps)
        ctx.dims = (B, C, N)
        ctx.mark_non_differentiable(argc)
        return out, argc

    @staticmethod
    def backward(ctx, dout, _dargc):
        return _autograd_backward(_PWD, ctx, dout)


class _StackDiscMax(torch.autograd.Function):
    """x (B, C, N) -> m (B * N,), the channel max of lrelu(conv4(..)): the fused
    forward, and the fused backward scaled per row by the incoming gradient.
    conv5 and the logsumexp after it are 16 numbers per point and stay in torch,
    so both of the module's outputs are differentiable through this one node.
    The kernel also forms d_out per row; on this path it is discarded, and the
    module's disc_out is torch's value computed from m, not the kernel's."""

    @staticmethod
    def forward(ctx, x, *params):
        B, C, N = x.shape
        rows = _point_major(x.detach())
        M = B * N
        m = torch.empty(M, device=x.device)
        d = torch.empty(M, device=x.device)
        argc = torch.empty(M, device=x.device, dtype=torch.int32)
        ps = [p.detach().contiguous() for p in params]
        stackdisc_forward(rows, C, 0, M, PWD_NONE, PWD_NONE, ps, m, argc, d, None)
        ctx.save_for_backward(rows, m, argc, *ps)
        ctx.dims = (B, C, N)
        return m

    @staticmethod
    def backward(ctx, dm):
        return (*_autograd_backward(_STK, ctx, dm), None, None)  # conv5 acts after this node


class _FusedDiscNet(nn.Module):
    """What the two fused discriminators share: conv1..conv4 (ncls -> 64 -> 64
    -> 64 -> 128, registered first and in this order, so the state_dicts are the
    reference's) and the checks of the constructor's ranges and of the input."""
    fills_rows = False  # PointwiseDiscNet: B * N must fill rows of input_pts

    def __init__(self, input_pts, input_dim):
        super().__init__()
        if not 2 <= int(input_dim) <= PWD_MAX_DIM:
            raise ValueError(f"input_dim: the fused discriminator takes 2..{PWD_MAX_DIM} "
                             f"channels, got {input_dim}")
        if int(input_pts) < 1:
            raise ValueError(f"input_pts: expected a positive point count, got {input_pts}")
        self.input_pts = int(input_pts)
        self.input_dim = int(input_dim)
        self.conv1 = nn.Conv1d(input_dim, 64, 1)
        self.conv2 = nn.Conv1d(64, 64, 1)
        self.conv3 = nn.Conv1d(64, 64, 1)
        self.conv4 = nn.Conv1d(64, 128, 1)

    def check_input(self, x):
        if x.dim() != 3 or x.shape[1] != self.input_dim:
            raise ValueError(f"x: expected B x {self.input_dim} x N, got {tuple(x.shape)}")
        if self.fills_rows and (x.shape[0] * x.shape[2]) % self.input_pts:
            raise ValueError(f"x: {x.shape[0]} x {x.shape[2]} points do not fill rows of "
                             f"input_pts = {self.input_pts}")
        if not x.is_floating_point() or x.dtype != torch.float32:
            raise TypeError(f"x: expected torch.float32, got {x.dtype}")

    def _apply_fused(self, fn, x):
        self.check_input(x)
        if x.device.type != "cuda":
            raise ValueError(f"x: pcadv ops run on the HIP device only (got {x.device})")
        return fn.apply(x, *[p for _, p in self.named_parameters()])


class PointwiseDiscNet(_FusedDiscNet):
    """models/discriminator.py:53-79.  forward(x: B x input_dim x N) ->
    B*N/input_pts x input_pts (B x N when N == input_pts)."""
    fills_rows = True

    def forward(self, x):
        out, _ = self._apply_fused(_PointwiseDisc, x)
        return out.view(-1, self.input_pts)


class StackDiscNet(_FusedDiscNet):
    """models/discriminator.py:139-175.  forward(x: B x input_dim x N) ->
    (shape_logits B x num_shapes x N, disc_out B x N x 1)."""

    def __init__(self, input_pts, input_dim, num_shapes):
        super().__init__(input_pts, input_dim)
        if not 2 <= int(num_shapes) <= STACK_MAX_SHAPES:
            raise ValueError(f"num_shapes: the fused discriminator takes 2..{STACK_MAX_SHAPES} "
                             f"shape classes, got {num_shapes}")
        self.num_shapes = int(num_shapes)
        self.conv5 = nn.Conv1d(1, num_shapes, 1)

    def forward(self, x):
        m = self._apply_fused(_StackDiscMax, x)
        B, _, N = x.shape
        shape_logits = self.conv5(m.view(B, 1, N))  # B x S x N
        out = torch.logsumexp(shape_logits.transpose(2, 1), dim=2, keepdim=True)
        return shape_logits, out / (out + 1.0)


class BaseDiscNet(nn.Module):
    """models/discriminator.py:82-98, the dual discriminator's shared trunk.
    forward(x: B x input_dim x N) -> B x output_dim x N.  conv4 is registered,
    as in the reference, and never used: it receives no gradient."""

    def __init__(self, input_pts, input_dim, output_dim):
        super().__init__()
        self.input_pts = input_pts
        self.input_dim, self.output_dim = int(input_dim), int(output_dim)
        self.conv1 = nn.Conv1d(input_dim, 64, 1)
        self.conv2 = nn.Conv1d(64, 64, 1)
        self.conv3 = nn.Conv1d(64, output_dim, 1)
        self.conv4 = nn.Conv1d(output_dim, output_dim, 1)
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def forward(self, x):
        for conv in (self.conv1, self.conv2, self.conv3):
            x = self.leaky_relu(conv(x))
        return x


class ShapeDiscNet(nn.Module):
    """models/discriminator.py:100-117.  forward(x: B x shared_output_dim x N)
    -> B x num_shapes (the max runs over the points of each cloud)."""

    def __init__(self, shared_output_dim, num_shapes):
        super().__init__()
        self.interm_dim = 512
        self.shared_output_dim, self.num_shapes = int(shared_output_dim), int(num_shapes)
        self.conv = nn.Conv1d(shared_output_dim, self.interm_dim, 1)
        self.fc1 = nn.Linear(self.interm_dim, 64)
        self.fc2 = nn.Linear(64, num_shapes)
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def forward(self, x):
        x = self.leaky_relu(self.conv(x))
        x = torch.max(x, 2, keepdim=False)[0].view(-1, self.interm_dim)
        return self.fc2(self.leaky_relu(self.fc1(x)))


class PointDiscNet(nn.Module):
    """models/discriminator.py:119-137.  forward(x: B x shared_output_dim x N)
    -> B*N/input_pts x input_pts: per point the max over the 128 channels."""

    def __init__(self, shared_output_dim, input_pts):
        super().__init__()
        self.input_pts = input_pts
        self.shared_output_dim = int(shared_output_dim)
        self.conv1 = nn.Conv1d(shared_output_dim, 256, 1)
        self.conv2 = nn.Conv1d(256, 128, 1)
        self.conv3 = nn.Conv1d(128, 128, 1)
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.2, inplace=True)

    def forward(self, x):
        for conv in (self.conv1, self.conv2, self.conv3):
            x = self.leaky_relu(conv(x))
        x = torch.max(x.transpose(2, 1), 2, keepdim=True)[0]
        return x.view(-1, self.input_pts)

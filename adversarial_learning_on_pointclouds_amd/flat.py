"""What every fused train step keeps on the host side of its kernels: one
network's parameters, gradients and Adam moments as flat f32 buffers the torch
module and optimizer see as views (FlatAdam), and the warm-up / capture /
restore of a HIP graph (capture_graphs).  Plain torch: no native library, and
FlatAdam runs on any device.
"""
from __future__ import annotations

import torch


def pad64(n):
    """n floats rounded up to a 256-byte boundary."""
    return (n + 63) // 64 * 64


def sequential_layout(module, layout=None, start=0):
    """`layout` ({name: offset}, default empty) extended by the module's other
    parameters in named_parameters() order from `start`, each padded to 64
    floats.  Returns (layout, numel)."""
    layout, off = dict(layout or {}), start
    for name, p in module.named_parameters():
        if name not in layout:
            layout[name] = off
            off += pad64(p.numel())
    return layout, off


def _step_tensor(optimizer, p, t):
    """'step' as torch.optim.Adam keeps it for p: an f32 scalar on p's device
    when its group is capturable or fused (the step then runs on the device,
    and Adam refuses a CPU count), a CPU f32 scalar otherwise."""
    for g in optimizer.param_groups:
        if any(q is p for q in g["params"]):
            if g.get("capturable", False) or g.get("fused", False):
                return torch.tensor(float(t), dtype=torch.float32, device=p.device)
            break
    return torch.tensor(float(t), dtype=torch.float32)


def set_optimizer_step(optimizer, t):
    """Every state entry's 'step' = t (the device step counter's value)."""
    if optimizer is None:
        return
    for p, st in optimizer.state.items():
        if st:
            st["step"] = _step_tensor(optimizer, p, t)


class FlatAdam:
    """One network's training state as flat f32 buffers: `param`, `grad`, `m`,
    `v` of `numel` floats, parameter `name` at `layout[name]`.

    The module's values are copied in and each p.data becomes a view of
    `param`; Adam state the optimizer already holds (a load_state_dict before
    the first iteration, or the views of a step object the trainer replaced)
    is copied into `m` / `v` and its largest 'step' is `t0`; each p.grad becomes
    a view of `grad` (`grad_views`, in named_parameters() order) and the
    optimizer's exp_avg / exp_avg_sq views of `m` / `v`, so checkpoints, eval
    passes and optimizer.state_dict() keep working on the same memory.

    layout=None: sequential_layout(module).  grad=: a caller's buffer of numel
    floats (the adversarial steps place both networks' gradients in one)."""

    def __init__(self, module, optimizer, device, layout=None, numel=None, grad=None):
        named = list(module.named_parameters())
        if layout is None:
            layout, numel = sequential_layout(module)
        elif {n for n, _ in named} != set(layout):
            raise ValueError(f"{type(module).__name__}: parameters "
                             f"{sorted({n for n, _ in named} ^ set(layout))} "
                             "do not match the fused-step layout")
        if numel is None:
            numel = max(layout[n] + p.numel() for n, p in named)
        self.module, self.optimizer = module, optimizer
        self.layout, self.numel = layout, int(numel)
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.offsets = [layout[n] for n in self.names]
        self.param, self.m, self.v = (torch.zeros(self.numel, device=device, dtype=torch.float32)
                                      for _ in range(3))
        if grad is None:
            grad = torch.zeros(self.numel, device=device, dtype=torch.float32)
        elif grad.numel() != self.numel or grad.dtype != torch.float32 or not grad.is_contiguous():
            raise ValueError(f"grad: {self.numel} contiguous float32 expected")
        self.grad = grad
        self.t0 = 0
        for p, o in zip(self.params, self.offsets):
            k = p.numel()
            self.param[o:o + k].copy_(p.detach().reshape(-1))
            st = optimizer.state.get(p) if optimizer is not None else None
            if st and "exp_avg" in st:
                self.m[o:o + k].copy_(st["exp_avg"].detach().reshape(-1))
                self.v[o:o + k].copy_(st["exp_avg_sq"].detach().reshape(-1))
                self.t0 = max(self.t0, int(float(st.get("step", 0))))
            p.data = self.param[o:o + k].view_as(p)
        self.grad_views = list(self.views(self.grad).values())
        self.bind(self.t0)

    def views(self, flat):
        """{name: the parameter-shaped view of a buffer laid out like `param`}."""
        return {n: flat[o:o + p.numel()].view_as(p)
                for n, p, o in zip(self.names, self.params, self.offsets)}

    def bind(self, step):
        """p.grad = its view of `grad`; the optimizer's state = views of `m` /
        `v` with 'step' = the completed-step count."""
        mv, vv = self.views(self.m), self.views(self.v)
        for n, p, gv in zip(self.names, self.params, self.grad_views):
            p.grad = gv
            if self.optimizer is not None:
                self.optimizer.state[p] = {"step": _step_tensor(self.optimizer, p, step),
                                           "exp_avg": mv[n], "exp_avg_sq": vv[n]}


def adam_hyper(optimizer):
    """(lr, betas, eps) of the optimizer's first param group, as floats."""
    g = optimizer.param_groups[0]
    return float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"])


def snapshot(state):
    """Copies of the tensors a capture's warm-up changes.  Detached, under
    no_grad: a clone of a parameter made with grad mode on would hold its
    AccumulateGrad node (created on the launching stream) alive into the
    capture, where it then runs on the wrong stream (the HIP runtime crashed
    at capture end).  Checked, so a future state list cannot bring it back."""
    with torch.no_grad():
        saved = [t.detach().clone() for t in state]
    bad = [i for i, t in enumerate(saved) if t.grad_fn is not None or t.requires_grad]
    if bad:
        raise RuntimeError(f"capture state snapshot {bad} carries autograd history")
    return saved


def restore(state, saved):
    with torch.no_grad():
        for dst, src in zip(state, saved):
            dst.copy_(src)


def capture_graphs(device, warmup, captures, state, sync_before_capture=False):
    """HIP graphs of `captures` (one callable -> its graph, a sequence of them
    -> a list, each in a graph of its own) after one run of `warmup` on a side
    stream, outside the capture.  `state` lists the tensors the warm-up (and a
    capture that dies half way) changes: they are what they were before, also
    when the warm-up or a capture raises.  sync_before_capture: a device
    synchronize between the warm-up and the capture (warm-ups that start
    collectives)."""
    single = callable(captures)
    saved = snapshot(state)
    try:
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            warmup()
        cur.wait_stream(side)
        if sync_before_capture:
            torch.cuda.synchronize()
        graphs = []
        for fn in ([captures] if single else captures):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs.append(g)
    finally:
        torch.cuda.synchronize()
        restore(state, saved)
    return graphs[0] if single else graphs

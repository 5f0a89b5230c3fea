"""Data-parallel adversarial step: one process per GPU, RCCL over xGMI.

The reference is single-process (train_classification.py:93); the north star
adds data parallelism.  Clouds are independent, so each rank runs the fused
step on its own B-cloud shards of the GT and noGT batches; the only exchange
is an all-reduce(AVG) of the concatenated generator + discriminator gradient
buffer (811 240 + 238 785 fp32 = 4.2 MB) between backward and the replicated
Adam updates.  With equal shards this equals the single-process step on the
global batch, since CE/BCE are batch means (mean of per-rank means).

By default (round 6) the iteration is the whole step without Adam, ONE
all-reduce of the buffer, then both Adams, and over RCCL the three are
captured as ONE HIP graph (capture_single).  The round-5 default - two
buckets overlapped with the backward (the head and discriminator gradients,
3.6 MB, all-reduced on RCCL's stream while the feature backward runs; the
conv1..conv4 bucket, 0.58 MB, beside the first bucket's Adam) - stays
available as overlap=True: on a one-rank RCCL group it cost 62 us per
iteration over the plain step against 11 us for the captured single
all-reduce, and its kernel trace shows the feature backward waiting for the
RCCL kernel, so the overlap it was built for does not happen (bench.py
--config dp1).
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .flat import capture_graphs


def _avg_(t, group=None):
    _avg_async(t, group)()


def _avg_async(t, group=None):
    """Start all-reduce(AVG) of t; returns the wait() that completes it."""
    if dist.get_backend(group) == "nccl":
        work = dist.all_reduce(t, op=dist.ReduceOp.AVG, group=group, async_op=True)
        return work.wait
    work = dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group, async_op=True)  # gloo: no AVG
    world = dist.get_world_size(group)

    def done():
        work.wait()
        t.div_(world)
    return done


class DataParallelAdvStep:
    """Wraps an AdvTrainStep-like object exposing grads(), adam(), grad_flat,
    g_param, d_param and losses.

    Device-drawn dropout masks and soft D labels are keyed by the GLOBAL
    batch's rows (global_rng, default): this rank is taken to hold rows
    [rank B, rank B + B) of the global GT and no-GT batches, the step's seed
    becomes rank 0's, and so the ranks draw exactly the slices of the
    one-process step on the global batch (pcadv_adv_args.rng_rank / rng_world).
    global_rng=False keeps the step's own keying (every rank then draws the
    SAME masks for its local rows unless the seeds differ)."""

    def __init__(self, step, group=None, broadcast_params=True, overlap=None, global_rng=True):
        """overlap=True: bucket the all-reduce around the feature backward (the
        round-5 form; needs a step with parts); default: one all-reduce."""
        self.step, self.group = step, group
        self.overlap = overlap
        self.graph_form = None  # set by graphed()
        if broadcast_params:  # identical initial weights on every rank
            dist.broadcast(step.g_param, src=0, group=group)
            dist.broadcast(step.d_param, src=0, group=group)
        if global_rng and hasattr(step, "set_rng_rank"):
            step.set_rng_rank(dist.get_rank(group), dist.get_world_size(group))
            seed = torch.tensor([step.seed & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64,
                                device=step.g_param.device if dist.get_backend(group) == "nccl"
                                else "cpu")
            dist.broadcast(seed, src=dist.get_global_rank(group, 0) if group is not None else 0,
                           group=group)
            step.seed = int(seed.item())

    def _split(self):
        return bool(self.overlap) and getattr(self.step, "supports_parts", False)

    def __call__(self, pts_gt, labels, pts_nogt, masks=None, soft=None, semi=False):
        # semi: each rank's pseudo-label CE is the mean over its own kept clouds,
        # so the averaged gradient weights ranks equally (the global-batch mean
        # would weight them by their kept counts)
        s = self.step
        if self._split():
            s(pts_gt, labels, pts_nogt, masks, soft, apply_adam=False, semi=semi, part=1)
            done = _avg_async(s.early_grads(), self.group)
            s(pts_gt, labels, pts_nogt, masks, soft, apply_adam=False, semi=semi, part=2)
            done()
            if getattr(s, "supports_split_adam", False):
                done_late = _avg_async(s.late_grads(), self.group)
                s.adam(part=1)  # the early bucket's parameters, beside the late all-reduce
                done_late()
                s.adam(part=2)
                return s.losses
            _avg_(s.late_grads(), self.group)
        else:
            s.grads(pts_gt, labels, pts_nogt, masks, soft, semi=semi)
            _avg_(s.grad_flat, self.group)
        s.adam()
        return s.losses

    def graphed(self, pts_gt, labels, pts_nogt):
        """The iteration over resident buffers as replayable graphs: ONE graph
        with the collectives captured over RCCL (capture_single), graphs around
        eager collectives otherwise (gloo cannot be captured).  If the RCCL
        capture itself fails (a runtime that refuses to capture the collective:
        every rank takes the same branch, so the ranks stay in step), the
        iteration falls back to the graphs around eager all-reduces and
        self.graph_form says so."""
        if dist.get_backend(self.group) == "nccl":
            try:
                g = self.capture_single(pts_gt, labels, pts_nogt)
                self.graph_form = "one graph, all-reduce captured"
                return g
            except RuntimeError as e:  # torch reports capture failures as RuntimeError
                torch.cuda.synchronize()
                self.graph_form = f"graphs around eager all-reduces (capture failed: {e})"[:300]
                dist.barrier(group=self.group)
        else:
            self.graph_form = "graphs around eager all-reduces (gloo)"
        return self.capture(pts_gt, labels, pts_nogt)

    def capture(self, pts_gt, labels, pts_nogt):
        """HIP graphs for the compute halves around the (eager) all-reduce."""
        s = self.step
        if self._split():
            g_fwd = (s.capture_on(pts_gt, labels, pts_nogt, apply_adam=False, part=1),
                     s.capture_on(pts_gt, labels, pts_nogt, apply_adam=False, part=2))
        else:
            g_fwd = s.capture_on(pts_gt, labels, pts_nogt, apply_adam=False)
        parts = (1, 2) if self._split() and getattr(s, "supports_split_adam", False) else (0,)

        def warmup():
            for part in parts:
                s.adam(part=part)
        g_adam = capture_graphs(s.device, warmup, [lambda part=part: s.adam(part=part)
                                                   for part in parts], s.graph_state())
        return _DPGraph(g_fwd, g_adam, s, self.group)

    def capture_single(self, pts_gt, labels, pts_nogt):
        """The whole data-parallel iteration as ONE HIP graph: the step's parts,
        the two all-reduces (captured on RCCL's stream, forked from and joined
        back to the capturing stream by the collectives' own event waits) and
        the split Adam, in the order __call__ issues them.  One replay per
        iteration instead of four graphs around host-issued collectives
        (VERDICT r05 item 6).  State is left as it was before the capture."""
        s = self.step
        def body():
            self(pts_gt, labels, pts_nogt)
        # the warm-up initialises the communicators and kernels; its collectives
        # are through before the capture begins
        return capture_graphs(s.device, body, body, s.graph_state(), sync_before_capture=True)


class _DPGraph:
    def __init__(self, g_fwd, g_adam, step, group):
        self.g_fwd, self.g_adam, self.step, self.group = g_fwd, g_adam, step, group

    def replay(self):
        s = self.step
        if isinstance(self.g_fwd, tuple):  # bucketed, overlapped with the feature backward
            self.g_fwd[0].replay()
            done = _avg_async(s.early_grads(), self.group)
            self.g_fwd[1].replay()
            done()
            if len(self.g_adam) == 2:  # early bucket's Adam beside the late all-reduce
                done_late = _avg_async(s.late_grads(), self.group)
                self.g_adam[0].replay()
                done_late()
                self.g_adam[1].replay()
                return s.losses
            _avg_(s.late_grads(), self.group)
        else:
            self.g_fwd.replay()
            _avg_(s.grad_flat, self.group)
        self.g_adam[0].replay()
        return s.losses

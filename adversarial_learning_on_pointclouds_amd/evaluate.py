"""Native test passes: run_testing / run_testing_seg (utils/trainer.py:30-69,
:72-143) over a DeviceCloudLoader without per-op Python or a host sync per
batch.

A pass takes the loader's epoch order once, replays one HIP graph per full
batch (the batch gathered at a device cursor with the loader's own Philox
jitter, the model's eval-mode forward launches, pcadv_row_eval, the cursor /
RNG-step epilogue), runs a ragged last batch through the same launches
eagerly, and ends with one copy of the device accumulator (and, for seg, the
per-cloud IoU records) to pinned memory and one event wait.  The logits are
bitwise the module's in eval mode, so predictions, accuracy and IoU are the
module path's; the loss differs from torch's CrossEntropyLoss by f32 rounding.

There is no fallback inside this module: an evaluator refuses what it does not
cover (trainer.run_testing* decide which path a configuration takes).
"""
from __future__ import annotations

import weakref

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream_ptr
from .dataset import DeviceCloudLoader
from .flat import capture_graphs
from .metric import object_names, part_ranges
from .pointnet import PointNetCls

__all__ = ["ClsEvaluator", "SegEvaluator", "evaluator_for", "MAX_CLASSES"]

MAX_CLASSES = 64  # pcadv_row_eval: a row's classes over 16 lanes x 4


class _Evaluator:
    KIND = None

    def __init__(self, model, loader):
        if type(loader) is not DeviceCloudLoader:
            raise TypeError(f"{type(self).__name__} evaluates a DeviceCloudLoader (the split resident "
                            f"on the HIP device), got {type(loader).__name__}; other loaders take "
                            "the module path of trainer.run_testing*")
        if loader.kind != self.KIND:
            raise TypeError(f"{type(self).__name__}: a {self.KIND} loader is required, got "
                            f"{loader.kind}")
        if loader.world != 1:
            raise ValueError(f"{type(self).__name__}: sharded (data-parallel) loaders are not covered")
        self._check_model(model)
        self.lib = _lib.load()
        self._model = weakref.ref(model)  # the cache is keyed by the model: no cycle through it
        self.loader = loader
        dev = self.device = loader.device
        B, N = loader.B, loader.npts
        self.B, self.N = B, N
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)  # batch cursor | RNG step
        self.order = torch.zeros(loader.order_len, dtype=torch.int64, device=dev)
        self.pts = torch.zeros(B, N, 3, device=dev)
        self.lab = torch.zeros(B, int(loader.labels.shape[1]), dtype=torch.int64, device=dev)
        self.acc = torch.zeros(4, dtype=torch.float64, device=dev)
        self.acc_host = torch.zeros(4, dtype=torch.float64, pin_memory=True)
        self.done = torch.cuda.Event()
        nb = self.lib.pcadv_row_eval_workspace_bytes(self._rows(B))
        self.ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        self.logits = None   # the last full batch's logits (the graph's static output)
        self.graph = None
        self._key = None
        self.captures = 0    # graphs captured so far (a re-flattened model recaptures)

    # ---- per task ---------------------------------------------------------
    def _check_model(self, model):
        raise NotImplementedError

    def _rows(self, b):
        raise NotImplementedError

    def _gather_extra(self):
        return {}

    def _eval_batch(self, batch, b, graphed, base):
        raise NotImplementedError

    # ---- the pass ---------------------------------------------------------
    def model(self):
        m = self._model()
        if m is None:
            raise RuntimeError("the evaluator's model is gone")
        return m

    def _state_key(self):
        m = self.model()
        return (tuple(p.data_ptr() for p in m.parameters()), getattr(m, "precision", None),
                float(m.dropout.p) if hasattr(m, "dropout") else None)

    def _full_batch(self):
        """One full batch at the device cursor: gather, forward, metrics,
        cursor and RNG step += 1 (the graph's body; also run eagerly)."""
        ld = self.loader
        j = ld._gather_job(self.order, self.counters[0:1], self.pts, self.lab, **self._gather_extra())
        j.step = self.counters[1:2].data_ptr()  # the pass's own copy of the loader's RNG step
        check(self.lib.pcadv_gather_clouds_at(j.src, j.n_src, j.npts, j.src_npts, j.order, j.cursor,
                                              j.B, j.src_lab, j.lab_width, j.src_seg, j.sigma,
                                              j.clip, j.seed, j.step, j.out, j.out_lab, j.out_seg,
                                              j.rng_row0, stream_ptr()), "pcadv_gather_clouds_at")
        self._eval_batch(None, self.B, True, 0)
        check(self.lib.pcadv_iter_epilogue(ptr(self.counters), 2, None, 0, None, 0, None,
                                           stream_ptr()), "pcadv_iter_epilogue")

    def _capture(self):
        def warmup():
            self.counters[0:1].zero_()  # it gathers batch 0 of whatever order is held
            self._full_batch()
        g = capture_graphs(self.device, warmup, self._full_batch, [self.counters, self.acc])
        self.graph = g
        self.captures += 1

    @torch.no_grad()
    def run(self, use_graph=True):
        """One pass over the loader's split: the totals as a dict (see the
        subclasses).  The loader's generator and RNG step end where iterating
        it once would leave them."""
        ld = self.loader
        nfull = ld.order_len // self.B
        rag = 0 if ld.drop_last else ld.order_len - nfull * self.B
        key = self._state_key()
        if key != self._key:  # parameters re-flattened (a train step object), precision, p
            self.graph, self._key = None, key
        if use_graph and nfull and self.graph is None:
            self._capture()
        self.order.copy_(ld.epoch_order())
        self.counters[0:1].zero_()
        self.counters[1:2].copy_(ld.step)
        self.acc.zero_()
        for _ in range(nfull):
            if use_graph:
                self.graph.replay()
            else:
                self._full_batch()
        ld.step.copy_(self.counters[1:2])
        if rag:
            idx = self.order[nfull * self.B:].contiguous()
            self._eval_batch(ld.gather(idx, _checked=True), rag, False, nfull * self.B)
        return self._finish(nfull * self.B + rag)

    def _read(self, pairs):
        """One batch of device -> pinned copies, one event wait."""
        for host, devt in pairs:
            host.copy_(devt, non_blocking=True)
        self.done.record()
        self.done.synchronize()

    def _row_eval(self, logits, ld_, labels, M, ncls, *, N=0, group_cat=None, cat_stride=0,
                  cursor=None, iou=None, cat=None):
        check(self.lib.pcadv_row_eval(ptr(logits), ld_, ptr(labels), M, ncls, None, N,
                                      ptr(group_cat), cat_stride,
                                      ptr(self.parts) if N else None, len(object_names) if N else 0,
                                      ptr(cursor), ptr(iou), ptr(cat), ptr(self.acc), ptr(self.ws),
                                      self.ws.numel(), stream_ptr()), "pcadv_row_eval")


class ClsEvaluator(_Evaluator):
    """run_testing's pass for PointNetCls(feature_transform=False) over a
    ModelNet DeviceCloudLoader.  run() -> {"correct", "loss_sum", "rows",
    "batches"}: the number of right predictions, the sum over the batches of
    each batch's mean CE (what the reference adds with loss.item()), clouds and
    batches seen."""

    KIND = "modelnet_gt"

    def _check_model(self, model):
        if not isinstance(model, PointNetCls) or model.feature_transform:
            raise TypeError("ClsEvaluator: PointNetCls(feature_transform=False) is required")
        if not 2 <= model.fc3.out_features <= MAX_CLASSES:
            raise ValueError(f"ClsEvaluator: 2..{MAX_CLASSES} classes, got {model.fc3.out_features}")

    def _rows(self, b):
        return b

    def forward(self, pts):
        """The eval-mode module forward's own launches (pcadv_feat_fwd, three
        pcadv_linear_fwd; dropout off): bitwise model.eval()(pts)[0]."""
        m = self.model()
        f = m.feat
        gmax, _, _ = ops.feat_fwd(pts, f.conv1.weight, f.conv1.bias, f.conv2.weight, f.conv2.bias,
                                  f.conv3.weight, f.conv3.bias, f.conv4.weight, f.conv4.bias)
        h = ops.linear_fwd(gmax, m.fc1.weight, m.fc1.bias, ops.ACT_RELU, None, 0.0)
        h = ops.linear_fwd(h, m.fc2.weight, m.fc2.bias, ops.ACT_RELU, None, float(m.dropout.p))
        return ops.linear_fwd(h, m.fc3.weight, m.fc3.bias, ops.ACT_NONE, None, 0.0)

    def _eval_batch(self, batch, b, graphed, base):
        pts, lab = (self.pts, self.lab[:, 0]) if batch is None else batch
        logits = self.forward(pts.contiguous())
        if graphed:
            self.logits = logits
        ncls = logits.shape[1]
        self._row_eval(logits, ncls, lab.contiguous(), b, ncls)

    def _finish(self, n):
        self._read([(self.acc_host, self.acc)])
        a = self.acc_host.tolist()
        return {"correct": int(a[0]), "loss_sum": a[1], "rows": int(a[2]), "batches": int(a[3])}


class SegEvaluator(_Evaluator):
    """run_testing_seg's pass for PointNetSeg over a ShapeNet DeviceCloudLoader.
    run() -> {"correct", "loss_sum", "rows", "batches", "iou", "cat"}: right
    points, the sum of the batches' mean CE, points and batches seen, and per
    cloud, in pass order, its mean part IoU (f64, bitwise metric.get_iou) and
    its category.  A pass at B=16, N=2 048 holds about 250 MB (the forward's
    activations in the graph's pool)."""

    KIND = "shapenet_gt"

    def __init__(self, model, loader):
        super().__init__(model, loader)
        dev, n = self.device, loader.order_len
        self.seg = torch.zeros(self.B, self.N, dtype=torch.int64, device=dev)
        self.oh = torch.zeros(self.B, 1, loader.ds.num_classes, device=dev)
        self.parts = torch.tensor(part_ranges(), dtype=torch.int32, device=dev)
        self.iou = torch.zeros(max(n, 1), dtype=torch.float64, device=dev)
        self.cat = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.iou_host = torch.zeros(max(n, 1), dtype=torch.float64, pin_memory=True)
        self.cat_host = torch.zeros(max(n, 1), dtype=torch.int32, pin_memory=True)

    def _check_model(self, model):
        from .seg import PointNetSeg
        if not isinstance(model, PointNetSeg):
            raise TypeError("SegEvaluator: PointNetSeg is required")
        if not 2 <= model.output_dim <= MAX_CLASSES:
            raise ValueError(f"SegEvaluator: 2..{MAX_CLASSES} part labels, got {model.output_dim}")

    def _rows(self, b):
        return b * self.N

    def _gather_extra(self):
        return {"out_seg": self.seg}

    def forward(self, pts, oh):
        """seg.seg_forward at the model's precision, as the module's forward
        calls it: point-major logits (b * N, C), bitwise the module's."""
        from .seg import seg_forward
        m = self.model()
        b = pts.shape[0]
        fw = seg_forward(pts.float().contiguous(), oh.float().reshape(b, 1, 16),
                         [p for _, p in m.named_parameters()], precision=m.precision)
        return fw["logits"]

    def _eval_batch(self, batch, b, graphed, base):
        if batch is None:
            self.oh.zero_()
            self.oh.scatter_(2, self.lab[:, :1].unsqueeze(1), 1.0)  # one_hot (shapeNetData.py)
            pts, oh, seg = self.pts, self.oh, self.seg
            cat, stride = self.lab, int(self.lab.shape[1])
        else:
            pts, oh, seg = batch
            cat, stride = oh[:, 0, :].argmax(1).contiguous(), 1
        logits = self.forward(pts, oh)
        if graphed:
            self.logits = logits
        ncls = logits.shape[1]
        # full batches write their records at cursor * B; the ragged one after them
        self._row_eval(logits, ncls, seg.contiguous().view(-1), b * self.N, ncls, N=self.N,
                       group_cat=cat, cat_stride=stride,
                       cursor=self.counters[0:1] if graphed else None,
                       iou=self.iou[base:], cat=self.cat[base:])

    def _finish(self, n):
        self._read([(self.acc_host, self.acc), (self.iou_host, self.iou), (self.cat_host, self.cat)])
        a = self.acc_host.tolist()
        return {"correct": int(a[0]), "loss_sum": a[1], "rows": int(a[2]), "batches": int(a[3]),
                "iou": np.array(self.iou_host[:n].numpy(), copy=True),
                "cat": np.array(self.cat_host[:n].numpy(), copy=True)}


_CACHE = weakref.WeakKeyDictionary()  # model -> its evaluator (one graph for a run's test passes)


def evaluator_for(model, loader, cls):
    ev = _CACHE.get(model)
    if type(ev) is not cls or ev.loader is not loader:
        ev = _CACHE[model] = cls(model, loader)
    return ev

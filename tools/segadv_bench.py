"""Time of the adversarial segmentation step against the generator-only step
on the same 32 clouds, both as replayed HIP graphs on seeded synthetic data:

  adv: SegAdvTrainStep, B = 16 + 16 (GT + no-GT), N = 2048, PointNetSeg(50) +
       PointwiseDiscNet(2048, 50), device-drawn labels
  seg: SegTrainStep, B = 32, N = 2048, PointNetSeg(50)

The difference is the cost of the discriminator (its fused forward with the
BCE terms, its fused backward, the second Adam, the input concatenation),
less the cross entropy of the 16 no-GT clouds that the adversarial step does
not compute.  After a warm-up, `--rounds` rounds alternate `--steps` replays
of each graph between device events; medians, spread and the per-kernel share
are printed and written to profiles/segadv_bench.json.  Needs the MI355X.

    python tools/segadv_bench.py [--rounds 7] [--steps 20] [--out profiles/segadv_bench.json]

--semi times instead the adversarial step with run_training_seg_semi's term
(semi=True, a threshold that keeps about half the no-GT points) against the
same step without it, alternated the same way, into
profiles/segadv_semi_bench.json.

--stack times run_training_seg_stack's step (SegStackTrainStep with
StackDiscNet(2048, 50, 16)) against the pointwise adversarial step and the
generator-only step, three graphs on the same 32 clouds and equal generators,
alternated the same way, with the two discriminators' launches alone, into
profiles/segstack_bench.json.

--stack --regu times run_training_seg_stack_regulization's step
(SegStackReguTrainStep with PointNetSeg_regulization(50), fstn's last layer
scaled so the feature transform starts near the identity) against the stacked
step of the same run (the conv / fc weights equal, the same 32 clouds and the
same StackDiscNet weights), alternated the same way, into
profiles/segregu_bench.json.

--stack --semi (and --stack --regu --semi) times the stacked step with the
stacked semi loops' term in its two forms against the same step without it,
three graphs alternated the same way at lr 0 with a threshold that keeps about
half the no-GT points: "fused", what the package runs (the scan inside the D
forward, pcadv_stackdisc_forward_semi, then pcadv_row_semi_apply after the D
backward), and "composed", put together here and not a switch in the package
(the plain D forward, then the two-launch pcadv_row_semi_ce on d_out[M:] after
the D backward).  Into profiles/segstack_semi_bench.json, one entry per
generator ("stack" / "regu").

--dual times run_training_seg_dual's step (SegDualTrainStep with BaseDiscNet /
ShapeDiscNet / PointDiscNet, G's Adam and the two SGDs) as a replayed graph
against trainer._seg_dual_body on equal modules (the reference's iteration
through autograd and torch's own kernels, eager: it reads its losses on the
host as the reference does), with the pointwise adversarial step for scale,
alternated the same way, into profiles/segdual_bench.json.

--loop NAME[,NAME...] (seg, stack, regu, dual, or all) times the loops users
call - run_training_seg, _seg_stack, _seg_stack_regulization, _seg_dual - over
two ShapeNet DeviceCloudLoaders built from synthetic resident splits (256
clouds each, B = 16, N = 2048, no files), wall clock per iteration.  The test
pass and the checkpoint writes are stubbed out; the stub synchronizes the
device and takes the time at iterations 0, K and 2K (--iters K), and the figure
is the second interval's, so the first one absorbs the set-up (the steps'
construction, the graph captures).  One JSON line per loop goes to stdout (and
is appended to --jsonl).  --root DIR imports the package from another tree (the
parent commit built into ablib/): a comparison alternates
fresh processes of the two trees.  --step-graphs adds each step's own captured
time (capture_on, replayed between device events).  --loop-report FILES...
turns the collected lines into profiles/seg_loops_graph_bench.json.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _inputs(rng, B, N):
    pts = torch.from_numpy(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)).cuda()
    cls = torch.from_numpy(np.eye(16, dtype=np.float32)[rng.integers(0, 16, B)][:, None, :]).cuda()
    seg = torch.from_numpy(rng.integers(0, 50, (B, N))).cuda()
    return pts, cls, seg


def _time(graph, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _d_alone(step, M, steps):
    """The D launches alone (forward with losses, backward + finish) on a
    logits-shaped input, as eager launches between device events (so each
    figure includes the host's launch cost: an upper bound on the kernels)."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    dev = step.device
    lg = torch.randn(2 * M, 50, device=dev) * 2
    out, argc = torch.empty(2 * M, device=dev), torch.empty(2 * M, device=dev, dtype=torch.int32)
    dd, da = torch.empty(2 * M, device=dev), torch.empty(M, device=dev)
    dl, ws = torch.empty(2 * M, 50, device=dev), D.pwdisc_workspace(2 * M, dev)
    losses = torch.zeros(4, device=dev)

    def fwd():
        D.pwdisc_forward(lg, 50, M, M, D.PWD_SOFTMAX, D.PWD_LOG_SOFTMAX, step.d_params, out, argc,
                         ws, losses=losses, seed=1, step_count=step.step_count, dout_d=dd,
                         dout_adv=da)

    def bwd():
        D.pwdisc_backward(lg, 50, M, M, D.PWD_SOFTMAX, D.PWD_LOG_SOFTMAX, step.d_params, out, argc,
                          ws, dd, step.d_grad_views, dout_adv=da, lambda_adv=0.01, dlogits=dl)
    res = {}
    for name, fn in (("d_forward_ms", fwd), ("d_backward_ms", bwd)):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        res[name] = a.elapsed_time(b) / steps
    return res


def _stack_d_alone(step, M, steps):
    """_d_alone for the stacked discriminator's launches."""
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    dev = step.device
    lg = torch.randn(2 * M, 50, device=dev) * 2
    m, d_out = torch.empty(2 * M, device=dev), torch.empty(2 * M, device=dev)
    argc = torch.empty(2 * M, device=dev, dtype=torch.int32)
    dd, da = torch.empty(2 * M, device=dev), torch.empty(M, device=dev)
    dl, ws = torch.empty(2 * M, 50, device=dev), D.stackdisc_workspace(2 * M, dev)
    losses, bad = torch.zeros(5, device=dev), torch.zeros(1, device=dev, dtype=torch.int32)
    labels = torch.zeros(M // 2048, device=dev, dtype=torch.int32)

    def fwd():
        D.stackdisc_forward(lg, 50, M, M, D.PWD_SOFTMAX, D.PWD_LOG_SOFTMAX, step.d_params, m, argc,
                            d_out, ws, losses=losses, shape_label=labels, pts_per_cloud=2048,
                            lambda_disc_shape=1.0, seed=1, step_count=step.step_count, dm_d=dd,
                            dm_adv=da, grads5=step.d_grad_views[8:10], bad_rows=bad)

    def bwd():
        D.stackdisc_backward(lg, 50, M, M, D.PWD_SOFTMAX, D.PWD_LOG_SOFTMAX, step.d_params, m, argc,
                             ws, dd, step.d_grad_views, dm_adv=da, lambda_adv=0.01, dlogits=dl)
    res = {}
    for name, fn in (("d_forward_ms", fwd), ("d_backward_ms", bwd)):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        res[name] = a.elapsed_time(b) / steps
    return res


def _stack(a):
    """--stack: SegStackTrainStep against SegAdvTrainStep and SegTrainStep."""
    import adversarial_learning_on_pointclouds_amd as pc
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    gens = [pc.PointNetSeg(50).cuda() for _ in range(3)]
    for g in gens[1:]:
        g.load_state_dict(gens[0].state_dict())
    stack = pc.SegStackTrainStep(gens[0], pc.StackDiscNet(N, 50, 16).cuda(), lr=1e-4, lr_D=1e-4,
                                 lambda_adv=0.01, lambda_disc_shape=1.0, seed=5)
    adv = pc.SegAdvTrainStep(gens[1], pc.PointwiseDiscNet(N, 50).cuda(), lr=1e-4, lr_D=1e-4,
                             lambda_adv=0.01, seed=5)
    sup = pc.SegTrainStep(gens[2], lr=1e-4)
    halves = (pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
              pts[B:].contiguous(), cls[B:].contiguous())
    graphs = {"stack": stack.capture_on(*halves), "adv": adv.capture_on(*halves),
              "seg": sup.capture_on(pts, cls, seg)}
    for g in graphs.values():  # warm-up
        _time(g, 5)
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(_time(g, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    diffs = [s - p for s, p in zip(times["stack"], times["adv"])]
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "what": {"stack": "SegStackTrainStep B=16+16 N=2048 fp32, graph replay",
                    "adv": "SegAdvTrainStep B=16+16 N=2048 fp32, graph replay",
                    "seg": "SegTrainStep B=32 N=2048 fp32, graph replay"}}
    for k in graphs:
        out[k + "_ms"] = {"median": med[k], "min": min(times[k]), "max": max(times[k]),
                          "rounds": times[k]}
    out["stack_over_adv_us"] = {"median_of_medians": 1e3 * (med["stack"] - med["adv"]),
                                "per_round": [1e3 * x for x in diffs],
                                "median": 1e3 * statistics.median(diffs),
                                "min": 1e3 * min(diffs), "max": 1e3 * max(diffs)}
    out["round_spread_us"] = {k: 1e3 * (max(v) - min(v)) for k, v in times.items()}
    out["d_cost_ms"] = {"stack": med["stack"] - med["seg"], "adv": med["adv"] - med["seg"]}
    out["losses_last"] = [float(x) for x in stack.losses.tolist()]
    out["bad_rows_last"] = int(stack.bad_rows.item())
    out["d_alone"] = {"stack": _stack_d_alone(stack, B * N, a.steps),
                      "adv": _d_alone(adv, B * N, a.steps)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"stack_ms": med["stack"], "adv_ms": med["adv"], "seg_ms": med["seg"],
                      "stack_over_adv_us": out["stack_over_adv_us"]["median"],
                      "round_spread_us": out["round_spread_us"], "d_alone": out["d_alone"]}))


def _dual(a):
    """--dual: SegDualTrainStep (graph) against _seg_dual_body (eager autograd)
    and SegAdvTrainStep (graph)."""
    import copy
    import adversarial_learning_on_pointclouds_amd as pc
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    halves = (pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
              pts[B:].contiguous(), cls[B:].contiguous())
    lrs = dict(lr=1e-4, lr_D_shape=1e-4, lr_D_point=1e-4)

    def nets():
        return (pc.BaseDiscNet(N, 50, 256).cuda(), pc.ShapeDiscNet(256, 16).cuda(),
                pc.PointDiscNet(256, N).cuda())
    g_dual, d_dual = pc.PointNetSeg(50).cuda(), nets()
    g_body, d_body = copy.deepcopy(g_dual), copy.deepcopy(d_dual)
    g_adv = copy.deepcopy(g_dual)
    dual = pc.SegDualTrainStep(g_dual, *d_dual, lambda_adv=0.01, lambda_disc_shape=1.0, seed=5,
                               **lrs)
    adv = pc.SegAdvTrainStep(g_adv, pc.PointwiseDiscNet(N, 50).cuda(), lr=1e-4, lr_D=1e-4,
                             lambda_adv=0.01, seed=5)
    shared, shape, point = d_body
    opts = (torch.optim.Adam(g_body.parameters(), lr=1e-4),
            torch.optim.SGD(list(shape.parameters()) + list(shared.parameters()), lr=1e-4),
            torch.optim.SGD(list(point.parameters()) + list(shared.parameters()), lr=1e-4))
    crit = (torch.nn.BCEWithLogitsLoss(), torch.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss())
    pools = (ImagePool(0), ImagePool(0))
    bargs = argparse.Namespace(device="cuda", lambda_seg=1.0, lambda_adv=0.01,
                               lambda_disc_shape=1.0)
    last = {}

    def body():
        last["v"] = trainer._seg_dual_body(g_body, shared, shape, point, *opts, *crit, *pools,
                                           *halves, bargs)

    class Eager:
        def replay(self):
            body()
    graphs = {"dual": dual.capture_on(*halves), "body": Eager(), "adv": adv.capture_on(*halves)}
    for g in graphs.values():  # warm-up
        _time(g, 5)
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(_time(g, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "what": {"dual": "SegDualTrainStep B=16+16 N=2048 fp32, graph replay",
                    "body": "trainer._seg_dual_body on equal modules, eager autograd",
                    "adv": "SegAdvTrainStep B=16+16 N=2048 fp32, graph replay"}}
    for k in graphs:
        out[k + "_ms"] = {"median": med[k], "min": min(times[k]), "max": max(times[k]),
                          "rounds": times[k]}
    out["dual_beats_body_in_every_round"] = all(d < b for d, b in zip(times["dual"],
                                                                      times["body"]))
    out["body_over_dual"] = med["body"] / med["dual"]
    out["dual_over_adv_ms"] = med["dual"] - med["adv"]
    out["losses_last"] = {"dual": [float(x) for x in dual.losses.tolist()], "body": last["v"]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("dual_beats_body_in_every_round", "body_over_dual",
                                          "dual_over_adv_ms")}
                     | {k + "_ms": [med[k], min(times[k]), max(times[k])] for k in graphs}))


def _regu(a):
    """--stack --regu: SegStackReguTrainStep against SegStackTrainStep."""
    import adversarial_learning_on_pointclouds_amd as pc
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    g_regu, g_stack = pc.PointNetSeg_regulization(50).cuda(), pc.PointNetSeg(50).cuda()
    with torch.no_grad():
        g_regu.fstn.fc3.weight.mul_(0.02)
        g_regu.fstn.fc3.bias.mul_(0.02)
    g_stack.load_state_dict({k: v for k, v in g_regu.state_dict().items()
                             if not k.startswith(("stn.", "fstn."))})
    d_regu, d_stack = pc.StackDiscNet(N, 50, 16).cuda(), pc.StackDiscNet(N, 50, 16).cuda()
    d_stack.load_state_dict(d_regu.state_dict())
    kw = dict(lr=1e-4, lr_D=1e-4, lambda_adv=0.01, lambda_disc_shape=1.0, seed=5)
    regu = pc.SegStackReguTrainStep(g_regu, d_regu, lambda_regu=0.001, **kw)
    stack = pc.SegStackTrainStep(g_stack, d_stack, **kw)
    halves = (pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
              pts[B:].contiguous(), cls[B:].contiguous())
    graphs = {"regu": regu.capture_on(*halves), "stack": stack.capture_on(*halves)}
    for g in graphs.values():  # warm-up
        _time(g, 5)
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(_time(g, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    diffs = [r - s for r, s in zip(times["regu"], times["stack"])]
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "what": {"regu": "SegStackReguTrainStep B=16+16 N=2048 fp32, graph replay",
                    "stack": "SegStackTrainStep B=16+16 N=2048 fp32, graph replay"}}
    for k in graphs:
        out[k + "_ms"] = {"median": med[k], "min": min(times[k]), "max": max(times[k]),
                          "rounds": times[k]}
    out["regu_over_stack_ms"] = {"median_of_medians": med["regu"] - med["stack"],
                                 "per_round": diffs, "median": statistics.median(diffs),
                                 "min": min(diffs), "max": max(diffs)}
    out["regu_over_stack_share"] = (med["regu"] - med["stack"]) / med["stack"]
    out["round_spread_us"] = {k: 1e3 * (max(v) - min(v)) for k, v in times.items()}
    out["losses_last"] = {"regu": [float(x) for x in regu.losses.tolist()],
                          "stack": [float(x) for x in stack.losses.tolist()]}
    out["bad_rows_last"] = {"regu": int(regu.bad_rows.item()), "stack": int(stack.bad_rows.item())}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"regu_ms": med["regu"], "stack_ms": med["stack"],
                      "regu_over_stack_ms": out["regu_over_stack_ms"]["median"],
                      "share": out["regu_over_stack_share"],
                      "round_spread_us": out["round_spread_us"],
                      "losses_last": out["losses_last"]["regu"]}))


def _semi(a):
    """--semi: the adversarial step with run_training_seg_semi's term against
    the same step without it, two graphs over the same inputs and equal models,
    alternated.  Both Adams run at lr 0, so the parameters and with them the
    kept share (the threshold is the median of the first step's no-GT D
    outputs) stay what they are over the replays; the launches are the same."""
    import adversarial_learning_on_pointclouds_amd as pc
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    args = (pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
            pts[B:].contiguous(), cls[B:].contiguous())
    steps = {}
    for k in ("plain", "semi"):
        g, d = pc.PointNetSeg(50).cuda(), pc.PointwiseDiscNet(N, 50).cuda()
        if steps:
            g.load_state_dict(steps["plain"].model.state_dict())
            d.load_state_dict(steps["plain"].model_D.state_dict())
        steps[k] = pc.SegAdvTrainStep(g, d, lr=0.0, lr_D=0.0, lambda_adv=0.01, seed=5,
                                      keep_activations=(k == "plain"))
    steps["plain"](*args)
    th = float(steps["plain"].d_out[B * N:].median().item())
    steps["plain"].keep_activations, steps["plain"].fw, steps["plain"].d_out = False, None, None
    steps["semi"].semi_th = th
    graphs = {"plain": steps["plain"].capture_on(*args),
              "semi": steps["semi"].capture_on(*args, semi=True)}
    for g in graphs.values():  # warm-up
        _time(g, 5)
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(_time(g, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    diffs = [s - p for s, p in zip(times["semi"], times["plain"])]
    kept = int(steps["semi"].kept.item())
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "what": "SegAdvTrainStep B=16+16 N=2048 fp32, graph replay, semi=True against "
                   "semi=False, alternated, lr 0",
           "semi_th": th, "kept": kept, "kept_share": kept / float(B * N),
           "plain_ms": {"median": med["plain"], "min": min(times["plain"]),
                        "max": max(times["plain"]), "rounds": times["plain"]},
           "semi_ms": {"median": med["semi"], "min": min(times["semi"]), "max": max(times["semi"]),
                       "rounds": times["semi"]},
           "semi_cost_us": {"median_of_medians": 1e3 * (med["semi"] - med["plain"]),
                            "per_round": [1e3 * x for x in diffs],
                            "median": 1e3 * statistics.median(diffs),
                            "min": 1e3 * min(diffs), "max": 1e3 * max(diffs)},
           "round_spread_us": {"plain": 1e3 * (max(times["plain"]) - min(times["plain"])),
                               "semi": 1e3 * (max(times["semi"]) - min(times["semi"]))},
           "losses_last": [float(x) for x in steps["semi"].losses_semi.tolist()]}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"plain_ms": med["plain"], "semi_ms": med["semi"],
                      "semi_cost_us": out["semi_cost_us"]["median"],
                      "round_spread_us": out["round_spread_us"], "kept_share": out["kept_share"]}))


def _composed(base):
    """`base` with the semi term composed from the existing launches: the plain D
    forward and backward, then pcadv_row_semi_ce on the no-GT rows."""
    import ctypes
    from adversarial_learning_on_pointclouds_amd._lib import check, stream_ptr

    class Composed(base):
        def _disc(self, logits, ncls, M, N, cls_gt, d, dws, soft0, soft1, semi):
            d_out = super()._disc(logits, ncls, M, N, cls_gt, d, dws, soft0, soft1, False)
            if semi:
                p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
                ws = torch.empty(self.lib.pcadv_row_semi_ce_workspace_bytes(M), dtype=torch.uint8,
                                 device=self.device)
                check(self.lib.pcadv_row_semi_ce(
                    p(logits[M:]), logits.stride(0), p(d_out[M:]), M, ncls, self.semi_th,
                    self.lambda_semi, p(d[M:]), d.stride(0), None, p(self.loss_buf[self._SEMI:]),
                    p(self.kept_buf), p(ws), ws.numel(), stream_ptr()), "pcadv_row_semi_ce")
            return d_out
    return Composed


def _stack_semi(a):
    """--stack [--regu] --semi: the stacked step without the term, with the fused
    term and with the composed term, three graphs over the same inputs and equal
    models, alternated.  Both Adams run at lr 0, so the parameters and with them
    the kept share stay what they are over the replays."""
    import adversarial_learning_on_pointclouds_amd as pc
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    args = (pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
            pts[B:].contiguous(), cls[B:].contiguous())
    base = pc.SegStackReguTrainStep if a.regu else pc.SegStackTrainStep
    G = pc.PointNetSeg_regulization if a.regu else pc.PointNetSeg
    kw = dict(lr=0.0, lr_D=0.0, lambda_adv=0.01, lambda_disc_shape=1.0, seed=5)
    if a.regu:
        kw["lambda_regu"] = 0.001
    steps = {}
    for k, cls_ in (("plain", base), ("fused", base), ("composed", _composed(base))):
        g, d = G(50).cuda(), pc.StackDiscNet(N, 50, 16).cuda()
        if steps:
            g.load_state_dict(steps["plain"].model.state_dict())
            d.load_state_dict(steps["plain"].model_D.state_dict())
        elif a.regu:
            with torch.no_grad():  # the feature transform starts near the identity (--regu)
                g.fstn.fc3.weight.mul_(0.02)
                g.fstn.fc3.bias.mul_(0.02)
        steps[k] = cls_(g, d, keep_activations=(k == "plain"), **kw)
    steps["plain"](*args)
    th = float(steps["plain"].d_out[B * N:].median().item())
    steps["plain"].keep_activations, steps["plain"].fw, steps["plain"].d_out = False, None, None
    steps["fused"].semi_th = steps["composed"].semi_th = th
    graphs = {k: s.capture_on(*args, semi=(k != "plain")) for k, s in steps.items()}
    for g in graphs.values():  # warm-up
        _time(g, 5)
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(_time(g, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}

    def diff(x, y):
        d = [1e3 * (p - q) for p, q in zip(times[x], times[y])]
        return {"median_of_medians": 1e3 * (med[x] - med[y]), "per_round": d,
                "median": statistics.median(d), "min": min(d), "max": max(d)}
    f_c = diff("fused", "composed")
    same = all(torch.equal(steps["fused"].grad, steps[k].grad) for k in ("composed",))
    entry = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
             "what": f"{base.__name__} B=16+16 N=2048 fp32, graph replay, lr 0: semi=False, "
                     "semi=True (fused: scan in the D forward + pcadv_row_semi_apply), semi=True "
                     "(composed: plain D forward + pcadv_row_semi_ce), alternated",
             "semi_th": th, "kept": {k: int(steps[k].kept.item()) for k in ("fused", "composed")},
             "kept_share": int(steps["fused"].kept.item()) / float(B * N),
             "fused_over_plain_us": diff("fused", "plain"),
             "composed_over_plain_us": diff("composed", "plain"),
             "fused_over_composed_us": f_c,
             "fused_not_slower_rounds": sum(x <= 0 for x in f_c["per_round"]),
             "fused_ships": sum(x <= 0 for x in f_c["per_round"]) * 2 > a.rounds,
             "generator_gradients_bitwise_equal": bool(same),
             "round_spread_us": {k: 1e3 * (max(v) - min(v)) for k, v in times.items()},
             "losses_last": {k: [float(x) for x in steps[k].losses_semi.tolist()]
                             for k in ("fused", "composed")}}
    for k in graphs:
        entry[k + "_ms"] = {"median": med[k], "min": min(times[k]), "max": max(times[k]),
                            "rounds": times[k]}
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["regu" if a.regu else "stack"] = entry
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k + "_ms": med[k] for k in graphs}
                     | {k: entry[k]["median"] for k in ("fused_over_plain_us", "composed_over_plain_us",
                                                        "fused_over_composed_us")}
                     | {k: entry[k] for k in ("fused_not_slower_rounds", "fused_ships", "kept_share",
                                              "generator_gradients_bitwise_equal")}))


LOOPS = ("seg", "stack", "regu", "dual")


def _synthetic_split(D, cls, n, npts, seed):
    """An in-memory ShapeNet split: no file is read."""
    rng = np.random.default_rng(seed)
    ds = object.__new__(cls)
    ds.num_classes, ds.npts = 16, npts
    ds.select_data = rng.uniform(-1, 1, (n, npts, 3)).astype(np.float32)
    ds.select_labels = rng.integers(0, 16, (n, 1)).astype(np.int64)
    if cls is D.ShapeNetDatasetGT:
        ds.select_segs = rng.integers(0, 50, (n, npts)).astype(np.int64)
    return ds


def _loop_nets(pc, name, N):
    """(G, [D nets]) with D's biases zero and its weights Xavier: the stacked
    D's output then starts, and at the lr used here stays, inside [0, 1]."""
    G = (pc.PointNetSeg_regulization(50) if name == "regu" else pc.PointNetSeg(50)).cuda()
    if name == "dual":
        Ds = [pc.BaseDiscNet(N, 50, 256), pc.ShapeDiscNet(256, 16), pc.PointDiscNet(256, N)]
    else:
        Ds = [pc.PointwiseDiscNet(N, 50) if name == "seg" else pc.StackDiscNet(N, 50, 16)]
    Ds = [d.cuda() for d in Ds]
    with torch.no_grad():
        for d in Ds:
            for k, p in d.named_parameters():
                if k.endswith("bias"):
                    p.zero_()
                elif p.dim() > 1:
                    torch.nn.init.xavier_uniform_(p)
    return G, Ds


def _loop_opts(name, G, Ds, lr):
    opt = torch.optim.Adam(G.parameters(), lr=lr)
    if name == "dual":
        S, H, P = Ds
        return [opt, torch.optim.SGD(list(H.parameters()) + list(S.parameters()), lr=lr),
                torch.optim.SGD(list(P.parameters()) + list(S.parameters()), lr=lr)]
    return [opt, torch.optim.Adam(Ds[0].parameters(), lr=lr)]


def _loop_one(a, name):
    """One loop's wall clock per iteration in this process."""
    import tempfile
    import time
    import adversarial_learning_on_pointclouds_amd as pc
    from adversarial_learning_on_pointclouds_amd import dataset as D
    from adversarial_learning_on_pointclouds_amd import trainer
    from adversarial_learning_on_pointclouds_amd.image_pool import ImagePool
    B, N, K = 16, 2048, a.iters
    torch.manual_seed(0)
    gt = D.DeviceCloudLoader(_synthetic_split(D, D.ShapeNetDatasetGT, a.clouds, N, 0), B,
                             shuffle=True, seed=1, drop_last=True)
    ng = D.DeviceCloudLoader(_synthetic_split(D, D.ShapeNetDataset_noGT, a.clouds, N, 1), B,
                             shuffle=True, seed=2, drop_last=True)
    G, Ds = _loop_nets(pc, name, N)
    opts = _loop_opts(name, G, Ds, 1e-5)
    stamps = []

    def testing(*_a, **_k):  # the test pass, stubbed: a device sync and a time stamp
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return 0.0, 0.0, 0.0, 0.0
    trainer.run_testing_seg = trainer.run_testing_seg_regulization = testing
    save0, trainer.torch.save = torch.save, (lambda *_a, **_k: None)  # checkpoints: stubbed

    class Log:
        n = 0
        last = ""

        def info(self, s):
            if s.startswith("iter"):
                self.n, self.last = self.n + 1, s
    log = Log()
    with tempfile.TemporaryDirectory() as tmp:
        args = argparse.Namespace(device="cuda", total_iterations=2 * K + 1, lambda_seg=1.0,
                                  lambda_adv=0.01, lambda_disc_shape=1.0, lambda_regu=0.001,
                                  iter_test_epoch=K, exp_dir=tmp, tensorboard=False, input_pts=N,
                                  seed=5, use_graph=not a.no_graph)
        ce = torch.nn.CrossEntropyLoss()
        head = (gt, ng, enumerate(gt), enumerate(ng), [None], [0] * B, G)
        tail = (ImagePool(0), ImagePool(0), log, log, None, args)
        try:
            if name == "dual":
                trainer.run_training_seg_dual(*head, *Ds, torch.nn.BCEWithLogitsLoss(), ce, ce,
                                              *opts, *tail)
            elif name == "seg":
                trainer.run_training_seg(*head, Ds[0], torch.nn.BCEWithLogitsLoss(), ce, *opts,
                                         *tail)
            elif name == "stack":
                trainer.run_training_seg_stack(*head, Ds[0], torch.nn.BCELoss(), ce, ce, *opts,
                                               *tail)
            else:
                trainer.run_training_seg_stack_regulization(*head, Ds[0], torch.nn.BCELoss(), ce,
                                                            torch.nn.MSELoss(), ce, *opts, *tail)
        finally:
            trainer.torch.save = save0
    assert len(stamps) == 3 and log.n == 2 * K + 1, (len(stamps), log.n)
    graphed = hasattr(trainer, "_SegPairIteration") and not a.no_graph
    res = {"loop": name, "tree": a.tag, "graphed": graphed, "iters": K, "B": B, "N": N,
           "clouds": a.clouds, "ms_per_iter": 1e3 * (stamps[2] - stamps[1]) / K,
           "first_interval_ms_per_iter": 1e3 * (stamps[1] - stamps[0]) / K, "last_line": log.last}
    if a.step_graphs:
        res["step_graph_ms"] = _loop_step_graph(pc, name, a)
    return res


def _loop_step_graph(pc, name, a):
    """The step's own captured graph on resident inputs (what the other modes of
    this tool time), replayed between device events."""
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    halves = (pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
              pts[B:].contiguous(), cls[B:].contiguous())
    G, Ds = _loop_nets(pc, name, N)
    kw = dict(lr=1e-5, lambda_adv=0.01, seed=5)
    if name == "dual":
        st = pc.SegDualTrainStep(G, *Ds, lambda_disc_shape=1.0, lr_D_shape=1e-5, lr_D_point=1e-5,
                                 **kw)
    elif name == "seg":
        st = pc.SegAdvTrainStep(G, Ds[0], lr_D=1e-5, **kw)
    elif name == "stack":
        st = pc.SegStackTrainStep(G, Ds[0], lr_D=1e-5, lambda_disc_shape=1.0, **kw)
    else:
        st = pc.SegStackReguTrainStep(G, Ds[0], lr_D=1e-5, lambda_disc_shape=1.0,
                                      lambda_regu=0.001, **kw)
    g = st.capture_on(*halves)
    _time(g, 5)
    return statistics.median(_time(g, 20) for _ in range(5))


def _loop(a):
    names = LOOPS if a.loop == "all" else tuple(a.loop.split(","))
    for n in names:
        if n not in LOOPS:
            sys.exit(f"--loop: {n!r} is not one of {LOOPS}")
    for n in names:
        line = json.dumps(_loop_one(a, n))
        print(line, flush=True)
        if a.jsonl:
            os.makedirs(os.path.dirname(a.jsonl) or ".", exist_ok=True)
            with open(a.jsonl, "a") as f:
                f.write(line + "\n")


def _loop_report(a):
    """profiles/seg_loops_graph_bench.json from the lines of alternated parent /
    tree processes (round r = the r-th line of each tree for a loop)."""
    rows = []
    for path in a.loop_report:
        with open(path) as f:
            rows += [json.loads(l) for l in f if l.strip().startswith("{")]
    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "what": "run_training_seg* over two ShapeNet DeviceCloudLoaders (synthetic resident "
                   "splits), B=16+16 N=2048 fp32, wall-clock ms per iteration over the second of "
                   "two intervals of `iters` iterations, test pass and checkpoint writes stubbed; "
                   "parent = the parent commit's loop (eager step, host read per iteration), "
                   "tree = this tree's graph-fed loop; fresh processes, alternated",
           "loops": {}}
    for name in LOOPS:
        per = {t: [r["ms_per_iter"] for r in rows if r["loop"] == name and r["tree"] == t]
               for t in ("parent", "tree")}
        n = min(len(per["parent"]), len(per["tree"]))
        if not n:
            continue
        wins = sum(t < p for p, t in zip(per["parent"][:n], per["tree"][:n]))
        e = {"rounds": n, "iters": next(r["iters"] for r in rows if r["loop"] == name),
             "tree_faster_rounds": wins, "graphed_ships": wins * 2 > n}
        for t in ("parent", "tree"):
            v = per[t][:n]
            e[t + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v),
                            "rounds": v}
        e["speedup_median"] = e["parent_ms"]["median"] / e["tree_ms"]["median"]
        sg = [r["step_graph_ms"] for r in rows if r["loop"] == name and "step_graph_ms" in r]
        if sg:
            e["step_graph_ms"] = statistics.median(sg)
        e["tree_graphed"] = all(r["graphed"] for r in rows
                                if r["loop"] == name and r["tree"] == "tree")
        out["loops"][name] = e
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"parent": v["parent_ms"]["median"], "tree": v["tree_ms"]["median"],
                          "tree_faster_rounds": v["tree_faster_rounds"], "rounds": v["rounds"],
                          "step_graph_ms": v.get("step_graph_ms")}
                      for k, v in out["loops"].items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--semi", action="store_true",
                    help="time semi=True against semi=False (profiles/segadv_semi_bench.json); "
                         "with --stack [--regu]: the stacked step's fused and composed term "
                         "(profiles/segstack_semi_bench.json)")
    ap.add_argument("--stack", action="store_true",
                    help="time SegStackTrainStep against both (profiles/segstack_bench.json)")
    ap.add_argument("--regu", action="store_true",
                    help="with --stack: time SegStackReguTrainStep against SegStackTrainStep "
                         "(profiles/segregu_bench.json)")
    ap.add_argument("--dual", action="store_true",
                    help="time SegDualTrainStep against the autograd body and the pointwise step "
                         "(profiles/segdual_bench.json)")
    ap.add_argument("--loop", default=None,
                    help="time the loops users call: seg, stack, regu, dual (comma-separated) or all")
    ap.add_argument("--iters", type=int, default=200, help="--loop: iterations per interval")
    ap.add_argument("--clouds", type=int, default=256, help="--loop: clouds per synthetic split")
    ap.add_argument("--root", default=None,
                    help="--loop: import the package from this tree (the parent built into ablib/)")
    ap.add_argument("--tag", default=None, help="--loop: 'parent' or 'tree' (default: by --root)")
    ap.add_argument("--no-graph", action="store_true", help="--loop: args.use_graph = False")
    ap.add_argument("--step-graphs", action="store_true",
                    help="--loop: also time each step's own captured graph")
    ap.add_argument("--jsonl", default=None, help="--loop: append the result lines to this file")
    ap.add_argument("--loop-report", nargs="+", default=None,
                    help="collected --loop lines -> profiles/seg_loops_graph_bench.json")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.regu and not a.stack:
        ap.error("--regu goes with --stack")
    if a.loop_report:
        a.out = a.out or os.path.join("profiles", "seg_loops_graph_bench.json")
        return _loop_report(a)
    if a.loop:
        if not torch.cuda.is_available():
            sys.exit("segadv_bench: no HIP device (the loops are timed on the MI355X only)")
        if a.root:  # the other tree's package in front of this one's
            sys.path.insert(0, os.path.abspath(a.root))
        a.tag = a.tag or ("parent" if a.root else "tree")
        return _loop(a)
    if a.out is None:
        a.out = os.path.join("profiles", "segdual_bench.json" if a.dual else
                             "segstack_semi_bench.json" if a.semi and a.stack else
                             "segadv_semi_bench.json" if a.semi else
                             "segregu_bench.json" if a.regu else
                             "segstack_bench.json" if a.stack else "segadv_bench.json")
    if not torch.cuda.is_available():
        sys.exit("segadv_bench: no HIP device (the steps are timed on the MI355X only)")
    if a.dual:
        return _dual(a)
    if a.semi and a.stack:
        return _stack_semi(a)
    if a.semi:
        return _semi(a)
    if a.regu:
        return _regu(a)
    if a.stack:
        return _stack(a)
    import adversarial_learning_on_pointclouds_amd as pc
    B, N = 16, 2048
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    pts, cls, seg = _inputs(rng, 2 * B, N)
    g_adv = pc.PointNetSeg(50).cuda()
    d_adv = pc.PointwiseDiscNet(N, 50).cuda()
    g_seg = pc.PointNetSeg(50).cuda()
    g_seg.load_state_dict(g_adv.state_dict())
    adv = pc.SegAdvTrainStep(g_adv, d_adv, lr=1e-4, lr_D=1e-4, lambda_adv=0.01, seed=5)
    sup = pc.SegTrainStep(g_seg, lr=1e-4)
    graphs = {
        "adv": adv.capture_on(pts[:B].contiguous(), cls[:B].contiguous(), seg[:B].contiguous(),
                              pts[B:].contiguous(), cls[B:].contiguous()),
        "seg": sup.capture_on(pts, cls, seg),
    }
    for g in graphs.values():  # warm-up
        _time(g, 5)
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(_time(g, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "what": {"adv": "SegAdvTrainStep B=16+16 N=2048 fp32, graph replay",
                    "seg": "SegTrainStep B=32 N=2048 fp32, graph replay"},
           "adv_ms": {"median": med["adv"], "min": min(times["adv"]), "max": max(times["adv"]),
                      "rounds": times["adv"]},
           "seg_ms": {"median": med["seg"], "min": min(times["seg"]), "max": max(times["seg"]),
                      "rounds": times["seg"]},
           "d_cost_ms": med["adv"] - med["seg"],
           "d_share_of_adv_step": (med["adv"] - med["seg"]) / med["adv"],
           "losses_last": [float(x) for x in adv.losses.tolist()]}
    out.update(_d_alone(adv, B * N, a.steps))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"adv_ms": med["adv"], "seg_ms": med["seg"], "d_cost_ms": out["d_cost_ms"],
                      "d_share": out["d_share_of_adv_step"], "d_forward_ms": out["d_forward_ms"],
                      "d_backward_ms": out["d_backward_ms"]}))


if __name__ == "__main__":
    main()

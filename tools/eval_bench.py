"""Wall time of whole test passes, native (evaluate.py) against the module path
(args.native_eval = False), on seeded synthetic splits of the real sizes held
in DeviceCloudLoaders:

  cls: 2 468 clouds x 1 024 points (ModelNet40 test), jitter on, B = 32, PointNetCls(40)
  seg: 2 874 clouds x 2 048 points (ShapeNet test), B = 16, PointNetSeg(50)

After one warm-up pass of each form, five passes of each, alternated in one
process; the host clock around run_testing / run_testing_seg (each ends in the
pass's own sync).  Prints the medians and the spread and writes
profiles/eval_bench.json.  Needs the MI355X: no fallback.

    python tools/eval_bench.py [--passes 5] [--out profiles/eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class _Log:
    def info(self, s):
        pass


def _modelnet(n, npts, seed):
    from adversarial_learning_on_pointclouds_amd import dataset as D
    rng = np.random.default_rng(seed)
    ds = object.__new__(D.ModelNetDatasetGT)
    ds.npoints, ds.data_augmentation, ds.sample_list = npts, True, None
    ds.select_data = rng.uniform(-1, 1, (n, npts, 3)).astype(np.float32)
    ds.select_labels = rng.integers(0, 40, n).astype(np.int32)
    return ds


def _shapenet(n, npts, seed):
    from adversarial_learning_on_pointclouds_amd import dataset as D
    from adversarial_learning_on_pointclouds_amd.metric import part_ranges
    rng = np.random.default_rng(seed)
    ds = object.__new__(D.ShapeNetDatasetGT)
    ds.num_classes, ds.npts, ds.sample_list = 16, npts, None
    ds.select_data = rng.uniform(-1, 1, (n, npts, 3)).astype(np.float32)
    ds.select_labels = rng.integers(0, 16, n).astype(np.int64)
    table = np.array(part_ranges())
    first, count = table[ds.select_labels, 0], table[ds.select_labels, 1]
    ds.select_segs = (first[:, None] + rng.integers(0, 1 << 30, (n, npts)) % count[:, None]).astype(np.int64)
    return ds


def _abi_calls(fn):
    """The C-ABI calls fn() makes, by name (each is one or more kernel launches)."""
    from adversarial_learning_on_pointclouds_amd import _lib
    lib = _lib.load()
    seen, saved = {}, {}
    for name in _lib.SIGNATURES:
        if name.endswith("_workspace_bytes") or name in ("pcadv_last_error", "pcadv_abi_version"):
            continue
        orig = getattr(lib, name)
        saved[name] = orig

        def spy(*a, _o=orig, _n=name):
            seen[_n] = seen.get(_n, 0) + 1
            return _o(*a)
        setattr(lib, name, spy)
    try:
        fn()
    finally:
        for name, orig in saved.items():
            setattr(lib, name, orig)
    torch.cuda.synchronize()
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_bench: no HIP device (the test passes are timed on the MI355X only)")
    import adversarial_learning_on_pointclouds_amd as pc
    from adversarial_learning_on_pointclouds_amd import dataset as D
    from adversarial_learning_on_pointclouds_amd import evaluate, trainer
    crit = torch.nn.CrossEntropyLoss()
    log = _Log()
    torch.manual_seed(0)
    work = {}
    ds = _modelnet(2468, 1024, 1)
    cls_model = pc.PointNetCls(k=40).cuda()
    cls_ld = D.DeviceCloudLoader(ds, 32, shuffle=False, seed=3)
    assert cls_ld.sigma > 0
    work["cls"] = dict(
        what="2468 x 1024, jitter on, B=32, PointNetCls(40)", loader=cls_ld, model=cls_model,
        run=lambda native: trainer.run_testing(
            cls_ld, cls_model, crit, log, 0, None,
            argparse.Namespace(device="cuda", batch_size=32, native_eval=native)),
        ev=evaluate.ClsEvaluator)
    sds = _shapenet(2874, 2048, 2)
    seg_model = pc.PointNetSeg(50).cuda()
    seg_ld = D.DeviceCloudLoader(sds, 16, shuffle=False, seed=4)
    work["seg"] = dict(
        what="2874 x 2048, B=16, PointNetSeg(50)", loader=seg_ld, model=seg_model,
        run=lambda native: trainer.run_testing_seg(
            seg_ld, sds, seg_model, crit, log, 0, None,
            argparse.Namespace(device="cuda", input_pts=2048, native_eval=native)),
        ev=evaluate.SegEvaluator)
    out = {"device": torch.cuda.get_device_name(0), "passes": a.passes, "workloads": {}}
    for name, w in work.items():
        first = {True: w["run"](True), False: w["run"](False)}  # warm-up (capture, allocator)
        times = {True: [], False: []}
        for _ in range(a.passes):
            for native in (True, False):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                w["run"](native)
                times[native].append(time.perf_counter() - t0)
        ev = evaluate.evaluator_for(w["model"], w["loader"], w["ev"])
        ev.counters[0:1].zero_()
        with torch.no_grad():
            calls = _abi_calls(ev._full_batch)
        torch_ops = 2 if name == "seg" else 0  # the one-hot's zero_ and scatter_
        r = {"what": w["what"], "batches": len(w["loader"])}
        for native, key in ((True, "native"), (False, "module")):
            t = sorted(times[native])
            r[key] = {"median_s": statistics.median(t), "min_s": t[0], "max_s": t[-1],
                      "spread_s": t[-1] - t[0], "times_s": times[native],
                      "metrics": [float(x) for x in first[native]]}
        r["speedup_median"] = r["module"]["median_s"] / r["native"]["median_s"]
        r["faster_by_more_than_the_spread"] = r["native"]["max_s"] < r["module"]["min_s"]
        r["native_graph_abi_calls_per_batch"] = calls
        r["native_graph_calls_per_batch"] = sum(calls.values()) + torch_ops
        r["native_host_syncs_per_pass"] = 1
        r["module_host_syncs_per_batch"] = 3 if name == "cls" else 5
        out["workloads"][name] = r
        print(f"{name}: {w['what']}: native {r['native']['median_s'] * 1e3:.1f} ms "
              f"[{r['native']['min_s'] * 1e3:.1f}, {r['native']['max_s'] * 1e3:.1f}]  module "
              f"{r['module']['median_s'] * 1e3:.1f} ms [{r['module']['min_s'] * 1e3:.1f}, "
              f"{r['module']['max_s'] * 1e3:.1f}]  x{r['speedup_median']:.2f}  "
              f"calls per graphed batch {r['native_graph_calls_per_batch']}")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"native_ms": v["native"]["median_s"] * 1e3,
                          "module_ms": v["module"]["median_s"] * 1e3}
                      for k, v in out["workloads"].items()}))


if __name__ == "__main__":
    main()

"""bench.py's plain / --full split and --dump-outputs: the argument defaults and
the dump writer on the CPU, and one short plain run on the GPU whose dumped
arrays must be what its result line reports."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    # importing bench.py opts in to its graph dispatch setting (os.environ.setdefault):
    # set the variable through monkeypatch first, which puts back what was there
    # before, "absent" included, once the test is over
    monkeypatch.setenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE",
                       os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0"))
    monkeypatch.syspath_prepend(REPO)
    return importlib.import_module("bench")


def test_plain_and_full_defaults(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.repeats, a.steps, a.warmup, a.dump_outputs) == (False, 1, 7, 2, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.repeats, a.dump_outputs) == (True, 3, "d")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--repeats", "2"])
    assert bench.parse().repeats == 2
    for cfg in ("trainer", "dp1"):  # whole-run differences / alternated forms stay medians of 3
        monkeypatch.setattr(sys, "argv", ["bench.py", "--config", cfg])
        assert bench.parse().repeats == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_sample_is_fixed_and_bounded(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 << 10)
    rng = np.random.default_rng(0)
    snap = {"small": rng.standard_normal(10).astype(np.float32),
            "big": rng.standard_normal(100000).astype(np.float32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), snap)
    total = 0
    for name in snap:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total <= 64 << 10
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), snap["small"])
    big = np.load(tmp_path / "a" / "big.npy")
    assert 1000 < big.size < snap["big"].size and np.isin(big, snap["big"]).all()


def test_dump_outputs_whole_while_the_dump_fits(bench, tmp_path, monkeypatch):
    """One array far above limit / n, but the dump as a whole under the limit:
    nothing is sampled, every array keeps its shape."""
    monkeypatch.setattr(bench, "DUMP_LIMIT", 256 << 10)
    rng = np.random.default_rng(1)
    snap = {f"s{k}": rng.standard_normal((3, 5)).astype(np.float32) for k in range(30)}
    snap["big"] = rng.standard_normal((128, 200)).astype(np.float32)  # 100 KB > 256 KB / 31
    bench.dump_outputs(str(tmp_path), snap)
    for name, a in snap.items():
        x = np.load(tmp_path / f"{name}.npy")
        assert x.shape == a.shape and np.array_equal(x, a)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 256 << 10


def test_dump_outputs_replaces_an_earlier_dump(bench, tmp_path):
    """A folder reused for another config holds the new run's arrays only;
    files that are not arrays are not touched."""
    (tmp_path / "notes.txt").write_text("kept")
    bench.dump_outputs(str(tmp_path), {"G.w": np.ones(3, np.float32), "D.w": np.ones(2, np.float32)})
    bench.dump_outputs(str(tmp_path), {"G.w": np.zeros(3, np.float32)})
    assert sorted(os.listdir(tmp_path)) == ["G.w.npy", "notes.txt"]
    assert np.array_equal(np.load(tmp_path / "G.w.npy"), np.zeros(3, np.float32))


def test_dump_outputs_cuts_only_the_largest(bench, tmp_path, monkeypatch):
    """Past the limit the small arrays stay whole and the large ones share what
    is left, so the limit is used, not an equal share per array."""
    monkeypatch.setattr(bench, "DUMP_LIMIT", 128 << 10)
    rng = np.random.default_rng(2)
    snap = {"a": rng.standard_normal((100, 300)).astype(np.float32),   # 120 KB
            "b": rng.standard_normal((50, 300)).astype(np.float32),    # 60 KB
            "c": rng.standard_normal((10, 10)).astype(np.float32),
            "d": rng.standard_normal(7).astype(np.float32)}
    bench.dump_outputs(str(tmp_path), snap)
    got = {k: np.load(tmp_path / f"{k}.npy") for k in snap}
    assert np.array_equal(got["c"], snap["c"]) and np.array_equal(got["d"], snap["d"])
    budget = (128 << 10) - 4 * 4096 - snap["c"].nbytes - snap["d"].nbytes
    for k in ("a", "b"):  # both above budget / 2: cut to it
        assert got[k].ndim == 1 and got[k].nbytes == budget // 2 // 4 * 4
        assert np.isin(got[k], snap[k]).all()
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 128 << 10


def test_headline_dump_is_whole(bench, tmp_path):
    """The adversarial step's models on the CPU: 54 arrays, 8 MB, fc1's weight
    and gradient 2 MB each - far under the limit, so each file holds the whole
    array in its own shape."""
    import torch
    import adversarial_learning_on_pointclouds_amd as pc
    mods = [("G", pc.PointNetCls(k=40)), ("D", pc.DeepConvDiscNet(40, 1))]
    for _, m in mods:
        for q in m.parameters():
            q.grad = torch.full_like(q, 0.5)
    snap = bench.snapshot_outputs({"losses": torch.zeros(6), "logits": torch.zeros(64, 40)}, mods)
    bench.dump_outputs(str(tmp_path), snap)
    assert len(snap) == 54 and len(os.listdir(tmp_path)) == 54
    for prefix, m in mods:
        for name, q in m.named_parameters():
            x = np.load(tmp_path / f"{prefix}.{name}.npy")
            assert x.shape == tuple(q.shape) and np.array_equal(x, q.detach().numpy())
            g = np.load(tmp_path / f"{prefix}.{name}.grad.npy")
            assert g.shape == tuple(q.shape) and (g == 0.5).all()
    assert np.load(tmp_path / "G.fc1.weight.npy").shape == (512, 1024)
    assert 8.0e6 < sum(a.nbytes for a in snap.values()) < 8.8e6


@pytest.mark.gpu
def test_plain_run_dumps_what_it_reports(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=REPO, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    # a plain run: one region of exactly --steps steps, nothing measured besides it
    assert j["steps"] == 3 and len(j["timing"]["regions_s"]) == 1
    assert j["ms_per_step"] == pytest.approx(j["timing"]["regions_s"][0] / 3 * 1e3, abs=1e-3)
    # value = 2B clouds x steps / region; regions_s is printed rounded to 1 us, value to 0.1
    region = j["timing"]["regions_s"][0]
    assert j["value"] == pytest.approx(64 * 3 / region, rel=0.5e-6 / region + 1e-5, abs=0.06)
    for key in ("roofline", "fp32_equivalent", "cpu_baseline"):
        assert key not in j
    files = sorted(os.listdir(out))
    assert "losses.npy" in files and "logits.npy" in files
    assert "G.feat.conv4.weight.npy" in files and "G.feat.conv4.weight.grad.npy" in files
    assert "D.fc.weight.npy" in files and "D.fc.weight.grad.npy" in files
    arrays = {f: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["logits.npy"].shape == (64, 40)
    assert arrays["G.feat.conv4.weight.npy"].shape == (1024, 128, 1)
    # the largest arrays (2 MB each) come out whole, with their shape
    assert arrays["G.fc1.weight.npy"].shape == (512, 1024)
    assert arrays["G.fc1.weight.grad.npy"].shape == (512, 1024)
    assert arrays["D.conv2.weight.npy"].shape == (256, 512, 1)
    assert np.abs(arrays["G.feat.conv4.weight.grad.npy"]).max() > 0
    assert np.allclose(arrays["losses.npy"][:4], j["losses_last_step"], atol=1e-5)

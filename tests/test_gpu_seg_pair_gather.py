"""dataset.gather_seg_pair (pcadv_gather_seg_pair): the adversarial seg steps'
packed input - pts [GT; no-GT], the one-hot class vectors, the GT part ids - in
one launch, bitwise what the two loaders' gather_at and _pack's one-hot give.
Outputs are pre-filled with NaN / -1, so an element the kernel skips shows up.
MI355X only."""
import os

import numpy as np
import pytest
import torch

from adversarial_learning_on_pointclouds_amd import dataset as D

pytestmark = pytest.mark.gpu
H5 = os.path.join(os.path.dirname(__file__), "golden", "h5")
DEV = "cuda"


def _list(tmp_path, names):
    p = tmp_path / "files.txt"
    p.write_text("".join(os.path.join(H5, n) + "\n" for n in names))
    return str(p)


def _synthetic(cls, n, npts, seed):
    """An in-memory ShapeNet split (no file): n clouds of npts points."""
    rng = np.random.default_rng(seed)
    ds = object.__new__(cls)
    ds.num_classes, ds.npts = 16, npts
    ds.select_data = rng.uniform(-1, 1, (n, npts, 3)).astype(np.float32)
    ds.select_labels = rng.integers(0, 16, (n, 1)).astype(np.int64)
    if cls is D.ShapeNetDatasetGT:
        ds.select_segs = rng.integers(0, 50, (n, npts)).astype(np.int64)
    return ds


def _loaders(B, npts, n_gt=7, n_ng=10, seed=0):
    gt = D.DeviceCloudLoader(_synthetic(D.ShapeNetDatasetGT, n_gt, npts, seed), B, seed=3)
    ng = D.DeviceCloudLoader(_synthetic(D.ShapeNetDataset_noGT, n_ng, npts, seed + 1), B, seed=4)
    return gt, ng


def _orders(gt, ng, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(ld.n, generator=g).to(DEV) for ld in (gt, ng)]


def _cursors(a, b):
    return [torch.tensor([a], device=DEV, dtype=torch.int32),
            torch.tensor([b], device=DEV, dtype=torch.int32)]


def _prefilled(B, N):
    return (torch.full((2 * B, N, 3), float("nan"), device=DEV),
            torch.full((2 * B, 1, 16), float("nan"), device=DEV),
            torch.full((B, N), -1, device=DEV, dtype=torch.int64))


def _reference(gt, ng, orders, cursors):
    """The two loaders' own gather_at and _pack: (pts, cls, seg) packed."""
    outs = []
    for ld, order, cur in zip((gt, ng), orders, cursors):
        pts = torch.full((ld.B, ld.npts, 3), float("nan"), device=DEV)
        lab = torch.full((ld.B, 1), -1, device=DEV, dtype=torch.int64)
        seg = None if ld.segs is None else torch.full((ld.B, ld.npts), -1, device=DEV,
                                                      dtype=torch.int64)
        ld.gather_at(order, cur, pts, lab, seg)
        outs.append(ld._pack(pts, lab, seg))
    (pg, cg, sg), (pn, cn) = outs
    return torch.cat([pg, pn]), torch.cat([cg, cn]), sg


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, ref):
    for g, r, name in zip(got, ref, ("pts", "cls", "seg")):
        assert g.shape == r.shape and torch.equal(_bits(g), _bits(r)), name


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("npts", [1, 48, 257])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_pair_equals_the_two_gathers_and_the_one_hot(B, npts, last):
    """Splits of 7 and 10 clouds; npts 257 = one full 256-thread block and a
    partial one, 48 and 1 less than a block; the cursor at the first and at
    each split's last whole batch."""
    gt, ng = _loaders(B, npts)
    orders = _orders(gt, ng)
    cursors = _cursors(gt.n // B - 1, ng.n // B - 1) if last else _cursors(0, 0)
    got = _prefilled(B, npts)
    D.gather_seg_pair(gt, ng, orders, cursors, *got)
    _same(got, _reference(gt, ng, orders, cursors))
    assert got[1].sum().item() == 2 * B  # one 1 per row, zeros written


def test_pair_on_the_fixture_split(tmp_path):
    """The ShapeNet fixture split 3 GT / 4 no-GT clouds, 48 of its 50 points."""
    lst = _list(tmp_path, ["shapenet_latest.h5"])
    rows = np.array([0, 2, 5])
    gt = D.DeviceCloudLoader(D.ShapeNetDatasetGT(rows, lst, num_classes=16, num_pts=48), 2, seed=1)
    ng = D.DeviceCloudLoader(D.ShapeNetDataset_noGT(rows, lst, num_classes=16, num_pts=48), 2,
                             seed=2)
    assert (gt.n, ng.n) == (3, 4)
    orders = _orders(gt, ng, seed=5)
    for cursors in (_cursors(0, 0), _cursors(0, 1)):
        got = _prefilled(2, 48)
        D.gather_seg_pair(gt, ng, orders, cursors, *got)
        _same(got, _reference(gt, ng, orders, cursors))


def test_each_half_jitters_with_its_own_job():
    """sigma on, the two loaders' step counters at different values: each half
    is still bitwise its loader's gather_at (its own seed, step, rng_row0)."""
    gt, ng = _loaders(2, 48)
    gt.sigma = ng.sigma = 0.01
    gt.step.fill_(3)
    ng.step.fill_(11)
    orders, cursors = _orders(gt, ng), _cursors(1, 2)
    got = _prefilled(2, 48)
    D.gather_seg_pair(gt, ng, orders, cursors, *got)
    ref = _reference(gt, ng, orders, cursors)
    _same(got, ref)
    src = torch.cat([gt.pts[orders[0][2:4]], ng.pts[orders[1][4:6]]])
    j = got[0] - src
    assert 0 < j.abs().max().item() <= 0.05 + 1e-6 and not torch.equal(j[:2], j[2:])


def test_an_order_entry_outside_the_split_leaves_its_rows():
    gt, ng = _loaders(3, 48)
    orders, cursors = _orders(gt, ng), _cursors(1, 0)
    good = [o.clone() for o in orders]
    orders[0][3 + 1] = gt.n       # GT batch 1, row 1
    orders[1][0] = -1             # no-GT batch 0, row 0
    got = _prefilled(3, 48)
    D.gather_seg_pair(gt, ng, orders, cursors, *got)
    ref = _reference(gt, ng, good, cursors)
    skipped_pts = [1, 3 + 0]
    for r in range(6):
        if r in skipped_pts:
            assert torch.isnan(got[0][r]).all() and torch.isnan(got[1][r]).all(), r
        else:
            assert torch.equal(_bits(got[0][r]), _bits(ref[0][r])), r
            assert torch.equal(_bits(got[1][r]), _bits(ref[1][r])), r
    assert (got[2][1] == -1).all()
    assert torch.equal(got[2][[0, 2]], ref[2][[0, 2]])


def test_advancing_the_cursors_gives_the_next_batches():
    gt, ng = _loaders(2, 48)
    orders, cursors = _orders(gt, ng), _cursors(0, 0)
    a, b = _prefilled(2, 48), _prefilled(2, 48)
    D.gather_seg_pair(gt, ng, orders, cursors, *a)
    for c in cursors:
        c += 1
    D.gather_seg_pair(gt, ng, orders, cursors, *b)
    _same(b, _reference(gt, ng, orders, cursors))
    assert not torch.equal(a[0][:2], b[0][:2]) and not torch.equal(a[0][2:], b[0][2:])
    assert not torch.equal(a[2], b[2])


def test_argument_checks():
    gt, ng = _loaders(2, 48)
    orders, cursors = _orders(gt, ng), _cursors(0, 0)
    pts, cls, seg = _prefilled(2, 48)
    with pytest.raises(ValueError, match="shapenet_gt"):
        D.gather_seg_pair(ng, gt, orders, cursors, pts, cls, seg)
    with pytest.raises(ValueError, match="cls"):
        D.gather_seg_pair(gt, ng, orders, cursors, pts, cls[:, :, :8].contiguous(), seg)
    with pytest.raises(ValueError, match="pts"):
        D.gather_seg_pair(gt, ng, orders, cursors, pts[:3], cls, seg)
    with pytest.raises(ValueError, match="order"):
        D.gather_seg_pair(gt, ng, [orders[0][:3], orders[1]], cursors, pts, cls, seg)
    other = D.DeviceCloudLoader(_synthetic(D.ShapeNetDataset_noGT, 5, 48, 9), 3, seed=4)
    with pytest.raises(ValueError, match="loaders differ"):
        D.gather_seg_pair(gt, other, orders, cursors, pts, cls, seg)

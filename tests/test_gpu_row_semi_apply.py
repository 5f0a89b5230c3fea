"""pcadv_row_semi_apply (csrc/semi.hip: the one-launch gradient pass with K in
device memory) on test_gpu_row_semi.py's cases: against the float64 restatement
(semi_seg_ref) and, bitwise, against what pcadv_row_semi_ce adds on the same
inputs.  MI355X only."""
import ctypes

import numpy as np
import pytest
import torch

import semi_seg_ref as R
from adversarial_learning_on_pointclouds_amd import _lib
from adversarial_learning_on_pointclouds_amd.discriminator import row_semi_apply

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _apply(x, d_out, th, scale, ncls, K, prefill=None, want_labels=True):
    """Host arrays in, (dlogits, labels) out; K goes to device memory."""
    tx, td = _dev(x), _dev(np.asarray(d_out, np.float32))
    tg = _dev(np.zeros_like(x) if prefill is None else prefill.copy())
    lab = torch.full((x.shape[0],), -7, dtype=torch.int32, device=DEV) if want_labels else None
    kept = torch.tensor([K], dtype=torch.int32, device=DEV)
    row_semi_apply(tx, ncls, td, th, scale, kept, tg, lab)
    torch.cuda.synchronize()
    return tg.cpu().numpy(), None if lab is None else lab.cpu().numpy()


def _two_launch(x, d_out, th, scale, ncls, prefill=None):
    """pcadv_row_semi_ce on the same inputs: (dlogits, K)."""
    lib = _lib.load()
    tx, td = _dev(x), _dev(np.asarray(d_out, np.float32))
    tg = _dev(np.zeros_like(x) if prefill is None else prefill.copy())
    M = x.shape[0]
    ws = torch.empty(lib.pcadv_row_semi_ce_workspace_bytes(M), dtype=torch.uint8, device=DEV)
    loss, kept = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.pcadv_row_semi_ce(_p(tx), tx.shape[1], _p(td), M, ncls, th, scale, _p(tg),
                                     tg.shape[1], None, _p(loss), _p(kept), _p(ws), ws.numel(),
                                     _lib.stream_ptr()), "pcadv_row_semi_ce")
    torch.cuda.synchronize()
    return tg.cpu().numpy(), int(kept.item())


def _row_err(g, ref, keep):
    num = np.abs(g[keep].astype(np.float64) - ref[keep]).max(axis=1)
    return float((num / np.abs(ref[keep]).max(axis=1)).max())


def _inputs(M, ncls, ld, seed):
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((M, ld))).astype(np.float32)
    x[:, ncls:] = 1e30  # columns past ncls are not the row's
    d_out = rng.uniform(0.0, 1.0, M).astype(np.float32)
    d_out[0] = 0.75  # the single-row case keeps its row
    return rng, x, d_out


@pytest.mark.parametrize("M,ncls,ld", [(1, 2, 2), (63, 3, 5), (257, 50, 50), (1000, 64, 64),
                                       (300, 50, 52), (40007, 50, 52)])
def test_shapes(M, ncls, ld):
    """Labels exact, the gradient within 1e-5 relative per kept row of f64 and
    bitwise pcadv_row_semi_ce's, from a zero prefill and on a random one, where
    ignored rows and columns [ncls, ld) keep the prefill's bits.  40007 rows:
    more than one row per slot, the last workgroup partly filled."""
    rng, x, d_out = _inputs(M, ncls, ld, 10 * M + ncls)
    th, scale = 0.5, 2.5
    _, g_r, lab_r, K_r = R.semi_ce(x[:, :ncls], d_out, th, scale)
    keep = lab_r != R.IGNORE
    g, lab = _apply(x, d_out, th, scale, ncls, K_r)
    assert np.array_equal(lab, lab_r) and K_r > 0
    e_g = _row_err(g[:, :ncls], g_r, keep)
    print(f"M={M} ncls={ncls} ld={ld}: K {K_r}, gradient rel err per row, max {e_g:.2e}")
    assert e_g <= 1e-5
    assert not g[~keep].any() and not g[:, ncls:].any()
    g2, K2 = _two_launch(x, d_out, th, scale, ncls)
    assert K2 == K_r and np.array_equal(g.view(np.uint32), g2.view(np.uint32))
    pre = rng.standard_normal((M, ld)).astype(np.float32)
    g3, _ = _apply(x, d_out, th, scale, ncls, K_r, prefill=pre, want_labels=False)
    assert np.array_equal(g3[~keep], pre[~keep]) and np.array_equal(g3[:, ncls:], pre[:, ncls:])
    assert not np.array_equal(g3[keep][:, :ncls], pre[keep][:, :ncls])
    g4, _ = _two_launch(x, d_out, th, scale, ncls, prefill=pre)
    assert np.array_equal(g3.view(np.uint32), g4.view(np.uint32))


def test_k_zero_touches_nothing_but_labels():
    M, ncls, ld = 300, 50, 52
    rng, x, d_out = _inputs(M, ncls, ld, 1)
    pre = rng.standard_normal((M, ld)).astype(np.float32)
    g, lab = _apply(x, d_out, 2.0, 1.0, ncls, 0, prefill=pre)
    assert np.all(lab == 255)
    assert np.array_equal(g.view(np.uint32), pre.view(np.uint32))
    # no row counts as kept with K = 0, whatever the threshold says
    g, lab = _apply(x, d_out, 0.5, 1.0, ncls, 0, prefill=pre)
    assert np.all(lab == 255) and np.array_equal(g.view(np.uint32), pre.view(np.uint32))


def test_k_is_read_from_memory():
    """Twice the K in memory halves the gradient (a power of two: exactly)."""
    M, ncls, ld = 257, 50, 50
    _, x, d_out = _inputs(M, ncls, ld, 4)
    _, _, lab_r, K = R.semi_ce(x, d_out, 0.5, 1.0)
    g1, _ = _apply(x, d_out, 0.5, 1.0, ncls, K)
    g2, _ = _apply(x, d_out, 0.5, 2.0, ncls, 2 * K)
    g3, _ = _apply(x, d_out, 0.5, 1.0, ncls, 2 * K)
    assert g1.any() and np.array_equal(g1, g2) and np.array_equal(g1, 2.0 * g3)


def test_threshold_equality_and_nan():
    M, ncls, ld = 257, 50, 50
    _, x, d_out = _inputs(M, ncls, ld, 2)
    th = np.float32(0.3125)
    d_out = (d_out + 1.0).astype(np.float32)
    d_out[100] = th
    d_out[101] = np.nextafter(th, np.float32(1))
    d_out[102] = np.nan
    _, g_r, lab_r, K_r = R.semi_ce(x, d_out, float(th), 1.0)
    g, lab = _apply(x, d_out, float(th), 1.0, ncls, K_r)
    assert K_r == M - 1 and lab[100] == 255 and not g[100].any()
    assert np.array_equal(lab, lab_r) and g[101].any() and g[102].any()
    assert _row_err(g, g_r, lab_r != 255) <= 1e-5


@pytest.mark.parametrize("ncls,ld", [(50, 50), (7, 7), (64, 64), (50, 52)])
def test_ties_take_the_first_index(ncls, ld):
    rng = np.random.default_rng(ncls + ld)
    groups = [(0, ncls - 1), (1, ncls - 1), (0, 1), (2, ncls // 2, ncls - 1), (0, 3, ncls - 1),
              (3, 4, 5), (ncls - 2, ncls - 1)]
    x = rng.uniform(-4, 4, (len(groups) + 1, ld)).astype(np.float32)
    for r, grp in enumerate(groups):
        x[r, list(grp)] = np.float32(5.25)  # bit-identical maxima
    x[-1, :] = np.float32(-1.75)  # all equal
    x[:, ncls:] = 1e30
    d_out = np.ones(len(x), np.float32)
    g, lab = _apply(x, d_out, 0.5, 1.0, ncls, len(x))
    assert lab.tolist() == [grp[0] for grp in groups] + [0]
    _, g_r, lab_r, _ = R.semi_ce(x[:, :ncls], d_out, 0.5, 1.0)
    assert _row_err(g[:, :ncls], g_r, np.ones(len(x), bool)) <= 1e-5


def test_separate_strides_and_unaligned_base():
    """ldd != ld, and logits starting 4 bytes into an allocation (no 16-byte loads)."""
    M, ncls, ld, ldd = 130, 50, 52, 64
    rng, x, d_out = _inputs(M, ncls, ld, 6)
    _, g_r, lab_r, K = R.semi_ce(x[:, :ncls], d_out, 0.5, 1.0)
    keep = lab_r != 255
    pre = np.zeros((M, ldd), np.float32)
    pre[:, ncls:] = 3.0
    tx, td = _dev(x), _dev(d_out)
    kept = torch.tensor([K], dtype=torch.int32, device=DEV)
    tg = _dev(pre)
    lab = torch.zeros(M, dtype=torch.int32, device=DEV)
    row_semi_apply(tx, ncls, td, 0.5, 1.0, kept, tg, lab)
    g = tg.cpu().numpy()
    assert np.array_equal(lab.cpu().numpy(), lab_r) and np.all(g[:, ncls:] == 3.0)
    assert _row_err(g[:, :ncls], g_r, keep) <= 1e-5
    buf = torch.zeros(M * ld + 1, device=DEV)
    tx1 = buf[1:].view(M, ld)
    tx1.copy_(tx)
    tg1 = torch.zeros(M, ld, device=DEV)
    row_semi_apply(tx1, ncls, td, 0.5, 1.0, kept, tg1)
    assert np.array_equal(tg1.cpu().numpy()[:, :ncls], g[:, :ncls])  # both paths: the same bits


def test_graph_replay_adds_each_time():
    M, ncls, ld = 600, 50, 52
    _, x, d_out = _inputs(M, ncls, ld, 8)
    _, _, _, K = R.semi_ce(x[:, :ncls], d_out, 0.5, 1.0)
    g1, _ = _apply(x, d_out, 0.5, 1.0, ncls, K)
    tx, td = _dev(x), _dev(d_out)
    tg = torch.zeros(M, ld, device=DEV)
    kept = torch.tensor([K], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        row_semi_apply(tx, ncls, td, 0.5, 1.0, kept, tg)
    torch.cuda.synchronize()
    assert not tg.any()  # capturing ran nothing
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(tg.cpu().numpy(), g1)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(tg.cpu().numpy(), g1 + g1)  # g + g is exact


def test_bad_arguments_are_refused():
    lib = _lib.load()
    t = torch.zeros(4, 70, device=DEV)
    d = torch.zeros(4, device=DEV)
    k = torch.ones(1, dtype=torch.int32, device=DEV)
    for ncls, ld in ((1, 70), (65, 70), (50, 40)):
        rc = lib.pcadv_row_semi_apply(_p(t), ld, _p(d), 4, ncls, 0.5, 1.0, _p(k), _p(t), ld, None,
                                      _lib.stream_ptr())
        assert rc != 0 and b"row_semi_apply" in lib.pcadv_last_error()
    for args in ((None, _p(d), _p(k), _p(t)), (_p(t), None, _p(k), _p(t)), (_p(t), _p(d), None, _p(t)),
                 (_p(t), _p(d), _p(k), None)):
        rc = lib.pcadv_row_semi_apply(args[0], 70, args[1], 4, 50, 0.5, 1.0, args[2], args[3], 70,
                                      None, _lib.stream_ptr())
        assert rc != 0
    assert lib.pcadv_row_semi_apply(_p(t), 70, _p(d), 0, 50, 0.5, 1.0, _p(k), _p(t), 70, None,
                                    _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not t.any()

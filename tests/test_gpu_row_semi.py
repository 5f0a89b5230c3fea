"""pcadv_row_semi_ce (csrc/semi.hip) against the float64 restatement
(semi_seg_ref): keep rule, first-index pseudo-labels, the kept rows' mean loss,
the gradient ADDED to dlogits, untouched memory, determinism, graph replay.
MI355X only."""
import ctypes

import numpy as np
import pytest
import torch

import semi_seg_ref as R
from adversarial_learning_on_pointclouds_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch(tx, td, th, scale, tg, ncls, lab=None, loss=None, kept=None, ws=None):
    """One call on device tensors (tx [M][ld], td [M], tg [M][ldd] updated in place)."""
    lib = _lib.load()
    M = tx.shape[0]
    if ws is None:
        ws = torch.empty(lib.pcadv_row_semi_ce_workspace_bytes(M), dtype=torch.uint8, device=DEV)
    _lib.check(lib.pcadv_row_semi_ce(_p(tx), tx.shape[1], _p(td), M, ncls, th, scale, _p(tg),
                                     tg.shape[1], _p(lab), _p(loss), _p(kept), _p(ws), ws.numel(),
                                     _lib.stream_ptr()), "pcadv_row_semi_ce")


def _call(x, d_out, th, scale, ncls, prefill=None, want_labels=True):
    """x f32 [M][ld], d_out f32 [M], prefill f32 [M][ldd] (zeros [M][ld] when
    None) on the host.  Returns (dlogits, labels, loss, K) on the host."""
    tx = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    td = torch.from_numpy(np.ascontiguousarray(d_out, dtype=np.float32)).to(DEV)
    tg = torch.from_numpy(np.zeros_like(x) if prefill is None else prefill.copy()).to(DEV)
    lab = torch.full((x.shape[0],), -7, dtype=torch.int32, device=DEV) if want_labels else None
    loss = torch.full((1,), -7.0, device=DEV)
    kept = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _launch(tx, td, th, scale, tg, ncls, lab, loss, kept)
    torch.cuda.synchronize()
    return (tg.cpu().numpy(), None if lab is None else lab.cpu().numpy(), float(loss.item()),
            int(kept.item()))


def _row_err(g, ref, keep):
    """Per kept row max |g - ref| / max |ref| over the row; the largest."""
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
                                       (300, 50, 52)])
def test_shapes(M, ncls, ld):
    """Labels and K exact, the loss within 1e-5 relative, the gradient within
    1e-5 relative per kept row (from a zero prefill: the sum is the gradient
    itself).  On a random prefill the result is prefill + gradient: each element
    within the same bound plus one f32 spacing of the prefilled value (the
    addition rounds once), and ignored rows and columns [ncls, ld) keep the
    prefill's bits."""
    rng, x, d_out = _inputs(M, ncls, ld, 10 * M + ncls)
    th, scale = 0.5, 2.5
    loss_r, g_r, lab_r, K_r = R.semi_ce(x[:, :ncls], d_out, th, scale)
    keep = lab_r != R.IGNORE
    g, lab, loss, K = _call(x, d_out, th, scale, ncls)
    assert np.array_equal(lab, lab_r) and K == K_r and K > 0
    e_loss = abs(loss - loss_r) / loss_r
    e_g = _row_err(g[:, :ncls], g_r, keep)
    print(f"M={M} ncls={ncls} ld={ld}: K {K}, loss {loss!r} f64 {loss_r!r} rel {e_loss:.2e}; "
          f"gradient rel err per row, max {e_g:.2e}")
    assert e_loss <= 1e-5 and e_g <= 1e-5
    assert not g[~keep].any() and not g[:, ncls:].any()
    pre = rng.standard_normal((M, ld)).astype(np.float32)
    g2, lab2, loss2, K2 = _call(x, d_out, th, scale, ncls, prefill=pre, want_labels=False)
    assert loss2 == loss and K2 == K
    assert np.array_equal(g2[~keep], pre[~keep]) and np.array_equal(g2[:, ncls:], pre[:, ncls:])
    diff = np.abs(g2[keep][:, :ncls].astype(np.float64) - (pre[keep][:, :ncls].astype(np.float64) + g_r[keep]))
    bound = 1e-5 * np.abs(g_r[keep]).max(axis=1, keepdims=True) + np.spacing(np.abs(pre[keep][:, :ncls]))
    assert np.all(diff <= bound)
    assert not np.array_equal(g2[keep][:, :ncls], pre[keep][:, :ncls])  # something was added


def test_several_rows_per_slot():
    """Above 32768 rows a workgroup walks more than one row per slot (32 rows per
    workgroup here, the last one partly filled)."""
    M, ncls, ld = 40007, 50, 52
    rng, x, d_out = _inputs(M, ncls, ld, 3)
    loss_r, g_r, lab_r, K_r = R.semi_ce(x[:, :ncls], d_out, 0.5, 3.0)
    keep = lab_r != R.IGNORE
    pre = np.zeros((M, ld), np.float32)
    pre[:, ncls:] = rng.standard_normal((M, ld - ncls)).astype(np.float32)
    g, lab, loss, K = _call(x, d_out, 0.5, 3.0, ncls, prefill=pre)
    assert np.array_equal(lab, lab_r) and K == K_r
    e_loss, e_g = abs(loss - loss_r) / loss_r, _row_err(g[:, :ncls], g_r, keep)
    print(f"M={M}: K {K}, loss rel {e_loss:.2e}, gradient rel err per row, max {e_g:.2e}")
    assert e_loss <= 1e-5 and e_g <= 1e-5
    assert not g[~keep][:, :ncls].any() and np.array_equal(g[:, ncls:], pre[:, ncls:])


def test_all_ignored_touches_nothing():
    M, ncls, ld = 300, 50, 52
    rng, x, d_out = _inputs(M, ncls, ld, 1)
    pre = rng.standard_normal((M, ld)).astype(np.float32)
    g, lab, loss, K = _call(x, d_out, 2.0, 1.0, ncls, prefill=pre)
    assert loss == 0.0 and K == 0 and np.all(lab == 255)
    assert np.array_equal(g.view(np.uint32), pre.view(np.uint32))


def test_all_kept_and_threshold_equality():
    """Every row above the threshold; then one d_out exactly equal to it is the
    only ignored row (D_out <= semi_TH), a NaN d_out is kept (NaN <= TH is False)."""
    M, ncls, ld = 257, 50, 50
    _, x, d_out = _inputs(M, ncls, ld, 2)
    th = np.float32(0.3125)
    d_out = (d_out + 1.0).astype(np.float32)
    g, lab, loss, K = _call(x, d_out, float(th), 1.0, ncls)
    loss_r, g_r, lab_r, _ = R.semi_ce(x, d_out, float(th), 1.0)
    assert K == M and np.array_equal(lab, lab_r) and abs(loss - loss_r) <= 1e-5 * loss_r
    assert _row_err(g, g_r, lab_r != 255) <= 1e-5
    d_out[100] = th
    d_out[101] = np.nextafter(th, np.float32(1))
    d_out[102] = np.nan
    g, lab, loss, K = _call(x, d_out, float(th), 1.0, ncls)
    assert K == M - 1 and lab[100] == 255 and not g[100].any()
    assert lab[101] == lab_r[101] and lab[102] == lab_r[102] and g[101].any() and g[102].any()


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
    g, lab, loss, K = _call(x, d_out, 0.5, 1.0, ncls)
    assert lab.tolist() == [grp[0] for grp in groups] + [0] and K == len(x)
    loss_r, g_r, lab_r, _ = R.semi_ce(x[:, :ncls], d_out, 0.5, 1.0)
    assert np.array_equal(lab, lab_r) and abs(loss - loss_r) <= 1e-5 * loss_r
    assert _row_err(g[:, :ncls], g_r, np.ones(len(x), bool)) <= 1e-5


def test_large_logits_stay_finite():
    M, ncls = 64, 50
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([-80.0, 80.0], np.float32), (M, ncls))
    x[0, :] = -80.0
    x[1, :] = 80.0
    x[2, :] = -80.0
    x[2, 17] = 80.0
    d_out = np.ones(M, np.float32)
    g, lab, loss, K = _call(x, d_out, 0.5, 1.0, ncls)
    loss_r, g_r, lab_r, _ = R.semi_ce(x, d_out, 0.5, 1.0)
    assert K == M and np.isfinite(loss) and np.all(np.isfinite(g))
    assert np.array_equal(lab, lab_r) and abs(loss - loss_r) <= 1e-5 * loss_r
    # row 2's gradient is 49 exp(-160) / M ~ 1e-70: below f32's range, 0 on the device
    assert _row_err(g, g_r, np.abs(g_r).max(axis=1) > 1e-30) <= 1e-5
    assert np.abs(g_r[2]).max() < 1e-60 and not g[2].any()


def test_separate_strides_and_unaligned_base():
    """ldd != ld, and logits starting 4 bytes into an allocation (no 16-byte loads)."""
    M, ncls, ld, ldd = 130, 50, 52, 64
    rng, x, d_out = _inputs(M, ncls, ld, 6)
    loss_r, g_r, lab_r, K_r = R.semi_ce(x[:, :ncls], d_out, 0.5, 1.0)
    keep = lab_r != 255
    pre = np.zeros((M, ldd), np.float32)
    pre[:, ncls:] = 3.0
    g, lab, loss, K = _call(x, d_out, 0.5, 1.0, ncls, prefill=pre)
    assert np.array_equal(lab, lab_r) and K == K_r and np.all(g[:, ncls:] == 3.0)
    assert _row_err(g[:, :ncls], g_r, keep) <= 1e-5
    buf = torch.zeros(M * ld + 1, device=DEV)
    tx = buf[1:].view(M, ld)
    tx.copy_(torch.from_numpy(x))
    tg = torch.zeros(M, ld, device=DEV)
    loss_t, kept_t = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    _launch(tx, torch.from_numpy(d_out).to(DEV), 0.5, 1.0, tg, ncls, None, loss_t, kept_t)
    assert int(kept_t.item()) == K and float(loss_t.item()) == loss
    assert np.array_equal(tg.cpu().numpy()[:, :ncls], g[:, :ncls])  # both paths: the same bits


def test_two_calls_are_bitwise_equal():
    M, ncls, ld = 1000, 50, 52
    rng, x, d_out = _inputs(M, ncls, ld, 7)
    pre = rng.standard_normal((M, ld)).astype(np.float32)
    a = _call(x, d_out, 0.5, 1.0, ncls, prefill=pre)
    b = _call(x, d_out, 0.5, 1.0, ncls, prefill=pre)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1]) and np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes()
    assert a[3] == b[3]


def test_graph_replay_adds_each_time():
    """One call captured in a graph and replayed twice adds the gradient twice;
    the workspace is not touched by the host in between."""
    lib = _lib.load()
    M, ncls, ld = 600, 50, 52
    _, x, d_out = _inputs(M, ncls, ld, 8)
    g1, _, loss1, K1 = _call(x, d_out, 0.5, 1.0, ncls)
    tx, td = torch.from_numpy(x).to(DEV), torch.from_numpy(d_out).to(DEV)
    tg = torch.zeros(M, ld, device=DEV)
    loss, kept = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.full((lib.pcadv_row_semi_ce_workspace_bytes(M),), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(tx, td, 0.5, 1.0, tg, ncls, None, loss, kept, ws)
    torch.cuda.synchronize()
    assert not tg.any()  # capturing ran nothing
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(tg.cpu().numpy(), g1)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(tg.cpu().numpy(), g1 + g1)  # g + g is exact
    assert float(loss.item()) == loss1 and int(kept.item()) == K1


def test_bad_arguments_are_refused():
    lib = _lib.load()
    t = torch.zeros(4, 70, device=DEV)
    d = torch.zeros(4, device=DEV)
    nb = lib.pcadv_row_semi_ce_workspace_bytes(4)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    one = torch.zeros(1, device=DEV)
    for ncls, ld in ((1, 70), (65, 70), (50, 40)):
        rc = lib.pcadv_row_semi_ce(_p(t), ld, _p(d), 4, ncls, 0.5, 1.0, _p(t), ld, None, _p(one),
                                   None, _p(ws), nb, _lib.stream_ptr())
        assert rc != 0
    rc = lib.pcadv_row_semi_ce(_p(t), 70, _p(d), 4, 50, 0.5, 1.0, _p(t), 70, None, _p(one), None,
                               _p(ws), 8, _lib.stream_ptr())
    assert rc != 0

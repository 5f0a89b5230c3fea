"""Edge shapes of the point-wise and T-Net kernels (csrc/pointwise.hip,
k_conv_max128 in csrc/feat_fwd.hip) at the C entry points, through ops.* or,
where a wrapper hides an argument, through the library directly.

Exact tests: every input (x, w, b, dy, y, dgmax, gmax_relu, a prefilled dx) is
an integer-valued f32 from {-3, .., 3}, so every product and every partial sum
is exactly representable in f32 whatever the summation order and through the
f32 MFMA (the largest sums are ~1e4 against 2^24; _exact asserts it).  The
reference is the same operation in numpy float64 and the pass condition is
exact equality, no tolerance, no element excluded.  y (for act') and gmax_relu
are independent integer arrays, not recomputed from x: no mask can flip.

Real-valued: the regulariser's generic branch (k != 64) against the oracle at
the bounds of test_gpu_tnet.test_regularizer_fwd_bwd, the zero-norm clouds
(T T^T = I exactly: zero gradient, not 0/0), and ClsFtTrainStep's step counter.
MI355X only."""
import numpy as np
import pytest
import torch

from oracle import pointnet_np as onp
from golden_util import grad_err, rel_err
from test_oracle_regularizer import GENERIC, ORTHO, reg_batch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_learning_on_pointclouds_amd import _lib, ops
    from adversarial_learning_on_pointclouds_amd._lib import PcadvError, ptr, stream_ptr

DEV = "cuda"
NONE, RELU = 0, 1
EINVAL = -1          # PCADV_EINVAL (include/pcadv.h)
SENT = 777.0         # fills outputs before a launch: an unwritten element shows
PAIRS = [(64, 3), (64, 64), (64, 128), (128, 64), (128, 128)]  # pw_bwd_weight's (O, K)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _np(t):
    return t.detach().cpu().numpy()


def _ints(rng, *shape):
    return rng.integers(-3, 4, shape).astype(np.float32)


def _exact(got, ref, what):
    """got (f32, from the device) == ref (float64) exactly, every element."""
    ref = np.asarray(ref, np.float64)
    assert np.abs(ref).max(initial=0.0) < 2 ** 24, what
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got.astype(np.float64) != ref
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                           f"{tuple(np.argwhere(bad)[0])}: {got[bad][0]} != {ref[bad][0]}")


def _act(ref, act):
    return np.maximum(ref, 0) if act == RELU else ref


def _dz(dy, y, act):
    return dy.astype(np.float64) * (y > 0) if act == RELU else dy.astype(np.float64)


def _misaligned(a):
    """A device copy of `a` whose storage starts one float past a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, device=DEV)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(_t(a))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT, device=DEV, dtype=dtype)


def _untouched(*ts):
    return all(bool((t == SENT).all()) for t in ts)


# ---------------------------------------------------------------------------
# pcadv_pw_fwd
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("K", [3, 64, 128])
@pytest.mark.parametrize("O", [32, 64, 96, 160])
def test_pw_fwd_exact(K, O):
    rng = np.random.default_rng(1000 * K + O)
    w, b = _ints(rng, O, K), _ints(rng, O)
    wt, bt = _t(w), _t(b)
    for M in (1, 63, 65, 200):
        x = _ints(rng, M, K)
        xt = _t(x)
        assert xt.data_ptr() % 16 == 0
        lin = x.astype(np.float64) @ w.astype(np.float64).T
        for act in (NONE, RELU):
            _exact(_np(ops.pw_fwd(xt, wt, bt, act)), _act(lin + b, act), f"M={M} act={act}")
        _exact(_np(ops.pw_fwd(xt, wt, None, RELU)), _act(lin, RELU), f"M={M} b=None")


def test_pw_fwd_single_kmajor_matrix():
    rng = np.random.default_rng(11)
    x, T, b = _ints(rng, 130, 64), _ints(rng, 64, 64), _ints(rng, 64)
    y = ops.pw_fwd(_t(x), _t(T), _t(b), RELU, kmajor=True, rows_per_w=0)
    _exact(_np(y), _act(x.astype(np.float64) @ T + b, RELU), "[K][O], one matrix")


@pytest.mark.parametrize("O", [64, 128])
@pytest.mark.parametrize("M", [192, 150])
def test_pw_fwd_kmajor_stack(M, O):
    """One [K][O] matrix per 64 rows; at M = 150 the last one covers 22 rows."""
    rng = np.random.default_rng(M + O)
    x, T = _ints(rng, M, 64), _ints(rng, 3, 64, O)
    y = ops.pw_fwd(_t(x), _t(T), None, NONE, kmajor=True, rows_per_w=64)
    ref = np.concatenate([x[64 * g:64 * g + 64].astype(np.float64) @ T[g] for g in range(3)])
    _exact(_np(y), ref, "[K][O] stack")


@pytest.mark.parametrize("K,O", [(64, 64), (128, 96), (3, 64)])
def test_pw_fwd_omajor_stack(K, O):
    """One [O][K] matrix per 64 rows (ops.pw_fwd takes a single one: direct call)."""
    rng = np.random.default_rng(7 * K + O)
    M = 192
    x, W, b = _ints(rng, M, K), _ints(rng, 3, O, K), _ints(rng, O)
    xt, Wt, bt, y = _t(x), _t(W), _t(b), _sent(M, O)
    rc = _lib.load().pcadv_pw_fwd(ptr(xt), M, K, ptr(Wt), ptr(bt), O, RELU, 0, 64, ptr(y),
                                  stream_ptr())
    assert rc == 0
    ref = np.concatenate([x[64 * g:64 * g + 64].astype(np.float64) @ W[g].T for g in range(3)])
    _exact(_np(y), _act(ref + b, RELU), "[O][K] stack")


@pytest.mark.parametrize("K,O,M", [(64, 96, 65), (128, 160, 200), (64, 32, 1)])
def test_pw_fwd_misaligned_weight(K, O, M):
    """An [O][K] weight one float past a 16-byte boundary takes the scalar loads
    (WView::aligned16() false); x and y stay 16-byte aligned."""
    rng = np.random.default_rng(K + O + M)
    x, w, b = _ints(rng, M, K), _ints(rng, O, K), _ints(rng, O)
    xt = _t(x)
    assert xt.data_ptr() % 16 == 0
    y = ops.pw_fwd(xt, _misaligned(w), _t(b), RELU)
    assert y.data_ptr() % 16 == 0
    _exact(_np(y), _act(x.astype(np.float64) @ w.T + b, RELU), "misaligned [O][K]")


def test_pw_chain_rejects_misaligned_weight():
    rng = np.random.default_rng(5)
    x = _t(_ints(rng, 2, 64, 3))
    ws = [_t(_ints(rng, 64, 3)), _misaligned(_ints(rng, 64, 64)), _t(_ints(rng, 64, 64)),
          _t(_ints(rng, 128, 64))]
    with pytest.raises(RuntimeError, match=r"rc=-1\).*16-byte aligned"):
        ops.pw_chain(x, [(w, None, RELU, False, 0) for w in ws])


# ---------------------------------------------------------------------------
# pcadv_pw_bwd_data
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("O", [64, 128])
@pytest.mark.parametrize("K", [3, 32, 64, 96, 128, 160])
def test_pw_bwd_data_exact(O, K):
    rng = np.random.default_rng(1000 * O + K)
    w = _ints(rng, O, K)
    wt = _t(w)
    for M in (1, 63, 130) + ((257,) if K == 3 else ()):
        dy, y, dx0 = _ints(rng, M, O), _ints(rng, M, O), _ints(rng, M, K)
        dyt, yt = _t(dy), _t(y)
        for act in (NONE, RELU):
            ref = _dz(dy, y, act) @ w
            ya = yt if act == RELU else None
            _exact(_np(ops.pw_bwd_data(dyt, ya, act, wt, K)), ref, f"M={M} act={act}")
            acc = ops.pw_bwd_data(dyt, ya, act, wt, K, out=_t(dx0))
            _exact(_np(acc), dx0 + ref, f"M={M} act={act} accumulate")


@pytest.mark.parametrize("O", [64, 128])
@pytest.mark.parametrize("aligned", [True, False])
def test_pw_bwd_data_kmajor_stack(aligned, O):
    """dx = dy T^T with one [K][O] transform per 64 rows; T one float off a
    16-byte boundary takes the scalar loads."""
    rng = np.random.default_rng(31 + O + aligned)
    M, K = 192, 64
    dy, T = _ints(rng, M, O), _ints(rng, 3, K, O)
    Tt = _t(T) if aligned else _misaligned(T)
    dx = ops.pw_bwd_data(_t(dy), None, NONE, Tt, K, kmajor=True, rows_per_w=64)
    ref = np.concatenate([dy[64 * g:64 * g + 64].astype(np.float64) @ T[g].T for g in range(3)])
    _exact(_np(dx), ref, "[K][O] stack")


# ---------------------------------------------------------------------------
# pcadv_pw_bwd_weight, pcadv_pw_wgrad_finish
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("O,K", PAIRS)
def test_pw_bwd_weight_exact(O, K):
    rng = np.random.default_rng(100 * O + K)
    for M in (1, 31, 129, 300):
        dy, y, x = _ints(rng, M, O), _ints(rng, M, O), _ints(rng, M, K)
        dyt, yt, xt = _t(dy), _t(y), _t(x)
        for act in (NONE, RELU):
            dz = _dz(dy, y, act)
            dw, db = ops.pw_bwd_weight(dyt, yt if act == RELU else None, act, xt)
            _exact(_np(dw)[0], dz.T @ x, f"dW M={M} act={act}")
            _exact(_np(db)[0], dz.sum(0), f"db M={M} act={act}")
        dw, db = ops.pw_bwd_weight(dyt, yt, RELU, xt, need_db=False)
        assert db is None
        _exact(_np(dw)[0], _dz(dy, y, RELU).T @ x, f"dW M={M} without db")


@pytest.mark.parametrize("O,K,kmajor", [(o, k, False) for o, k in PAIRS]
                         + [(o, k, True) for o, k in PAIRS if k != 3])  # K = 3: [O][K] only
def test_pw_bwd_weight_grouped(O, K, kmajor):
    """One gradient per 128 rows (a single slab each), [O][K] and [K][O]."""
    rng = np.random.default_rng(100 * O + K + kmajor)
    M = 384
    dy, y, x = _ints(rng, M, O), _ints(rng, M, O), _ints(rng, M, K)
    dw, db = ops.pw_bwd_weight(_t(dy), _t(y), RELU, _t(x), rows_per_group=128, kmajor=kmajor)
    dz = _dz(dy, y, RELU).reshape(3, 128, O)
    ref = np.einsum("gmo,gmk->gok", dz, x.reshape(3, 128, K).astype(np.float64))
    _exact(_np(dw), ref.transpose(0, 2, 1) if kmajor else ref, "grouped dW")
    _exact(_np(db), dz.sum(1), "grouped db")


WGRAD_JOBS = [(100, 64, 3, True), (300, 64, 64, True), (2100, 64, 128, True),
              (100, 128, 64, True), (300, 128, 128, True), (2100, 64, 3, True),
              (100, 128, 128, False), (2100, 128, 64, False)]  # (M, O, K, with db)


def _deferred(rng, specs):
    jobs, outs = [], []
    for M, O, K, with_db in specs:
        dy, y, x = _ints(rng, M, O), _ints(rng, M, O), _ints(rng, M, K)
        dw, db = _sent(O, K), _sent(O)
        ops.pw_bwd_weight(_t(dy), _t(y), RELU, _t(x), need_db=with_db, dw_out=dw,
                          db_out=db if with_db else None, defer=jobs)
        dz = _dz(dy, y, RELU)
        outs.append((dw, db, dz.T @ x, dz.sum(0), with_db))
    return jobs, outs


def test_pw_wgrad_finish_mixed_jobs():
    """Eight jobs of 1, 3 and 17 slabs and five widths in one launch: most of the
    16 waves get an empty slab range, narrower jobs' blocks return early."""
    jobs, outs = _deferred(np.random.default_rng(77), WGRAD_JOBS)
    assert _untouched(*[o[0] for o in outs])  # the slab launches write no gradient
    ops.pw_wgrad_finish(jobs)
    for (M, O, K, _), (dw, db, rw, rb, with_db) in zip(WGRAD_JOBS, outs):
        _exact(_np(dw), rw, f"dW of job M={M} O={O} K={K}")
        if with_db:
            _exact(_np(db), rb, f"db of job M={M} O={O} K={K}")


def test_pw_wgrad_finish_rejects_nine_jobs():
    jobs, outs = _deferred(np.random.default_rng(78), [(100, 64, 64, True)] * 9)
    with pytest.raises(RuntimeError, match=r"rc=-1\)"):
        ops.pw_wgrad_finish(jobs)
    assert _untouched(*[o[0] for o in outs], *[o[1] for o in outs])


# ---------------------------------------------------------------------------
# pcadv_conv_max_bwd
# ---------------------------------------------------------------------------

CMB_SHAPES = [(1, 1, 128, 1024), (3, 130, 128, 1024), (17, 64, 64, 128), (33, 200, 128, 256),
              (2, 129, 20, 100)]


def _cmb(dg, gidx, gmax, x, w, need_dx=True, need_db=True, dx_relu=False):
    """pcadv_conv_max_bwd into sentinel-filled outputs -> (dx, dw, db)."""
    C, N, K = x.shape
    O = w.shape[0]
    dx, dw, db = _sent(C, N, K), _sent(O, K), _sent(O)
    keep = [_t(dg), _t(gidx, torch.int32), None if gmax is None else _t(gmax), _t(x), _t(w)]
    rc = _lib.load().pcadv_conv_max_bwd(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), C,
                                        N, K, ptr(keep[4]), O, ptr(dw), ptr(db) if need_db else None,
                                        ptr(dx) if need_dx else None, int(dx_relu), stream_ptr())
    assert rc == 0
    return _np(dx), _np(dw), _np(db)


def _cmb_ref(dg, gidx, gmax, x, w):
    C, N, K = x.shape
    g = dg.astype(np.float64) * (gmax > 0) if gmax is not None else dg.astype(np.float64)
    rows = x[np.arange(C)[:, None], gidx].astype(np.float64)          # (C, O, K)
    dw = np.einsum("co,cok->ok", g, rows)
    dx = np.zeros((C, N, K))
    for c in range(C):
        np.add.at(dx[c], gidx[c], g[c][:, None] * w.astype(np.float64))
    return dx, dw, g.sum(0)


def _cmb_inputs(rng, C, N, K, O, pattern):
    gidx = {"uniform": rng.integers(0, N, (C, O)), "last": np.full((C, O), N - 1),
            "first": np.zeros((C, O), np.int64)}[pattern].astype(np.int32)
    gmax = _ints(rng, C, O)            # about 4 / 7 of it <= 0
    gmax[0, :2] = [0.0, -0.0]
    return _ints(rng, C, O), gidx, gmax, _ints(rng, C, N, K), _ints(rng, O, K)


@pytest.mark.parametrize("pattern", ["uniform", "last", "first"])
@pytest.mark.parametrize("C,N,K,O", CMB_SHAPES)
def test_conv_max_bwd_exact(C, N, K, O, pattern):
    """Every row of dx is compared: rows without hits must be 0 over the sentinel."""
    rng = np.random.default_rng(C * 1000 + N + O)
    dg, gidx, gmax, x, w = _cmb_inputs(rng, C, N, K, O, pattern)
    assert (gmax <= 0).mean() > 0.4
    for gm in (None, gmax):
        rx, rw, rb = _cmb_ref(dg, gidx, gm, x, w)
        dx, dw, db = _cmb(dg, gidx, gm, x, w)
        what = f"{pattern} gmax_relu={gm is not None}"
        _exact(dw, rw, "dW " + what)
        _exact(db, rb, "db " + what)
        _exact(dx, rx, "dx " + what)


@pytest.mark.parametrize("C,N,K,O", CMB_SHAPES)
def test_conv_max_bwd_optional_outputs(C, N, K, O):
    rng = np.random.default_rng(C * 1000 + N + O + 1)
    dg, gidx, gmax, x, w = _cmb_inputs(rng, C, N, K, O, "uniform")
    rx, rw, rb = _cmb_ref(dg, gidx, gmax, x, w)
    dx, dw, db = _cmb(dg, gidx, gmax, x, w, need_dx=False)
    assert (dx == SENT).all()
    _exact(dw, rw, "dW, no dx")
    _exact(db, rb, "db, no dx")
    dx, dw, db = _cmb(dg, gidx, gmax, x, w, need_db=False)
    assert (db == SENT).all()
    _exact(dw, rw, "dW, db = NULL")
    _exact(dx, rx, "dx, db = NULL")
    # dx stored as the layer below's dz: x holds zeros and negatives
    assert (x == 0).any() and (x < 0).any()
    dx, dw, _ = _cmb(dg, gidx, gmax, x, w, dx_relu=True)
    _exact(dx, rx * (x > 0), "dx_relu")
    _exact(dw, rw, "dW, dx_relu")


# ---------------------------------------------------------------------------
# pcadv_conv_max_fwd, O != 1024 (k_conv_max128)
# ---------------------------------------------------------------------------

def _cmf_check(x, w, b, relu, what):
    y = np.einsum("cnk,ok->cno", x.astype(np.float64), w.astype(np.float64)) + b
    if relu:
        y = np.maximum(y, 0)
    gmax, gidx = ops.conv_max_fwd(_t(x), _t(w), _t(b), relu)
    _exact(_np(gmax), y.max(1), "gmax " + what)
    gi = _np(gidx)
    first = y.argmax(1)  # numpy's argmax: the first index of the maximum
    assert gi.dtype == np.int32 and np.array_equal(gi, first), \
        f"gidx {what}: {int((gi != first).sum())} channels off the first index of the maximum"
    return y, gi


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("O", [128, 256, 384])
def test_conv_max_fwd_small_o_exact(O, relu):
    rng = np.random.default_rng(O + relu)
    w, b = _ints(rng, O, 128), _ints(rng, O)
    for C in (1, 3):
        for N in (1, 37, 64, 65, 200):
            y, _ = _cmf_check(_ints(rng, C, N, 128), w, b, relu, f"C={C} N={N}")
    ties = (y == y.max(1, keepdims=True)).sum(1)
    assert (ties > 1).any()  # the integer data ties: the first-index rule is exercised


@pytest.mark.parametrize("relu", [False, True])
def test_conv_max_fwd_small_o_duplicated_rows(relu):
    """Every point row sits at two random positions: the earlier one must win
    for every channel, across the two lanes that share a channel too."""
    rng = np.random.default_rng(9 + relu)
    C, n, O = 3, 100, 256
    x = np.empty((C, 2 * n, 128), np.float32)
    for c in range(C):
        pos = rng.permutation(2 * n).reshape(n, 2)
        rows = _ints(rng, n, 128)
        x[c, pos[:, 0]] = rows
        x[c, pos[:, 1]] = rows
    y, gi = _cmf_check(x, _ints(rng, O, 128), _ints(rng, O), relu, "duplicated rows")
    dup = (y == y.max(1, keepdims=True)).sum(1)
    assert (dup >= 2).all()


def test_conv_max_fwd_small_o_relu_all_negative_channels():
    rng = np.random.default_rng(21)
    C, N, O = 3, 130, 128
    b = _ints(rng, O)
    b[::3] = -2000.0  # below any 128-term dot product of {-3..3}: negative at every point
    y, gi = _cmf_check(_ints(rng, C, N, 128), _ints(rng, O, 128), b, True, "all-negative channels")
    assert (y[:, :, ::3] == 0).all() and (gi[:, ::3] == 0).all()


# ---------------------------------------------------------------------------
# argument rejection: PCADV_EINVAL from the host check, nothing written
# ---------------------------------------------------------------------------

def test_rejected_arguments():
    lib = _lib.load()
    s = stream_ptr()
    x64, x32, x3 = (torch.zeros(384, k, device=DEV) for k in (64, 32, 3))
    w = torch.zeros(128 * 128, device=DEV)
    y = _sent(384, 128)
    assert lib.pcadv_pw_fwd(ptr(x64), 200, 64, ptr(w), None, 64, NONE, 1, 100, ptr(y), s) == EINVAL
    assert lib.pcadv_pw_fwd(ptr(x32), 200, 32, ptr(w), None, 64, NONE, 0, 0, ptr(y), s) == EINVAL
    assert _untouched(y)

    dy = torch.zeros(384, 128, device=DEV)
    dw, db = _sent(3, 128, 128), _sent(3, 128)
    nb = lib.pcadv_pw_bwd_weight_workspace_bytes(384, 128, 128)
    ws = _sent(nb // 4)
    for M, O, K, xk, rpg in ((384, 64, 64, x64, 64), (300, 64, 64, x64, 128), (384, 128, 3, x3, 0)):
        rc = lib.pcadv_pw_bwd_weight(ptr(dy), None, NONE, ptr(xk), M, O, K, rpg, 0, ptr(dw), ptr(db),
                                     ptr(ws), nb, s)
        assert rc == EINVAL, (M, O, K, rpg)
    assert _untouched(dw, db, ws)

    xc = torch.zeros(2, 64, 128, device=DEV)
    gmax, gidx = _sent(2, 128), _sent(2, 128, dtype=torch.int32)
    b = torch.zeros(128, device=DEV)
    for K, O in ((64, 128), (128, 100)):
        rc = lib.pcadv_conv_max_fwd(ptr(xc), 2, 64, K, ptr(w), ptr(b), O, 0, ptr(gmax), ptr(gidx), s)
        assert rc == EINVAL, (K, O)
    assert _untouched(gmax, gidx)

    T = torch.zeros(2, 65, 65, device=DEV)
    norms, reg = _sent(2), _sent(1)
    assert lib.pcadv_tnet_reg_fwd(ptr(T), 2, 65, ptr(norms), ptr(reg), s) == EINVAL
    assert _untouched(norms, reg)


def test_transform_rejects_ragged_clouds():
    """Feature-transform clouds of N % 64 != 0 points are unsupported: a clean error."""
    x = torch.zeros(2, 100, 64, device=DEV)
    T = torch.zeros(2, 64, 64, device=DEV)
    with pytest.raises(PcadvError, match=r"rc=-1\).*multiple of 64"):
        ops.TransformFunction.apply(x, T)


# ---------------------------------------------------------------------------
# k_tnet_reg: the generic (k != 64) branch, the zero-norm clouds, the counter
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("k", [3, 16, 63])
def test_regularizer_generic_k(k, B):
    rng = np.random.default_rng(10 * k + B)
    T = (np.eye(k)[None] + 0.1 * rng.normal(size=(B, k, k))).astype(np.float32)
    Tt = _t(T)
    reg, _ = ops.tnet_reg_fwd(Tt)
    dT = ops.tnet_reg_bwd(Tt, torch.full((1,), 0.5, device=DEV))
    e_reg = abs(reg.item() - onp.feature_transform_regularizer(T))
    e_g = rel_err(_np(dT), 0.5 * onp.regularizer_bwd(T))
    print(f"k={k} B={B}: reg err {e_reg:.2e}, gradient rel_err {e_g:.2e}")
    assert e_reg < 1e-5
    assert e_g < 1e-5


def _reg_step(T, dT, step, grad=0.25):
    """pcadv_tnet_reg_step (the accumulate form) -> (norms, reg)."""
    B, k = T.shape[0], T.shape[1]
    norms, reg = _sent(B), _sent(1)
    g = torch.full((1,), grad, device=DEV)
    rc = _lib.load().pcadv_tnet_reg_step(ptr(T), B, k, ptr(norms), ptr(reg), ptr(g), ptr(dT),
                                         ptr(step), stream_ptr())
    assert rc == 0
    return norms, reg


def test_regularizer_zero_norm_clouds():
    """T T^T = I exactly (I, a signed permutation): norm 0 and the zero
    gradient (torch.norm's backward there), not 2 g / (B 0) * 0 = NaN."""
    T = reg_batch(64)
    Tt = _t(T)
    ref = 0.25 * onp.regularizer_bwd(T)
    reg, norms = ops.tnet_reg_fwd(Tt)
    dT = _np(ops.tnet_reg_bwd(Tt, torch.full((1,), 0.25, device=DEV)))
    n = _np(norms)
    assert (n[list(ORTHO)] == 0).all() and (n[list(GENERIC)] > 1).all()
    assert abs(reg.item() - onp.feature_transform_regularizer(T)) < 1e-5
    for b in ORTHO:
        assert not dT[b].any(), f"cloud {b}: {np.isnan(dT[b]).sum()} NaN"
    for b in GENERIC:
        e = grad_err(dT[b], ref[b])
        print(f"cloud {b}: max-rel {e[0]:.2e}")
        assert rel_err(dT[b], ref[b]) < 1e-5 and e[0] < 1e-5
    # the accumulate form: the orthogonal clouds' dT keeps its bits (a -0.f too)
    pre = np.random.default_rng(3).normal(size=T.shape).astype(np.float32)
    pre[:, 0, 0] = -0.0
    acc = _t(pre)
    step = torch.full((1,), 41, device=DEV, dtype=torch.int32)
    norms2, _ = _reg_step(Tt, acc, step)
    got = _np(acc)
    assert torch.equal(norms2, norms) and step.item() == 42
    for b in ORTHO:
        assert np.array_equal(got[b].view(np.int32), pre[b].view(np.int32))
    for b in GENERIC:
        assert rel_err(got[b] - pre[b], ref[b]) < 1e-5


@pytest.mark.parametrize("B", [1, 4])
def test_reg_step_advances_the_count_once_per_launch(B):
    T = _t(reg_batch(64)[4 - B:])
    step = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    for want in (8, 9):
        _reg_step(T, torch.zeros_like(T), step)
        assert step.item() == want


def _ft_model(seed, identity_transform=False):
    import adversarial_learning_on_pointclouds_amd as pc
    G = onp.make_params(onp.cls_ft_spec(40), seed=seed)
    if identity_transform:  # STNkd's fc3 zero: T = 0 + I
        G["feat.fstn.fc3.weight"][...] = 0
        G["feat.fstn.fc3.bias"][...] = 0
    m = pc.PointNetCls(k=40, feature_transform=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in G.items()})
    return m.to(DEV)


def _batch(seed, B, N):
    rng = np.random.default_rng(seed)
    return (_t(rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)),
            _t(rng.integers(0, 40, B), torch.int64))


def test_cls_ft_step_identity_transform_stays_finite():
    from adversarial_learning_on_pointclouds_amd.step import ClsFtTrainStep
    B, N = 4, 128
    model = _ft_model(91, identity_transform=True)
    st = ClsFtTrainStep(model, B, N, seed=5)
    losses = st(*_batch(92, B, N)).cpu().numpy()
    assert losses[1] == 0 and np.isfinite(losses[0])
    assert bool(torch.isfinite(st.g_grad).all())
    for name, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), name
    assert st.step_count.item() == 1


def test_cls_ft_step_grads_only_calls_advance_the_count():
    """apply_adam=False: every call advances the count by 1 (after the head drew
    its dropout masks at the count before), so repeated calls draw fresh masks,
    and the count alone selects them."""
    from adversarial_learning_on_pointclouds_amd.step import ClsFtTrainStep
    B, N = 4, 128
    st = ClsFtTrainStep(_ft_model(93), B, N, seed=5)
    pts, lab = _batch(94, B, N)
    p0, c0 = st.g_param.clone(), st.step_count.item()
    grads = []
    for i in range(3):
        if i == 2:
            st.step_count.fill_(c0)
        st(pts, lab, mask=None, apply_adam=False)
        grads.append(st.g_grad.clone())
        assert st.step_count.item() == (c0 if i == 2 else c0 + i) + 1
    assert torch.equal(st.g_param, p0)
    assert not torch.equal(grads[0], grads[1])
    assert torch.equal(grads[0], grads[2])

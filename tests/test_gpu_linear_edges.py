"""Edge tests of the public linear entry points (pcadv_linear_fwd /
pcadv_linear_bwd, csrc/linear.hip and csrc/wgrad.h) against float64 with
gemm_ref.sum_bound: weight gradients over the first m_w < M rows (block and
wave forms, m_w = 0), dx == NULL, an activation or dropout applied on the fly
next to dw at the 64 / 65 / 128-row switches, forward reductions of 4 .. 2052
(above 1024 in rounds) with one-row and one-column outputs and the added
identity, backward-data reductions that are no multiple of 4 and run in
rounds, and the device-drawn dropout of a (seed, step) pair in the backward.
MI355X only."""
import ctypes

import numpy as np
import pytest
import torch

import head_ref as ref
from gemm_ref import EPS, sum_bound

pytestmark = pytest.mark.gpu

DEV = "cuda"
NONE, RELU, LRELU = 0, 1, 2
ACT = {NONE: None, RELU: "relu", LRELU: "lrelu"}
P = 0.3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _rand(seed, *shapes):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]


def _worst(got, val, bnd, what):
    got = got.cpu().numpy().astype(np.float64).reshape(val.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    print(f"{what} {r.max():.3e}")
    assert r.max() <= 1.0, (what, float(r.max()))


def _dz(dy, y, act, mask):
    """dz = dy act'(y) mask keep in float64."""
    dz = np.asarray(dy, np.float64) * ref.slope(y, ACT[act])
    return dz if mask is None else dz * (np.asarray(mask, np.float64) * ref.keep_of(P))


def _check_bwd(dy, y, act, mask, x, w, m_w, dx, dw, db, tag):
    """dx, dw, db (each may be None) against float64; an activation or mask
    applied on the fly costs each dz term two more roundings."""
    dz = _dz(dy, y, act, mask)
    extra = 0 if act == NONE and mask is None else 2
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    if dx is not None:
        _worst(dx, dz @ w64, sum_bound(dz.shape[1] + extra, np.abs(dz) @ np.abs(w64)), f"{tag} dx")
    if dw is not None:
        dW, SW, dB, SB = ref.wgrad(dz[:m_w], x64[:m_w])
        _worst(dw, dW, sum_bound(m_w + extra, SW), f"{tag} dw")
        _worst(db, dB, sum_bound(m_w + extra, SB), f"{tag} db")


@pytest.mark.parametrize("M,m_w,N,K", [(96, 64, 256, 512), (40, 17, 30, 20), (300, 129, 40, 36),
                                       (96, 0, 256, 512), (40, 0, 30, 20)])
def test_bwd_weight_rows_m_w(M, m_w, N, K):
    """dw and db sum over the first m_w rows only (block form, wave form, two
    slabs); m_w = 0 gives zeros, as the header's sum says."""
    from adversarial_learning_on_pointclouds_amd import ops
    dy, x, w = _rand(M + N, (M, N), (M, K), (N, K))
    dw0, db0 = torch.full((N, K), np.nan, device=DEV), torch.full((N,), np.nan, device=DEV)
    dx, dw, db = ops.linear_bwd(_t(dy), _t(dy), NONE, None, 0.0, _t(x), _t(w), m_w=m_w,
                                dw_out=dw0, db_out=db0)
    if m_w == 0:
        assert (dw == 0).all() and (db == 0).all()
    _check_bwd(dy, dy, NONE, None, x, w, m_w, dx, dw, db, f"m_w {M},{m_w},{N},{K}")


@pytest.mark.parametrize("M,m_w,N,K", [(96, 64, 256, 512), (40, 17, 30, 20)])
def test_bwd_without_dx_is_bitwise(M, m_w, N, K):
    from adversarial_learning_on_pointclouds_amd import ops
    dy, x, w = _rand(7 + M, (M, N), (M, K), (N, K))
    args = (_t(dy), _t(dy), NONE, None, 0.0, _t(x), _t(w))
    _, dw, db = ops.linear_bwd(*args, m_w=m_w)
    dx2, dw2, db2 = ops.linear_bwd(*args, need_dx=False, m_w=m_w)
    assert dx2 is None and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("m_w", [64, 65, 128])
@pytest.mark.parametrize("act,masked", [(RELU, True), (LRELU, False), (NONE, True)])
def test_bwd_weight_with_activation_or_mask(m_w, act, masked):
    """The on-the-fly dz next to dw: four chunks at 64 rows, eight from 65 on,
    128 the most (129 is refused on the host: tests/test_cpu_host.py)."""
    from adversarial_learning_on_pointclouds_amd import ops
    M, N, K = 130, 40, 36
    dy, y, x, w = _rand(m_w + act, (M, N), (M, N), (M, K), (N, K))
    mask = (np.random.default_rng(m_w).random((M, N)) >= P).astype(np.float32) if masked else None
    dx, dw, db = ops.linear_bwd(_t(dy), _t(y), act, None if mask is None else _t(mask), P, _t(x),
                                _t(w), m_w=m_w)
    _check_bwd(dy, y, act, mask, x, w, m_w, dx, dw, db, f"act {act} mask {masked} m_w {m_w}")


@pytest.mark.parametrize("K", [4, 60, 1028, 2052])
@pytest.mark.parametrize("M,N", [(1, 1), (1, 17), (17, 1), (17, 17)])
def test_fwd_shapes(M, N, K):
    from adversarial_learning_on_pointclouds_amd import ops
    act = (K // 4 + M + N) % 3
    x, w, b = _rand(K + M + N, (M, K), (N, K), (N,))
    y = ops.linear_fwd(_t(x), _t(w), _t(b), act)
    v, S = ref.linear_fwd(x, w, b, ACT[act])
    _worst(y, v, ref.bound(K + 1, v, S, 1), f"fwd {M},{N},{K} act {act}")


@pytest.mark.parametrize("act", [NONE, RELU, LRELU])
def test_fwd_adds_the_identity(act):
    """add_identity_k = 3: the flattened 3 x 3 identity after the activation."""
    from adversarial_learning_on_pointclouds_amd import ops
    M, K = 5, 60
    x, w, b = _rand(act, (M, K), (9, K), (9,))
    y = ops.linear_fwd(_t(x), _t(w), _t(b), act, add_identity_k=3)
    v, S = ref.linear_fwd(x, w, b, ACT[act])
    v = v + np.eye(3).reshape(9)
    _worst(y, v, ref.bound(K + 1, v, S, 2), f"fwd identity act {act}")


@pytest.mark.parametrize("N", [1028, 2050])
@pytest.mark.parametrize("act", [RELU, LRELU])
def test_bwd_data_long_reductions_with_activation_and_mask(N, act):
    """dx over a reduction above 1024 (in rounds), N % 4 != 0 at 2050 (the
    scalar dz loads), activation and mask applied on the fly."""
    from adversarial_learning_on_pointclouds_amd import ops
    M, K = 17, 20
    dy, y, x, w = _rand(N + act, (M, N), (M, N), (M, K), (N, K))
    mask = (np.random.default_rng(N).random((M, N)) >= P).astype(np.float32)
    dx, dw, db = ops.linear_bwd(_t(dy), _t(y), act, _t(mask), P, _t(x), _t(w), need_dw=False)
    assert dw is None and db is None
    _check_bwd(dy, y, act, mask, x, w, M, dx, None, None, f"bwd data N {N} act {act}")


def test_bwd_redraws_the_forwards_dropout():
    """A forward with (seed, step), then a backward with the same pair: bitwise
    the backward with the explicit mask recovered from that forward, and not the
    one at step + 1."""
    from adversarial_learning_on_pointclouds_amd import _lib
    lib = _lib.load()
    M, N, K, seed = 40, 30, 20, 0x1234ABCD5678
    x, w, b, dy = (_t(a) for a in _rand(3, (M, K), (N, K), (N,), (M, N)))
    step = torch.tensor([7], dtype=torch.int32, device=DEV)
    y = torch.empty(M, N, device=DEV)
    P_, s = _lib.ptr, _lib.stream_ptr
    _lib.check(lib.pcadv_linear_fwd(P_(x), P_(w), P_(b), P_(y), M, N, K, NONE, None, P_(step), seed, P,
                                    0, s()), "pcadv_linear_fwd")
    mask = (y != 0).float()  # act NONE: a kept output is s (x w^T + b), never exactly 0 here
    n = mask.numel()
    assert abs(float(mask.mean()) - (1 - P)) <= 5 * np.sqrt(P * (1 - P) / n)

    def bwd(mask_t, step_t):
        out = [torch.full(sh, np.nan, device=DEV) for sh in ((M, K), (N, K), (N,))]
        _lib.check(lib.pcadv_linear_bwd(P_(dy), P_(y), NONE, P_(mask_t), P_(step_t), seed, P, P_(x), P_(w),
                                        P_(out[0]), P_(out[1]), P_(out[2]), M, M, N, K, s()),
                   "pcadv_linear_bwd")
        return out
    drawn, given = bwd(None, step), bwd(mask, None)
    for a, g in zip(drawn, given):
        assert torch.equal(a, g)
    _check_bwd(dy.cpu().numpy(), y.cpu().numpy(), NONE, mask.cpu().numpy(), x.cpu().numpy(),
               w.cpu().numpy(), M, *drawn, "bwd rng")
    step += 1
    assert not torch.equal(bwd(None, step)[0], drawn[0])

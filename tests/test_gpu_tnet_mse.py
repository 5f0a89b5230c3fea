"""pcadv_tnet_mse_reg (csrc/segtnet.hip) against float64 on the host: k in
{3, 64, 128}, groups (1, 0), (2, 2) and (1, 3).

The bound, with u = 2^-24, A = |T| |T|^T and S = T T^T - I in float64:

  the kernel's S has |dS_ij| <= eS_ij = (k + 1) u (A_ij + [i = j])
    (a k-term fma chain, and the subtraction of 1 on the diagonal);
  loss_g: each S_ij^2 moves by at most 2 |S_ij| eS_ij + eS_ij^2, and the sum of
    the non-negative squares (at most 16 per thread in order, a 10-level tree
    over the threads, up to four row-block sums per cloud over the group's
    clouds in order, the division) adds at most (16 + 10 + 4 B_g + 4) u of
    itself; all over B_g k^2;
  dT: G = S T computed from the kernel's S moves by eS |T| + (k + 1) u
    (|S| + eS) |T|; the coefficient scale 4 / (B_g k^2) carries three roundings
    and the product one ((k + 5) u in all on the second term, 4 u more on the
    first), and the final add into dT rounds once: 2 u (|dT_0| + coef |G|).
"""
import ctypes

import numpy as np
import pytest
import torch

import segregu_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
GROUPS = [(1, 0), (2, 2), (1, 3)]


def _lib():
    from adversarial_learning_on_pointclouds_amd import _lib
    return _lib.load(), _lib.stream_ptr()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _run(T, B0, scale, dT0):
    lib, s = _lib()
    C, k, _ = T.shape
    Tt = _dev(T)
    loss = torch.full((2,), -1.0, device=DEV)
    ws = torch.empty(4 * C, device=DEV)
    dT = None if dT0 is None else _dev(dT0)
    rc = lib.pcadv_tnet_mse_reg(_p(Tt), C, B0, k, scale, _p(loss), _p(dT), _p(ws), s)
    assert rc == 0, lib.pcadv_last_error()
    torch.cuda.synchronize()
    return loss.cpu().numpy(), None if dT is None else dT.cpu().numpy()


def _bounds(T, B0, scale, dT0):
    T = T.astype(np.float64)
    C, k, _ = T.shape
    aT = np.abs(T)
    S = np.matmul(T, T.transpose(0, 2, 1)) - np.eye(k)[None]
    eS = (k + 1) * U * (np.matmul(aT, aT.transpose(0, 2, 1)) + np.eye(k)[None])
    per = (2 * np.abs(S) * eS + eS ** 2).sum((1, 2))
    sq = (S ** 2).sum((1, 2))
    lb = np.zeros(2)
    db = np.zeros_like(T)
    for g, (lo, hi) in enumerate(((0, B0), (B0, C))):
        if hi == lo:
            continue
        Bg = hi - lo
        lb[g] = (per[lo:hi].sum() + (16 + 10 + 4 * Bg + 4) * U * sq[lo:hi].sum()) / (Bg * k * k)
        coef = abs(scale) * 4.0 / (Bg * k * k)
        G = np.abs(np.matmul(S[lo:hi], T[lo:hi]))
        eG = (1 + 4 * U) * np.matmul(eS[lo:hi], aT[lo:hi]) \
            + (k + 5) * U * np.matmul(np.abs(S[lo:hi]) + eS[lo:hi], aT[lo:hi])
        db[lo:hi] = coef * eG + 2 * U * (np.abs(dT0[lo:hi]) + coef * G)
    return lb, db


@pytest.mark.parametrize("B0,B1", GROUPS)
@pytest.mark.parametrize("k", [3, 64, 128])
def test_identity_is_exactly_zero(k, B0, B1):
    C = B0 + B1
    T = np.broadcast_to(np.eye(k, dtype=np.float32), (C, k, k)).copy()
    rng = np.random.default_rng(k + C)
    dT0 = rng.normal(size=(C, k, k)).astype(np.float32)
    dT0[0, 0, :2] = [0.0, -0.0]  # a signed zero stays as it is, too
    loss, dT = _run(T, B0, 3.0, dT0)
    assert loss[0] == 0.0 and loss[1] == 0.0
    assert dT.tobytes() == dT0.tobytes()


@pytest.mark.parametrize("spread", [0.02, 0.7])
@pytest.mark.parametrize("B0,B1", GROUPS)
@pytest.mark.parametrize("k", [3, 64, 128])
def test_random_vs_float64(k, B0, B1, spread):
    """T = I + spread N(0, 1) / sqrt(k): near the identity and far from it."""
    C = B0 + B1
    rng = np.random.default_rng(100 * k + 10 * C + int(100 * spread))
    T = (np.eye(k)[None] + spread * rng.normal(size=(C, k, k)) / np.sqrt(k)).astype(np.float32)
    dT0 = (0.01 * rng.normal(size=(C, k, k))).astype(np.float32)
    scale = 2.5
    runs = [_run(T, B0, scale, dT0) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    loss, dT = runs[0]
    want_l, want_g = ref.mse_reg(T, B0, scale)
    lb, db = _bounds(T, B0, scale, dT0)
    el = np.abs(loss - want_l)
    eg = np.abs(dT - (dT0.astype(np.float64) + want_g))
    print(f"loss {loss} reference {want_l} err/bound {el / np.maximum(lb, 1e-300)}; "
          f"dT err/bound {np.max(eg / np.maximum(db, 1e-300)):.3f}")
    assert want_l[0] > 0 and (B1 == 0) == (want_l[1] == 0)
    assert np.all(el <= lb)
    assert np.all(eg <= db)
    assert not np.array_equal(dT, dT0)
    # dT = NULL: the loss alone, the same bits
    loss2, none = _run(T, B0, scale, None)
    assert none is None and loss2.tobytes() == loss.tobytes()


def test_bad_arguments():
    lib, s = _lib()
    T = _dev(np.zeros((2, 8, 8), np.float32))
    loss = torch.full((2,), -1.0, device=DEV)
    ws = torch.empty(8, device=DEV)
    call = lambda **o: lib.pcadv_tnet_mse_reg(  # noqa: E731
        o.get("T", _p(T)), o.get("C", 2), o.get("B0", 1), o.get("k", 8), 1.0,
        o.get("loss", _p(loss)), None, o.get("ws", _p(ws)), s)
    bad = [call(k=6), call(k=132), call(k=0), call(B0=3), call(B0=0), call(C=-1), call(T=None),
           call(loss=None), call(ws=None)]
    assert all(rc == -1 for rc in bad), bad
    assert call(C=0, B0=0) == 0
    torch.cuda.synchronize()
    assert loss.tolist() == [-1.0, -1.0]

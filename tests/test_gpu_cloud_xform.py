"""pcadv_cloud_xform_fwd / _bwd (csrc/segtnet.hip) against float64 on the host:
k in {3, 128}, C in {1, 3}, Npts in {1, 63, 128, 257} (one point, a partial
tile, whole tiles, more than one workgroup with a tail), dense and strided
operands (the x3 column block of the [rows][960] buffer), every output inside
canary-filled padding.

Bound per element: the f32 summation bound n 2^-24 sum|a||b| with the float64
operands, n the number of terms of the element's sum: k for y; k + 2 for dx
(the k products, the addend and the value already in dx, the last two as
products with 1, so their magnitudes are in the sum); Npts for dT, Npts + 1
with accumulate (the value already in dT).  A masked dx element is exactly
what it was."""
import ctypes

import numpy as np
import pytest
import torch

import segregu_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
CANARY = 7777.25
EINVAL = -1


def _lib():
    from adversarial_learning_on_pointclouds_amd import _lib
    return _lib.load(), _lib.stream_ptr()


class Buf:
    """rows x k values at column `off` of rows of `ld` floats, inside a
    canary-filled allocation with `pad` canaries before and after."""

    def __init__(self, vals, ld, off, pad=64):
        rows, k = vals.shape
        self.rows, self.k, self.ld, self.off, self.pad = rows, k, ld, off, pad
        host = np.full(2 * pad + rows * ld, CANARY, np.float32)
        host[pad:pad + rows * ld].reshape(rows, ld)[:, off:off + k] = vals
        self.host = host
        self.t = torch.from_numpy(host.copy()).to(DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * (self.pad + self.off))

    def read(self):
        """(the values, whether everything around them is untouched)."""
        got = self.t.cpu().numpy()
        inner = got[self.pad:self.pad + self.rows * self.ld].reshape(self.rows, self.ld)
        vals = inner[:, self.off:self.off + self.k].copy()
        mask = np.ones_like(got, bool)
        mask[self.pad:self.pad + self.rows * self.ld].reshape(self.rows, self.ld)[
            :, self.off:self.off + self.k] = False
        return vals, bool(np.array_equal(got[mask], self.host[mask]))


def _layout(strided, k):
    return (960, 320) if strided else (k, 0)


def _data(k, C, Npts, seed):
    rng = np.random.default_rng(seed)
    rows = C * Npts
    x = rng.normal(size=(rows, k)).astype(np.float32)
    x[rng.random(x.shape) < 0.15] = 0.0  # exact zeros: the mask is x > 0, not x >= 0
    assert rows < 8 or ((x == 0).any() and (x < 0).any())
    T = (rng.normal(size=(C, k, k)) / np.sqrt(k)).astype(np.float32)
    dy = rng.normal(size=(rows, k)).astype(np.float32)
    add = rng.normal(size=(rows, k)).astype(np.float32)
    dx0 = rng.normal(size=(rows, k)).astype(np.float32)
    dT0 = rng.normal(size=(C, k, k)).astype(np.float32)
    return x, T, dy, add, dx0, dT0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


SHAPES = [(k, C, Npts) for k in (3, 128) for C in (1, 3) for Npts in (1, 63, 128, 257)]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("k,C,Npts", SHAPES)
def test_xform_fwd(k, C, Npts, strided):
    lib, s = _lib()
    x, T, *_ = _data(k, C, Npts, 1000 * k + 10 * Npts + C)
    ld, off = _layout(strided, k)
    xb = Buf(x, ld, off)
    Tt = _dev(T)
    outs = []
    for _ in range(2):
        yb = Buf(np.full((C * Npts, k), CANARY, np.float32), ld if strided else k, off)
        assert lib.pcadv_cloud_xform_fwd(xb.ptr, ld, _p(Tt), yb.ptr, yb.ld, C, Npts, k, s) == 0
        torch.cuda.synchronize()
        y, clean = yb.read()
        assert clean, "xform_fwd wrote outside y"
        outs.append(y)
    assert np.array_equal(outs[0], outs[1])
    x3 = x.reshape(C, Npts, k).astype(np.float64)
    want = ref.xform_fwd(x3, T).reshape(C * Npts, k)
    bound = k * U * np.matmul(np.abs(x3), np.abs(T.astype(np.float64))).reshape(C * Npts, k)
    err = np.abs(outs[0] - want)
    print(f"max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    assert xb.read()[1]


# (accumulate, add given, relu_x)
COMBOS = [(0, False, 0), (1, True, 1), (0, True, 0), (1, False, 1)]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("k,C,Npts", SHAPES)
def test_xform_bwd(k, C, Npts, strided):
    lib, s = _lib()
    x, T, dy, add, dx0, dT0 = _data(k, C, Npts, 2000 * k + 10 * Npts + C)
    rows = C * Npts
    ld, off = _layout(strided, k)
    xb, dyb = Buf(x, ld, off), Buf(dy, ld, off)
    Tt, addt = _dev(T), _dev(add)
    x3, dy3, T64 = x.reshape(C, Npts, k), dy.reshape(C, Npts, k), T.astype(np.float64)
    for accumulate, with_add, relu in COMBOS:
        dT_ref, ddx = ref.xform_bwd(dy3, x3, T, add if with_add else None, relu)
        outs = []
        for _ in range(2):
            dxb = Buf(dx0, ld, off)
            dTb = Buf(dT0.reshape(C * k, k), k, 0)
            rc = lib.pcadv_cloud_xform_bwd(dyb.ptr, ld, xb.ptr, ld, _p(Tt), dTb.ptr, accumulate,
                                           dxb.ptr, ld, _p(addt) if with_add else None, relu, C,
                                           Npts, k, s)
            assert rc == 0
            torch.cuda.synchronize()
            (dx, c1), (dT, c2) = dxb.read(), dTb.read()
            assert c1 and c2, "xform_bwd wrote outside dx / dT"
            outs.append((dx, dT))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        dx, dT = outs[0]
        # dT: Npts terms (+ the value accumulated into)
        want = dT_ref + (dT0 if accumulate else 0.0)
        mag = np.matmul(np.abs(x3.astype(np.float64)).transpose(0, 2, 1), np.abs(dy3.astype(np.float64)))
        bound = (Npts + accumulate) * U * (mag + (np.abs(dT0) if accumulate else 0.0))
        err = np.abs(dT.reshape(C, k, k) - want)
        print(f"acc={accumulate} add={with_add} relu={relu}: dT err/bound "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}", end="; ")
        assert np.all(err <= bound)
        # dx: k + 2 terms
        want = dx0.astype(np.float64) + ddx.reshape(rows, k)
        mag = np.matmul(np.abs(dy3.astype(np.float64)), np.abs(T64).transpose(0, 2, 1)).reshape(rows, k)
        mag = mag + np.abs(dx0) + (np.abs(add) if with_add else 0.0)
        bound = (k + 2) * U * mag
        err = np.abs(dx - want)
        print(f"dx err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
        if relu:
            dead = ~(x > 0)
            assert np.array_equal(dx[dead], dx0[dead])
            assert rows < 8 or not np.array_equal(dx[~dead], dx0[~dead])
    assert xb.read()[1] and dyb.read()[1]


def test_xform_bwd_nullable_outputs():
    """dT alone (the k = 3 use) and dx alone."""
    lib, s = _lib()
    k, C, Npts = 3, 2, 70
    x, T, dy, add, dx0, dT0 = _data(k, C, Npts, 5)
    xt, dyt, Tt = _dev(x), _dev(dy), _dev(T)
    dTb = Buf(dT0.reshape(C * k, k), k, 0)
    assert lib.pcadv_cloud_xform_bwd(_p(dyt), k, _p(xt), k, _p(Tt), dTb.ptr, 0, None, 0, None, 0, C,
                                     Npts, k, s) == 0
    dxb = Buf(dx0, k, 0)
    assert lib.pcadv_cloud_xform_bwd(_p(dyt), k, _p(xt), k, _p(Tt), None, 0, dxb.ptr, k, None, 0, C,
                                     Npts, k, s) == 0
    torch.cuda.synchronize()
    dT_ref, ddx = ref.xform_bwd(dy.reshape(C, Npts, k), x.reshape(C, Npts, k), T)
    (dT, c1), (dx, c2) = dTb.read(), dxb.read()
    assert c1 and c2
    assert np.max(np.abs(dT.reshape(C, k, k) - dT_ref)) <= 1e-4
    assert np.max(np.abs(dx - dx0 - ddx.reshape(-1, k))) <= 1e-5


def test_bad_arguments_return_einval_without_a_launch():
    from adversarial_learning_on_pointclouds_amd import _lib as L
    lib, s = _lib()
    k, C, Npts = 128, 2, 40
    x, T, dy, add, dx0, dT0 = _data(k, C, Npts, 6)
    xt, dyt, Tt, addt = _dev(x), _dev(dy), _dev(T), _dev(add)
    yb = Buf(np.full((C * Npts, k), CANARY, np.float32), k, 0)
    dxb = Buf(dx0, k, 0)
    dTb = Buf(dT0.reshape(C * k, k), k, 0)
    fwd = lambda **o: lib.pcadv_cloud_xform_fwd(  # noqa: E731
        o.get("x", _p(xt)), o.get("ldx", k), o.get("T", _p(Tt)), o.get("y", yb.ptr), o.get("ldy", k),
        o.get("C", C), o.get("Npts", Npts), o.get("k", k), s)
    bwd = lambda **o: lib.pcadv_cloud_xform_bwd(  # noqa: E731
        _p(dyt), o.get("lddy", k), _p(xt), o.get("ldx", k), o.get("T", _p(Tt)),
        o.get("dT", dTb.ptr), 0, o.get("dx", dxb.ptr), o.get("lddx", k), o.get("add", None), 0,
        o.get("C", C), o.get("Npts", Npts), o.get("k", k), s)
    bad = [fwd(k=64), fwd(k=0), fwd(ldx=k - 1), fwd(ldy=3), fwd(C=-1), fwd(Npts=-5), fwd(x=None),
           fwd(T=None), fwd(y=None), bwd(k=64), bwd(lddy=5), bwd(ldx=5), bwd(lddx=k - 1),
           bwd(dT=None, dx=None), bwd(dx=None, add=_p(addt)), bwd(C=-1), bwd(T=None),
           bwd(T=ctypes.c_void_p(Tt.data_ptr() + 4))]
    assert all(rc == EINVAL for rc in bad), bad
    assert lib.pcadv_last_error()
    # zero rows: a no-op
    assert fwd(C=0) == 0 and fwd(Npts=0) == 0 and bwd(C=0) == 0 and bwd(Npts=0) == 0
    torch.cuda.synchronize()
    for b in (yb, dxb, dTb):
        vals, clean = b.read()
        assert clean and np.array_equal(vals, b.host[b.pad:b.pad + b.rows * b.ld].reshape(b.rows, b.ld))
    assert L.SIGNATURES["pcadv_cloud_xform_fwd"] and L.ABI_VERSION == 11

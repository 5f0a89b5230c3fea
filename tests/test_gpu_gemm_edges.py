"""Edge shapes and dispatch forms of the dense GEMM engine (csrc/gemm.hip)
through its C ABI, against the float64 references of tests/gemm_ref.py on the
case tables of tests/gemm_edge_cases.py (both checked on the CPU by
tests/test_gemm_ref.py).  MI355X only.

Harness (class Op): every operand is a view into a larger allocation.  Input
padding (the columns between width and stride, the rows after the last one, the
floats before the base) holds NaN, so a result that consumed a stray read turns
NaN; output padding holds a sentinel and must come back bit-identical, so a
stray write shows.  Neither leaves the allocation.

Tolerances (none measured).  Three-product GEMMs: 2e-5 (|A| |B|^T) + 1e-6, plus
2e-6 (1 + |base|) when accumulating; six-product GEMMs: a twentieth of that
product bound plus 1e-5 (both as tests/test_gpu_seg.py).  The exact-f32 kernels
(k_gemm_small, the column and slab sums, k_cmx_dw, k_cmx_dx, the re-evaluated
conv + max values): gemm_ref.sum_bound, (n + 8) 2^-23 sum|terms| for a sum of n
terms in any order.  pcadv_row_ce: as test_gpu_seg.test_row_ce_kernel_forms."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gemm_edge_cases as ec
import gemm_ref as ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_learning_on_pointclouds_amd import _lib
    from adversarial_learning_on_pointclouds_amd._lib import check, stream_ptr

DEV = "cuda"
NAN = float("nan")
SENT = 777.0    # f32 output padding
SENT_BF = 3.0   # bf16 output padding (exact in bf16)
SENT_I = -7     # int32 output padding
_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


class Op:
    """A [rows][cols] operand with row stride ld inside a larger allocation:
    8 (+ off) elements before the base, two rows and 8 elements after the last
    row, all holding `fill` like the columns between cols and ld."""

    def __init__(self, rows, cols, ld=None, off=0, data=None, fill=NAN, dtype=torch.float32):
        ld = cols if ld is None else ld
        assert ld >= cols and rows > 0 and cols > 0
        self.shape, self.ld, self.start = (rows, cols), ld, 8 + off
        host = torch.full((self.start + (rows + 2) * ld + 8,), fill, dtype=dtype)
        if data is not None:
            src = torch.from_numpy(np.ascontiguousarray(data)).reshape(rows, cols)
            host.as_strided(self.shape, (ld, 1), self.start).copy_(src.to(dtype))
        self.buf = host.to(DEV)
        self.orig = self.buf.clone()
        assert self.buf.data_ptr() % 16 == 0

    @property
    def p(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.start * self.buf.element_size())

    def view(self, buf=None):
        return (self.buf if buf is None else buf).as_strided(self.shape, (self.ld, 1), self.start)

    def np(self):
        v = self.view()
        return (v.float() if v.dtype == torch.bfloat16 else v).cpu().numpy()

    def bits(self):
        return self.buf.view(_BITS[self.buf.element_size()])

    def padding_intact(self):
        """Everything outside the [rows][cols] view is bit-identical to what it held."""
        t = self.buf.clone()
        self.view(t).copy_(self.view(self.orig))
        return torch.equal(t.view(_BITS[t.element_size()]), self.orig.view(_BITS[t.element_size()]))

    def unchanged(self):
        return torch.equal(self.bits(), self.orig.view(_BITS[self.buf.element_size()]))


def _p(op):
    return None if op is None else op.p


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _ws(nbytes):
    """A workspace holding NaN: a sum that reads a slab nobody wrote turns NaN."""
    t = torch.full((nbytes // 4 + 4,), NAN, device=DEV)
    assert t.data_ptr() % 16 == 0
    return t, ctypes.c_void_p(t.data_ptr())


def _within(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite outputs"
    err = np.abs(got - want)
    bad = err > bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        b = np.broadcast_to(bound, err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside the bound, first at {i}: "
                             f"got {got[i]!r} want {want[i]!r} err {err[i]:.3e} bound {b[i]:.3e}")


def _case_id(c):
    return "ta{ta}tb{tb}-p{precise}a{acc}-v{want}-{M}x{N}x{K}".format(**c)


# ---------------------------------------------------------------------------
# pcadv_gemm: the MFMA kernels (M > 32) and k_gemm_small (M <= 32)
# ---------------------------------------------------------------------------
def _gemm_data(c, seed):
    rng = np.random.default_rng(seed)
    M, N, K = c["M"], c["N"], c["K"]
    d = dict(A=_f32(rng, *((K, M) if c["ta"] else (M, K))), B=_f32(rng, *((K, N) if c["tb"] else (N, K))),
             bias=None if c["bias"] == "none" else _f32(rng, N),
             rows=_f32(rng, (M + c["rpg"] - 1) // c["rpg"], N) if c["rpg"] else None,
             base=_f32(rng, M, N), mask=_f32(rng, M, N) if c["ldm"] else None)
    return d


def _gemm_run(c, d):
    """One pcadv_gemm call on the case's layout; returns the operands (alive)."""
    M, N, K = c["M"], c["N"], c["K"]
    o = dict(a=Op(*d["A"].shape, c["lda"], c["a_off"], d["A"]),
             b=Op(*d["B"].shape, c["ldb"], c["b_off"], d["B"]),
             c=Op(M, N, c["ldc"], c["c_off"], d["base"] if c["acc"] else None, fill=SENT),
             bias=None if d["bias"] is None else Op(1, N, off=int(c["bias"] == "off"), data=d["bias"]),
             rows=None if d["rows"] is None else Op(*d["rows"].shape, data=d["rows"]),
             mask=None if d["mask"] is None else Op(M, N, c["ldm"], c["m_off"], d["mask"]),
             hi=Op(M, N, c["ldcp"], fill=SENT_BF, dtype=torch.bfloat16) if c["ldcp"] else None,
             lo=Op(M, N, c["ldcp"], fill=SENT_BF, dtype=torch.bfloat16) if c["ldcp"] else None)
    check(_lib.load().pcadv_gemm(o["a"].p, c["lda"], c["ta"], o["b"].p, c["ldb"], c["tb"], o["c"].p,
                                 c["ldc"], M, N, K, _p(o["bias"]), _p(o["rows"]), c["rpg"], c["relu"],
                                 c["acc"], _p(o["mask"]), c["ldm"], c["precise"], _p(o["hi"]),
                                 _p(o["lo"]), c["ldcp"], stream_ptr()), "pcadv_gemm")
    torch.cuda.synchronize()
    return o


def _gemm_bound(c, d, exact):
    want, S = ref.gemm_ref(d["A"], d["B"], c["ta"], c["tb"], d["bias"], d["rows"], c["rpg"], c["relu"],
                           c["acc"], d["base"], d["mask"])
    if exact:  # k_gemm_small: K products, the bias terms and the accumulate target in f32
        return want, ref.sum_bound(c["K"] + 3, S)
    P = ref.gemm_ref(d["A"], d["B"], c["ta"], c["tb"])[1]
    bound = 2e-5 * P / 20 + 1e-5 if c["precise"] else 2e-5 * P + 1e-6
    if c["acc"]:
        bound = bound + 2e-6 * (1 + np.abs(d["base"].astype(np.float64)))
    return want, bound


def _gemm_check(c, d, o, exact, what):
    want, bound = _gemm_bound(c, d, exact)
    got = o["c"].np()
    _within(got, want, bound, what)
    if d["mask"] is not None:
        assert (got[d["mask"] <= 0] == 0).all(), what
    assert o["c"].padding_intact(), f"{what}: a store outside C"
    for k in ("a", "b", "bias", "rows", "mask"):
        assert o[k] is None or o[k].unchanged(), f"{what}: input {k} written"
    if o["hi"] is not None:  # the planes are the split of the f32 output, ragged tile included
        C = o["c"].view()
        h = C.to(torch.bfloat16)
        assert torch.equal(o["hi"].view(), h), what
        assert torch.equal(o["lo"].view(), (C - h.float()).to(torch.bfloat16)), what
        assert o["hi"].padding_intact() and o["lo"].padding_intact(), f"{what}: a store outside the planes"


@pytest.mark.parametrize("i", range(len(ec.GEMM_CASES)), ids=[_case_id(c) for c in ec.GEMM_CASES])
def test_gemm_mfma_forms(i):
    c = ec.GEMM_CASES[i]
    d = _gemm_data(c, 100 + i)
    o = _gemm_run(c, d)
    _gemm_check(c, d, o, False, _case_id(c))
    if not c["precise"] and c["K"] < 16:
        # too short a reduction for three products: the dispatch takes the six-product form
        assert torch.equal(o["c"].bits(), _gemm_run(dict(c, precise=1), d)["c"].bits()), _case_id(c)


@pytest.mark.parametrize("tb", [0, 1])
def test_gemm_small_forms(tb):
    """k_gemm_small<TB> on every (M, N, K) of the table: both row blocks, the
    ragged column block, the K % 4 tail of the 16-B loop, with and without
    vectorisable operands, the bias terms, accumulate -> ReLU -> mask."""
    failures = []
    for i, c in enumerate(ec.SMALL_CASES):
        if c["tb"] != tb:
            continue
        d = _gemm_data(c, 5000 + i)
        try:
            _gemm_check(c, d, _gemm_run(c, d), True, _case_id(c))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} cases failed:\n" + "\n".join(failures[:10])


@pytest.mark.parametrize("tb", [0, 1])
def test_gemm_boundary_between_small_and_mfma(tb):
    """M = 32 (k_gemm_small) and M = 33 (the MFMA kernel) on the same data, with
    the whole epilogue: each within its own bound of the same float64 rows."""
    c33 = ec.gemm_case(2, 33, 50, 100, 0, tb, 0, 1, 3, relu=1, bias="al", rpg=5, ldm=53, ldc=52, c_off=0)
    assert ec.gemm_abi_problems(c33) == []
    d33 = _gemm_data(c33, 33 + tb)
    c32 = dict(c33, M=32)
    d32 = {k: (v if v is None or k in ("B", "bias") else v[:32]) for k, v in d33.items()}
    d32["rows"] = d33["rows"]  # [7][N]: rows 0..31 use its first 7 groups either way
    o33, o32 = _gemm_run(c33, d33), _gemm_run(c32, d32)
    _gemm_check(c33, d33, o33, False, "M=33")
    _gemm_check(c32, d32, o32, True, "M=32")
    w33, b33 = _gemm_bound(c33, d33, False)
    _within(o32["c"].np(), o33["c"].np()[:32], b33[:32] + _gemm_bound(c32, d32, True)[1], "M=32 vs M=33")


# ---------------------------------------------------------------------------
# pcadv_gemm_bf2
# ---------------------------------------------------------------------------
def _planes_of(x, ldo):
    """f32 [rows][cols] -> its bf16 hi / lo planes with row stride ldo (pcadv_split_bf2)."""
    rows, cols = x.shape
    src = Op(rows, cols, cols + 4, 0, x)
    hi = Op(rows, cols, ldo, dtype=torch.bfloat16)
    lo = Op(rows, cols, ldo, dtype=torch.bfloat16)
    check(_lib.load().pcadv_split_bf2(src.p, cols + 4, rows, cols, hi.p, lo.p, ldo, stream_ptr()), "split")
    torch.cuda.synchronize()
    assert hi.padding_intact() and lo.padding_intact()
    xt = src.view()
    assert torch.equal(hi.view(), xt.to(torch.bfloat16))
    assert torch.equal(lo.view(), (xt - hi.view().float()).to(torch.bfloat16))
    hi.orig, lo.orig = hi.buf.clone(), lo.buf.clone()  # inputs from here on
    return hi, lo


def _bf2_check(c, seed):
    lib = _lib.load()
    M, N, K = c["M"], c["N"], c["K"]
    cc = dict(c, ta=0, tb=0, precise=0, lda=K, ldb=K, a_off=0, b_off=0)
    d = _gemm_data(cc, seed)
    ah, al = _planes_of(d["A"], c["lda"])
    bh, bl = _planes_of(d["B"], c["ldb"])
    o = _gemm_run(cc, d)  # pcadv_gemm on the f32 matrices, the same epilogue operands and layout
    C = Op(M, N, c["ldc"], 0, d["base"] if c["acc"] else None, fill=SENT)
    hi = Op(M, N, c["ldcp"], fill=SENT_BF, dtype=torch.bfloat16) if c["ldcp"] else None
    lo = Op(M, N, c["ldcp"], fill=SENT_BF, dtype=torch.bfloat16) if c["ldcp"] else None
    check(lib.pcadv_gemm_bf2(ah.p, al.p, c["lda"], bh.p, bl.p, c["ldb"], C.p, c["ldc"], _p(hi), _p(lo),
                             c["ldcp"], M, N, K, _p(o["bias"]), _p(o["rows"]), c["rpg"], c["relu"],
                             c["acc"], _p(o["mask"]), c["ldm"], stream_ptr()), "pcadv_gemm_bf2")
    torch.cuda.synchronize()
    what = f"bf2 {M}x{N}x{K} acc={c['acc']}"
    _gemm_check(cc, d, o, False, what + " (f32 operands)")
    # bitwise pcadv_gemm's result, padding included (same layout, same sentinel)
    assert torch.equal(C.bits(), o["c"].bits()), what
    if hi is not None:
        assert torch.equal(hi.bits(), o["hi"].bits()) and torch.equal(lo.bits(), o["lo"].bits()), what
    for x in (ah, al, bh, bl):
        assert x.unchanged(), what


@pytest.mark.parametrize("i", range(len(ec.BF2_CASES)),
                         ids=["{M}x{N}x{K}-a{acc}".format(**c) for c in ec.BF2_CASES])
def test_gemm_bf2_edges_bitwise(i):
    """K % 32 == 16, N % 4 != 0, plane strides K + 8, ldcp = N + 4, accumulate
    and mask: bitwise pcadv_gemm on the f32 matrices, which is itself held to
    the three-product bound; output planes equal to the split of C."""
    assert ec.bf2_kernel(ec.BF2_CASES[i]) in ("x3", "x3_glds")
    _bf2_check(ec.BF2_CASES[i], 700 + i)


@pytest.mark.parametrize("acc", [0, 1])
def test_gemm_bf2_256_tile_ragged_rows_half_k_tile(acc):
    assert ec.bf2_kernel(ec.BF2_BIG_CASES[acc]) == "big"
    _bf2_check(ec.BF2_BIG_CASES[acc], 799 + acc)


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------
def _wgrad_run(c, d, mode, g=None):
    """pcadv_gemm_wgrad in one call (mode "one": the default finish, "split":
    PCADV_WGRAD_SPLIT_FINISH=1) or as slabs + finish (mode "slabs", with the
    data gradient g = (GemmDesc, its operands) enqueued by the slabs call)."""
    lib = _lib.load()
    rows, O, Kin, rpg = c["rows"], c["O"], c["Kin"], c["rpg"]
    o = dict(dz=Op(rows, O, c["ldz"], c["dz_off"], d["dZ"]), x=Op(rows, Kin, c["ldx"], c["x_off"], d["X"]),
             dw=Op(O, Kin, c["ldo"], 0, d["W0"] if c["acc"] else None, fill=SENT),
             db=Op(1, O, data=d["b0"] if c["acc"] else None, fill=SENT) if c["db"] else None,
             gs=Op(rows // rpg, O, fill=SENT) if c["gs"] else None)
    nb = lib.pcadv_gemm_wgrad_workspace_bytes(rows, O, Kin, rpg)
    assert nb > 0
    o["ws"], wsp = _ws(nb)
    if mode == "slabs":
        desc = _lib.WgradDesc(o["dz"].p, c["ldz"], o["x"].p, c["ldx"], rows, O, Kin, o["dw"].p, c["ldo"],
                              _p(o["db"]), _p(o["gs"]), rpg, c["acc"], wsp, nb)
        check(lib.pcadv_gemm_wgrad_slabs(ctypes.byref(desc), ctypes.byref(g[0]) if g else None,
                                         stream_ptr()), "pcadv_gemm_wgrad_slabs")
        check(lib.pcadv_wgrad_finish(ctypes.byref(desc), 1, stream_ptr()), "pcadv_wgrad_finish")
    else:
        os.environ["PCADV_WGRAD_SPLIT_FINISH"] = "1" if mode == "split" else "0"
        try:
            check(lib.pcadv_gemm_wgrad(o["dz"].p, c["ldz"], o["x"].p, c["ldx"], rows, O, Kin, o["dw"].p,
                                       c["ldo"], _p(o["db"]), _p(o["gs"]), rpg, c["acc"], wsp, nb,
                                       stream_ptr()), "pcadv_gemm_wgrad")
        finally:
            del os.environ["PCADV_WGRAD_SPLIT_FINISH"]
    torch.cuda.synchronize()
    return o


def _wgrad_data(c, seed):
    rng = np.random.default_rng(seed)
    dZ = _f32(rng, c["rows"], c["O"]) * (rng.random((c["rows"], c["O"])) > 0.5)
    return dict(dZ=dZ.astype(np.float32), X=_f32(rng, c["rows"], c["Kin"]), W0=_f32(rng, c["O"], c["Kin"]),
                b0=_f32(rng, c["O"]))


def _wgrad_check(c, d, o, what):
    dW, db, gs = ref.wgrad_ref(d["dZ"], d["X"], c["rpg"])
    a64 = np.abs(d["dZ"].astype(np.float64))
    bound = 1e-6 * (a64.T @ np.abs(d["X"].astype(np.float64))) + 1e-5
    if c["acc"]:
        dW = dW + d["W0"]
        bound = bound + 2e-6 * (1 + np.abs(d["W0"].astype(np.float64)))
    _within(o["dw"].np(), dW, bound, what + " dW")
    assert o["dw"].padding_intact(), what
    if o["db"] is not None:
        S = a64.sum(0) + (np.abs(d["b0"]) if c["acc"] else 0)
        _within(o["db"].np()[0], db + (d["b0"] if c["acc"] else 0), ref.sum_bound(c["rows"] + 1, S), what + " db")
        assert o["db"].padding_intact(), what
    if o["gs"] is not None:
        S = a64.reshape(-1, c["rpg"], c["O"]).sum(1)
        _within(o["gs"].np(), gs, ref.sum_bound(c["rpg"], S), what + " gsum")
        assert o["gs"].padding_intact(), what
    assert o["dz"].unchanged() and o["x"].unchanged(), what


@pytest.mark.parametrize("shape", ec.WGRAD_SHAPES, ids=["x".join(map(str, s)) for s in ec.WGRAD_SHAPES])
def test_gemm_wgrad_edges(shape):
    """Strides above the widths, a base offset on dz / x (the four vector forms
    of the slab GEMM), db / gsum / both NULL, accumulate; the one-launch finish,
    the separate slab sums and the slabs + finish calls bitwise equal."""
    for v, variant in enumerate(ec.WGRAD_VARIANTS):
        c = ec.wgrad_case(shape, variant)
        d = _wgrad_data(c, 31 * shape[0] + shape[2] + v)
        what = f"wgrad {shape} {variant}"
        one = _wgrad_run(c, d, "one")
        _wgrad_check(c, d, one, what)
        for mode in ("split", "slabs"):
            other = _wgrad_run(c, d, mode)
            for k in ("dw", "db", "gs"):
                assert one[k] is None or torch.equal(one[k].bits(), other[k].bits()), (what, mode, k)


@pytest.mark.parametrize("i", range(len(ec.PAIR_CASES)),
                         ids=["{kind}-w{O}x{K}-g{Og}x{Kg}-p{precise}a{acc}".format(**c) for c in ec.PAIR_CASES])
def test_gemm_wgrad_slabs_pair_forms(i):
    """pcadv_gemm_wgrad_slabs with a data gradient: as one launch where both
    forms pair (every combination of the two vector forms, either precision,
    plain and accumulating, masked), and each alone where g is skinny or its b
    cannot be read by vectors: every output bitwise that of its own launch, and
    the data gradient within its bound."""
    c = ec.PAIR_CASES[i]
    lib = _lib.load()
    M, O, K, Og, Kg, rpg = ec.PAIR_M, c["O"], c["K"], c["Og"], c["Kg"], c["rpg"]
    Mg = 20 if c["kind"] == "skinny" else M
    ldb = Kg + 1 if c["kind"] == "oddb" else Kg
    wc = dict(rows=M, rpg=rpg, O=O, Kin=K, ldz=O, ldx=K, ldo=K, dz_off=0, x_off=0, db=1,
              gs=int(rpg > 0), acc=0)
    d = _wgrad_data(wc, 900 + i)
    rng = np.random.default_rng(950 + i)
    shared = (O, K) == (Og, Kg)  # a layer's own pair: g reads the dz that w reads
    A = d["dZ"][:Mg] if shared else _f32(rng, Mg, Og)
    W, Y, c0 = _f32(rng, Og, Kg), _f32(rng, Mg, Kg), _f32(rng, Mg, Kg)
    gc = dict(M=Mg, N=Kg, K=Og, ta=0, tb=1, precise=c["precise"], acc=c["acc"], relu=0, lda=Og, a_off=0,
              ldb=ldb, b_off=0, ldc=Kg, c_off=0, bias="none", rpg=0, ldm=Kg, m_off=0, ldcp=0)
    assert ec.gemm_abi_problems(gc) == []
    gd = dict(A=A, B=W, bias=None, rows=None, base=c0, mask=Y)

    def g_operands(dz):
        o = dict(a=dz if shared else Op(Mg, Og, data=A), b=Op(Og, Kg, ldb, 0, W),
                 c=Op(Mg, Kg, Kg, 0, c0, fill=SENT), mask=Op(Mg, Kg, Kg, 0, Y))
        return o, (o["a"].p, Og, 0, o["b"].p, ldb, 1, o["c"].p, Kg, Mg, Kg, Og, None, None, 0, 0, c["acc"],
                   o["mask"].p, Kg, c["precise"], None, None, 0)

    own = _wgrad_run(wc, d, "one")
    og, args = g_operands(own["dz"])
    check(lib.pcadv_gemm(*args, stream_ptr()), "pcadv_gemm")
    torch.cuda.synchronize()
    _wgrad_check(wc, d, own, "own wgrad")
    want, bound = _gemm_bound(gc, gd, Mg <= 32)
    _within(og["c"].np(), want, bound, "own data gradient")

    # the same two through one pcadv_gemm_wgrad_slabs call
    o = dict(dz=Op(M, O, data=d["dZ"]), x=Op(M, K, data=d["X"]), dw=Op(O, K, fill=SENT),
             db=Op(1, O, fill=SENT), gs=Op(M // rpg, O, fill=SENT) if rpg else None)
    nb = lib.pcadv_gemm_wgrad_workspace_bytes(M, O, K, rpg)
    ws, wsp = _ws(nb)
    pg, args = g_operands(o["dz"])
    desc = _lib.WgradDesc(o["dz"].p, O, o["x"].p, K, M, O, K, o["dw"].p, K, o["db"].p, _p(o["gs"]), rpg,
                          0, wsp, nb)
    gdesc = _lib.GemmDesc(*args)
    check(lib.pcadv_gemm_wgrad_slabs(ctypes.byref(desc), ctypes.byref(gdesc), stream_ptr()), "slabs + g")
    check(lib.pcadv_wgrad_finish(ctypes.byref(desc), 1, stream_ptr()), "finish")
    torch.cuda.synchronize()
    for k in ("dw", "db", "gs"):
        assert o[k] is None or torch.equal(o[k].bits(), own[k].bits()), (k, c)
    assert torch.equal(pg["c"].bits(), og["c"].bits()), c
    assert all(t.unchanged() for t in (o["dz"], o["x"], pg["a"], pg["b"], pg["mask"])), c


@pytest.mark.parametrize("B,O,K0,K1,acc", ec.WSMALL_CASES)
def test_wgrad_small_edges(B, O, K0, K1, acc):
    """pcadv_wgrad_small (exact f32, rows in order): one and two operands, K % 4
    tails, into a wider dw at a column offset."""
    rng = np.random.default_rng(B + O + K0 + K1)
    s, x0, x1 = _f32(rng, B, O), _f32(rng, B, K0), _f32(rng, B, max(K1, 1))
    ldo, w0 = 3 + K0 + K1 + 2, _f32(rng, O, 3 + K0 + K1 + 2)
    ts, t0, t1 = Op(B, O, O + 1, data=s), Op(B, K0, K0 + 2, data=x0), Op(B, max(K1, 1), K1 + 3, data=x1)
    dw = Op(O, ldo, data=w0, fill=SENT)
    at = lambda col: ctypes.c_void_p(dw.p.value + 4 * col)  # noqa: E731
    check(_lib.load().pcadv_wgrad_small(ts.p, O + 1, B, O, t0.p, K0 + 2, K0, at(3), t1.p if K1 else None,
                                        K1 + 3, K1, at(3 + K0) if K1 else None, ldo, acc, stream_ptr()),
          "pcadv_wgrad_small")
    torch.cuda.synchronize()
    want, S = w0.astype(np.float64), np.zeros(w0.shape)
    s64 = s.astype(np.float64)
    for col, x, k in ((3, x0, K0), (3 + K0, x1, K1)):
        want[:, col:col + k] = acc * want[:, col:col + k] + s64.T @ x[:, :k]
        S[:, col:col + k] = acc * np.abs(w0[:, col:col + k]) + np.abs(s64).T @ np.abs(x[:, :k].astype(np.float64))
    _within(dw.np(), want, ref.sum_bound(B + 1, S), "wgrad_small")
    got = dw.np()
    assert np.array_equal(got[:, :3], w0[:, :3]) and np.array_equal(got[:, 3 + K0 + K1:], w0[:, 3 + K0 + K1:])
    assert dw.padding_intact() and ts.unchanged() and t0.unchanged() and t1.unchanged()


# ---------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", ec.COLSUM_M)
def test_colsum_and_group_colsum_edges(M):
    lib = _lib.load()
    for N in ec.COLSUM_N:
        rng = np.random.default_rng(1000 * M + N)
        X, Y, out0 = _f32(rng, M, N), _f32(rng, M, N), _f32(rng, N)
        nb = lib.pcadv_colsum_workspace_bytes(M, N)
        for masked, wide, acc in ((0, 0, 0), (1, 1, 0), (0, 1, 1), (1, 0, 1)):
            what = f"colsum M={M} N={N} masked={masked} wide={wide} acc={acc}"
            ld, ldm = (N + 3, N + 1) if wide else (N, N)
            x, y = Op(M, N, ld, data=X), Op(M, N, ldm, data=Y) if masked else None
            out = Op(1, N, data=out0 if acc else None, fill=SENT)
            ws, wsp = _ws(nb)
            check(lib.pcadv_colsum(x.p, _p(y), ld, ldm, M, N, out.p, acc, wsp, nb, stream_ptr()), what)
            torch.cuda.synchronize()
            Xm = np.where(Y > 0, X, 0) if masked else X
            S = np.abs(Xm.astype(np.float64)).sum(0) + (np.abs(out0) if acc else 0)
            _within(out.np()[0], ref.colsum_ref(X, Y if masked else None) + (out0 if acc else 0),
                    ref.sum_bound(M + 1, S), what)
            assert out.padding_intact() and x.unchanged(), what
        for rpg in ec.GROUP_RPG:
            if M % rpg:
                continue
            for masked in (0, 1):
                what = f"group_colsum M={M} N={N} rpg={rpg} masked={masked}"
                x, y = Op(M, N, N + 3, data=X), Op(M, N, N + 1, data=Y) if masked else None
                out = Op(M // rpg, N, fill=SENT)
                check(lib.pcadv_group_colsum(x.p, _p(y), N + 3, N + 1, M, N, rpg, out.p, stream_ptr()), what)
                torch.cuda.synchronize()
                Xm = np.where(Y > 0, X, 0) if masked else X
                S = np.abs(Xm.astype(np.float64)).reshape(M // rpg, rpg, N).sum(1)
                _within(out.np(), ref.group_colsum_ref(X, rpg, Y if masked else None),
                        ref.sum_bound(rpg, S), what)
                assert out.padding_intact(), what


# ---------------------------------------------------------------------------
# conv + max over the points, f32 form and plane form
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_max_case(shape):
    """Inputs and float64 references of one shape, computed once and shared by
    the forms (never modified): with and without the bias."""
    x, w, b, neg, skip = ec.conv_max_inputs(shape)
    z0 = x.astype(np.float64) @ w.astype(np.float64).T
    thr = 1e-5 * np.abs(z0).max(1)
    absdot = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T  # [C][Npts][O]
    refs = {hb: ref.conv_max_ref(x, w, b if hb else None, 0, skip, z0=z0)[:3] for hb in (0, 1)}
    return x, w, b, neg, skip, thr, absdot, refs


def _conv_max_check(shape, planes):
    lib = _lib.load()
    C, Npts, K, O = shape
    x, w, b, neg, skip, thr, absdot, refs = _conv_max_case(shape)
    ldx = K + 4
    assert ec.conv_max_abi_problems(shape, ldx, 8, K + 8) == []
    xo, wo, bo = Op(C * Npts, K, ldx, data=x.reshape(C * Npts, K)), Op(O, K, data=w), Op(1, O, data=b)
    if planes:
        xh, xl = _planes_of(x.reshape(C * Npts, K), K + 8)
        wh, wl = _planes_of(w, K)
    nb = lib.pcadv_conv_max_x3_workspace_bytes(C, Npts, O)
    ci, oi = np.arange(C)[:, None], np.arange(O)[None, :]

    def run(relu, hb, what):
        gmax, gidx = Op(C, O, fill=SENT), Op(C, O, fill=SENT_I, dtype=torch.int32)
        ws, wsp = _ws(nb)
        if planes:
            check(lib.pcadv_conv_max_bf2(xo.p, ldx, xh.p, xl.p, K + 8, C, Npts, K, wo.p, wh.p, wl.p,
                                         bo.p if hb else None, O, relu, gmax.p, gidx.p, wsp, nb,
                                         stream_ptr()), what)
        else:
            check(lib.pcadv_conv_max_x3(xo.p, ldx, C, Npts, K, wo.p, bo.p if hb else None, O, relu,
                                        gmax.p, gidx.p, wsp, nb, stream_ptr()), what)
        torch.cuda.synchronize()
        return gmax, gidx

    for relu in (0, 1):
        for hb in (1, 0):
            what = f"conv_max {shape} planes={planes} relu={relu} bias={hb}"
            gmax, gidx = run(relu, hb, what)
            assert gmax.padding_intact() and gidx.padding_intact() and xo.unchanged(), what
            gm, gi = gmax.np(), gidx.np()
            val, idx, gap = refs[hb]
            assert ((gi >= 0) & (gi < Npts)).all(), what
            # the pooled value is the f32 dot product at the returned index (+ bias, ReLU)
            z_at = (x.astype(np.float64)[ci, gi] * w.astype(np.float64)[None]).sum(-1) + (b if hb else 0)
            S = absdot[ci, gi, oi] + (np.abs(b) if hb else 0)
            _within(gm, np.maximum(z_at, 0) if relu else z_at, ref.sum_bound(K + 1, S), what + " value")
            # the index: the float64 argmax, or at a near-tie either of the two best
            # (then its value lies within the gap of the maximum)
            near = gap <= thr
            assert near.mean() <= ec.NEAR_TIE_CAP, what
            live = (val > 0) if relu else np.ones(val.shape, bool)  # relu(max) = 0: any index pools 0
            wrong = (gi != idx) & live
            assert not (wrong & ~near).any(), (what, int((wrong & ~near).sum()), np.argwhere(wrong & ~near)[:5])
            assert (val - z_at <= gap + 1e-12)[wrong].all(), what
            for c, p in skip:  # the later twin never wins: equal f32 values, the first index ranks first
                assert (gi[c] != p).all(), what
                assert (gi[c] == ec.conv_max_twin(Npts)[0]).mean() > 0.15, what
            if relu:  # the channel that is negative at every point pools exactly 0
                assert (gm[:, neg] == 0).all(), what
    if planes and ec.conv_max_plane_kernel(shape) == "big":
        # the 256-tile kernel staged through registers (PCADV_GEMM_GLDS=0) instead of by LDS-DMA:
        # the same MFMAs in the same order
        os.environ["PCADV_GEMM_GLDS"] = "0"
        try:
            g2, i2 = run(1, 0, "register staging")
        finally:
            del os.environ["PCADV_GEMM_GLDS"]
        assert torch.equal(g2.bits(), gmax.bits()) and torch.equal(i2.bits(), gidx.bits())


@pytest.mark.parametrize("shape", ec.CONVMAX_SHAPES, ids=["x".join(map(str, s)) for s in ec.CONVMAX_SHAPES])
def test_conv_max_x3_edges(shape):
    _conv_max_check(shape, planes=False)


@pytest.mark.parametrize("shape", ec.CONVMAX_SHAPES, ids=["x".join(map(str, s)) for s in ec.CONVMAX_SHAPES])
def test_conv_max_bf2_edges(shape):
    """The plane-staged form: the 128-tile kernel on ragged clouds
    (gemm_launch_grid<2, 2, 2, 3>) and the 256-tile kernel at its smallest shape."""
    _conv_max_check(shape, planes=True)


# ---------------------------------------------------------------------------
# its backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.CMXBWD_CASES, ids=["x".join(map(str, s)) for s in ec.CMXBWD_CASES])
def test_conv_max_x3_bwd_edges(case):
    """K < 512 (idle lanes), K in (512, 1024] (k_cmx_dw's second column block),
    C > 8 (the second pass over the clouds), O % 32 != 0, ldx / lddx above K,
    every combination of absent outputs; two runs bitwise equal."""
    lib = _lib.load()
    C, Npts, O, K, has_dw, has_db, has_dx = case
    ldx, lddx = K + 4, K + 8
    assert ec.cmx_bwd_abi_problems(case, ldx, lddx) == []
    rng = np.random.default_rng(C + 10 * Npts + O + K)
    x = np.maximum(rng.standard_normal((C, Npts, K)), 0).astype(np.float32)
    w = _f32(rng, O, K)
    gm = (rng.random((C, O)) + 0.1).astype(np.float32)
    gm[rng.random((C, O)) < 0.3] = -1.0   # relu'd away
    # half the channels on a few heavy points (a hit list cut across the waves), half anywhere
    heavy = np.array([3 % Npts, Npts // 2, Npts - 1])
    gi = np.where(rng.random((C, O)) < 0.5, rng.choice(heavy, (C, O)), rng.integers(0, Npts, (C, O))).astype(np.int32)
    dg = _f32(rng, C, O)
    dg[rng.random((C, O)) < 0.1] = 0.0
    base = _f32(rng, C * Npts, K)
    ops = [Op(C, O, data=dg), Op(C, O, data=gm), Op(C, O, data=gi, fill=SENT_I, dtype=torch.int32),
           Op(C * Npts, K, ldx, data=x.reshape(C * Npts, K)), Op(O, K, data=w)]
    tdg, tgm, tgi, tx, tw = ops
    for relu_x in (0, 1):
        what = f"cmx_bwd {case} relu_x={relu_x}"
        runs = []
        for _ in range(2):
            dw = Op(O, K, fill=SENT) if has_dw else None
            db = Op(1, O, fill=SENT) if has_db else None
            dx = Op(C * Npts, K, lddx, data=base, fill=SENT) if has_dx else None
            check(lib.pcadv_conv_max_x3_bwd(tdg.p, tgm.p, tgi.p, tx.p, ldx, C, Npts, O, K, tw.p, _p(dw),
                                            _p(db), _p(dx), lddx, relu_x, stream_ptr()), what)
            torch.cuda.synchronize()
            runs.append((dw, db, dx))
        for a, b in zip(*runs):
            assert a is None or torch.equal(a.bits(), b.bits()), what
        dw, db, dx = runs[0]
        rdw, rdb, rdx, Sdw, Sdx, hits = ref.cmx_bwd_ref(dg, gm, gi, x, w, relu_x, base)
        if dw is not None:
            _within(dw.np(), rdw, ref.sum_bound(C, Sdw), what + " dw")
            assert dw.padding_intact(), what
        if db is not None:
            Sb = np.abs(dg.astype(np.float64) * (gm > 0)).sum(0)
            _within(db.np()[0], rdb, ref.sum_bound(C, Sb), what + " db")
            assert db.padding_intact(), what
        if dx is not None:
            # a point's sum: its hits, the base, and up to 8 partial sums merged across the waves
            _within(dx.np().reshape(C, Npts, K), rdx, ref.sum_bound(hits[:, :, None] + 9, Sdx), what + " dx")
            assert dx.padding_intact(), what
        assert all(o.unchanged() for o in ops), what


# ---------------------------------------------------------------------------
# row cross entropy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["edge", "big"])
@pytest.mark.parametrize("M,C", ec.ROWCE_CASES)
def test_row_ce_kernel_boundaries(M, C, mode):
    """M = 256 / 257 and C = 63 / 64 / 65 (the boundaries of the three kernels)
    with ld = C + 3; labels only 0 and C - 1; logits up to +-80, where a softmax
    without the maximum subtracted overflows."""
    lib = _lib.load()
    lg, y = ec.row_ce_inputs(M, C, mode)
    ld, scale = C + 3, 0.7
    tl, ty = Op(M, C, ld, data=lg), _t(y, torch.int64)
    dl, loss = Op(M, C, ld, fill=SENT), Op(1, 1, fill=SENT)
    nb = lib.pcadv_row_ce_workspace_bytes(M)
    ws, wsp = _ws(nb)
    check(lib.pcadv_row_ce(tl.p, ld, ctypes.c_void_p(ty.data_ptr()), M, C, ctypes.c_float(scale), loss.p,
                           dl.p, wsp, nb, stream_ptr()), "pcadv_row_ce")
    torch.cuda.synchronize()
    what = f"row_ce M={M} C={C} {mode} ({ec.row_ce_kernel(M, C)})"
    ref_loss, ref_g = ref.row_ce_ref(lg, y, scale)
    _within(loss.np(), [[ref_loss]], 1e-5 * max(1.0, abs(ref_loss)), what + " loss")
    _within(dl.np(), ref_g, 1e-6 * max(1.0, np.abs(ref_g).max()), what + " gradient")
    assert dl.padding_intact() and loss.padding_intact() and tl.unchanged(), what

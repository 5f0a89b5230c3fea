"""Every form of the feature forward (k_point_mlp + k_conv4_max,
csrc/feat_fused.hip) at its edge shapes, through the C ABI, on the cases of
tests/feat_fwd_cases.py (checked on the CPU by tests/test_feat_fwd_cases.py).
MI355X only.

Integers: every product, split and partial sum is exact, so x3, gmax and gidx
must equal numpy's bit for bit (max and first argmax, the bias included), in
bf16 mode too.  Random data: float64 references with derived bounds
(feat_fwd_cases.random_stats); the measured margins go to
profiles/feat_fwd_edges.txt, the assertions use the bounds.

Harness (class Pad): every operand and output is a view into a larger
allocation.  What surrounds an input holds NaN, so a stray read turns the
result NaN; what surrounds an output holds a sentinel and must come back
bit-identical, so a stray write shows: the rows after the last cloud of x3
among them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import feat_fwd_cases as fc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_learning_on_pointclouds_amd import _lib
    from adversarial_learning_on_pointclouds_amd._lib import check, stream_ptr

DEV = "cuda"
NAN = float("nan")
SENT = 776.0   # output padding (exact in bf16)
SENT_I = -7
_BITS = {2: torch.int16, 4: torch.int32}
BEFORE, AFTER = 64, 3 * 128 + 8  # elements around the view: 16-B aligned, three x3 rows and more after


class Pad:
    """A flat array of n elements inside a larger allocation filled with `fill`."""

    def __init__(self, n=None, data=None, fill=NAN, dtype=torch.float32):
        if data is not None:
            data = torch.from_numpy(np.ascontiguousarray(data)).reshape(-1)
            n = data.numel()
        self.n = n
        host = torch.full((BEFORE + n + AFTER,), fill, dtype=dtype)
        if data is not None:
            host[BEFORE:BEFORE + n] = data.to(dtype)
        self.buf = host.to(DEV)
        self.orig = self.buf.clone()
        assert (self.buf.data_ptr() + BEFORE * self.buf.element_size()) % 16 == 0

    @property
    def p(self):
        return ctypes.c_void_p(self.buf.data_ptr() + BEFORE * self.buf.element_size())

    def view(self):
        return self.buf[BEFORE:BEFORE + self.n]

    def np(self, *shape):
        v = self.view()
        return (v.float() if v.dtype == torch.bfloat16 else v).cpu().numpy().reshape(shape)

    def bits(self):
        return self.buf.view(_BITS[self.buf.element_size()])

    def unchanged(self):
        return torch.equal(self.bits(), self.orig.view(_BITS[self.buf.element_size()]))

    def padding_intact(self):
        t = self.orig.clone()
        t[BEFORE:BEFORE + self.n] = self.view()
        return torch.equal(t.view(_BITS[t.element_size()]), self.bits())


def _x3_dtype(precision):
    return torch.bfloat16 if precision == 2 else torch.float32


def _conv4(x, W, b, precision, relu=None):
    """pcadv_conv4_max (or pcadv_conv_max_fwd with relu 0 / 1) on padded
    operands; returns gmax, gidx as numpy after checking every padding."""
    C, N, _ = x.shape
    ox = Pad(data=x, dtype=_x3_dtype(precision))
    ow, ob = Pad(data=W), Pad(data=b)
    og, oi = Pad(C * 1024, fill=SENT), Pad(C * 1024, fill=SENT_I, dtype=torch.int32)
    lib = _lib.load()
    if relu is None:
        check(lib.pcadv_conv4_max(ox.p, C, N, ow.p, ob.p, og.p, oi.p, precision, stream_ptr()),
              "pcadv_conv4_max")
    else:
        assert precision == 0
        check(lib.pcadv_conv_max_fwd(ox.p, C, N, 128, ow.p, ob.p, 1024, relu, og.p, oi.p, stream_ptr()),
              "pcadv_conv_max_fwd")
    torch.cuda.synchronize()
    assert og.padding_intact() and oi.padding_intact(), "a store outside gmax / gidx"
    assert ox.unchanged() and ow.unchanged() and ob.unchanged(), "an input was written"
    return og.np(C, 1024), oi.np(C, 1024)


def _report(what, gmax, gidx, want_max, want_idx):
    bad = np.argwhere((gidx != want_idx) | (gmax != want_max))
    print(f"{what}: {len(bad)} of {gidx.size} channels differ")
    return [(int(c), int(o), int(gidx[c, o]), int(want_idx[c, o]), float(gmax[c, o]), float(want_max[c, o]))
            for c, o in bad[:8]]


def _case_id(c):
    return "-".join(str(v) for v in c)


# ---------------------------------------------------------------------------
# integers, exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CONV4_CASES, ids=_case_id)
def test_conv4_max_integers_exact(case):
    """gmax and gidx equal numpy's max and first argmax on every channel with
    no tolerance: a unique winner at point N - 1 and in every wave group's
    units, equal winners in the two lane halves, in one lane's rows, in two
    units of a step, in steps of equal and unequal buffer parity and in units
    of different wave groups (feat_fwd_cases.pattern_positions)."""
    form, C, N, precision = case
    d = fc.unit_integer_case(form, C, N)
    gmax, gidx = _conv4(d["x"], d["W"], d["b"], precision)
    assert np.isfinite(gmax).all()
    bad = _report(_case_id(case), gmax, gidx, d["gmax"], d["gidx"])
    assert not bad, bad


@pytest.mark.parametrize("C,N", fc.RELU_CASES)
def test_conv_max_fwd_relu_exact(C, N):
    """pcadv_conv_max_fwd at K = 128, O = 1024 (the T-Nets' conv3 + max) on the
    plain and the two-group form: without the ReLU numpy's max / first argmax,
    with it (0, point 0) where every value is <= 0 and the rest unchanged."""
    form = fc.conv4_form(C, N, 0)
    d = fc.unit_integer_case(form, C, N)
    assert (d["gmax"] <= 0).sum() > 100
    for relu in (0, 1):
        want = fc.relu_reference(d["gmax"], d["gidx"]) if relu else (d["gmax"], d["gidx"])
        gmax, gidx = _conv4(d["x"], d["W"], d["b"], 0, relu=relu)
        bad = _report(f"{form} C={C} N={N} relu={relu}", gmax, gidx, *want)
        assert not bad, bad


@functools.lru_cache(maxsize=1)
def _mlp_case(C, N):
    """The points and numpy's x3, max and first argmax, shared by both precisions."""
    pts = fc.mlp_points(C, N, 40 + C + N)
    return (pts,) + fc.mlp_reference(pts, fc.mlp_weights())


@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,N", fc.MLP_CASES)
def test_point_mlp_integers_exact(C, N, precision):
    """pcadv_feat_fwd / pcadv_feat_fwd_bf16 on integer points: x3 equals numpy
    bitwise (f32, or bf16) in every cloud, nothing is stored past a cloud's
    ragged tile (the next cloud's rows, or the canary after the last), gmax /
    gidx of the same call equal numpy on that x3, and a second run is bitwise
    the first (the two-tile form defers a tile's stores into the next tile)."""
    w = fc.mlp_weights()
    pts, want_x3, want_max, want_idx = _mlp_case(C, N)
    lib = _lib.load()
    fn = lib.pcadv_feat_fwd_bf16 if precision else lib.pcadv_feat_fwd
    dt = torch.bfloat16 if precision else torch.float32
    ins = [Pad(data=a) for a in (pts, w["w1"], w["b1"], w["w2"], w["b2"], w["w3"], w["b3"], w["w4"], w["b4"])]
    nb = lib.pcadv_feat_fwd_workspace_bytes(C, N)
    ws = torch.full((nb // 4 + 4,), NAN, device=DEV)
    runs = []
    for _ in range(2):
        ox = Pad(C * N * 128, fill=SENT, dtype=dt)
        og, oi = Pad(C * 1024, fill=SENT), Pad(C * 1024, fill=SENT_I, dtype=torch.int32)
        check(fn(ins[0].p, C, N, *[o.p for o in ins[1:]], ox.p, og.p, oi.p,
                 ctypes.c_void_p(ws.data_ptr()), nb, stream_ptr()), "pcadv_feat_fwd")
        torch.cuda.synchronize()
        assert ox.padding_intact(), "a store outside x3"
        assert og.padding_intact() and oi.padding_intact(), "a store outside gmax / gidx"
        runs.append((ox, og, oi))
    assert all(o.unchanged() for o in ins), "an input was written"
    ox, og, oi = runs[0]
    x3 = ox.np(C, N, 128)
    nbad = int((x3 != want_x3).sum())
    print(f"{fc.mlp_form(C, N, precision)['inst']} C={C} N={N}: {nbad} of {x3.size} x3 elements differ")
    assert nbad == 0, np.argwhere(x3 != want_x3)[:8].tolist()
    bad = _report(f"{fc.conv4_form(C, N, 2 if precision else 0)} C={C} N={N}", og.np(C, 1024), oi.np(C, 1024),
                  want_max, want_idx)
    assert not bad, bad
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.bits(), b.bits()), "two runs differ"


# ---------------------------------------------------------------------------
# random data against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.RANDOM_CASES, ids=_case_id)
def test_conv4_max_random_vs_f64(case):
    """Non-integer data: the lo planes, the dropped lo x lo product and the
    exact re-evaluation.  gmax within the derived bound of the float64 value at
    the returned index; the index the float64 first argmax wherever the two
    best float64 values differ by at least twice the screening bound; the
    winner never further below the maximum than that.  The pairs left out stay
    under the 2 % cap (checked from the reference alone on the CPU)."""
    form, C, N, precision = case
    d = fc.random_case(C, N)
    gmax, gidx = _conv4(d["xb"] if precision == 2 else d["x"], d["W"], d["b"], precision)
    assert np.isfinite(gmax).all()
    s = fc.random_stats(d, precision, gmax, gidx)
    print(f"{_case_id(case)}: {100 * s['share']:.3f} % of the pairs too close, smallest gap {s['min_gap']:.3e}; "
          f"measured max |gmax - f64| / sum|x w| = {s['err_rel']:.3e}, "
          f"max (f64 max - f64 at gidx) / sum|x w| = {s['miss_rel']:.3e}")
    assert s["share"] <= fc.GAP_CAP
    assert s["bad_value"] == 0 and s["bad_index"] == 0 and s["bad_miss"] == 0, s


@pytest.mark.parametrize("N,precision", fc.XCD_CASES)
def test_conv4_max_64_and_65_clouds_bitwise(N, precision):
    """The first 64 clouds of a 65-cloud launch (260 workgroups: no XCD remap)
    equal the 64-cloud launch of the same clouds (256: remapped) bit for bit."""
    d = fc.random_case(65, N)
    x = d["xb"] if precision == 2 else d["x"]
    g65, i65 = _conv4(x, d["W"], d["b"], precision)
    g64, i64 = _conv4(x[:64], d["W"], d["b"], precision)
    print(f"{fc.conv4_form(65, N, precision)} N={N}: {(i65[:64] != i64).sum()} gidx, "
          f"{(g65[:64].view(np.int32) != g64.view(np.int32)).sum()} gmax differ")
    assert np.array_equal(i65[:64], i64) and np.array_equal(g65[:64].view(np.int32), g64.view(np.int32))

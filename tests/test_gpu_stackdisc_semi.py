"""pcadv_stackdisc_forward_semi (csrc/pwdisc.hip: k_stk_fwd<true>) on every shape
of stackdisc_cases.SHAPES: every output of pcadv_stackdisc_forward bitwise, and
the semi-supervised term's scan (K, the keep mask, loss_semi) against the f64
restatement semi_seg_ref.semi_ce fed the kernel's own stored d_out.  MI355X
only."""
import functools

import numpy as np
import pytest
import torch

import semi_seg_ref as R
import stackdisc_cases as cases
import stackdisc_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 12345.0
OUTPUTS = ("m", "argc", "d_out", "S", "losses", "dm_d", "dm_adv", "dw5", "db5", "bad")


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


class Runner:
    """One case's device buffers; run(th) is one forward (th None: the plain
    entry point) and returns numpy copies of everything it wrote."""

    def __init__(self, c, shape, lg=None):
        from adversarial_learning_on_pointclouds_amd import discriminator as D
        self.D, self.c, self.shape = D, c, shape
        n0, n1, ncls, ld, maxwg, _ = shape
        M = n0 + n1
        self.buf = torch.full((M, ld), SENTINEL, device=DEV)
        self.buf[:, :ncls] = _t(c["lg"] if lg is None else lg)
        self.ps = [_t(p) for p in c["params"]]
        self.S = c["params"][9].size
        self.ws = D.stackdisc_workspace(M, DEV, maxwg)
        self.soft = dict(soft0=_t(c["soft0"]), soft1=_t(c["soft1"]))
        self.labels = _t(c["labels"], torch.int32)
        self.loss_semi = torch.full((1,), SENTINEL, device=DEV)
        self.kept = torch.full((1,), -7, device=DEV, dtype=torch.int32)
        self.out = None

    def launch(self, th):
        n0, n1, ncls, _, maxwg, ppc = self.shape
        M = n0 + n1
        if self.out is None:
            self.out = dict(
                m=torch.empty(M, device=DEV), d_out=torch.empty(M, device=DEV),
                argc=torch.empty(M, device=DEV, dtype=torch.int32),
                S=torch.empty(M, self.S, device=DEV), losses=torch.empty(5, device=DEV),
                dm_d=torch.empty(M, device=DEV), dm_adv=torch.empty(n1, device=DEV),
                dw5=torch.empty(self.S, 1, 1, device=DEV), db5=torch.empty(self.S, device=DEV),
                bad=torch.empty(1, device=DEV, dtype=torch.int32))
        o = self.out
        semi = {} if th is None else dict(semi_th=th, loss_semi=self.loss_semi, kept=self.kept)
        self.D.stackdisc_forward(
            self.buf, ncls, n0, n1, ref.SOFTMAX, ref.LOG_SOFTMAX, self.ps, o["m"], o["argc"],
            o["d_out"], self.ws, shape_logits=o["S"], losses=o["losses"], shape_label=self.labels,
            pts_per_cloud=ppc, lambda_disc_shape=cases.LAMBDA_SHAPE, dm_d=o["dm_d"],
            dm_adv=o["dm_adv"], grads5=(o["dw5"], o["db5"]), bad_rows=o["bad"],
            max_workgroups=maxwg, **self.soft, **semi)

    def fill(self):
        for t in self.out.values():
            t.fill_(77)
        self.loss_semi.fill_(SENTINEL)
        self.kept.fill_(-7)

    def read(self):
        torch.cuda.synchronize()
        assert int(self.ws[:4].view(torch.int32).item()) == 0  # the ticket is left zero
        k = {n: t.cpu().numpy().copy() for n, t in self.out.items()}
        k["loss_semi"], k["K"] = self.loss_semi.cpu().numpy()[0], int(self.kept.item())
        return k

    def run(self, th):
        self.launch(th)  # allocates on the first call
        self.fill()
        self.launch(th)
        return self.read()


@functools.lru_cache(maxsize=None)
def case(shape):
    """The case's inputs, its runner, the plain forward's outputs and a threshold
    at the median of the no-GT rows' d_out (about half the rows kept)."""
    c = cases.make_inputs(shape, 16)
    r = Runner(c, shape)
    plain = r.run(None)
    n0 = shape[0]
    d1 = plain["d_out"][n0:]
    th = float(np.float32(np.median(d1))) if d1.size else 0.5  # an f32: the kernel's threshold
    return c, r, plain, th


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_same_outputs(k, plain, what=""):
    for n in OUTPUTS:
        assert np.array_equal(_bits(k[n]), _bits(plain[n])), (what, n)


def check_scan(k, lg, n0, th, what=""):
    """K exact and loss_semi within 1e-5 relative of the restatement on the
    kernel's own d_out.  Returns (loss, f64 loss, keep mask)."""
    loss_r, _, lab_r, K_r = R.semi_ce(lg[n0:], k["d_out"][n0:], th)
    keep = lab_r != R.IGNORE
    assert k["K"] == K_r == int(keep.sum()), (what, k["K"], K_r)
    if K_r == 0:
        assert k["loss_semi"] == 0.0
    else:
        e = abs(float(k["loss_semi"]) - loss_r) / loss_r
        print(f"{what}: K {K_r} of {len(keep)}, loss_semi {k['loss_semi']!r} f64 {loss_r!r} rel {e:.2e}")
        assert e <= 1e-5, (what, e)
    return float(k["loss_semi"]), loss_r, keep


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_outputs_bitwise_and_scan(shape):
    """At the median threshold, above every output (K = 0, loss 0) and below
    every output (K = n1)."""
    c, r, plain, th = case(shape)
    n0, n1 = shape[:2]
    k = r.run(th)
    check_same_outputs(k, plain, "median")
    check_scan(k, c["lg"], n0, th, f"{shape}")
    if n1 > 1:
        assert 0 < k["K"] < n1
    k = r.run(2.0)
    check_same_outputs(k, plain, "above")
    assert k["K"] == 0 and k["loss_semi"] == 0.0 and np.float32(k["loss_semi"]).tobytes() == b"\0" * 4
    k = r.run(-1.0)
    check_same_outputs(k, plain, "below")
    assert k["K"] == n1
    check_scan(k, c["lg"], n0, -1.0, f"{shape} all kept")


@pytest.mark.parametrize("shape", [(65, 200, 50, 50, 0, 13), (300, 700, 50, 50, 3, 50)])
def test_threshold_equality_is_ignored(shape):
    """The threshold set to one row's stored d_out: that row is ignored, and the
    next f32 below it as threshold keeps the row."""
    c, r, plain, _ = case(shape)
    n0 = shape[0]
    d1 = plain["d_out"][n0:]
    v = np.sort(d1)[len(d1) // 3]
    k = r.run(float(v))
    assert k["K"] == int((d1 > v).sum()) and (d1 == v).sum() >= 1
    check_scan(k, c["lg"], n0, float(v), "equal")
    k2 = r.run(float(np.nextafter(v, np.float32(-1))))
    assert k2["K"] == k["K"] + int((d1 == v).sum())


def test_nan_row_is_kept():
    """One no-GT row's logit NaN: its d_out is NaN, NaN <= th is False, so the row
    is counted (the restatement's mask on the stored d_out agrees), and its loss,
    NaN, makes loss_semi NaN."""
    shape = (65, 200, 50, 50, 0, 13)
    c, r0, plain, th = case(shape)
    lg = c["lg"].copy()
    lg[65 + 77, 3] = np.nan
    r = Runner(c, shape, lg=lg)
    k = r.run(th)
    assert np.isnan(k["d_out"][65 + 77]) and np.isnan(k["d_out"]).sum() == 1
    keep = ~(k["d_out"][65:] <= th)
    assert keep[77] and k["K"] == int(keep.sum()) and np.isnan(k["loss_semi"])
    # a NaN above every finite threshold too
    k = r.run(2.0)
    assert k["K"] == 1


@pytest.mark.parametrize("shape", [(65, 200, 50, 50, 0, 13), (300, 700, 50, 50, 3, 50)])
def test_two_calls_and_graph_replays_bitwise(shape):
    """Two calls leave the same bits; a captured call replayed twice gives them
    again with no host touch of the workspace in between."""
    c, r, plain, th = case(shape)
    a = r.run(th)
    b = r.run(th)
    for n in OUTPUTS + ("loss_semi",):
        assert np.array_equal(_bits(a[n]), _bits(b[n])), n
    assert a["K"] == b["K"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.launch(th)
    for _ in range(2):
        r.fill()
        graph.replay()
        g = r.read()
        for n in OUTPUTS + ("loss_semi",):
            assert np.array_equal(_bits(a[n]), _bits(g[n])), n
        assert g["K"] == a["K"]


def test_confident_rows_do_not_cancel():
    """Logits x 10: most rows' exp sum beside the maximum is far below f32's
    epsilon, where log(1 + es) in f32 is 0.  loss_semi is within 1e-5 relative
    of f64; the naive f32 form log(sum of all exps) is printed for the record."""
    shape = (65, 200, 50, 50, 0, 13)
    c = cases.make_inputs(shape, 16)
    lg = (10.0 * c["lg"]).astype(np.float32)
    r = Runner(c, shape, lg=lg)
    k = r.run(-1.0)
    loss, loss_r, keep = check_scan(k, lg, 65, -1.0, "x10")
    z = lg[65:] - lg[65:].max(axis=1, keepdims=True)
    naive = float(np.log(np.exp(z).astype(np.float32).sum(axis=1, dtype=np.float32)).mean())
    print(f"naive f32 log(sum): {naive!r}, rel {abs(naive - loss_r) / loss_r:.2e}")


def test_bad_arguments_are_refused():
    from adversarial_learning_on_pointclouds_amd import _lib
    from adversarial_learning_on_pointclouds_amd import discriminator as D
    shape = (65, 200, 50, 50, 0, 13)
    c, r, plain, th = case(shape)
    r.launch(th)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):  # the scan needs the loss terms
        D.stackdisc_forward(r.buf, 50, 65, 200, ref.SOFTMAX, ref.LOG_SOFTMAX, r.ps, r.out["m"],
                            r.out["argc"], r.out["d_out"], None, semi_th=0.5,
                            loss_semi=r.loss_semi, kept=r.kept)
    lib = _lib.load()
    a = D._args(D._STK, r.buf, 50, 65, 200, ref.SOFTMAX, ref.LOG_SOFTMAX, r.ps, r.out["m"],
                r.out["argc"], r.ws, 0)
    a.d_out = r.out["d_out"].data_ptr()
    import ctypes
    sm = _lib.StackdiscSemi(0.5, r.loss_semi.data_ptr(), r.kept.data_ptr())
    # losses NULL
    assert lib.pcadv_stackdisc_forward_semi(ctypes.byref(a), ctypes.byref(sm), _lib.stream_ptr()) != 0
    assert b"losses" in lib.pcadv_last_error()
    assert lib.pcadv_stackdisc_forward_semi(ctypes.byref(a), None, _lib.stream_ptr()) != 0
    a.losses = r.out["losses"].data_ptr()
    sm2 = _lib.StackdiscSemi(0.5, None, r.kept.data_ptr())
    assert lib.pcadv_stackdisc_forward_semi(ctypes.byref(a), ctypes.byref(sm2), _lib.stream_ptr()) != 0
    torch.cuda.synchronize()

"""Float64 numpy restatements of the fused step's head and discriminator tail
(csrc/tail.hip and the fused-launch side of csrc/linear.hip: adv_head_part and
cls_step of csrc/capi.hip), one function per link of the chain, and the
teacher-forced checker tests/test_gpu_head_edges.py holds the kernels to
(checked itself on the CPU by tests/test_head_ref.py).

Every link function takes the link's inputs as stored and returns (value, S):
the float64 result and, per output element, the sum of the absolute values of
the terms the kernel adds.  The rounding bound of a link is

    bound(n, value, S, nmul, transc) = gemm_ref.sum_bound(n, S)
                                       + nmul * 2^-23 |value|
                                       + transc * max(1, |value|)

with n the number of terms really added (K products plus the bias), nmul the
multiplies after the sum (dropout keep, activation slope, lambda / B: one ulp
of the result each) and transc = 1e-6 for a value that goes through expf, logf
or log1pf (the figure tests/test_gpu_pwdisc.py and test_gpu_stackdisc.py use
for the same functions).  sum_bound holds for any summation order, so it covers
both forms of the discriminator conv1 input gradient.  Where a link's input is
not stored (conv5's output a5, the per-row loss gradient g) the reference's own
error of that input is propagated through |W| and folded into S (fold()), so one
formula serves every link.

No torch here."""
import numpy as np

from gemm_ref import EPS, sum_bound

TRANSC = 1e-6          # absolute error of expf / logf / log1pf values, x max(1, |v|)
EITHER_CAP = 0.02      # most z5 units of a case that may need the either-branch rule


def _f64(a):
    return np.asarray(a, np.float64)


def _mat(w):
    w = _f64(w)
    return w.reshape(w.shape[0], -1)


def keep_of(p):
    """The kernels' dropout scale: 1 / (1 - p) in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def bound(n, val, S, nmul=0, transc=0.0):
    v = np.abs(_f64(val))
    return sum_bound(n, S) + nmul * EPS * v + transc * np.maximum(1.0, v)


def fold(S, n, E):
    """S grown so that sum_bound(n, S) also covers a propagated absolute error E."""
    return _f64(S) + _f64(E) / ((n + 8) * EPS)


def slope(a, act):
    """act'(x) from the sign of the stored activation a = act(x)."""
    a = np.asarray(a)
    if act == "relu":
        return (a > 0).astype(np.float64)
    if act == "lrelu":
        return np.where(a > 0, 1.0, 0.2)
    return np.ones(a.shape)


# ---------------------------------------------------------------------------
# links
# ---------------------------------------------------------------------------

def linear_fwd(x, w, b, act=None, scale=None):
    """act(scale * (x w^T + b)); n = K + 1.  ReLU is 1-Lipschitz, so S stands;
    LeakyReLU scales the sum's error by its slope, except where the sum lies
    within its own bound of 0: there the kernel may sit on the other branch,
    |z' - 0.2 z| <= |z' - z| + 0.8 |z| < 1.8 bound."""
    x, w, b = _f64(x), _mat(w), _f64(b)
    z = x @ w.T + b
    S = np.abs(x) @ np.abs(w).T + np.abs(b)
    if scale is not None:
        z = z * _f64(scale)
        S = S * np.abs(_f64(scale))
    if act == "relu":
        return np.maximum(z, 0.0), S
    if act == "lrelu":
        e = sum_bound(x.shape[1] + 1, S)
        return np.where(z > 0, z, 0.2 * z), S * np.where(np.abs(z) <= e, 1.8, np.where(z > 0, 1.0, 0.2))
    return z, S


def bwd_data(dz, w, act=None, a=None, scale=None):
    """(dz w) act'(a) scale, stored as the dz of the layer below; n = dz's width."""
    dz, w = _f64(dz), _mat(w)
    m = slope(a, act) if act else 1.0
    if scale is not None:
        m = m * _f64(scale)
    return (dz @ w) * m, (np.abs(dz) @ np.abs(w)) * np.abs(m)


def wgrad(dz, x):
    """dW = dz^T x, db = the column sums of dz; n = the row count.
    Returns (dW, SW, db, Sb)."""
    dz, x = _f64(dz), _f64(x)
    return dz.T @ x, np.abs(dz).T @ np.abs(x), dz.sum(0), np.abs(dz).sum(0)


def log_softmax(x):
    x = _f64(x)
    s = x - x.max(1, keepdims=True)
    return s - np.log(np.exp(s).sum(1, keepdims=True))


def bce(x, y):
    """BCEWithLogits terms max(x, 0) - x y + log1p(exp(-|x|))."""
    x, y = _f64(x), _f64(y)
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-_f64(x)))


def row_g(x, y, f, B):
    """The per-row loss gradient g = f (sigmoid(x) - y) / B and its bound: a
    cancelling difference, 8 2^-23 f (sigmoid(x) + |y|) / B."""
    s, y = sigmoid(x), _f64(y)
    return f * (s - y) / B, 8 * EPS * f * (s + np.abs(y)) / B


def mean_bound(terms, tb, B):
    """Bound of a f32 mean of B terms whose own bounds are tb."""
    t = np.abs(_f64(terms))
    return (np.sum(tb) + sum_bound(B, t.sum())) / B + 2 * EPS * t.sum() / B


def softmax_grad(logits, onehot_idx, scale):
    """scale (softmax - onehot) and its bound: the softmax at the transcendental
    figure (|softmax| <= 1), two multiplies."""
    p = np.exp(log_softmax(logits))
    p[np.arange(p.shape[0]), onehot_idx] -= 1.0
    v = p * scale
    return v, abs(scale) * TRANSC + 3 * EPS * np.abs(v)


# ---------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------

class Report:
    """Worst error / bound ratio per link; a ratio above 1 is a failure."""

    def __init__(self):
        self.ratio = {}
        self.notes = {}

    def cmp(self, name, got, val, bnd):
        got, val = _f64(got), _f64(val)
        bnd = np.broadcast_to(_f64(bnd), val.shape)
        assert got.shape == val.shape, (name, got.shape, val.shape)
        err = np.abs(got - val)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bnd)
        r = np.where(np.isfinite(got), r, np.inf)
        worst = float(r.max()) if r.size else 0.0
        self.ratio[name] = max(self.ratio.get(name, 0.0), worst)
        return r

    def flag(self, name, ok, note=""):
        self.ratio[name] = max(self.ratio.get(name, 0.0), 0.0 if ok else np.inf)
        if not ok:
            self.notes[name] = note

    def failures(self):
        return {k: v for k, v in self.ratio.items() if not v <= 1.0}

    def lines(self, tag):
        return [f"{tag} {k} {v:.3e}" for k, v in self.ratio.items()]


def _head_fwd_links(rep, A, G, p, C):
    kp = keep_of(p)
    v, S = linear_fwd(A["gmax"][:C], G["fc1.weight"], G["fc1.bias"], "relu")
    rep.cmp("h1", A["h1"][:C], v, bound(1025, v, S))
    v, S = linear_fwd(A["h1"][:C], G["fc2.weight"], G["fc2.bias"], "relu", _f64(A["mask"][:C]) * kp)
    rep.cmp("h2", A["h2"][:C], v, bound(513, v, S, 1))
    v, S = linear_fwd(A["h2"][:C], G["fc3.weight"], G["fc3.bias"])
    rep.cmp("logits", A["logits"][:C], v, bound(257, v, S))


def _head_bwd_links(rep, A, G, gG, p, C):
    """dh2 <- dlogits, dh1, dgmax and the fc1..fc3 gradients over C rows."""
    kp = keep_of(p)
    v, S = bwd_data(A["dlogits"][:C], G["fc3.weight"], "relu", A["h2"][:C], _f64(A["mask"][:C]) * kp)
    rep.cmp("dh2", A["dh2"][:C], v, bound(40, v, S, 1))
    v, S = bwd_data(A["dh2"][:C], G["fc2.weight"], "relu", A["h1"][:C])
    rep.cmp("dh1", A["dh1"][:C], v, bound(256, v, S))
    v, S = bwd_data(A["dh1"][:C], G["fc1.weight"])
    rep.cmp("dgmax", A["dgmax"][:C], v, bound(512, v, S))
    for name, dz, x in (("fc1", A["dh1"], A["gmax"]), ("fc2", A["dh2"], A["h1"]),
                        ("fc3", A["dlogits"], A["h2"])):
        dW, SW, db, Sb = wgrad(dz[:C], x[:C])
        rep.cmp(f"g.{name}.weight", _mat(gG[f"{name}.weight"]), dW, bound(C, dW, SW))
        rep.cmp(f"g.{name}.bias", gG[f"{name}.bias"], db, bound(C, db, Sb))


def check_cls_step(A, G, gG, hp):
    """The cls step's links (C = B rows).  A: the stored arrays by name (gmax =
    the features given, dgmax = feat_dgmax, logits, losses, labels, mask and the
    workspace arrays); G / gG: the generator's parameters / gradients by name."""
    rep = Report()
    B, lam = hp["B"], hp["lambda_cls"]
    _head_fwd_links(rep, A, G, hp["p"], B)
    lg, y = _f64(A["logits"][:B]), np.asarray(A["labels"])
    lsm = log_softmax(lg)
    ce = -lsm[np.arange(B), y]
    v = ce / B
    rep.cmp("rowloss", A["rowloss"][:B], v, (TRANSC * np.maximum(1.0, ce) + 2 * EPS * ce) / B)
    s = _f64(A["rowloss"][:B])
    rep.cmp("losses[0]", A["losses"][:1], [s.sum()], [sum_bound(B, np.abs(s).sum())])
    v, bd = softmax_grad(lg, y, lam / B)
    rep.cmp("dlogits", A["dlogits"][:B], v, bd)
    _head_bwd_links(rep, A, G, gG, hp["p"], B)
    return rep


def a5_of(a4, D):
    """conv5's output from the stored a4: (a5, e5, pre, epre): the value, its
    bound, the pre-activation and the pre-activation's bound."""
    a4, w, b = _f64(a4), _mat(D["conv5.weight"]), _f64(D["conv5.bias"])
    pre = a4 @ w.T + b
    epre = sum_bound(65, np.abs(a4) @ np.abs(w).T + np.abs(b))
    a5 = np.where(pre > 0, pre, 0.2 * pre)
    return a5, epre + EPS * np.abs(a5), pre, epre


def either_branch(a4, D):
    """The units whose conv5 slope the stored a4 does not decide."""
    _, _, pre, epre = a5_of(a4, D)
    return np.abs(pre) <= epre


def check_adv_step(A, G, D, gG, gD, hp, y_known=True):
    """The adversarial step's links (C = 2B generator rows, R = 3B discriminator
    rows).  A: the stored arrays by name (as check_cls_step, plus soft_gt /
    soft_nogt when y_known); hp: B, p, lambda_cls, lambda_adv, semi,
    lambda_semi, semi_th.  y_known = False (device-drawn soft labels) leaves out
    what depends on them: z5, the adversarial rows of dd3 (their conv5 slopes are
    settled on z5), D's fc gradients and losses[2..3]."""
    rep = Report()
    B = hp["B"]
    C, R = 2 * B, 3 * B
    lam_c, lam_a = hp["lambda_cls"], hp["lambda_adv"]
    f32 = np.float32
    _head_fwd_links(rep, A, G, hp["p"], C)
    lg, y = _f64(A["logits"][:C]), np.asarray(A["labels"])
    lsm = log_softmax(lg)
    rep.cmp("din", A["din"][:C], lsm, bound(0, lsm, 0.0, 1, TRANSC))
    for nm in ("din", "d1", "d2", "d3", "dout"):
        rep.flag(f"dup.{nm}", np.array_equal(np.asarray(A[nm][C:R]).view(np.uint32),
                                             np.asarray(A[nm][B:C]).view(np.uint32)),
                 "rows [2B, 3B) differ from rows [B, 2B)")
    v, S = linear_fwd(A["din"][:R], D["conv1.weight"], D["conv1.bias"], "lrelu")
    rep.cmp("d1", A["d1"][:R], v, bound(41, v, S, 1))
    v, S = linear_fwd(A["d1"][:R], D["conv2.weight"], D["conv2.bias"], "lrelu")
    rep.cmp("d2", A["d2"][:R], v, bound(513, v, S, 1))
    v, S = linear_fwd(A["d2"][:R], D["conv3.weight"], D["conv3.bias"], "lrelu")
    rep.cmp("d3", A["d3"][:R], v, bound(257, v, S, 1))
    v, S = linear_fwd(A["d3"][:C], D["conv4.weight"], D["conv4.bias"], "lrelu")
    rep.cmp("a4", A["a4"][:C], v, bound(257, v, S, 1))
    # conv5 + fc in one kernel: a5 is not stored, its bound goes through |wf|
    a5, e5, pre5, epre5 = a5_of(A["a4"][:C], D)
    wf, bf = _mat(D["fc.weight"]), _f64(D["fc.bias"])
    v = a5 @ wf.T + bf
    S = fold(np.abs(a5) @ np.abs(wf).T + np.abs(bf), 65, e5 @ np.abs(wf).T)
    dout = _f64(A["dout"][:R])
    rep.cmp("dout", dout[:C, None], v, bound(65, v, S))

    # ---- losses -------------------------------------------------------------
    ce = -lsm[np.arange(B), y]
    rep.cmp("losses[0]", A["losses"][:1], [ce.mean()],
            [mean_bound(ce, TRANSC * np.maximum(1.0, ce), B)])
    t = bce(dout[C:R], 1.0)
    rep.cmp("losses[1]", A["losses"][1:2], [t.mean()],
            [mean_bound(t, TRANSC * np.maximum(1.0, t) + 3 * EPS * np.abs(dout[C:R]), B)])
    if y_known:
        for k, rows, ys in ((2, slice(0, B), A["soft_gt"]), (3, slice(B, C), A["soft_nogt"])):
            t = bce(dout[rows], ys)
            tb = TRANSC * np.maximum(1.0, t) + 3 * EPS * np.abs(dout[rows])
            rep.cmp(f"losses[{k}]", A["losses"][k:k + 1], [0.5 * t.mean()],
                    [0.5 * mean_bound(t, tb, B) + EPS * 0.5 * t.mean()])
    keep = dout[C:R].astype(f32) > f32(hp["semi_th"])
    kept = int(keep.sum())
    am = lg[B:C].argmax(1)  # first index on equal values, as the kernel's
    if hp.get("semi"):
        t = -lsm[B:C][np.arange(B), am][keep]
        v = t.mean() if kept else 0.0
        rep.cmp("losses[4]", A["losses"][4:5], [v], [TRANSC * max(1.0, abs(v))] if kept else [0.0])
        rep.flag("losses[5]", np.asarray(A["losses"])[5] == f32(kept) / f32(B),
                 f"kept ratio {np.asarray(A['losses'])[5]} != {kept} / {B}")

    # ---- the discriminator's backward ----------------------------------------
    s5 = np.where(pre5 > 0, 1.0, 0.2)
    amb = np.abs(pre5) <= epre5
    if y_known:
        ysoft = np.concatenate([_f64(A["soft_gt"]).reshape(B), _f64(A["soft_nogt"]).reshape(B)])
        g, eg = row_g(dout[:C], ysoft, 0.5, B)
        gw = g[:, None] * wf
        z5 = _f64(A["z5"][:C])

        def z5_link(s):
            v = gw * s
            return v, eg[:, None] * np.abs(wf) * s + bound(1, v, np.abs(v), 1)
        v, bd = z5_link(s5)
        v2, bd2 = z5_link(np.where(pre5 > 0, 0.2, 1.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            swap = amb & (np.abs(z5 - v) / bd > np.abs(z5 - v2) / bd2)
        s5 = np.where(swap, 1.2 - s5, s5)  # 1 <-> 0.2: the branch the kernel took
        v, bd = z5_link(s5)
        rep.cmp("z5", z5, v, bd)
        share = float(amb.mean())
        rep.ratio["either_branch_share/cap"] = share / EITHER_CAP
        dW, SW, db, Sb = wgrad(g[:, None], a5)
        SW = fold(SW, C, eg[:, None].T @ np.abs(a5) + np.abs(g)[:, None].T @ e5)
        rep.cmp("d.fc.weight", _mat(gD["fc.weight"]), dW, bound(C, dW, SW))
        rep.cmp("d.fc.bias", gD["fc.bias"], db, bound(C, db, fold(Sb, C, eg.sum())))
    v, S = bwd_data(A["z5"][:C], D["conv5.weight"], "lrelu", A["a4"][:C])
    rep.cmp("z4", A["z4"][:C], v, bound(64, v, S, 1))
    v, S = bwd_data(A["z4"][:C], D["conv4.weight"], "lrelu", A["d3"][:C])
    rep.cmp("dd3", A["dd3"][:C], v, bound(64, v, S, 1))
    if y_known:
        # adversarial rows: g, z5 and z4 formed here from the stored dout, the
        # twin row's conv5 slopes (as settled above) and its stored a4 signs
        g, eg = row_g(dout[C:R], 1.0, lam_a, B)
        z5r = g[:, None] * wf * s5[B:C]
        e5r = eg[:, None] * np.abs(wf) * s5[B:C] + bound(1, z5r, np.abs(z5r), 1)
        w5, w4 = _mat(D["conv5.weight"]), _mat(D["conv4.weight"])
        s4 = slope(A["a4"][B:C], "lrelu")
        z4r = (z5r @ w5) * s4
        e4r = (e5r @ np.abs(w5)) * s4 + bound(64, z4r, (np.abs(z5r) @ np.abs(w5)) * s4, 1)
        s3 = slope(A["d3"][C:R], "lrelu")
        v = (z4r @ w4) * s3
        S = fold((np.abs(z4r) @ np.abs(w4)) * s3, 64, (e4r @ np.abs(w4)) * s3)
        rep.cmp("dd3.adv", A["dd3"][C:R], v, bound(64, v, S, 1))
    v, S = bwd_data(A["dd3"][:R], D["conv3.weight"], "lrelu", A["d2"][:R])
    rep.cmp("dd2", A["dd2"][:R], v, bound(256, v, S, 1))
    v, S = bwd_data(A["dd2"][:R], D["conv2.weight"], "lrelu", A["d1"][:R])
    rep.cmp("dd1", A["dd1"][:R], v, bound(256, v, S, 1))
    for name, dz, x in (("conv1", A["dd1"], A["din"]), ("conv2", A["dd2"], A["d1"]),
                        ("conv3", A["dd3"], A["d2"]), ("conv4", A["z4"], A["d3"]),
                        ("conv5", A["z5"], A["a4"])):
        dW, SW, db, Sb = wgrad(dz[:C], x[:C])
        rep.cmp(f"d.{name}.weight", _mat(gD[f"{name}.weight"]), dW, bound(C, dW, SW))
        rep.cmp(f"d.{name}.bias", gD[f"{name}.bias"], db, bound(C, db, Sb))

    # ---- dlogits ----------------------------------------------------------------
    v, bd = softmax_grad(lg[:B], y, lam_c / B)
    rep.cmp("dlogits.gt", A["dlogits"][:B], v, bd)
    ddin, S = bwd_data(A["dd1"][C:R], D["conv1.weight"])
    e_dd = bound(512, ddin, S)
    pn = np.exp(_f64(A["din"][B:C]))
    s = ddin.sum(1, keepdims=True)
    e_s = e_dd.sum(1, keepdims=True) + sum_bound(40, np.abs(ddin).sum(1, keepdims=True))
    v = ddin - pn * s
    bd = e_dd + pn * e_s + np.abs(s) * TRANSC * pn + 2 * EPS * (np.abs(ddin) + np.abs(pn * s))
    if hp.get("semi") and kept:
        sc = hp["lambda_semi"] / kept
        t = pn.copy()
        t[np.arange(B), am] -= 1.0
        t = t * sc * keep[:, None]
        v = v + t
        bd = bd + (sc * TRANSC + 3 * EPS * np.abs(t)) * keep[:, None] + EPS * np.abs(v)
    rep.cmp("dlogits.nogt", A["dlogits"][B:C], v, bd)
    _head_bwd_links(rep, A, G, gG, hp["p"], C)
    return rep


# ---------------------------------------------------------------------------
# the links chained end to end (each on the previous link's output)
# ---------------------------------------------------------------------------

def _lrelu(z):
    return np.where(z > 0, z, z * z.dtype.type(0.2))


def chain_adv_fwd(inp, G, D, hp, dt=np.float64):
    """Forward of the adversarial step's head on inp = dict(gmax [2B][1024],
    labels, mask [2B][256], soft_gt, soft_nogt) in dtype dt."""
    c = lambda a: np.asarray(a, dt)  # noqa: E731
    m = lambda w: c(w).reshape(w.shape[0], -1)  # noqa: E731
    B = hp["B"]
    A = dict(gmax=c(inp["gmax"]), mask=c(inp["mask"]), labels=np.asarray(inp["labels"]),
             soft_gt=c(inp["soft_gt"]), soft_nogt=c(inp["soft_nogt"]))
    kp = dt(keep_of(hp["p"]))
    A["h1"] = np.maximum(A["gmax"] @ m(G["fc1.weight"]).T + c(G["fc1.bias"]), 0)
    A["h2"] = np.maximum((A["h1"] @ m(G["fc2.weight"]).T + c(G["fc2.bias"])) * (A["mask"] * kp), 0)
    A["logits"] = A["h2"] @ m(G["fc3.weight"]).T + c(G["fc3.bias"])
    s = A["logits"] - A["logits"].max(1, keepdims=True)
    lsm = s - np.log(np.exp(s).sum(1, keepdims=True))
    A["din"] = np.concatenate([lsm, lsm[B:]])
    x = A["din"]
    for i in range(1, 6):
        x = _lrelu(x @ m(D[f"conv{i}.weight"]).T + c(D[f"conv{i}.bias"]))
        A[f"d{i}" if i < 4 else f"a{i}"] = x
    A["dout"] = (x @ m(D["fc.weight"]).T + c(D["fc.bias"]))[:, 0]
    return A


def chain_adv_bwd(A, G, D, hp, dt=np.float64):
    """Losses, the backward and every gradient on the forward arrays A (as
    chain_adv_fwd's) in dtype dt.  Returns (A completed as the step stores it:
    a4 / z4 / z5 cut to rows [0, 2B), a5 dropped; gG, gD)."""
    c = lambda a: np.asarray(a, dt)  # noqa: E731
    m = lambda w: c(w).reshape(w.shape[0], -1)  # noqa: E731
    B = hp["B"]
    C, R = 2 * B, 3 * B
    A = dict(A)
    y = A["labels"]
    lsm, dout = A["din"][:C], A["dout"]
    ysoft = np.concatenate([c(A["soft_gt"]).reshape(B), c(A["soft_nogt"]).reshape(B), np.ones(B, dt)])
    f = np.concatenate([np.full(C, 0.5, dt), np.full(B, hp["lambda_adv"], dt)])
    t = np.maximum(dout, 0) - dout * ysoft + np.log1p(np.exp(-np.abs(dout)))
    losses = np.zeros(6, dt)
    losses[0] = -lsm[np.arange(B), y].mean()
    losses[1] = t[C:].mean()
    losses[2], losses[3] = dt(0.5) * t[:B].mean(), dt(0.5) * t[B:C].mean()
    g = f * (1 / (1 + np.exp(-dout)) - ysoft) / dt(B)
    sl = lambda a: np.where(a > 0, dt(1), dt(0.2))  # noqa: E731
    z5 = g[:, None] * m(D["fc.weight"]) * sl(A["a5"])
    z4 = (z5 @ m(D["conv5.weight"])) * sl(A["a4"])
    A["dd3"] = (z4 @ m(D["conv4.weight"])) * sl(A["d3"])
    A["dd2"] = (A["dd3"] @ m(D["conv3.weight"])) * sl(A["d2"])
    A["dd1"] = (A["dd2"] @ m(D["conv2.weight"])) * sl(A["d1"])
    gD = {}
    for nm, dz, x in (("conv1", A["dd1"], A["din"]), ("conv2", A["dd2"], A["d1"]),
                      ("conv3", A["dd3"], A["d2"]), ("conv4", z4, A["d3"]), ("conv5", z5, A["a4"]),
                      ("fc", g[:, None], A["a5"])):
        gD[f"{nm}.weight"] = (dz[:C].T @ x[:C]).reshape(np.shape(D[f"{nm}.weight"]))
        gD[f"{nm}.bias"] = dz[:C].sum(0)
    p = np.exp(lsm)
    dl = p[:B].copy()
    dl[np.arange(B), y] -= 1
    dl *= dt(hp["lambda_cls"]) / dt(B)
    ddin = A["dd1"][C:] @ m(D["conv1.weight"])
    dn = ddin - p[B:] * ddin.sum(1, keepdims=True)
    keep = dout[C:].astype(np.float32) > np.float32(hp["semi_th"])
    kept = int(keep.sum())
    if hp.get("semi"):
        am = A["logits"][B:C].argmax(1)
        if kept:
            t = p[B:].copy()
            t[np.arange(B), am] -= 1
            dn = dn + t * keep[:, None] * (dt(hp["lambda_semi"]) / dt(kept))
            losses[4] = -lsm[B:][np.arange(B), am][keep].mean()
        losses[5] = np.float32(kept) / np.float32(B)
    A["dlogits"] = np.concatenate([dl, dn])
    kp = dt(keep_of(hp["p"]))
    A["dh2"] = (A["dlogits"] @ m(G["fc3.weight"])) * (A["h2"] > 0) * (A["mask"] * kp)
    A["dh1"] = (A["dh2"] @ m(G["fc2.weight"])) * (A["h1"] > 0)
    A["dgmax"] = A["dh1"] @ m(G["fc1.weight"])
    gG = {}
    for nm, dz, x in (("fc1", A["dh1"], A["gmax"]), ("fc2", A["dh2"], A["h1"]),
                      ("fc3", A["dlogits"], A["h2"])):
        gG[f"{nm}.weight"], gG[f"{nm}.bias"] = dz.T @ x, dz.sum(0)
    A["losses"] = losses
    A["z5"], A["z4"], A["a4"] = z5[:C], z4[:C], A["a4"][:C]
    del A["a5"]
    return A, gG, gD


def chain_cls(inp, G, hp, dt=np.float64):
    """The cls step's head on inp = dict(gmax [B][1024], labels, mask) in dtype
    dt: (A, gG) as the step stores them."""
    c = lambda a: np.asarray(a, dt)  # noqa: E731
    m = lambda w: c(w).reshape(w.shape[0], -1)  # noqa: E731
    B = hp["B"]
    A = dict(gmax=c(inp["gmax"]), mask=c(inp["mask"]), labels=np.asarray(inp["labels"]))
    y = A["labels"]
    kp = dt(keep_of(hp["p"]))
    A["h1"] = np.maximum(A["gmax"] @ m(G["fc1.weight"]).T + c(G["fc1.bias"]), 0)
    A["h2"] = np.maximum((A["h1"] @ m(G["fc2.weight"]).T + c(G["fc2.bias"])) * (A["mask"] * kp), 0)
    A["logits"] = A["h2"] @ m(G["fc3.weight"]).T + c(G["fc3.bias"])
    s = A["logits"] - A["logits"].max(1, keepdims=True)
    lsm = s - np.log(np.exp(s).sum(1, keepdims=True))
    A["rowloss"] = -lsm[np.arange(B), y] / dt(B)
    A["losses"] = np.asarray([A["rowloss"].sum()], dt)
    dl = np.exp(lsm)
    dl[np.arange(B), y] -= 1
    A["dlogits"] = dl * (dt(hp["lambda_cls"]) / dt(B))
    A["dh2"] = (A["dlogits"] @ m(G["fc3.weight"])) * (A["h2"] > 0) * (A["mask"] * kp)
    A["dh1"] = (A["dh2"] @ m(G["fc2.weight"])) * (A["h1"] > 0)
    A["dgmax"] = A["dh1"] @ m(G["fc1.weight"])
    gG = {}
    for nm, dz, x in (("fc1", A["dh1"], A["gmax"]), ("fc2", A["dh2"], A["h1"]),
                      ("fc3", A["dlogits"], A["h2"])):
        gG[f"{nm}.weight"], gG[f"{nm}.bias"] = dz.T @ x, dz.sum(0)
    return A, gG

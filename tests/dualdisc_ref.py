"""A numpy float64 restatement of the dual discriminator of run_training_seg_dual
(models/discriminator.py:82-137, utils/trainer.py:2236-2286): the three nets,
the four loss terms' D side, their backward and the two SGD steps with the
reference's gradient clearing.  Rows are points (point-major), weights the
reference's [out][in(, 1)].

Max winners are np.argmax's: the first index on ties.  The LeakyReLU slope is
taken from the activation's OUTPUT (0.2 at exactly 0), as the backward of
torch's in-place LeakyReLU does.  A caller comparing a device result can pass
that result's own activations (`slopes`) and winners (`argc` / `gidx`), so a
pre-activation within rounding of 0, or a near-tie, does not route a whole
gradient element differently on the two sides."""
import numpy as np

LEAK = 0.2
TRUNK = ("conv1", "conv2", "conv3")
POINT = ("conv1", "conv2", "conv3")


def lrelu(z):
    return np.where(z > 0, z, LEAK * z)


def slope(y):
    return np.where(y > 0, 1.0, LEAK)


def mat(w):
    return np.asarray(w, np.float64).reshape(w.shape[0], -1)


def softmax(x):
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def log_softmax(x):
    s = x - x.max(1, keepdims=True)
    return s - np.log(np.exp(s).sum(1, keepdims=True))


def mlp_fwd(x, params, names):
    """[x, lrelu(layer 1), ...] of the named 1x1 conv layers."""
    acts = [np.asarray(x, np.float64)]
    for n in names:
        acts.append(lrelu(acts[-1] @ mat(params[n + ".weight"]).T
                          + np.asarray(params[n + ".bias"], np.float64)))
    return acts


def mlp_bwd(dz, acts, params, names, slopes=None, need_dx=False):
    """dz: the gradient of the last layer's pre-activation.  Returns ({name:
    gradient}, dx or None).  slopes: the activations whose signs give the
    LeakyReLU slopes (default: acts)."""
    slopes = acts if slopes is None else slopes
    grads, dx = {}, None
    for i in range(len(names) - 1, -1, -1):
        w = params[names[i] + ".weight"]
        grads[names[i] + ".weight"] = (dz.T @ acts[i]).reshape(w.shape)
        grads[names[i] + ".bias"] = dz.sum(0)
        if i:
            dz = (dz @ mat(w)) * slope(np.asarray(slopes[i], np.float64))
        elif need_dx:
            dx = dz @ mat(w)
    return grads, dx


def bce_logits(z, y):
    return np.mean(np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z))))


def point_terms(x0, n0, S, P, soft0, soft1, lambda_adv=1.0, argc=None, slopes=None):
    """PointDiscNet(BaseDiscNet(x0)) on the n0 GT rows then the no-GT rows, the
    three BCE-with-logits terms and their gradients.  Returns a dict: acts (x0
    and the six activations), out, argc, loss_adv, loss_gt, loss_ng (the halves
    of loss_D_point), dout_d, dout_adv, gS / gP (gradients of loss_D_point) and
    dx0_adv (the gradient of lambda_adv loss_adv at the no-GT rows of x0)."""
    x0 = np.asarray(x0, np.float64)
    R, n1 = x0.shape[0], x0.shape[0] - n0
    at = mlp_fwd(x0, S, TRUNK)
    ap = mlp_fwd(at[-1], P, POINT)
    acts = at + ap[1:]
    y = acts[-1]
    arg = y.argmax(1) if argc is None else np.asarray(argc, np.int64)
    out = y[np.arange(R), arg]
    sg = 1.0 / (1.0 + np.exp(-out))
    r = dict(acts=acts, out=out, argc=arg)
    r["loss_gt"] = 0.5 * bce_logits(out[:n0], soft0) if n0 else 0.0
    r["loss_ng"] = 0.5 * bce_logits(out[n0:], soft1) if n1 else 0.0
    r["loss_adv"] = bce_logits(out[n0:], 1.0) if n1 else 0.0
    dout_d = np.zeros(R)
    if n0:
        dout_d[:n0] = 0.5 * (sg[:n0] - soft0) / n0
    if n1:
        dout_d[n0:] = 0.5 * (sg[n0:] - soft1) / n1
    dout_adv = (sg[n0:] - 1.0) / max(n1, 1)
    r["dout_d"], r["dout_adv"] = dout_d, dout_adv
    sl = acts if slopes is None else slopes
    win = slope(np.asarray(sl[-1], np.float64)[np.arange(R), arg])
    names = [("S", n) for n in TRUNK] + [("P", n) for n in POINT]
    allp = {f"{k}.{n}.{t}": (S if k == "S" else P)[f"{n}.{t}"] for k, n in names
            for t in ("weight", "bias")}
    flat = [f"{k}.{n}" for k, n in names]
    dz = np.zeros_like(y)
    dz[np.arange(R), arg] = dout_d * win
    g, _ = mlp_bwd(dz, acts, allp, flat, slopes=sl)
    r["gS"] = {k[2:]: v for k, v in g.items() if k.startswith("S.")}
    r["gP"] = {k[2:]: v for k, v in g.items() if k.startswith("P.")}
    if n1:
        dz = np.zeros((n1, y.shape[1]))
        dz[np.arange(n1), arg[n0:]] = lambda_adv * dout_adv * win[n0:]
        _, dx = mlp_bwd(dz, [a[n0:] for a in acts], allp, flat,
                        slopes=[np.asarray(a)[n0:] for a in sl], need_dx=True)
        r["dx0_adv"] = dx
    return r


def shape_terms(x0, C, N, S, H, labels, lam, gidx=None, slopes=None, pooled_sign=None):
    """ShapeDiscNet(BaseDiscNet(x0)) on C clouds of N rows and lam x
    CrossEntropyLoss(., labels).  Returns a dict: acts, gmax (the conv's max
    over the points before the LeakyReLU), gidx, logits, loss (unscaled), gS /
    gH (gradients of lam x loss) and dh3 (the gradient at the trunk's last
    pre-activation)."""
    acts = mlp_fwd(x0, S, TRUNK)
    h3 = acts[-1]
    Wc, bc = mat(H["conv.weight"]), np.asarray(H["conv.bias"], np.float64)
    z = (h3 @ Wc.T + bc).reshape(C, N, -1)
    gi = z.argmax(1) if gidx is None else np.asarray(gidx, np.int64)
    gmax = np.take_along_axis(z, gi[:, None, :], 1)[:, 0, :]
    pooled = lrelu(gmax)
    W1, W2 = mat(H["fc1.weight"]), mat(H["fc2.weight"])
    f1 = lrelu(pooled @ W1.T + H["fc1.bias"])
    s = f1 @ W2.T + H["fc2.bias"]
    ls = log_softmax(s)
    loss = -ls[np.arange(C), labels].mean()
    ds = np.exp(ls)
    ds[np.arange(C), labels] -= 1.0
    ds *= lam / C
    gH = {"fc2.weight": ds.T @ f1, "fc2.bias": ds.sum(0)}
    df1 = (ds @ W2) * slope(f1)
    gH["fc1.weight"], gH["fc1.bias"] = df1.T @ pooled, df1.sum(0)
    dg = (df1 @ W1) * slope(pooled if pooled_sign is None else np.asarray(pooled_sign, np.float64))
    dz = np.zeros((C, N, z.shape[2]))
    o = np.arange(z.shape[2])
    for c in range(C):
        dz[c, gi[c], o] = dg[c]
    dz = dz.reshape(C * N, -1)
    gH["conv.weight"] = (dz.T @ h3).reshape(H["conv.weight"].shape)
    gH["conv.bias"] = dz.sum(0)
    sl = acts if slopes is None else slopes
    dh3 = (dz @ Wc) * slope(np.asarray(sl[-1], np.float64))
    gS, _ = mlp_bwd(dh3, acts, S, TRUNK, slopes=sl)
    return dict(acts=acts, gmax=gmax, gidx=gi, pooled=pooled, logits=s, loss=loss, gS=gS, gH=gH,
                dh3=dh3)


def new_state(S, H, P):
    """Float64 copies of the three nets' parameters and the point head's
    never-cleared gradient sum A_P."""
    f = lambda d: {k: np.asarray(v, np.float64).copy() for k, v in d.items()}  # noqa: E731
    st = dict(S=f(S), H=f(H), P=f(P))
    st["A_P"] = {k: np.zeros_like(v) for k, v in st["P"].items()}
    return st


def d_iteration(st, pred_gt, pred_ng, cls_gt, soft_gt, soft_ng, lr_point, lr_shape, lam,
                clear_A_P=False, old_trunk=False, step_trunk_once=False):
    """The D side of one iteration (utils/trainer.py:2236-2286) on predictions
    (B, ncls, N), in place on `st`.  The three flags each undo one quirk of the
    reference (a test's way to show that it would catch the tidied-up loop).
    Returns a dict of the terms and of the gradients as the loop leaves them in
    .grad: trunk g_S^P + g_S^H (conv4: zeros), point head A_P, shape head g_H."""
    B, ncls, N = pred_gt.shape
    rows = lambda p: np.asarray(p, np.float64).transpose(0, 2, 1).reshape(B * N, ncls)  # noqa: E731
    x0 = np.concatenate([softmax(rows(pred_gt)), log_softmax(rows(pred_ng))])
    M = B * N
    pt = point_terms(x0, M, st["S"], st["P"], np.asarray(soft_gt, np.float64).reshape(M),
                     np.asarray(soft_ng, np.float64).reshape(M))
    if clear_A_P:
        st["A_P"] = {k: np.zeros_like(v) for k, v in st["A_P"].items()}
    S_before = {k: v.copy() for k, v in st["S"].items()}
    for k, g in pt["gP"].items():
        st["A_P"][k] = st["A_P"][k] + g
        st["P"][k] = st["P"][k] - lr_point * st["A_P"][k]
    if not step_trunk_once:
        for k, g in pt["gS"].items():
            st["S"][k] = st["S"][k] - lr_point * g
    labels = np.asarray(cls_gt).reshape(B, 16).argmax(1)
    sh = shape_terms(x0[:M], B, N, S_before if old_trunk else st["S"], st["H"], labels, lam)
    gS = {k: pt["gS"][k] + sh["gS"][k] for k in sh["gS"]}
    for k, g in sh["gH"].items():
        st["H"][k] = st["H"][k] - lr_shape * g
    for k, g in gS.items():
        st["S"][k] = st["S"][k] - lr_shape * g
    gS["conv4.weight"] = np.zeros_like(st["S"]["conv4.weight"])
    gS["conv4.bias"] = np.zeros_like(st["S"]["conv4.bias"])
    return dict(point=pt, shape=sh, loss_adv=pt["loss_adv"],
                loss_D_point=pt["loss_gt"] + pt["loss_ng"], loss_D_shape=sh["loss"],
                grads=dict(S=gS, H=sh["gH"], P={k: v.copy() for k, v in st["A_P"].items()}))

"""Shapes, weights and inputs of the dual-discriminator tests (CPU and GPU)."""
import numpy as np

from golden_util import GRAD_TOL_L2, GRAD_TOL_MAX, assert_grad_close

NSHAPES = 16
GAP = 1e-5       # a point whose two best channels are closer is left out of the arg-max check
LEFT_OUT = 0.005  # the share of such points a generated case may have


def dual_specs(input_dim=50, num_shapes=NSHAPES):
    """models/discriminator.py:82-137: the state_dict entries of BaseDiscNet(
    input_pts, input_dim, 256) (its unused conv4 included), ShapeDiscNet(256,
    num_shapes) and PointDiscNet(256, input_pts)."""
    def convs(dims, names):
        s = []
        for n, (o, c) in zip(names, dims):
            s += [(f"{n}.weight", (o, c, 1)), (f"{n}.bias", (o,))]
        return s
    return {
        "S": convs([(64, input_dim), (64, 64), (256, 64), (256, 256)],
                   ["conv1", "conv2", "conv3", "conv4"]),
        "H": convs([(512, 256)], ["conv"]) + [("fc1.weight", (64, 512)), ("fc1.bias", (64,)),
                                              ("fc2.weight", (num_shapes, 64)),
                                              ("fc2.bias", (num_shapes,))],
        "P": convs([(256, 256), (128, 256), (128, 128)], ["conv1", "conv2", "conv3"]),
    }


def g18_params(fx):
    """The three nets' initial weights of fixture g18 (seeded numpy, xavier)."""
    from oracle import pointnet_np as onp
    sp = dual_specs()
    return {k: onp.make_params(sp[k], seed=int(fx[s]), init="xavier")
            for k, s in (("S", "s_seed"), ("H", "h_seed"), ("P", "p_seed"))}


def random_params(seed, input_dim=50, bias=0.05):
    """Weights with the scale of a xavier init and small non-zero biases (a zero
    bias would hide a missing bias term or bias gradient)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, spec in dual_specs(input_dim).items():
        d = {}
        for name, shape in spec:
            if name.endswith("weight"):
                fan_in, fan_out = int(np.prod(shape[1:])), shape[0]
                d[name] = rng.normal(0, np.sqrt(2.0 / (fan_in + fan_out)), shape).astype(np.float32)
            else:
                d[name] = rng.uniform(-bias, bias, shape).astype(np.float32)
        out[k] = d
    return out


POINT_ROWS = [(70, 61), (0, 130), (64, 0), (1, 1)]
POINT_NCLS = [50, 5]


def point_seed(n0, n1, ncls):
    return 100 * n0 + n1 + ncls


def _draw_point_case(seed, n0, n1, ncls, pad):
    rng = np.random.default_rng(seed)
    R = n0 + n1
    logits = np.full((R, ncls + pad), 7777.0, np.float32)
    logits[:, :ncls] = rng.normal(0, 2.0, (R, ncls)).astype(np.float32)
    return dict(logits=logits, soft0=rng.uniform(0.7, 1.05, n0).astype(np.float32),
                soft1=rng.uniform(0.0, 0.305, n1).astype(np.float32),
                params=random_params(seed + 1, ncls))


def point_last_layer(case, n0, ncls):
    """The restatement's last activation (rows x 128) of a point case."""
    import dualdisc_ref as R
    lg = case["logits"][:, :ncls].astype(np.float64)
    x0 = np.concatenate([R.softmax(lg[:n0]), R.log_softmax(lg[n0:])])
    return R.mlp_fwd(R.mlp_fwd(x0, case["params"]["S"], R.TRUNK)[-1], case["params"]["P"],
                     R.POINT)[-1]


def point_case(seed, n0, n1, ncls, pad=3, modify=None):
    """Logits rows (n0 + n1, ncls + pad) with a sentinel in the padding columns,
    soft labels in the reference's ranges, and weights.  Guaranteed: by the
    restatement alone at most LEFT_OUT of the points have their two best
    channels closer than GAP (a draw that has more is redrawn from the next
    seed, so a few-row case never loses a point to the arg-max check).  modify:
    a function applied to the drawn case (e.g. to its weights) before that check."""
    for k in range(64):
        case = _draw_point_case(seed + 7919 * k, n0, n1, ncls, pad)
        if modify is not None:
            modify(case)
        if top2_gap_share(point_last_layer(case, n0, ncls)) <= LEFT_OUT:
            return case
    raise RuntimeError("point_case: no draw without near-ties")


def top2_gap_share(y):
    """The share of rows of y whose two largest entries are closer than GAP."""
    s = np.sort(np.asarray(y, np.float64), axis=1)
    return float(np.mean(s[:, -1] - s[:, -2] < GAP))


def assert_fx_close(fx, prefix, arr, name, tol_max=GRAD_TOL_MAX, tol_l2=GRAD_TOL_L2):
    """assert_grad_close against a fixture entry stored in full, or against its
    summary: the samples within tol_max of the tensor's largest entry, and the
    L2 norm and the largest entry within tol_l2 / tol_max."""
    arr = np.asarray(arr, np.float64)
    if prefix in fx:
        ref = np.asarray(fx[prefix], np.float64)
        if not ref.any():
            assert not arr.any(), f"{name}: expected exact zeros"
            return
        assert_grad_close(arr.reshape(ref.shape), ref, name, tol_max, tol_l2)
        return
    flat = arr.reshape(-1)
    amax, l2 = float(fx[prefix + ".absmax"]), float(fx[prefix + ".l2"])
    if amax == 0.0:
        assert not flat.any(), f"{name}: expected exact zeros"
        return
    e_val = np.abs(flat[fx[prefix + ".idx"]] - fx[prefix + ".val"]).max() / amax
    e_l2 = abs(np.linalg.norm(flat) - l2) / l2
    e_max = abs(np.abs(flat).max() - amax) / amax
    assert e_val <= tol_max and e_max <= tol_max and e_l2 <= tol_l2, \
        f"{name}: samples {e_val:.3e}, absmax {e_max:.3e} (tol {tol_max:g}), l2 {e_l2:.3e} (tol {tol_l2:g})"


def assert_param_close(fx, prefix, p, init, name, tol=1e-5):
    """A parameter against init + the fixture's float64 update (stored in full,
    or at its sample indexes), within tol of the parameter's largest entry."""
    p = np.asarray(p, np.float64).reshape(-1)
    init = np.asarray(init, np.float64).reshape(-1)
    if prefix in fx:
        ref = init + np.asarray(fx[prefix], np.float64).reshape(-1)
    else:
        idx = fx[prefix + ".idx"]
        p, ref = p[idx], init[idx] + fx[prefix + ".val"]
    scale = max(float(np.abs(init).max()), float(np.abs(ref).max()), 1e-30)
    e = float(np.abs(p - ref).max()) / scale
    assert e <= tol, f"{name}: {e:.3e} of the largest entry (tol {tol:g})"

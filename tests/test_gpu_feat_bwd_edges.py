"""The feature backward (k_feat_bwd_chunk / k_feat_bwd_finish, csrc/feat_bwd.hip,
csrc/feat_sort.h) where its branches go: the places the argmax lands.

Kernel level (pcadv_feat_bwd takes gidx as an input, so every hit pattern is
built directly): all inputs are integers or multiples of 1/4, chosen so that
every output's bound sum |a||b| times its granularity stays below 2^24.  Every
partial sum is then an f32 number whatever the order, and the kernel must
EQUAL the float64 reference (tests/feat_bwd_ref.py, pinned against autograd in
test_feat_bwd_ref.py): a dropped, doubled or misplaced hit fails at any
magnitude.  Each case asserts its own exactness bound and that at least half of
dW1, dW2 and dW3 is nonzero before it looks at the GPU.

Step level (the forms only pcadv_adv_step / pcadv_cls_step reach: the hit sort
done ahead of the chunk launch, the bf16 x3, the pts_a / pts_b split, the Adam
workgroups trailing the chunk launch): clouds of duplicated points, whose ties
force heavy rows, and the fused Adam at 1, 2, 3 and 16 chunks per cloud.
"""
import numpy as np
import pytest
import torch

from feat_bwd_ref import NAMES, feat_bwd_ref
from golden_util import assert_adam_update_close, assert_grad_close
from oracle import pointnet_np as onp

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_learning_on_pointclouds_amd import _lib, ops
    from adversarial_learning_on_pointclouds_amd.step import AdvTrainStep
    from test_gpu_parity import _argmax_ok, _cls_step, _feat_weights, _load, _make_step, _t
    import adversarial_learning_on_pointclouds_amd as pc

O = 1024
PCH = 128       # points per chunk workgroup
EXACT = 2.0 ** 24
# multiples of 1/GRAN: the points are quarters, so x1, x2 and the weight
# gradients they enter are; everything built from dg, W2..W4 and x3 is integer
GRAN = dict(dw1=4, db1=1, dw2=4, db2=1, dw3=4, db3=1, dw4=1, db4=1, x1=4, x2=4, dx3=1, dx2=1, dx1=1)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _tern(rng, shape, density, pos=0.5):
    """{-1, 0, 1}: nonzero with probability density, positive with pos among those."""
    nz = rng.random(shape) < density
    return (nz * np.where(rng.random(shape) < pos, 1.0, -1.0)).astype(np.float32)


def make_inputs(C, N, gidx, seed, wd=0.5, gd=1.0):
    """wd: density of W2..W4; gd: share of channels with dg != 0.  The biases
    lean positive and W2 leans positive so that most x1 / x2 are alive even at a
    single active row (the nonzero-share condition)."""
    rng = np.random.default_rng(seed)
    d = dict(
        w1=_tern(rng, (64, 3), 0.75), b1=_tern(rng, (64,), 0.9, 0.9),
        w2=_tern(rng, (64, 64), wd, 0.7), b2=_tern(rng, (64,), 0.6, 0.7),
        w3=_tern(rng, (128, 64), wd), w4=_tern(rng, (O, 128), wd))
    q = rng.integers(1, 5, (C, N, 3)) * rng.choice([-1, 1], (C, N, 3))
    d["pts"] = (q / 4.0).astype(np.float32)
    g = rng.integers(1, 3, (C, O)) * rng.choice([-1, 1], (C, O)) * (rng.random((C, O)) < gd)
    d["dg"] = g.astype(np.float32)
    x3 = rng.integers(1, 4, (C, N, 128)).astype(np.float32)
    u = rng.random((C, N, 128))
    x3[u < 0.2] *= -1.0
    x3[(u >= 0.2) & (u < 0.25)] = 0.0
    x3[(u >= 0.25) & (u < 0.3)] = -0.0
    d["x3"] = x3
    d["gidx"] = np.ascontiguousarray(gidx, np.int32)
    assert d["gidx"].shape == (C, O) and d["gidx"].min() >= 0 and d["gidx"].max() < N
    return d


def _spread(rng, channels, rows):
    """channels -> rows, every row at least once (len(channels) >= len(rows)), shuffled."""
    rows = np.asarray(rows)
    a = np.concatenate([rows, rng.choice(rows, len(channels) - len(rows))])
    return rng.permutation(a)


# ---- hit patterns: each returns (C, N, gidx, tweak or None) ------------------

def _one_row(C, N, row):
    return C, N, np.full((C, O), row), None


def _hull(rng):
    N = 200
    rows = [3, 64, 65, 127, 128, N - 1]
    return 2, N, np.stack([_spread(rng, np.arange(O), rows) for _ in range(2)]), None


def _heavy_then_singles(rng):
    """One row with 924 hits, then 100 rows with one hit each: the group that
    ends the heavy row flushes a row at every step of its unrolled loop."""
    g = np.empty((2, O), np.int64)
    for c, r0 in enumerate((5, 0)):
        perm = rng.permutation(O)
        g[c, perm[:924]] = r0
        g[c, perm[924:]] = r0 + 1 + np.arange(100)
    return 2, 128, g, None


def _active_rows(rng, k):
    """Chunk 0 of a 2-chunk cloud with exactly k active rows, the other
    channels in chunk 1 (k = 0: an empty chunk beside a full one).  k = 128:
    every point of a 1-chunk cloud active, 8 hits per row."""
    if k == 128:
        return 2, 128, np.stack([rng.permutation(np.repeat(np.arange(128), 8)) for _ in range(2)]), None
    g = np.empty((2, O), np.int64)
    for c in range(2):
        perm = rng.permutation(O)
        n0 = 0 if k == 0 else 512
        if k:
            g[c, perm[:n0]] = _spread(rng, perm[:n0], rng.choice(PCH, k, replace=False))
        g[c, perm[n0:]] = _spread(rng, perm[n0:], PCH + rng.choice(PCH, 128 if k == 0 else 40, replace=False))
    return 2, 256, g, None


def _batch_hits(rng, h):
    """Chunk 0 holds h hits in all (one batch: fewer than 12 leaves gather
    groups empty, the others exercise the 8-hit unroll's tail); the other
    channels land in chunk 1.  Cloud 0 spreads them over rows, cloud 1 puts
    them on one row."""
    g = np.empty((2, O), np.int64)
    for c in range(2):
        perm = rng.permutation(O)
        nrows = 1 if c else h // 3 + 1
        g[c, perm[:h]] = _spread(rng, perm[:h], rng.choice(PCH, nrows, replace=False))
        g[c, perm[h:]] = _spread(rng, perm[h:], PCH + rng.choice(72, 50, replace=False))
    return 2, 200, g, None


def _random(rng, C, N):
    return C, N, rng.integers(0, N, (C, O)), None


def _dg_zero_hits(rng):
    """Most hits carry dg == 0, on rows of their own too: those rows are active
    (they take a batch slot) and contribute nothing."""
    C, N, g, _ = _random(rng, 3, 200)

    def tweak(d, rng):
        d["dg"][rng.random((C, O)) < 0.7] = 0.0
        d["dg"][:, g[0] == g[0, 0]] = 0.0
    return C, N, g, tweak


def _dg_zero_cloud(rng):
    C, N, g, _ = _random(rng, 3, 200)

    def tweak(d, rng):
        d["dg"][1] = 0.0
    return C, N, g, tweak


def _x3_dead_rows(rng):
    """Active rows whose x3 is entirely <= 0 (negative, 0.0 and -0.0): nothing
    passes conv3's ReLU there, dW4 still gets the values."""
    C, N, g, _ = _random(rng, 2, 200)

    def tweak(d, rng):
        for c in range(C):
            rows = np.unique(g[c])[::3]
            v = -np.abs(d["x3"][c, rows])
            v[rng.random(v.shape) < 0.3] = 0.0
            d["x3"][c, rows] = v
    return C, N, g, tweak


def _dead_x1(rng, also_x2):
    """Points at the origin under non-positive conv1 biases: x1 is all zero on
    those rows (and with non-positive conv2 biases x2 too)."""
    C, N, g, _ = _random(rng, 2, 200)

    def tweak(d, rng):
        d["b1"] = -np.abs(d["b1"])
        if also_x2:
            d["b2"] = -np.abs(d["b2"])
        for c in range(C):
            d["pts"][c, np.unique(g[c])[::4]] = 0.0
    return C, N, g, tweak


CASES = {
    # name: (builder(rng), seed, wd, gd)
    "heavy_row0": (lambda r: _one_row(2, 128, 0), 1, 0.5, 1.0),
    "heavy_row127": (lambda r: _one_row(2, 128, 127), 2, 0.5, 1.0),
    "heavy_last_n129": (lambda r: _one_row(2, 129, 128), 3, 0.5, 1.0),
    "heavy_last_n200": (lambda r: _one_row(2, 200, 199), 4, 0.5, 1.0),
    "c1_n1": (lambda r: _one_row(1, 1, 0), 5, 0.5, 1.0),
    "hull": (_hull, 6, 0.5, 1.0),
    "heavy_then_singles": (_heavy_then_singles, 7, 0.5, 1.0),
    **{f"active_{k}": ((lambda r, k=k: _active_rows(r, k)), 10 + i, 0.5, 1.0)
       for i, k in enumerate((0, 1, 31, 32, 33, 64, 65, 128))},
    **{f"batch_hits_{h}": ((lambda r, h=h: _batch_hits(r, h)), 20 + i, 0.5, 1.0)
       for i, h in enumerate((1, 5, 11, 12, 13, 16, 17))},
    "dg_zero_hits": (_dg_zero_hits, 30, 0.5, 1.0),
    "dg_zero_cloud": (_dg_zero_cloud, 31, 0.5, 1.0),
    "x3_dead_rows": (_x3_dead_rows, 32, 0.5, 1.0),
    "x1_dead_rows": (lambda r: _dead_x1(r, False), 33, 0.5, 1.0),
    "x1_x2_dead_rows": (lambda r: _dead_x1(r, True), 34, 0.5, 1.0),
    # dw4_block: two waves per channel share the clouds 0/1, 1/1, 1/2, 16/17, 64/65, 65/65
    **{f"clouds_{C}": ((lambda r, C=C: _random(r, C, 16)), 40 + i, wd, gd)
       for i, (C, wd, gd) in enumerate(((1, 0.5, 1.0), (2, 0.5, 1.0), (3, 0.5, 1.0), (33, 0.3, 0.5),
                                        (129, 0.25, 0.25), (130, 0.25, 0.25)))},
    # reduce_slabs_block: 16 waves share nslabs = C * nchunk slabs
    **{f"slabs_{C * -(-N // PCH)}": ((lambda r, C=C, N=N: _random(r, C, N)), 50 + i, wd, gd)
       for i, (C, N, wd, gd) in enumerate(((1, 100, 0.5, 1.0), (7, 64, 0.4, 1.0), (5, 300, 0.5, 1.0),
                                           (8, 200, 0.4, 1.0), (17, 50, 0.35, 0.5),
                                           (65, 130, 0.25, 0.25), (130, 640, 0.25, 0.25),
                                           (43, 2048, 0.25, 0.25)))},
}


def build_case(name):
    builder, seed, wd, gd = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    C, N, gidx, tweak = builder(rng)
    d = make_inputs(C, N, gidx, seed, wd, gd)
    if tweak:
        tweak(d, rng)
    return d


def reference(d):
    return feat_bwd_ref(d["dg"], d["gidx"], d["pts"], d["w1"], d["b1"], d["w2"], d["b2"], d["w3"],
                        d["w4"], d["x3"])


def check_conditions(name, ref, bounds, inner):
    """The inputs make f32 exact in any order, and equality is not vacuous."""
    for k, b in list(bounds.items()) + list(inner.items()):
        worst = float(np.max(b)) * GRAN[k]
        assert worst < EXACT, f"{name}: {k} bound 2^{np.log2(worst):.1f} >= 2^24"
    for k in ("dw1", "dw2", "dw3"):
        share = float(np.count_nonzero(ref[k])) / ref[k].size
        assert share >= 0.5, f"{name}: only {share:.2f} of {k} is nonzero"
    assert np.count_nonzero(ref["dw4"]) > 0


# ---------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------

def _run_feat_bwd(d):
    t = {k: _t(v, torch.int32 if k == "gidx" else torch.float32) for k, v in d.items()}
    out = ops.feat_bwd(t["dg"], t["gidx"], t["pts"], t["w1"], t["b1"], t["w2"], t["b2"], t["w3"],
                       t["w4"], t["x3"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_feat_bwd_exact(name):
    d = build_case(name)
    assert np.signbit(d["x3"][d["x3"] == 0]).any() and not np.signbit(d["x3"][d["x3"] == 0]).all()
    ref, bounds, inner = reference(d)
    check_conditions(name, ref, bounds, inner)
    a = _run_feat_bwd(d)
    b = _run_feat_bwd(d)
    for k, x, y in zip(NAMES, a, b):
        got = x.cpu().numpy().reshape(ref[k].shape).astype(np.float64)
        bad = np.argwhere(got != ref[k])
        assert bad.size == 0, (f"{name}: {k} differs at {len(bad)} of {got.size} entries, first "
                               f"{tuple(bad[0])}: {got[tuple(bad[0])]} != {ref[k][tuple(bad[0])]}")
        assert np.array_equal(got, ref[k])
        assert torch.equal(x, y), f"{name}: {k} differs between two launches"


@pytest.mark.parametrize("what", ["workspace_short", "C0", "N0"])
def test_feat_bwd_rejects(what):
    """Host checks: an error code, nothing launched, nothing written."""
    lib = _lib.load()
    C, N = 2, 100
    d = make_inputs(C, N, np.zeros((C, O)), 0)
    t = {k: _t(v, torch.int32 if k == "gidx" else torch.float32) for k, v in d.items()}
    sizes = (192, 64, 4096, 64, 8192, 128, O * 128, O)
    grads = [torch.full((n,), 7.0, device="cuda") for n in sizes]
    nbytes = lib.pcadv_feat_bwd_workspace_bytes(C, N)
    ws = torch.full((nbytes,), 0x5A, device="cuda", dtype=torch.uint8)
    Cc, Nn, nb = {"workspace_short": (C, N, nbytes - 1), "C0": (0, N, nbytes), "N0": (C, 0, nbytes)}[what]
    torch.cuda.synchronize()
    rc = lib.pcadv_feat_bwd(ops.ptr(t["dg"]), ops.ptr(t["gidx"]), ops.ptr(t["pts"]), Cc, Nn,
                            *[ops.ptr(t[k]) for k in ("w1", "b1", "w2", "b2", "w3", "w4", "x3")],
                            *[ops.ptr(g) for g in grads], ops.ptr(ws), nb, ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(Exception):
        ops.check(rc, "pcadv_feat_bwd")
    for g in grads:
        assert bool((g == 7.0).all())
    assert bool((ws == 0x5A).all())


# ---------------------------------------------------------------------------
# step level: clouds of duplicated points
# ---------------------------------------------------------------------------

def _firsts(pattern, N):
    """The indices at which pattern's distinct points first occur."""
    if pattern == 0:
        return [0]
    if pattern == 1:
        return [0, N - 1] if N > 1 else [0]
    if pattern == 2:
        return sorted({i for i in (0, 3, 64, 65, 127, 128, N - 1) if i < N})
    if pattern == 3:
        return list(range(min(40, N)))
    return list(range(N))


def crafted_clouds(rng, n, N, first=0):
    """Cloud i takes pattern (first + i) % 5: every point is a copy of a distinct
    point that first occurs at or before it, so a tie can only be won at a
    first occurrence (the first index wins)."""
    pts = rng.uniform(-1, 1, (n, N, 3)).astype(np.float32)
    sets = []
    for i in range(n):
        f = np.asarray(_firsts((first + i) % 5, N))
        sets.append(f)
        for j in range(N):
            if j not in f:
                pts[i, j] = pts[i, rng.choice(f[f < j])]
    return pts, sets


def _assert_patterns(gidx, sets, first=0):
    heavy = 0
    for i, f in enumerate(sets):
        extra = np.setdiff1d(gidx[i], f)
        assert extra.size == 0, f"cloud {i}: argmax at {extra[:8]}, not a first occurrence"
        if (first + i) % 5 == 0:
            assert (gidx[i] == 0).all()
            heavy += 1
    assert heavy > 0


def _adv_batch(rng, B, N, crafted=True):
    if crafted:
        pg, s1 = crafted_clouds(rng, B, N)
        pn, s2 = crafted_clouds(rng, B, N, first=B)
        sets = s1 + s2
    else:
        pg = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        pn = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
        sets = None
    lab = rng.integers(0, 40, B)
    m1 = (rng.random((B, 256)) >= 0.3).astype(np.float32)
    m2 = (rng.random((B, 256)) >= 0.3).astype(np.float32)
    y1 = rng.uniform(0.7, 1.05, (B, 1)).astype(np.float32)
    y2 = rng.uniform(0.0, 0.305, (B, 1)).astype(np.float32)
    return (pg, lab, pn, m1, m2, y1, y2), sets


def _call_adv(step, batch, **kw):
    pg, lab, pn, m1, m2, y1, y2 = batch
    return step(_t(pg), _t(lab, torch.int64), _t(pn), masks=(_t(m1), _t(m2)),
                soft=(_t(y1), _t(y2)), **kw)


@pytest.mark.parametrize("B,N", [(4, 200), (32, 128)])
def test_adv_step_crafted_clouds_vs_oracle(B, N):
    """As test_adv_step_large_batch_vs_oracle, on clouds whose ties put whole
    clouds' channels on one or a few rows: (4, 200) is ragged, two chunks per
    cloud and the GT / no-GT split of the points; (32, 128) is 64 clouds of one
    chunk."""
    F32 = np.float32
    step, model, model_D = _make_step(B, N, g_seed=7, d_seed=8)
    batch, sets = _adv_batch(np.random.default_rng(4100 + B), B, N)
    pg, lab, pn, m1, m2, y1, y2 = batch
    G = onp.make_params(onp.cls_spec(40), seed=7)
    D = onp.make_params(onp.disc_spec(40, 1), seed=8, init="xavier")
    _, gidx, x3 = ops.feat_fwd(_t(np.concatenate([pg, pn])), *_feat_weights(G))
    gidx, x3g = gidx.cpu().numpy(), x3.cpu().numpy()
    _assert_patterns(gidx, sets)
    losses_ref, gG, gD, _ = onp.adv_step(G, D, None, None, pg, lab, pn, m1, m2, y1, y2,
                                         apply_adam=False)
    losses = _call_adv(step, batch, apply_adam=False).cpu().numpy()
    for i, k in enumerate(["loss_cls", "loss_adv", "loss_D_gt", "loss_D_nogt"]):
        assert abs(losses[i] - losses_ref[k]) < 1e-4, (k, losses[i], losses_ref[k])
    lg, _, c_gt = onp.cls_forward(G, pg, m1)
    _, dce = onp.cross_entropy(lg, lab)
    ln, _, c_ng = onp.cls_forward(G, pn, m2)
    lsm_ng = onp.log_softmax(ln)
    d_ng, acts_ng = onp.disc_forward(D, lsm_ng)
    _, dadv = onp.bce_with_logits(d_ng, np.ones_like(d_ng))
    _, dlsm = onp.disc_backward(D, acts_ng, F32(0.001) * dadv, need_params=False)
    dlog_ng = onp.log_softmax_bwd(lsm_ng, dlsm)
    W4, b4 = G["feat.conv4.weight"][:, :, 0], G["feat.conv4.bias"]
    _argmax_ok(gidx[:B], c_gt["am"], c_gt["x3"], W4, b4)
    _argmax_ok(gidx[B:], c_ng["am"], c_ng["x3"], W4, b4)
    ga = onp.cls_backward(G, dict(c_gt, x3=x3g[:B], am=gidx[:B]), dce)
    gb = onp.cls_backward(G, dict(c_ng, x3=x3g[B:], am=gidx[B:]), dlog_ng)
    for nm, p in model.named_parameters():
        if nm.startswith("feat."):
            assert_grad_close(p.grad.cpu().numpy(), (ga[nm] + gb[nm]).astype(F32), nm, 1e-4, 1e-5)
        else:
            assert_grad_close(p.grad.cpu().numpy(), gG[nm], nm)
    for nm, p in model_D.named_parameters():
        assert_grad_close(p.grad.cpu().numpy(), gD[nm], nm)


def test_adv_step_bf16_crafted_clouds_vs_oracle():
    """As test_adv_step_bf16_mode_same_activation (every generator gradient
    against the oracle's backward on the step's own bf16 activations, pooled
    features and argmax), at B = 4, N = 200 on the crafted clouds."""
    F32 = np.float32
    B, N = 4, 200
    G = onp.make_params(onp.cls_spec(40), seed=5)
    D = onp.make_params(onp.disc_spec(40, 1), seed=6, init="xavier")
    model = _load(pc.PointNetCls(k=40), onp.make_params(onp.cls_spec(40), seed=5))
    model_D = _load(pc.DeepConvDiscNet(40, 1), D)
    step = AdvTrainStep(model, model_D, B, N, seed=0, precision="bf16")
    batch, sets = _adv_batch(np.random.default_rng(4200), B, N)
    pg, lab, pn, m1, m2, y1, y2 = batch
    _call_adv(step, batch, apply_adam=False)
    x3s = step.saved_x3()
    assert x3s.dtype == torch.bfloat16
    gmax, gidx, x3 = ops.feat_fwd(_t(np.concatenate([pg, pn])), *_feat_weights(G), precision="bf16")
    assert torch.equal(x3, x3s)  # the step's own forward
    gmax, gidx, x3 = gmax.cpu().numpy(), gidx.cpu().numpy().astype(np.int64), x3.float().cpu().numpy()
    _assert_patterns(gidx, sets)
    _, _, c_gt = onp.cls_forward(G, pg, m1, precision="bf16")
    _, _, c_ng = onp.cls_forward(G, pn, m2, precision="bf16")
    lg, hg = onp.head_fwd(gmax[:B], G, m1)
    _, dce = onp.cross_entropy(lg, lab)
    ln, hn = onp.head_fwd(gmax[B:], G, m2)
    lsm_ng = onp.log_softmax(ln)
    d_ng, acts_ng = onp.disc_forward(D, lsm_ng)
    _, dadv = onp.bce_with_logits(d_ng, np.ones_like(d_ng))
    _, dlsm = onp.disc_backward(D, acts_ng, F32(0.001) * dadv, need_params=False)
    dlog_ng = onp.log_softmax_bwd(lsm_ng, dlsm)
    ga = onp.cls_backward(G, dict(c_gt, x3=x3[:B], am=gidx[:B], gmax=gmax[:B], head=hg), dce)
    gb = onp.cls_backward(G, dict(c_ng, x3=x3[B:], am=gidx[B:], gmax=gmax[B:], head=hn), dlog_ng)
    for nm, p in model.named_parameters():
        assert_grad_close(p.grad.cpu().numpy(), (ga[nm] + gb[nm]).astype(F32), nm, 1e-4, 1e-5)


def test_cls_step_crafted_clouds_vs_oracle():
    """As test_cls_step_large_batch_vs_oracle at B = 3, N = 300: 9 chunks, an
    odd count for the sort workgroups that take two chunks each."""
    B, N = 3, 300
    step, model = _cls_step(B, N, g_seed=9)
    rng = np.random.default_rng(4300)
    pts, sets = crafted_clouds(rng, B, N)
    lab = rng.integers(0, 40, B)
    m = (rng.random((B, 256)) >= 0.3).astype(np.float32)
    G = onp.make_params(onp.cls_spec(40), seed=9)
    logits, _, cache = onp.cls_forward(G, pts, m)
    l_ref, dlog = onp.cross_entropy(logits, lab)
    grads = onp.cls_backward(G, cache, dlog)
    _, gidx, x3 = ops.feat_fwd(_t(pts), *_feat_weights(G))
    gidx = gidx.cpu().numpy()
    _assert_patterns(gidx, sets)
    _argmax_ok(gidx, cache["am"], cache["x3"], G["feat.conv4.weight"][:, :, 0], G["feat.conv4.bias"])
    grads_same = onp.cls_backward(G, dict(cache, x3=x3.cpu().numpy(), am=gidx), dlog)
    loss = step(_t(pts), _t(lab, torch.int64), mask=_t(m), apply_adam=False)
    assert abs(float(loss[0]) - l_ref) < 1e-4
    for nm, p in model.named_parameters():
        if nm.startswith("feat."):
            assert_grad_close(p.grad.cpu().numpy(), grads_same[nm], nm, 1e-4, 1e-5)
        else:
            assert_grad_close(p.grad.cpu().numpy(), grads[nm], nm)


# ---------------------------------------------------------------------------
# the fused Adam at other chunk counts
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("N", [40, 200, 300, 2048])
def test_adv_step_fused_adam_chunk_counts(N):
    """The Adam workgroups trailing the chunk launch are indexed
    (y - nclouds) * nchunk + x over ceil((NDW4 + nba0 + nba1) / nchunk) rows:
    1, 2, 3 and 16 chunks here (1024 points, 8 chunks, is the other tests').
    Two steps, so the second runs on nonzero moments at step_count = 2.  Each
    step's update against the oracle's Adam on the step's own gradients, and no
    element left bitwise unchanged (a skipped workgroup leaves a run of them)
    unless its gradient is exactly zero or its exact update is below half an
    f32 spacing of the parameter.  Measured: up to 6 elements of a tensor have
    |g| < 4e-13 << eps at step 1 (5 of conv3.weight's 8192 at N = 40), where
    lr g / (|g| + eps) rounds away, and up to 8 have 0.9 m1 + 0.1 g2 cancel at
    step 2; every one of them is below the half spacing, a skipped workgroup's
    2048 float4 of ~1e-4 updates are not."""
    B = 4
    step, model, model_D = _make_step(B, N, g_seed=11, d_seed=12)
    G = onp.make_params(onp.cls_spec(40), seed=11)
    D = onp.make_params(onp.disc_spec(40, 1), seed=12, init="xavier")
    nets = ((model, G, onp.Adam(G)), (model_D, D, onp.Adam(D)))
    rng = np.random.default_rng(4400 + N)
    for it in range(2):
        batch, _ = _adv_batch(rng, B, N, crafted=False)
        old = [{nm: p.detach().cpu().numpy().copy() for nm, p in m.named_parameters()}
               for m, _, _ in nets]
        _call_adv(step, batch)
        torch.cuda.synchronize()
        assert int(step.step_count[0]) == it + 1
        for (m, P, opt), p_old in zip(nets, old):
            for nm in P:  # the reference steps from the step's own parameters
                P[nm][...] = p_old[nm]
            grads = {nm: p.grad.cpu().numpy().copy() for nm, p in m.named_parameters()}
            assert set(grads) == set(P)
            opt.step(grads)
            for nm, p in m.named_parameters():
                p_new = p.detach().cpu().numpy()
                assert np.isfinite(p_new).all(), nm
                assert_adam_update_close(p_new, p_old[nm], P[nm], p_old[nm], grads[nm],
                                         f"step {it + 1} {nm}")
                # exact (f64) size of this step's update from the oracle's moments:
                # lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
                t = it + 1
                upd = (opt.lr / (1 - opt.b1 ** t)) * np.abs(opt.m[nm].astype(np.float64)) / (
                    np.sqrt(opt.v[nm].astype(np.float64)) / np.sqrt(1 - opt.b2 ** t) + opt.eps)
                rounds_away = upd <= 0.505 * np.spacing(np.abs(p_old[nm])).astype(np.float64)
                same = (p_new.view(np.uint32) == p_old[nm].view(np.uint32)) & (grads[nm] != 0)
                bad = same & ~rounds_away
                if same.any():
                    print(f"step {t} {nm}: {int(same.sum())} unchanged with g != 0, max |g| among "
                          f"them {float(np.abs(grads[nm][same]).max()):.3e}")
                assert not bad.any(), (
                    f"step {t} {nm}: {int(bad.sum())} of {bad.size} elements kept their value, first "
                    f"at flat index {int(np.flatnonzero(bad)[0])}, g {grads[nm][bad][:4]}, "
                    f"update {upd[bad][:4]}")

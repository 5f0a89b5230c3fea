"""The float64 references of tests/gemm_ref.py against hand-computed 2 x 3
cases and torch float64 autograd, and the case tables of
tests/gemm_edge_cases.py against the ABI's stated requirements and the forms
they are meant to reach (a malformed case fails here, on the CPU).  No GPU."""
import numpy as np
import torch

import gemm_edge_cases as ec
import gemm_ref as ref


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------
A23 = np.array([[1.0, -2.0, 3.0], [0.5, 4.0, -1.0]])  # [M = 2][K = 3]
B23 = np.array([[2.0, 1.0, 0.0], [-1.0, 3.0, 2.0]])   # [N = 2][K = 3]


def test_gemm_ref_by_hand():
    # A B^T = [[1*2 - 2*1, -1 - 6 + 6], [1 + 4, -0.5 + 12 - 2]] = [[0, -1], [5, 9.5]]
    C, S = ref.gemm_ref(A23, B23)
    assert np.array_equal(C, [[0.0, -1.0], [5.0, 9.5]])
    assert np.array_equal(S, [[4.0, 13.0], [5.0, 14.5]])
    # the stored-transposed forms give the same product
    assert np.array_equal(ref.gemm_ref(A23, B23.T.copy(), tb=1)[0], C)
    assert np.array_equal(ref.gemm_ref(A23.T.copy(), B23.T.copy(), ta=1, tb=1)[0], C)
    # epilogue order: (sum + bias + bias_rows + base), ReLU, mask
    bias, rows, base = np.array([1.0, -1.0]), np.array([[10.0, 0.0], [-20.0, 1.0]]), np.full((2, 2), 0.5)
    mask = np.array([[1.0, 1.0], [1.0, 0.0]])
    got, S2 = ref.gemm_ref(A23, B23, bias=bias, bias_rows=rows, rpg=1, relu=1, accumulate=1,
                           base=base, cmask=mask)
    # [[0 + 1 + 10 + .5, -1 - 1 + 0 + .5], [5 + 1 - 20 + .5, 9.5 - 1 + 1 + .5]] = [[11.5, -1.5], [-13.5, 10]]
    assert np.array_equal(got, [[11.5, 0.0], [0.0, 0.0]])
    assert np.array_equal(S2, S + [[11.5, 1.5], [21.5, 2.5]])
    # the mask comes after the ReLU: a negative sum under a live mask is 0 either way,
    # a positive sum under a dead mask is 0
    assert ref.gemm_ref(A23, B23, cmask=-mask)[0].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    # rows_per_group = 2: both rows take bias_rows[0]
    assert np.array_equal(ref.gemm_ref(A23, B23, bias_rows=rows, rpg=2)[0], C + rows[0])


def test_gemm_ref_vs_torch():
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((7, 5)), rng.standard_normal((4, 5))
    bias, base, mask = rng.standard_normal(4), rng.standard_normal((7, 4)), rng.standard_normal((7, 4))
    rows = rng.standard_normal((3, 4))
    want = torch.relu(_t(A) @ _t(B).T + _t(bias) + _t(rows)[torch.arange(7) // 3] + _t(base)) * (_t(mask) > 0)
    got, _ = ref.gemm_ref(A.T.copy(), B.T.copy(), 1, 1, bias, rows, 3, 1, 1, base, mask)
    assert np.allclose(got, want.numpy(), rtol=0, atol=1e-14)


def test_wgrad_ref_by_hand_and_autograd():
    dz, x = A23.T.copy(), B23.T.copy()     # rows = 3 points, O = 2, Kin = 2
    dW, db, gs = ref.wgrad_ref(dz, x, rpg=3)
    assert np.array_equal(dW, A23 @ B23.T) and np.array_equal(db, [2.0, 3.5]) and np.array_equal(gs, [[2.0, 3.5]])
    assert ref.wgrad_ref(dz, x)[2] is None
    rng = np.random.default_rng(1)
    X, W, b, G = rng.standard_normal((6, 4)), rng.standard_normal((3, 4)), rng.standard_normal(3), rng.standard_normal((6, 3))
    tw, tb_ = _t(W).requires_grad_(True), _t(b).requires_grad_(True)
    ((_t(X) @ tw.T + tb_) * _t(G)).sum().backward()
    dW, db, gs = ref.wgrad_ref(G, X, rpg=2)
    assert np.allclose(dW, tw.grad.numpy(), atol=1e-14) and np.allclose(db, tb_.grad.numpy(), atol=1e-14)
    assert np.allclose(gs, G.reshape(3, 2, 3).sum(1), atol=1e-14)


def test_colsum_refs_by_hand():
    m = np.array([[1.0, 0.0, -1.0], [1.0, 1.0, 1.0]])
    assert ref.colsum_ref(A23).tolist() == [1.5, 2.0, 2.0]
    assert ref.colsum_ref(A23, m).tolist() == [1.5, 4.0, -1.0]
    assert ref.group_colsum_ref(A23, 1, m).tolist() == [[1.0, 0.0, 0.0], [0.5, 4.0, -1.0]]
    assert ref.group_colsum_ref(A23, 2).tolist() == [[1.5, 2.0, 2.0]]


def test_conv_max_ref_by_hand():
    x = A23.reshape(1, 2, 3)                       # one cloud of two points
    w = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]])
    b = np.array([0.0, 0.0, -2.0])
    # z = [[1, 2, -1], [0.5, -4, -1.5]]
    val, idx, gap, z = ref.conv_max_ref(x, w, b, relu=0)
    assert val.tolist() == [[1.0, 2.0, -1.0]] and idx.tolist() == [[0, 0, 0]]
    assert gap.tolist() == [[0.5, 6.0, 0.5]] and z.shape == (1, 2, 3)
    assert ref.conv_max_ref(x, w, b, relu=1)[0].tolist() == [[1.0, 2.0, 0.0]]
    # twins: the first index wins; leaving the later one out changes nothing but the gap
    xx = np.concatenate([x, x[:, :1]], 1)
    val2, idx2, gap2, _ = ref.conv_max_ref(xx, w, b)
    assert idx2.tolist() == [[0, 0, 0]] and gap2.tolist() == [[0.0, 0.0, 0.0]]
    val3, idx3, gap3, _ = ref.conv_max_ref(xx, w, b, skip=[(0, 2)])
    assert val3.tolist() == val.tolist() and idx3.tolist() == idx.tolist() and gap3.tolist() == gap.tolist()
    assert ref.conv_max_ref(x[:, :1], w, b)[2].tolist() == [[np.inf] * 3]
    assert np.array_equal(ref.near_tie_threshold(x, w), 1e-5 * np.array([[1.0, 4.0, 1.0]]))


def test_cmx_bwd_ref_vs_autograd():
    rng = np.random.default_rng(2)
    C, Npts, K, O = 3, 7, 4, 5
    x = np.maximum(rng.standard_normal((C, Npts, K)), 0)
    w, b, dg = rng.standard_normal((O, K)), rng.standard_normal(O) * 0.1, rng.standard_normal((C, O))
    base = rng.standard_normal((C, Npts, K))
    val, idx, _, _ = ref.conv_max_ref(x, w, b, relu=1)
    tx, tw, tb_ = _t(x).requires_grad_(True), _t(w).requires_grad_(True), _t(b).requires_grad_(True)
    pooled = torch.relu(tx @ tw.T + tb_).max(1)[0]
    assert np.allclose(pooled.detach().numpy(), val, atol=1e-14)
    (pooled * _t(dg)).sum().backward()
    dw, db, dx, Sdw, Sdx, hits = ref.cmx_bwd_ref(dg, val, idx, x, w, 0, base)
    assert np.allclose(dw, tw.grad.numpy(), atol=1e-13) and np.allclose(db, tb_.grad.numpy(), atol=1e-13)
    assert np.allclose(dx - base, tx.grad.numpy(), atol=1e-13)
    assert (Sdw >= np.abs(dw) - 1e-13).all() and (Sdx >= np.abs(dx) - 1e-13).all()
    assert hits.sum() == ((val > 0) & (dg != 0)).sum()
    # relu_x masks the additions (not the base) by [x > 0]
    dxm = ref.cmx_bwd_ref(dg, val, idx, x, w, 1, base)[2]
    assert np.allclose(dxm - base, tx.grad.numpy() * (x > 0), atol=1e-13)
    # by hand: one cloud, two points, the 2 x 3 matrix as x; both channels pick point 1
    dw, db, dx, _, _, hits = ref.cmx_bwd_ref(np.array([[2.0, -1.0]]), np.array([[1.0, 3.0]]),
                                             np.array([[1, 1]]), A23.reshape(1, 2, 3), B23)
    assert dw.tolist() == [[1.0, 8.0, -2.0], [-0.5, -4.0, 1.0]] and db.tolist() == [2.0, -1.0]
    assert dx.tolist() == [[[0.0, 0.0, 0.0], [5.0, -1.0, -2.0]]] and hits.tolist() == [[0, 2]]
    # gmax <= 0 kills a channel
    assert ref.cmx_bwd_ref(np.array([[2.0, -1.0]]), np.array([[0.0, 3.0]]), np.array([[1, 1]]),
                           A23.reshape(1, 2, 3), B23)[1].tolist() == [0.0, -1.0]


def test_row_ce_ref_by_hand_and_autograd():
    # two rows of three equal logits: CE = log 3, gradient (1/3 - onehot) * scale / 2
    loss, g = ref.row_ce_ref(np.zeros((2, 3)), np.array([0, 2]), scale=2.0)
    assert abs(loss - np.log(3.0)) < 1e-15
    assert np.allclose(g, [[1 / 3 - 1, 1 / 3, 1 / 3], [1 / 3, 1 / 3, 1 / 3 - 1]], atol=1e-15)
    rng = np.random.default_rng(3)
    lg, y = rng.uniform(-80, 80, (9, 6)), rng.integers(0, 6, 9)
    t = _t(lg).requires_grad_(True)
    tl = torch.nn.functional.cross_entropy(t, torch.from_numpy(y))
    tl.backward()
    loss, g = ref.row_ce_ref(lg, y, scale=0.7)
    assert abs(loss - tl.item()) < 1e-12 and np.allclose(g, 0.7 * t.grad.numpy(), atol=1e-15)
    assert np.isfinite(g).all()


def test_sum_bound_holds_for_f32_sums():
    rng = np.random.default_rng(4)
    for n in (1, 3, 100, 5000):
        t = rng.standard_normal(n).astype(np.float32)
        exact = t.astype(np.float64).sum()
        fwd = np.float32(0)
        for v in t:
            fwd = np.float32(fwd + v)
        for got in (fwd, t.sum(dtype=np.float32), np.sort(t).sum(dtype=np.float32)):
            assert abs(float(got) - exact) <= ref.sum_bound(n, np.abs(t).sum())


# ---------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------
def test_gemm_cases_are_well_formed_and_cover_the_forms():
    for c in ec.GEMM_CASES:
        assert ec.gemm_abi_problems(c) == [], c
        assert c["M"] > 32 and ec.gemm_vec_flags(c) == c["want"], c
    for ta, tb in ec.LAYOUTS:
        cs = [c for c in ec.GEMM_CASES if (c["ta"], c["tb"]) == (ta, tb)]
        assert {(c["precise"], c["acc"], ec.gemm_vec_flags(c)) for c in cs} >= {
            (p, a, f) for p in (0, 1) for a in (0, 1) for f in range(4)}
        # ... and every kernel behind them: three and six products
        assert {(ec.gemm_products(c), c["acc"], ec.gemm_vec_flags(c)) for c in cs} == {
            (n, a, f) for n in (3, 6) for a in (0, 1) for f in range(4)}
        assert {c["K"] for c in cs if not c["precise"] and c["K"] < 16} == {1, 3}
        assert {c["M"] for c in cs} >= set(ec.GEMM_M) and {c["N"] for c in cs} >= set(ec.GEMM_N)
        assert {c["K"] for c in cs} >= set(ec.GEMM_K)
        # every tile here is ragged (no M is a multiple of 128); the extras, once per layout
        assert any(c["bias"] == "off" for c in cs)
        assert {1, 50} <= {c["rpg"] for c in cs}
        assert any(c["ldm"] % 2 == 1 for c in cs)
        assert all(any(c["ldcp"] > c["N"] and c["acc"] == a for c in cs) for a in (0, 1))
        # an unaligned bias under an aligned C (cvec = 0 from the bias alone)
        assert any(c["bias"] == "off" and c["ldc"] % 4 == 0 and c["c_off"] == 0 for c in cs)
    assert 36 <= len(ec.GEMM_CASES) <= 64


def test_small_cases_are_well_formed_and_cover_the_forms():
    for c in ec.SMALL_CASES:
        assert ec.gemm_abi_problems(c) == [] and c["M"] <= 32 and c["ta"] == 0 and not c["ldcp"], c
    for tb in (0, 1):
        cs = [c for c in ec.SMALL_CASES if c["tb"] == tb]
        assert {(c["M"], c["N"], c["K"]) for c in cs} == {
            (m, n, k) for m in ec.SMALL_M for n in ec.SMALL_N for k in ec.SMALL_K}
        assert any(c["acc"] and c["relu"] and c["ldm"] and c["rpg"] for c in cs)
        assert any(c["acc"] and c["relu"] and c["ldm"] and c["bias"] != "none" for c in cs)
    # tb = 0: every shape with operands that allow the 16-B loop and without
    v = [c for c in ec.SMALL_CASES if c["tb"] == 0]
    for want in (True, False):
        assert {(c["M"], c["N"], c["K"]) for c in v
                if (c["lda"] % 4 == 0 and c["a_off"] == 0 and c["ldb"] % 4 == 0 and c["b_off"] == 0) == want} \
            == {(m, n, k) for m in ec.SMALL_M for n in ec.SMALL_N for k in ec.SMALL_K}


def test_bf2_cases_are_well_formed_and_cover_the_kernels():
    for c in ec.BF2_CASES + ec.BF2_BIG_CASES:
        assert ec.bf2_abi_problems(c) == [], c
        assert c["lda"] == c["K"] + 8 and c["ldb"] == c["K"] + 8
        assert c["ldcp"] == (c["N"] + 4 if c["N"] % 4 == 0 else 0)
    assert {ec.bf2_kernel(c) for c in ec.BF2_CASES} == {"x3", "x3_glds"}
    assert [ec.bf2_kernel(c) for c in ec.BF2_BIG_CASES] == ["big", "big"]
    assert {c["K"] % 32 for c in ec.BF2_CASES} == {0, 16} and any(c["N"] % 4 for c in ec.BF2_CASES)


def test_wgrad_and_pair_cases_are_well_formed_and_cover_the_forms():
    for c in ec.WGRAD_CASES:
        assert ec.wgrad_abi_problems(c) == [], c
        assert c["ldz"] > c["O"] and c["ldx"] > c["Kin"] and c["ldo"] > c["Kin"]
    assert {ec.wgrad_vec_flags(c) for c in ec.WGRAD_CASES} == {0, 1, 2, 3}
    assert {(c["db"], c["gs"]) for c in ec.WGRAD_CASES if c["rpg"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["rows"] // c["rpg"] > ec.WF_MAXG for c in ec.WGRAD_CASES if c["rpg"])
    assert any(c["O"] * c["Kin"] % 4 for c in ec.WGRAD_CASES) and any(c["acc"] for c in ec.WGRAD_CASES)
    kinds = {}
    for c in ec.PAIR_CASES:
        vw, vd, paired = ec.pair_forms(c)
        assert paired == (c["kind"] == "pair"), c
        kinds.setdefault(c["kind"], set()).add((vw, c["acc"], vd, 6 if c["precise"] else 3))
        assert ec.PAIR_M % c["rpg"] == 0 if c["rpg"] else True
    # every instantiation of the pair kernel, and the issue's own pairs among them
    assert kinds["pair"] == {(vw, a, vd, n) for vw in (1, 2, 3) for a in (0, 1) for vd in (2, 3) for n in (3, 6)}
    own = [c for c in ec.PAIR_CASES if c["kind"] == "pair" and (c["O"], c["K"]) == (c["Og"], c["Kg"])]
    assert {(c["O"], c["K"], c["precise"], c["acc"]) for c in own} == {
        (O, K, p, a) for O, K in ((50, 128), (128, 64)) for p in (0, 1) for a in (0, 1)}
    assert len(kinds["skinny"]) == 2 and all(k[2] < 2 for k in kinds["oddb"])
    for B, O, K0, K1, acc in ec.WSMALL_CASES:
        assert min(B, O, K0) > 0 and K1 >= 0


def test_conv_max_cases_are_well_formed_and_near_ties_are_rare():
    """The float64 reference alone, on the chosen seeds: the near-tie rule of the
    GPU test (gap <= 1e-5 max |x_p . w_o|: either of the two best may be
    returned) excuses at most 2 % of the (cloud, channel) pairs of any shape."""
    assert {ec.conv_max_plane_kernel(s) for s in ec.CONVMAX_SHAPES} == {"x3", "big"}
    for shape in ec.CONVMAX_SHAPES:
        C, Npts, K, O = shape
        assert ec.conv_max_abi_problems(shape, K + 4, 4, K + 8) == []
        x, w, b, neg, skip = ec.conv_max_inputs(shape)
        val, idx, gap, z = ref.conv_max_ref(x, w, b, relu=0, skip=skip)
        excused = gap <= ref.near_tie_threshold(x, w)
        assert excused.mean() <= ec.NEAR_TIE_CAP, (shape, excused.mean())
        assert (z[:, :, neg] < 0).all()
        if skip:
            (c, later), first = skip[0], ec.conv_max_twin(Npts)[0]
            assert first // 128 != later // 128 and np.array_equal(x[c, first], x[c, later])
            assert (idx[c] == first).mean() > 0.15  # the twin row is the maximum of many channels


def test_cmx_bwd_and_row_ce_cases_are_well_formed():
    for case in ec.CMXBWD_CASES:
        K = case[3]
        assert ec.cmx_bwd_abi_problems(case, K + 4, K + 8) == [], case
    assert any(c[3] > 512 and not c[6] for c in ec.CMXBWD_CASES)
    assert any(c[0] > 8 for c in ec.CMXBWD_CASES) and any(c[2] % 32 for c in ec.CMXBWD_CASES)
    assert {(c[4], c[5], c[6]) for c in ec.CMXBWD_CASES} >= {(1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1)}
    assert {ec.row_ce_kernel(M, C) for M, C in ec.ROWCE_CASES} == {"wave", "lds", "lane"}
    for M, C in ec.ROWCE_CASES:
        lg, y = ec.row_ce_inputs(M, C, "edge")
        assert set(np.unique(y)) <= {0, C - 1}
        lg, y = ec.row_ce_inputs(M, C, "big")
        assert np.abs(lg).max() <= 80.0 and (C == 1 or np.abs(lg).max() == 80.0)
        assert np.isfinite(ref.row_ce_ref(lg, y)[1]).all()

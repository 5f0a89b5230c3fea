"""Case tables of tests/test_gpu_gemm_edges.py (numpy only), with the host
dispatch's own predicates restated so that tests/test_gemm_ref.py can assert on
the CPU that every case satisfies the ABI's stated requirements
(include/pcadv.h) and that the tables reach the forms they are meant to reach.

An operand is described by its row stride ld (floats) and `off`, the number of
floats its base lies past a 16-byte boundary (0 or 1)."""
import numpy as np


def _al(width):
    """A row stride above the width with ld % 4 == 0."""
    return (width + 3) // 4 * 4 + 4


def _operand(width, vec, how):
    """(ld, off) of an operand that allows 16-B loads (vec), or that does not:
    an odd stride (how = 0) or a base one float past the boundary (how = 1)."""
    if vec:
        return _al(width), 0
    return (_al(width) + 1, 0) if how == 0 else (_al(width), 1)


# ---------------------------------------------------------------------------
# pcadv_gemm
# ---------------------------------------------------------------------------
LAYOUTS = [(0, 0), (0, 1), (1, 1)]  # (ta, tb)
GEMM_M, GEMM_N, GEMM_K = [33, 129, 257], [1, 50, 127, 130, 132], [1, 3, 31, 36, 100]
# A^T (ta = 1) is read by 16-B loads only when M % 4 == 0, which none of GEMM_M
# is: the cases that ask for that form take this M instead
GEMM_M_VEC = 260


def gemm_case(i, M, N, K, ta, tb, precise, acc, flag, **kw):
    """One pcadv_gemm call.  `flag` asks for the vector form (bit 0: A, bit 1: B);
    the epilogue's operands cycle with i unless given."""
    how = i % 2
    lda, a_off = _operand(M if ta else K, flag & 1, how)
    ldb, b_off = _operand(N if tb else K, flag & 2, 1 - how)
    ldc, c_off = _operand(N, i % 3 != 1, i % 2)
    c = dict(M=M, N=N, K=K, ta=ta, tb=tb, precise=precise, acc=acc, relu=i % 2, want=flag,
             lda=lda, a_off=a_off, ldb=ldb, b_off=b_off, ldc=ldc, c_off=c_off,
             bias=("none", "al", "off")[(i // 2) % 3], rpg=(0, 1, 0, 50)[(i + i // 4) % 4],
             ldm=((N + 2) | 1) if i % 5 < 2 else 0, m_off=0, ldcp=0)
    c.update(kw)
    return c


def _gemm_cases():
    out = []
    for ta, tb in LAYOUTS:
        j = 0
        for precise in (0, 1):
            for acc in (0, 1):
                for flag in range(4):
                    M = GEMM_M_VEC if ta and flag & 1 else GEMM_M[j % 3]
                    N = 132 if tb and flag & 2 else GEMM_N[j % 5]
                    kvec = (not ta and flag & 1) or (not tb and flag & 2)
                    # precise = 0 with K < 16 takes the six-product kernels (gemm_products):
                    # the three-product ones get K >= 16 here, the short K below
                    K = (36, 100)[j % 2] if kvec else GEMM_K[(2 * j + 1) % 5] if precise \
                        else (31, 36, 100)[j % 3]
                    kw = dict(rpg=0) if ta and flag & 1 else {}  # A^T by vectors: rpg % 4 == 0
                    out.append(gemm_case(len(out), M, N, K, ta, tb, precise, acc, flag, **kw))
                    j += 1
        # the output planes on a ragged tile (ldcp > N), through the plain
        # epilogue and through the masked / accumulating one
        for acc in (0, 1):
            out.append(gemm_case(len(out), 129, 132, 36, ta, tb, acc, acc, 3 if not ta else 2,
                                 ldc=136, c_off=0, bias="al", rpg=50, ldm=136 if acc else 0,
                                 ldcp=136))
        # precise = 0 at K < 16: the dispatch takes the six-product form
        out.append(gemm_case(len(out), 257, 132, 1, ta, tb, 0, 0, 2 if tb else 0))
        out.append(gemm_case(len(out), 33, 50, 3, ta, tb, 0, 1, 0))
    return out


GEMM_CASES = _gemm_cases()

SMALL_M, SMALL_N, SMALL_K = [1, 16, 17, 32], [1, 15, 17, 50], [1, 3, 5, 1030]


def _small_cases():
    out = []
    for tb in (0, 1):
        for M in SMALL_M:
            for N in SMALL_N:
                for K in SMALL_K:
                    for vec in ((3, 0) if tb == 0 else (0,)):
                        i = len(out)
                        out.append(gemm_case(i, M, N, K, 0, tb, 0, i % 2, vec, relu=(i // 2) % 2,
                                             rpg=(0, 1, 0, 5)[i % 4],
                                             ldm=0 if i % 3 == 2 else ((N + 2) | 1)))
    return out


SMALL_CASES = _small_cases()


def gemm_vec_flags(c):
    """gemm_vec_flags of csrc/gemm.hip for a pcadv_gemm call (one k range)."""
    avec = c["lda"] % 4 == 0 and c["a_off"] == 0
    bvec = c["ldb"] % 4 == 0 and c["b_off"] == 0
    kq = c["K"] % 4 == 0
    va = avec and (kq if c["ta"] == 0 else c["M"] % 4 == 0 and c["rpg"] % 4 == 0)
    vb = bvec and (kq if c["tb"] == 0 else c["N"] % 4 == 0)
    return int(va) | 2 * int(vb)


def gemm_products(c):
    """bf16 products per term: six when asked for (precise) and where a
    reduction is too short for the three-product error to average out."""
    return 6 if c["precise"] or c["K"] < 16 else 3


def gemm_cvec(c):
    """The epilogue's 16-B form: C, bias, bias_rows and the mask all allow it."""
    return (c["ldc"] % 4 == 0 and c["c_off"] == 0 and c["bias"] != "off"
            and (c["rpg"] == 0 or c["N"] % 4 == 0)
            and (c["ldm"] == 0 or (c["ldm"] % 4 == 0 and c["m_off"] == 0)))


def gemm_abi_problems(c):
    """The stated requirements of pcadv_gemm that the case breaks (none: [])."""
    bad = []
    if min(c["M"], c["N"], c["K"]) <= 0:
        bad.append("shape")
    if c["lda"] < (c["M"] if c["ta"] else c["K"]):
        bad.append("lda")
    if c["ldb"] < (c["N"] if c["tb"] else c["K"]):
        bad.append("ldb")
    if c["ldc"] < c["N"] or (c["ldm"] and c["ldm"] < c["N"]):
        bad.append("ldc / ldm")
    if c["ta"] and not c["tb"]:
        bad.append("A^T needs B^T")
    if c["ldcp"] and not (c["ldcp"] >= c["N"] and c["ldcp"] % 4 == 0 and c["N"] % 4 == 0
                          and gemm_cvec(c) and (c["ta"] or c["M"] > 32)):
        bad.append("output planes")
    if max(c["M"], c["N"], c["K"]) * max(c["lda"], c["ldb"], c["ldc"], c["ldm"]) * 4 >= 2 ** 31:
        bad.append("span")
    return bad


# ---------------------------------------------------------------------------
# pcadv_gemm_bf2: plane strides K + 8, ldcp = N + 4, accumulate and mask
# ---------------------------------------------------------------------------
BF2_SHAPES = [(129, 50, 16), (257, 132, 48), (128, 128, 32), (130, 256, 80)]
BF2_BIG = (7950, 2048, 16)  # the 256-tile kernel: a ragged row tile and half a k-tile


def _bf2_case(M, N, K, acc):
    q = N % 4 == 0
    return dict(M=M, N=N, K=K, lda=K + 8, ldb=K + 8, ldc=N + 4 if q else N + 3, acc=acc, relu=1,
                bias="al", rpg=50, ldm=(N + 4 if q else N + 3) if acc else 0, m_off=0, c_off=0,
                ldcp=N + 4 if q else 0)


BF2_CASES = [_bf2_case(M, N, K, acc) for M, N, K in BF2_SHAPES for acc in (0, 1)]
BF2_BIG_CASES = [dict(_bf2_case(*BF2_BIG, acc), rpg=4096) for acc in (0, 1)]


def bf2_abi_problems(c):
    bad = []
    if c["K"] % 16 or c["lda"] % 8 or c["ldb"] % 8 or c["lda"] < c["K"] or c["ldb"] < c["K"]:
        bad.append("K % 16, lda % 8, ldb % 8")
    if c["ldc"] < c["N"] or (c["ldm"] and c["ldm"] < c["N"]):
        bad.append("ldc / ldm")
    if c["ldcp"] and not (c["ldcp"] >= c["N"] and c["ldcp"] % 4 == 0 and c["N"] % 4 == 0
                          and gemm_cvec(c)):
        bad.append("output planes")
    return bad


def bf2_kernel(c):
    """The kernel launch_gemm_bf2 picks (default environment)."""
    M, N, K = c["M"], c["N"], c["K"]
    gl128 = M % 128 == 0 and N % 128 == 0 and K % 32 == 0
    big = N % 256 == 0 and ((M + 255) // 256) * (N // 256) >= 256
    if not gl128 and big:
        return "big_glds" if M % 256 == 0 and K % 32 == 0 else "big"
    return "x3_glds" if gl128 else "x3"


# ---------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------
# (rows, rpg, O, Kin); the last of the issue's five has 128 groups, above
# WF_MAXG = 64.  None of them has O % 4 == 0, which the 16-B form of dz^T
# needs, so a sixth shape is added for the four vector forms.
WGRAD_SHAPES = [(1, 0, 5, 3), (129, 0, 1, 1), (130, 0, 50, 36), (260, 65, 130, 7),
                (8320, 65, 33, 5), (130, 0, 52, 36)]
# (dz_off, x_off, db given, gsum given (where rpg > 0), accumulate)
WGRAD_VARIANTS = [(0, 0, 1, 1, 0), (1, 0, 1, 1, 1), (0, 1, 0, 1, 0), (1, 1, 1, 0, 0),
                  (0, 0, 0, 0, 1)]
WF_MAXG = 64


def wgrad_case(shape, variant):
    rows, rpg, O, Kin = shape
    dz_off, x_off, db, gs, acc = variant
    return dict(rows=rows, rpg=rpg, O=O, Kin=Kin, ldz=_al(O), ldx=_al(Kin), ldo=Kin + 3,
                dz_off=dz_off, x_off=x_off, db=db, gs=int(bool(gs and rpg)), acc=acc)


WGRAD_CASES = [wgrad_case(s, v) for s in WGRAD_SHAPES for v in WGRAD_VARIANTS]


def wgrad_vec_flags(c):
    va = c["ldz"] % 4 == 0 and c["dz_off"] == 0 and c["O"] % 4 == 0
    vb = c["ldx"] % 4 == 0 and c["x_off"] == 0 and c["Kin"] % 4 == 0
    return int(va) | 2 * int(vb)


def wgrad_abi_problems(c):
    bad = []
    if min(c["rows"], c["O"], c["Kin"]) <= 0 or c["ldz"] < c["O"] or c["ldx"] < c["Kin"] \
            or c["ldo"] < c["Kin"]:
        bad.append("shape")
    if c["rpg"] and c["rows"] % c["rpg"]:
        bad.append("rows % rows_per_group")
    if c["gs"] and not c["rpg"]:
        bad.append("gsum needs rows_per_group")
    return bad


# paired launch: M = 200; kind "pair" (one launch), "skinny" (g has 20 rows: the
# exact-f32 kernel, which cannot pair), "oddb" (g's b has an odd stride: no 16-B
# loads, cannot pair).  The weight gradient is dz [M][O]^T x [M][K]; the data
# gradient is a [M][Og] times b [Og][Kg] read as B^T.  (O, K) = (Og, Kg) in
# {(50, 128), (128, 64)} are a layer's own pair (g reads the dz that w reads);
# the mixed shapes reach the other combinations of the two vector forms.
PAIR_M = 200
PAIR_W = [(64, 50), (50, 128), (128, 64)]   # (O, K): vector forms 1, 2, 3 of <1,1,0,6,v>
PAIR_G = [(50, 128), (128, 64)]             # (Og, Kg): vector forms 2, 3 of <0,1,m,np,v>
PAIR_CASES = ([dict(O=O, K=K, Og=Og, Kg=Kg, precise=p, acc=a, kind="pair", rpg=100 if O == 128 else 0)
               for O, K in PAIR_W for Og, Kg in PAIR_G for p in (0, 1) for a in (0, 1)]
              + [dict(O=50, K=128, Og=50, Kg=128, precise=1, acc=1, kind="skinny", rpg=0),
                 dict(O=128, K=64, Og=128, Kg=64, precise=0, acc=0, kind="skinny", rpg=100),
                 dict(O=50, K=128, Og=50, Kg=128, precise=0, acc=1, kind="oddb", rpg=0),
                 dict(O=128, K=64, Og=128, Kg=64, precise=1, acc=0, kind="oddb", rpg=100)])


def pair_forms(c):
    """(the weight gradient's vector flags, the data gradient's, whether the
    two run as one launch) by the dispatch's rules; operands dense and aligned
    but for the odd stride of "oddb"."""
    vw = int(c["O"] % 4 == 0) | 2 * int(c["K"] % 4 == 0)
    ldb = c["Kg"] + 1 if c["kind"] == "oddb" else c["Kg"]
    vd = int(c["Og"] % 4 == 0) | 2 * int(ldb % 4 == 0 and c["Kg"] % 4 == 0)
    Mg = 20 if c["kind"] == "skinny" else PAIR_M
    return vw, vd, vw >= 1 and vd >= 2 and Mg > 32


# pcadv_wgrad_small: (B, O, K0, K1, accumulate); K1 = 0: one operand
WSMALL_CASES = [(3, 5, 7, 2, 1), (16, 33, 130, 0, 0), (1, 1, 1, 1, 0)]


# ---------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------
COLSUM_M, COLSUM_N = [1, 130, 513], [1, 64, 65, 257]
GROUP_RPG = [1, 65]

# ---------------------------------------------------------------------------
# conv + max over points, and its backward
# ---------------------------------------------------------------------------
# (C, Npts, K, O); the last is the smallest shape that takes the 256-tile
# kernel in the plane form: 32 x 8 = 256 tiles
CONVMAX_SHAPES = [(1, 1, 32, 50), (3, 127, 32, 130), (2, 129, 64, 128), (3, 300, 96, 33),
                  (32, 256, 64, 2048)]
NEAR_TIE_CAP = 0.02


def conv_max_twin(Npts):
    """Indices of the twin rows (equal rows in different 128-row tiles), or None."""
    return (5, 200) if Npts > 200 else (5, 128) if Npts > 128 else None


def conv_max_inputs(shape):
    """x [C][Npts][K] >= 0 (the output of a ReLU layer), w [O][K], b [O], the
    channel made negative everywhere, and the (cloud, point) of the later twin.
    Cloud C - 1 holds the twin pair: a positive row of large norm at both indices,
    so that it is the maximum of many channels."""
    C, Npts, K, O = shape
    rng = np.random.default_rng(C + 10 * Npts + 1000 * K + O)
    x = np.maximum(rng.standard_normal((C, Npts, K)), 0).astype(np.float32)
    w = (rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32)
    b = (rng.standard_normal(O) * 0.05).astype(np.float32)
    neg = O // 2
    w[neg] = -np.abs(w[neg]) - np.float32(0.01)
    b[neg] = np.float32(-0.1)
    skip = []
    tw = conv_max_twin(Npts)
    if tw:
        x[C - 1, tw[0]] = (2.0 * np.abs(rng.standard_normal(K)) + 0.5).astype(np.float32)
        x[C - 1, tw[1]] = x[C - 1, tw[0]]
        skip = [(C - 1, tw[1])]
    return x, w, b, neg, skip


def conv_max_abi_problems(shape, ldx, x_off, ldxp=0):
    C, Npts, K, O = shape
    bad = []
    if K % 32 or ldx % 4 or ldx < K:
        bad.append("K % 32, ldx % 4")
    if x_off % 4:
        bad.append("x 16-B aligned")
    if ldxp and (ldxp % 8 or ldxp < K):
        bad.append("ldxp % 8")
    return bad


def conv_max_plane_kernel(shape):
    C, Npts, K, O = shape
    big = O % 256 == 0 and Npts % 256 == 0 and ((C * Npts + 255) // 256) * (O // 256) >= 256
    return "big" if big else "x3"


# (C, Npts, O, K, dw, db, dx): the last three say which outputs are asked for
CMXBWD_CASES = [(C, Npts, O, K, 1, 1, 1) for C, Npts, O, K in
                [(1, 1, 1, 4), (9, 65, 33, 64), (2, 64, 50, 260), (3, 130, 4096, 512)]] + [
    (9, 65, 130, 1024, 1, 1, 0),   # K in (512, 1024]: k_cmx_dw's second column block; dx = NULL
    (9, 65, 33, 64, 0, 1, 1),      # dw = NULL with db given
    (9, 65, 33, 64, 0, 1, 0),      # the same without dx
    (2, 64, 50, 260, 0, 0, 1),     # dw = NULL, db = NULL with dx given
]


def cmx_bwd_abi_problems(case, ldx, lddx, x_off=0, dx_off=0):
    C, Npts, O, K, dw, db, dx = case
    bad = []
    if K % 4 or ldx % 4 or ldx < K or O > 4096:
        bad.append("K % 4, ldx % 4, O <= 4096")
    if dx and (K > 512 or lddx % 4 or lddx < K):
        bad.append("dx: K <= 512, lddx % 4")
    if x_off % 4 or dx_off % 4:
        bad.append("16-B aligned rows")
    return bad


# ---------------------------------------------------------------------------
# row cross entropy: (M, C), ld = C + 3
# ---------------------------------------------------------------------------
ROWCE_CASES = [(256, 64), (257, 64), (256, 65), (1, 1), (300, 63)]


def row_ce_kernel(M, C):
    if M <= 256 and C <= 64:
        return "wave"
    return "lds" if C <= 63 else "lane"


def row_ce_inputs(M, C, mode):
    """Logits [M][C] and labels: "edge" (labels only 0 and C - 1, logits 3 randn)
    or "big" (logits uniform in [-80, 80], any label)."""
    rng = np.random.default_rng(1000 * M + C + (7 if mode == "big" else 0))
    if mode == "big":
        lg = rng.uniform(-80.0, 80.0, (M, C)).astype(np.float32)
        if C > 1:
            lg[0, 0], lg[0, C - 1] = np.float32(80.0), np.float32(-80.0)
        return lg, rng.integers(0, C, M)
    lg = (rng.standard_normal((M, C)) * 3).astype(np.float32)
    return lg, rng.integers(0, 2, M) * (C - 1)

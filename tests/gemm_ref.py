"""Float64 numpy restatements of the dense GEMM engine's operations
(csrc/gemm.hip, the pcadv_gemm .. pcadv_row_ce block of include/pcadv.h): what
tests/test_gpu_gemm_edges.py holds the kernels to, checked themselves on the CPU
by tests/test_gemm_ref.py.  Every function takes the operands as stored and
works in float64 throughout."""
import numpy as np

EPS = 2.0 ** -23  # one f32 spacing at 1


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def gemm_ref(A, B, ta=0, tb=0, bias=None, bias_rows=None, rpg=0, relu=0, accumulate=0, base=None,
             cmask=None):
    """pcadv_gemm: A stored [M][K] (ta = 0) or [K][M] (ta = 1), B stored [N][K]
    (tb = 0) or [K][N] (tb = 1).  The epilogue in the engine's order: sum + bias
    + bias_rows[m // rpg] (+ base), then ReLU, then the mask (zero where cmask
    is not > 0).  Returns (C, S): the result and sum |terms| of every output
    element (|A| |B|^T + |bias| + |bias_rows| + |base|), the scale of the
    rounding bounds."""
    A, B = _f64(A), _f64(B)
    opA = A.T if ta else A
    opB = B if tb else B.T  # [K][N]
    C = opA @ opB
    S = np.abs(opA) @ np.abs(opB)
    M = C.shape[0]
    if bias is not None:
        C = C + _f64(bias)
        S = S + np.abs(_f64(bias))
    if bias_rows is not None:
        br = _f64(bias_rows)[np.arange(M) // rpg]
        C = C + br
        S = S + np.abs(br)
    if accumulate:
        C = C + _f64(base)
        S = S + np.abs(_f64(base))
    if relu:
        C = np.maximum(C, 0.0)
    if cmask is not None:
        C = np.where(np.asarray(cmask) > 0, C, 0.0)
    return C, S


def wgrad_ref(dz, x, rpg=0):
    """pcadv_gemm_wgrad: dW [O][Kin] = dz^T x, db [O] = the column sums of dz,
    gsum [rows / rpg][O] = the sums over each group of rpg rows (None when
    rpg = 0)."""
    dz, x = _f64(dz), _f64(x)
    gsum = dz.reshape(dz.shape[0] // rpg, rpg, dz.shape[1]).sum(1) if rpg else None
    return dz.T @ x, dz.sum(0), gsum


def colsum_ref(x, ymask=None):
    """pcadv_colsum: out[n] = sum_m x[m][n] [ymask[m][n] > 0]."""
    x = _f64(x)
    return (x if ymask is None else np.where(np.asarray(ymask) > 0, x, 0.0)).sum(0)


def group_colsum_ref(x, rpg, ymask=None):
    """pcadv_group_colsum: one row of column sums per rpg rows."""
    x = _f64(x)
    x = x if ymask is None else np.where(np.asarray(ymask) > 0, x, 0.0)
    return x.reshape(x.shape[0] // rpg, rpg, x.shape[1]).sum(1)


def conv_max_ref(x, w, b=None, relu=0, skip=(), z0=None):
    """pcadv_conv_max_x3 on x [C][Npts][K], w [O][K], b [O] or None.  Returns
    (val, idx, gap, z): val [C][O] the max over the points of x w^T + b (relu
    applied after the max), idx the first index that attains it, gap the
    difference between the two best values of each (cloud, channel) (inf with
    one point), z [C][Npts][O] the pre-activations.  `skip` lists (cloud, point)
    pairs left out of the ranking: the later of two bitwise equal rows, which a
    first-index max can never return.  z0 = x w^T when the caller has it."""
    z = _f64(x) @ _f64(w).T if z0 is None else z0
    if b is not None:
        z = z + _f64(b)
    r = z.copy()
    for c, p in skip:
        r[c, p, :] = -np.inf
    idx = r.argmax(1)
    val = np.take_along_axis(r, idx[:, None, :], 1)[:, 0, :]
    np.put_along_axis(r, idx[:, None, :], -np.inf, 1)
    gap = val - r.max(1) if z.shape[1] > 1 else np.full(val.shape, np.inf)
    return (np.maximum(val, 0.0) if relu else val), idx, gap, z


def near_tie_threshold(x, w):
    """The engine's near-tie scale per (cloud, channel): 1e-5 max_p |x_p . w_o|."""
    return 1e-5 * np.abs(_f64(x) @ _f64(w).T).max(1)


def cmx_bwd_ref(dgmax, gmax, gidx, x, w, relu_x=0, dx_base=None):
    """pcadv_conv_max_x3_bwd: g' = dgmax [gmax > 0];
    dw[o][k] = sum_c g'[c][o] x[c][gidx[c][o]][k], db[o] = sum_c g'[c][o],
    dx[c][p] = dx_base[c][p] + [x[c][p] > 0 if relu_x] sum_{o: gidx[c][o] = p} g'[c][o] w[o].
    Returns (dw, db, dx, Sdw, Sdx, hits): the sums, sum |terms| of dw and dx, and
    the number of channels that hit each point [C][Npts]."""
    dg, x, w = _f64(dgmax), _f64(x), _f64(w)
    C, Npts, K = x.shape
    gp = dg * (np.asarray(gmax) > 0)
    dw, Sdw = np.zeros(w.shape), np.zeros(w.shape)
    dx = np.zeros(x.shape) if dx_base is None else _f64(dx_base).reshape(x.shape).copy()
    Sdx = np.abs(dx)
    hits = np.zeros((C, Npts), np.int64)
    for c in range(C):
        rows = x[c, gidx[c]]
        dw += gp[c][:, None] * rows
        Sdw += np.abs(gp[c][:, None] * rows)
        add, sadd = np.zeros((Npts, K)), np.zeros((Npts, K))
        np.add.at(add, gidx[c], gp[c][:, None] * w)
        np.add.at(sadd, gidx[c], np.abs(gp[c][:, None] * w))
        np.add.at(hits[c], gidx[c], (gp[c] != 0).astype(np.int64))
        keep = x[c] > 0 if relu_x else np.ones((Npts, K), bool)
        dx[c] += add * keep
        Sdx[c] += sadd * keep
    return dw, gp.sum(0), dx, Sdw, Sdx, hits


def row_ce_ref(logits, labels, scale=1.0):
    """pcadv_row_ce: the mean over the rows of the cross entropy, and
    scale * d(mean)/dlogits = (softmax - onehot) * scale / M, with the row
    maximum subtracted before the exponentials."""
    x = _f64(logits)
    M = x.shape[0]
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    p = np.exp(x - lse[:, None])
    p[np.arange(M), labels] -= 1.0
    return (lse - x[np.arange(M), labels]).mean(), p * scale / M


def sum_bound(n, S):
    """|f32 sum of n terms in any order - exact| <= (n + 8) 2^-23 sum|terms|
    (the rigorous (n - 1) u bound with u = 2^-24, a factor of 2 in hand)."""
    return (n + 8) * EPS * np.asarray(S, np.float64)

"""Case tables and generators of tests/test_gpu_feat_fwd_edges.py (numpy only):
the feature forward's two kernels, k_point_mlp and k_conv4_max
(csrc/feat_fused.hip), at the edges of every form the host dispatch reaches.
tests/test_feat_fwd_cases.py checks on the CPU that the tables reach the forms
they are meant to reach, that the generated arrays have the properties the
exact comparison relies on, and that the comparison notices each slip it is
there for.

On small integers every product, bf16 split and partial sum of the pipeline is
exact (bf16 mode included) and the screening key drops only zero bits, so the
kernels' outputs must equal numpy's bit for bit.

Geometry of k_conv4_max.  A cloud is screened in 32-point units; unit u holds
points 32 u .. 32 u + 31 and belongs to step u // (P / 32).  A lane holds one
channel and the 16 rows (i & 3) + 8 (i >> 2) + 4 h of a unit (h = lane half).
The forms with wave groups (NGRP > 1) give unit u to group u % NGRP; group 0
collects the others' top two through LDS."""
import functools

import numpy as np

# the constants of feat_fused.hip that the dispatch reads (test_feat_fwd_cases
# compares them with the source)
C4_G2_MAXC = 63       # the largest cloud count of the wave-group forms
C4_CB = 256           # channels per workgroup (half that in the wave-group forms)
C4_O = 1024
PM_P = 64             # points per k_point_mlp tile
PM_ONE_BELOW = 1024   # tile count below which a workgroup takes one tile

PRECISIONS = ("fp32", "bf16", "bf16xb")  # pcadv_conv4_max's precision 0, 1, 2 (2: a bf16 x3)

# form -> the instantiation and its geometry: points per step, wave groups,
# whether a lane keeps its top two (fp32: re-evaluated exactly) or its top one
CONV4_FORMS = {
    "w16-fp32": dict(inst="k_conv4_max<3, C4W16>", P=128, NGRP=1, top2=True),
    "plain-fp32": dict(inst="k_conv4_max<3, false, false, false>", P=64, NGRP=1, top2=True),
    "plain-bf16": dict(inst="k_conv4_max<1, false, false, false>", P=64, NGRP=1, top2=False),
    "plain-bf16xb": dict(inst="k_conv4_max<1, false, true, false>", P=64, NGRP=1, top2=False),
    "p128-bf16": dict(inst="k_conv4_max<1, false, false, true>", P=128, NGRP=1, top2=False),
    "p128-bf16xb": dict(inst="k_conv4_max<1, false, true, true>", P=128, NGRP=1, top2=False),
    "g2-fp32": dict(inst="k_conv4_max<3, true, false, false>", P=64, NGRP=2, top2=True),
    "g2-bf16": dict(inst="k_conv4_max<1, true, false, false>", P=64, NGRP=2, top2=False),
    "g4-bf16xb": dict(inst="k_conv4_max<1, true, true, false>", P=128, NGRP=4, top2=False),
}
MLP_FORMS = {(np3, tpw): f"k_point_mlp<{np3}, {tpw}, false>" for np3 in (6, 1) for tpw in (1, 2)}


def conv4_form(C, N, precision):
    """launch_conv4_max_np restated: the form (C, N, precision) runs."""
    kind = PRECISIONS[precision]
    if C <= C4_G2_MAXC:
        return "g4-bf16xb" if precision == 2 else f"g2-{kind}"
    if N % 128 == 0:
        return "w16-fp32" if precision == 0 else f"p128-{kind}"
    return f"plain-{kind}"


def conv4_grid(C, N, precision):
    """(workgroups, whether the XCD remap renumbers them)."""
    nwg = C * (2 * C4_O // C4_CB if C <= C4_G2_MAXC else C4_O // C4_CB)
    return nwg, nwg % 8 == 0


def mlp_form(C, N, precision):
    """launch_feat_fwd_np restated (no gather): the instantiation, tiles per
    cloud, tile count and workgroups of k_point_mlp; precision 0 fp32, 1 bf16."""
    T = (N + PM_P - 1) // PM_P
    ntiles = C * T
    tpw = 1 if ntiles < PM_ONE_BELOW else 2
    return dict(inst=MLP_FORMS[(1 if precision else 6, tpw)], tpw=tpw, T=T, ntiles=ntiles,
                grid=ntiles if tpw == 1 else (ntiles + 1) // 2)


def geometry(form, N):
    g = dict(CONV4_FORMS[form])
    g["ups"] = g["P"] // 32                    # units per step
    g["U"] = (N + 31) // 32                    # units with a valid row
    g["S"] = (N + g["P"] - 1) // g["P"]        # steps
    # wave groups whose unit of the last step lies wholly past N
    g["past"] = [k for k in range(g["NGRP"]) if g["NGRP"] * (g["S"] - 1) + k >= g["U"]]
    return g


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even) as float32: the kernels' cast."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ---------------------------------------------------------------------------
# k_conv4_max<3, C4W16>: the positions of tests/test_gpu_conv4_w16.py
# ---------------------------------------------------------------------------
def _w16_positions(kind, N, rng):
    """Point indices of one distinct row, by where its equal values sit."""
    T = int(rng.integers(0, N // 16))   # a 16-point tile
    U = int(rng.integers(0, N // 64))   # a 64-point span
    S = int(rng.integers(0, N // 128))  # a 128-point step
    r = [int(v) for v in rng.integers(0, 4, 4)]
    if kind == 0:  # one tile, rows of different lane quarters (4 q + reg)
        q = rng.permutation(4)
        return [16 * T + 4 * int(q[0]) + r[0], 16 * T + 4 * int(q[1]) + r[1],
                16 * T + 4 * int(q[2]) + r[2]]
    if kind == 1:  # different tiles of one span
        t = rng.permutation(4)
        return [64 * U + 16 * int(t[0]) + 4 * r[0] + r[1], 64 * U + 16 * int(t[1]) + 4 * r[2] + r[3],
                64 * U + 16 * int(t[2]) + 4 * r[1] + r[0]]
    if kind == 2:  # both spans of a step, the later span's copy in the lower row
        return [128 * S + 64 + 16 * r[0] + 4 * r[1] + r[2], 128 * S + 16 * r[1] + 4 * r[3] + 3]
    # different steps (N = 128 has one: two spans then)
    s = rng.permutation(max(N // 128, 2))
    return [(128 * int(s[0]) + 16 * r[0] + 4 * r[1] + r[2]) % N,
            (128 * int(s[1]) + 64 + 16 * r[2] + 4 * r[3] + r[0]) % N]


def _w16_plant(c, N, rng, npairs):
    which = np.zeros(N, np.int64)
    for k in range(1, 2 * npairs + 1):
        which[_w16_positions((c + k) % 4, N, rng)] = k
    return which, None


# ---------------------------------------------------------------------------
# planted positions of the 32-point-unit forms
# ---------------------------------------------------------------------------
# a tie pattern places one row at several points (equal values in every
# channel: the first index must win); a row pattern places it at one point
TIE_PATTERNS = ("first_last", "halves", "lane3", "units", "steps_even", "steps_odd",
                "groups_up", "groups_down")
ROW_PATTERNS = ("last", "ragged_first", "full_last", "own_g1", "own_g2", "own_g3")


def _rows(nv, h=None, lo=0):
    return [r for r in range(lo, nv) if h is None or (r >> 2) & 1 == h]


def _pick(rng, seq):
    return int(seq[int(rng.integers(0, len(seq)))])


def pattern_positions(name, g, N, rng):
    """Point indices of pattern `name` in a cloud of N points for geometry g,
    or None where the geometry has no such place."""
    U, S, ups, NGRP, P = g["U"], g["S"], g["ups"], g["NGRP"], g["P"]
    nv = lambda u: min(32, N - 32 * u)  # valid rows of unit u
    if name == "last":          # the last valid row of the ragged (or last) unit
        return [N - 1]
    if name == "first_last":    # point 0 keeps a tie with point N - 1
        return [0, N - 1] if N >= 2 else None
    if name == "ragged_first":  # the first row of a ragged last unit
        return [32 * (U - 1)] if N % 32 and N > 32 else None
    if name == "full_last":     # the last row of the last full unit
        return [32 * (N // 32) - 1] if N % 32 and N > 32 else None
    if name == "halves":        # the two lane halves of one unit: the __shfl_xor(.., 32) merge
        us = [u for u in range(U) if nv(u) >= 8]
        if not us:
            return None
        u = _pick(rng, us)
        return [32 * u + _pick(rng, _rows(nv(u), 0)), 32 * u + _pick(rng, _rows(nv(u), 1))]
    if name == "lane3":         # three copies in one lane's rows: the two lowest are its top two
        us = [(u, h) for u in range(U) for h in (0, 1) if len(_rows(nv(u), h)) >= 3]
        if not us:
            return None
        u, h = us[int(rng.integers(0, len(us)))]
        return [32 * u + int(r) for r in rng.permutation(_rows(nv(u), h))[:3]]
    if name == "units":         # two units of one step in one wave, the later copy in the lower row
        if NGRP > 1:
            return None
        ss = [s for s in range(S) if ups * s + 1 < U]
        if not ss:
            return None
        s = _pick(rng, ss)
        ua, ub = sorted(int(v) for v in rng.permutation(range(ups * s, min(ups * s + ups, U)))[:2])
        rb = _pick(rng, _rows(nv(ub)))
        return [32 * ua + _pick(rng, _rows(32, lo=min(rb, 31))), 32 * ub + rb]
    if name in ("steps_even", "steps_odd"):  # two steps whose LDS buffers are the same / differ
        odd = name == "steps_odd"
        pairs = [(a, b) for a in range(S) for b in range(a + 1, S) if (b - a) % 2 == odd]
        if not pairs:
            return None
        a, b = pairs[int(rng.integers(0, len(pairs)))]
        pb = _pick(rng, range(P * b, min(P * b + P, N)))
        # the earlier step's copy in a row no lower than the later one's
        return [P * a + _pick(rng, [p for p in range(P) if p % 32 >= pb % 32]), pb]
    if name in ("groups_up", "groups_down"):  # units of different wave groups
        if NGRP == 1:
            return None
        up = name == "groups_up"  # the lower index in the higher group
        pairs = [(a, b) for a in range(U) for b in range(a + 1, U)
                 if (a % NGRP > b % NGRP if up else a % NGRP < b % NGRP)]
        if not pairs:
            return None
        a, b = pairs[int(rng.integers(0, len(pairs)))]
        return [32 * a + _pick(rng, _rows(32)), 32 * b + _pick(rng, _rows(nv(b)))]
    if name.startswith("own_g"):  # a unique winner in a unit of group k > 0: only the hand-off carries it
        k = int(name[5:])
        us = [u for u in range(U) if u % NGRP == k] if k < NGRP else []
        if not us:
            return None
        u = _pick(rng, us)
        return [32 * u + _pick(rng, _rows(nv(u)))]
    raise KeyError(name)


def applicable_patterns(form, N):
    """The patterns form's geometry has a place for at N points."""
    g, rng = geometry(form, N), np.random.default_rng(0)
    return [n for n in ROW_PATTERNS + TIE_PATTERNS if pattern_positions(n, g, N, rng) is not None]


def _unit_plant(form, rot):
    """Plants 2 npairs rows per cloud.  Cloud 0 always holds `last` and a
    unique winner in every other wave group; the remaining rows rotate over
    the tie patterns and the unit-edge rows (rot shifts the rotation per case)."""
    memo = {}

    def plant(c, N, rng, npairs):
        g = geometry(form, N)
        if N not in memo:
            memo[N] = [n for n in TIE_PATTERNS + ("ragged_first", "full_last", "last")
                       if pattern_positions(n, g, N, np.random.default_rng(0)) is not None]
        pool = memo[N]
        fixed = ["last"] + [f"own_g{k}" for k in range(1, g["NGRP"]) if k < g["U"]]
        which, names, taken = np.zeros(N, np.int64), {}, set()
        for k in range(1, 2 * npairs + 1):
            if c == 0 and k <= len(fixed):
                name = fixed[k - 1]
            else:
                name = pool[(rot + c * 2 * npairs + k) % len(pool)]
            pos = None
            for _ in range(20):  # a placement clear of the rows already planted
                p = pattern_positions(name, g, N, rng)
                if p is not None and len(set(p)) == len(p) and not taken & set(p):
                    pos = p
                    break
            if pos is None:  # no room left for the pattern: any free point
                free = [p for p in range(N) if p not in taken]
                if not free:
                    continue
                name, pos = "free", [_pick(rng, free)]
            which[pos] = k
            taken |= set(pos)
            names[k] = name
        return which, names
    return plant


# ---------------------------------------------------------------------------
# the conv4 integer generator
# ---------------------------------------------------------------------------
def conv4_integer_case(C, N, seed, plant, npairs=2, fmax=2, dmax=2):
    """C clouds of small integers in [-4, 4], each built from 1 + 2 npairs
    distinct rows: a filler f and pairs f +- d_j (so the filler, their midpoint,
    never beats both of a pair and the pooled point is one of the few planted
    rows, at most of the 1024 channels); W4 and the bias in [-4, 4] too.
    Returns x [C][N][128], W, b, numpy's max and first argmax of
    x W^T + b over the points (exact: |v| < 2^12, far below the 2^17 at which
    the key's dropped bits would not all be zero), the row number of every
    point (0 the filler) and the pattern name of every planted row."""
    rng = np.random.default_rng(seed)
    W = rng.integers(-4, 5, (1024, 128)).astype(np.float32)
    b = rng.integers(-4, 5, 1024).astype(np.float32)
    W64 = W.astype(np.float64)
    x = np.empty((C, N, 128), np.float32)
    gmax = np.empty((C, 1024), np.float32)
    gidx = np.empty((C, 1024), np.int64)
    whichs, names = np.zeros((C, N), np.int64), []
    for c in range(C):
        f = rng.integers(-fmax, fmax + 1, 128)
        ds = [rng.integers(-dmax, dmax + 1, 128) for _ in range(npairs)]
        rows = np.stack([f] + [f + s * d for d in ds for s in (1, -1)]).astype(np.float32)
        which, nm = plant(c, N, rng, npairs)
        x[c] = rows[which]
        # exact; the max over the points is the max over the distinct rows
        # present, at the first point that holds such a row
        vr = rows.astype(np.float64) @ W64.T + b
        first = np.full(len(rows), N, np.int64)
        np.minimum.at(first, which, np.arange(N))
        vr[first == N] = -np.inf
        gmax[c] = vr.max(0)
        gidx[c] = np.where(vr == vr.max(0), first[:, None], N).min(0)  # the first index of the maximum
        whichs[c] = which
        names.append(nm)
    return dict(x=x, W=W, b=b, gmax=gmax, gidx=gidx, which=whichs, names=names)


def w16_integer_case(N, seed, C=64):
    """The case of tests/test_gpu_conv4_w16.py: (x, W, b, gmax, gidx)."""
    d = conv4_integer_case(C, N, seed, _w16_plant)
    return d["x"], d["W"], d["b"], d["gmax"], d["gidx"]


def form_kind(form):
    """Forms of one kind (plain, p128, g2, g4) share their geometry, so their cases."""
    return form.split("-")[0]


@functools.lru_cache(maxsize=4)
def _unit_case(kind, C, N):
    form = next(f for f in CONV4_FORMS if form_kind(f) == kind)
    rot = (3 * C + N) % 11
    d = conv4_integer_case(C, N, 9000 + 131 * C + N, _unit_plant(form, rot), npairs=4, fmax=3, dmax=1)
    d["geom"] = geometry(form, N)
    return d


def unit_integer_case(form, C, N):
    """The integer case of a 32-point-unit form: four pairs around a filler in
    [-3, 3] with steps in [-1, 1] (a wide filler leaves about a quarter of the
    channels with a negative maximum in every cloud)."""
    return _unit_case(form_kind(form), C, N)


def conv4_values(d):
    """Every conv4 value of a case, float64 [C][N][1024] (small cases only)."""
    return d["x"].astype(np.float64) @ d["W"].astype(np.float64).T + d["b"]


def pattern_of_winner(d):
    """[C][1024] pattern names of the rows numpy's winners sit on ('' the filler)."""
    out = np.empty(d["gidx"].shape, object)
    for c in range(d["gidx"].shape[0]):
        k = d["which"][c][d["gidx"][c]]
        nm = d["names"][c] or {}
        out[c] = [nm.get(int(q), "") for q in k]
    return out


def mismatches(gmax, gidx, want_max, want_idx):
    """The exact comparison: the number of (cloud, channel) pairs whose value
    or index differs from numpy's."""
    return int(((np.asarray(gidx).astype(np.int64) != want_idx) | (np.asarray(gmax) != want_max)).sum())


def relu_reference(gmax, gidx):
    """The ReLU before the max: channels whose values are all <= 0 give 0 at
    point 0, the others are unchanged."""
    dead = gmax <= 0
    return np.where(dead, np.float32(0), gmax), np.where(dead, 0, gidx)


# the slips the exact comparison is there to notice, applied to the reference
def corrupt(d, how, group=None):
    """numpy's (max, argmax) of case d as a kernel with slip `how` would give
    them, or None where the case has no place for the slip."""
    v = conv4_values(d)
    C, N, _ = v.shape
    g = d["geom"]
    if how == "drop_last":          # a mask one row too narrow
        if N == 1:
            return np.full_like(d["gmax"], -np.inf), np.zeros_like(d["gidx"])
        v = v[:, :N - 1]
        return v.max(1).astype(np.float32), v.argmax(1)
    if how == "last_on_ties":       # the later of equal values
        if N == 1:
            return None
        return v.max(1).astype(np.float32), N - 1 - v[:, ::-1].argmax(1)
    if how == "drop_group":         # wave group `group` never handed over
        keep = np.array([(p // 32) % g["NGRP"] != group for p in range(N)])
        if g["NGRP"] == 1 or keep.all():
            return None
        w = np.where(keep[None, :, None], v, -np.inf)
        return w.max(1).astype(np.float32), w.argmax(1)
    if how == "empty_as_zero":      # an empty slot (no valid row) taken for (0, point 0)
        if not g["past"] and N >= 5:
            return None
        m, i = v.max(1), v.argmax(1)
        return np.where(m < 0, 0, m).astype(np.float32), np.where(m < 0, 0, i)
    raise KeyError(how)


# ---------------------------------------------------------------------------
# shape tables
# ---------------------------------------------------------------------------
# (form kind, cloud counts, precisions, point counts): the smallest shapes with
# S = 1, S = 2 and a reused LDS buffer (S = 3 or more), and N % P on both sides
# of every unit boundary.  65 clouds: 260 workgroups, so no XCD remap.
_CONV4_TABLE = [
    ("plain", (64, 65), (0, 1, 2), (1, 31, 33, 64, 65, 97, 192, 200)),
    ("p128", (64, 65), (1, 2), (128, 256, 384)),
    ("g2", (1, 3, 63), (0, 1), (1, 32, 33, 64, 65, 97, 129, 200)),
    ("g4", (1, 3, 63), (2,), (1, 33, 65, 97, 128, 129, 200, 257)),
]


def _conv4_cases():
    """(form, C, N, precision).  The product is trimmed where two entries cross
    no different boundary: 64 clouds (the remapped grid) and 63 clouds (a
    remapped grid of 504) run a ragged and a full N each, one cloud (8
    workgroups) every N, 3 and 65 clouds (24 remapped, 260 not) every N."""
    out = []
    for kind, Cs, precs, Ns in _CONV4_TABLE:
        for C in Cs:
            some = [n for n in Ns if n in (33, 65, 128, 192, 200, 256)]
            for N in (some if C in (63, 64) else Ns):
                for p in precs:
                    out.append((conv4_form(C, N, p), C, N, p))
    return out


CONV4_CASES = _conv4_cases()
# the ReLU before the max (the T-Nets' conv3 + max), fp32 only
RELU_CASES = [(65, 65), (65, 200), (1, 33), (1, 97), (1, 200), (3, 33), (3, 97), (3, 200)]
# k_point_mlp: (C, N); every one in both precisions
MLP_CASES = [(1, 1), (2, 37), (3, 64), (3, 65), (1, 129),  # one tile per workgroup
             (1024, 64),    # two: the smallest even tile count
             (205, 320),    # two: 1025 tiles, the last workgroup holds one
             (342, 130),    # two: T = 3, workgroups pair tiles of different clouds, two-row ragged tiles
             (16, 4033)]    # two: a ragged 64th tile
# random (non-integer) data: (form, C, N, precision), one ragged and one full
# shape per form (the 128-point-step forms have no ragged shape: two full ones)
RANDOM_CASES = [("plain-fp32", 65, 200, 0), ("plain-fp32", 65, 192, 0),
                ("plain-bf16", 65, 200, 1), ("plain-bf16", 65, 192, 1),
                ("plain-bf16xb", 65, 200, 2), ("plain-bf16xb", 65, 192, 2),
                ("p128-bf16", 65, 128, 1), ("p128-bf16", 65, 384, 1),
                ("p128-bf16xb", 65, 128, 2), ("p128-bf16xb", 65, 384, 2),
                ("w16-fp32", 65, 128, 0), ("w16-fp32", 65, 384, 0),
                ("g2-fp32", 3, 200, 0), ("g2-fp32", 3, 128, 0),
                ("g2-bf16", 3, 200, 1), ("g2-bf16", 3, 128, 1),
                ("g4-bf16xb", 3, 200, 2), ("g4-bf16xb", 3, 256, 2)]
# the same 64 clouds in a 64-cloud (remapped) and a 65-cloud launch
XCD_CASES = [(200, 0), (200, 1), (200, 2), (256, 0), (256, 1), (256, 2)]


# ---------------------------------------------------------------------------
# the k_point_mlp integer generator
# ---------------------------------------------------------------------------
def _sparse(rng, rows, cols, hi):
    """Four non-zeros per row: +-1 .. +-hi."""
    w = np.zeros((rows, cols), np.float32)
    for r in range(rows):
        k = rng.choice(cols, 4, replace=False)
        w[r, k] = rng.integers(1, hi + 1, 4) * rng.choice([-1, 1], 4)
    return w


# magnitudes the ranges below cannot exceed: x1 <= 3 * 2 + 1, x2 <= 4 * 7 + 1,
# x3 <= 4 * 2 * 29 + 1 (an integer below 256: exact in bf16),
# |v| <= 128 * 2 * 233 + 2 < 2^17
MLP_BOUNDS = dict(x1=7, x2=29, x3=233, v=128 * 2 * 233 + 2)


@functools.lru_cache(maxsize=2)
def mlp_weights(seed=5):
    rng = np.random.default_rng(seed)
    w = dict(w1=rng.integers(-1, 2, (64, 3)).astype(np.float32), b1=rng.integers(-1, 2, 64).astype(np.float32),
             w2=_sparse(rng, 64, 64, 1), b2=rng.integers(-1, 2, 64).astype(np.float32),
             w3=_sparse(rng, 128, 64, 2), b3=rng.integers(-1, 2, 128).astype(np.float32),
             w4=rng.integers(-2, 3, (1024, 128)).astype(np.float32),
             b4=rng.integers(-2, 3, 1024).astype(np.float32))
    # the 125 distinct integer points and what the pipeline makes of each
    # (float64 on integers: exact)
    grid = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(125, 3).astype(np.float64)
    f = {k: a.astype(np.float64) for k, a in w.items()}
    x1 = np.maximum(grid @ f["w1"].T + f["b1"], 0)
    x2 = np.maximum(x1 @ f["w2"].T + f["b2"], 0)
    x3 = np.maximum(x2 @ f["w3"].T + f["b3"], 0)
    w["table"] = dict(x1=x1, x2=x2, x3=x3, v=x3 @ f["w4"].T + f["b4"])
    return w


def mlp_points(C, N, seed, distinct=8):
    """Integer points in [-2, 2], float32 [C][N][3]; a cloud draws its points
    from `distinct` of the 125 (so every cloud has tied maxima in most channels
    and a negative maximum in more than a tenth of them)."""
    rng = np.random.default_rng(seed)
    own = rng.integers(-2, 3, (C, distinct, 3))
    pick = rng.integers(0, distinct, (C, N))
    return own[np.arange(C)[:, None], pick].astype(np.float32)


def mlp_reference(pts, w):
    """x3 [C][N][128] float32 and numpy's max / first argmax of conv4 over the
    points, through the table of the 125 distinct points."""
    t = w["table"]
    code = ((pts[..., 0] + 2) * 25 + (pts[..., 1] + 2) * 5 + (pts[..., 2] + 2)).astype(np.int64)
    x3 = t["x3"].astype(np.float32)[code]
    C, N = code.shape
    gmax, gidx = np.empty((C, 1024), np.float32), np.empty((C, 1024), np.int64)
    for c in range(C):
        first = np.full(125, N, np.int64)
        np.minimum.at(first, code[c], np.arange(N))
        v = np.where((first < N)[:, None], t["v"], -np.inf)
        m = v.max(0)
        gmax[c] = m
        gidx[c] = np.where(v == m, first[:, None], N).min(0)
    return x3, gmax, gidx


# ---------------------------------------------------------------------------
# random data against float64
# ---------------------------------------------------------------------------
EPS = 2.0 ** -23
GAP_CAP = 0.02  # the largest share of (cloud, channel) pairs whose top two lie too close to call


def sum_bound(n, S):
    """gemm_ref.sum_bound: |f32 sum of n terms in any order - exact| <= (n + 8) 2^-23 sum|terms|."""
    return (n + 8) * EPS * np.asarray(S, np.float64)


@functools.lru_cache(maxsize=2)
def random_case(C, N, seed=None):
    """ReLU'd Gaussian x3, W4 and b4 ~ 0.1 N(0, 1); x3 also as its bf16 rounding."""
    rng = np.random.default_rng(31000 + 7 * C + N if seed is None else seed)
    x = np.maximum(rng.standard_normal((C, N, 128)), 0).astype(np.float32)
    W = (0.1 * rng.standard_normal((1024, 128))).astype(np.float32)
    b = (0.1 * rng.standard_normal(1024)).astype(np.float32)
    return dict(x=x, xb=bf16_round(x), W=W, b=b)


def random_stats(d, precision, gmax=None, gidx=None):
    """The float64 reference of a random case and, given a kernel's output,
    where it leaves the derived bounds.

    fp32 (precision 0): the value bound at a point is sum_bound(129, sum|x w| +
    |b|) (128 products and the bias in f32, any order); the screening error is
    E = 3 2^-16 sum|x w| + 2^-17 (|v| + |b|).  A true
    maximum that was screened out leaves two points screened above it, so the
    winner lies within 2 max_p E of it: the index is compared wherever the two
    best float64 values differ by at least that.
    bf16 (1, 2): the reference runs on the bf16-rounded x3 and W4; a point's
    bound is B = sum_bound(129, sum|x^ w^| + |b|) + 2^-17 (|v| + |b|), for the
    value and, doubled and taken at the cloud's worst point, for the index."""
    x = (d["x"] if precision == 0 else d["xb"]).astype(np.float64)
    W = (d["W"] if precision == 0 else bf16_round(d["W"])).astype(np.float64)
    b = d["b"].astype(np.float64)
    C, N, _ = x.shape
    out = dict(pairs=C * 1024, close=0, min_gap=np.inf, bad_value=0, bad_index=0, bad_miss=0,
               err_rel=0.0, miss_rel=0.0)
    for c in range(C):
        v = x[c] @ W.T + b
        S = np.abs(x[c]) @ np.abs(W).T
        vb = sum_bound(129, S + np.abs(b))
        trunc = 2.0 ** -17 * (np.abs(v) + np.abs(b))
        if precision == 0:
            E = 3 * 2.0 ** -16 * S + trunc
        else:
            E = vb + trunc
            vb = E
        thr = 2 * E.max(0)
        first = v.argmax(0)
        top = v.max(0)
        if N > 1:
            w = v.copy()
            w[first, np.arange(1024)] = -np.inf
            gap = top - w.max(0)
        else:
            gap = np.full(1024, np.inf)
        sure = gap >= thr
        out["close"] += int((~sure).sum())
        out["min_gap"] = min(out["min_gap"], float(gap.min()))
        if gmax is None:
            continue
        gi = np.asarray(gidx[c]).astype(np.int64)
        inside = (gi >= 0) & (gi < N)
        gi = np.where(inside, gi, 0)
        o = np.arange(1024)
        err = np.abs(np.asarray(gmax[c], np.float64) - v[gi, o])
        miss = top - v[gi, o]
        out["bad_value"] += int((~inside | ~(err <= vb[gi, o])).sum())
        out["bad_index"] += int((sure & (gi != first)).sum())
        out["bad_miss"] += int((miss > thr + 2 * vb.max(0)).sum())
        out["err_rel"] = max(out["err_rel"], float((err / S[gi, o]).max()))
        out["miss_rel"] = max(out["miss_rel"], float((miss / S[gi, o]).max()))
    out["share"] = out["close"] / out["pairs"]
    return out

"""The case tables and generators of tests/feat_fwd_cases.py, checked on the
CPU: the restated dispatch against the constants of csrc/feat_fused.hip, the
tables against the forms and planted patterns they are meant to reach, the
generated arrays against the conditions the exact comparison relies on, the
comparison against each slip it is there to notice, and the random cases
against the cap on the pairs too close to call.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import feat_fwd_cases as fc

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "adversarial_learning_on_pointclouds_amd", "csrc", "feat_fused.hip")
UNIT_CASES = sorted({(fc.form_kind(f), C, N) for f, C, N, _ in fc.CONV4_CASES})
UNIT_FORMS = [f for f in fc.CONV4_FORMS if f != "w16-fp32"]
W16_CASES = [(64, 128), (64, 256), (64, 384)]  # tests/test_gpu_conv4_w16.py


def _id(c):
    return "-".join(str(v) for v in c)


# ---------------------------------------------------------------------------
# the dispatch and the tables
# ---------------------------------------------------------------------------
def test_constants_are_the_sources():
    src = open(SRC).read()

    def const(name):
        m = re.search(rf"constexpr int {name} = (\d+);", src)
        assert m, name
        return int(m.group(1))
    assert const("C4_G2_MAXC") == fc.C4_G2_MAXC == 63
    assert const("PM_ONE_BELOW") == fc.PM_ONE_BELOW == 1024
    assert const("PM_P") == fc.PM_P == 64
    assert const("C4_CB") == fc.C4_CB == 256
    assert const("C4_O") == fc.C4_O == 1024
    # the dispatch's own lines
    assert "if (C <= C4_G2_MAXC && !stamps)" in src and "else if (N % 128 == 0 && !stamps)" in src
    assert "const bool one = ntiles < PM_ONE_BELOW && !stamps;" in src
    assert "constexpr int P = G2 ? 32 * NGRP : 32 * UPS;" in src
    assert "return G2 ? (XB ? 4 : 2) : 1;" in src
    assert "if ((nwg & 7) == 0)" in src


def test_dispatch_by_hand():
    assert fc.conv4_form(63, 128, 0) == "g2-fp32" and fc.conv4_form(63, 128, 2) == "g4-bf16xb"
    assert fc.conv4_form(64, 128, 0) == "w16-fp32" and fc.conv4_form(64, 129, 0) == "plain-fp32"
    assert fc.conv4_form(64, 256, 1) == "p128-bf16" and fc.conv4_form(64, 256, 2) == "p128-bf16xb"
    assert fc.conv4_form(64, 64, 1) == "plain-bf16" and fc.conv4_form(1, 1, 1) == "g2-bf16"
    assert fc.conv4_grid(64, 200, 0) == (256, True) and fc.conv4_grid(65, 200, 0) == (260, False)
    assert fc.conv4_grid(3, 200, 0) == (24, True)
    g = fc.geometry("g4-bf16xb", 129)  # two steps of 128: unit 4 is group 0's, groups 1-3 have none
    assert (g["P"], g["ups"], g["U"], g["S"], g["past"]) == (128, 4, 5, 2, [1, 2, 3])
    g = fc.geometry("g2-fp32", 97)     # units 0-3: none past
    assert (g["S"], g["U"], g["past"]) == (2, 4, [])
    assert fc.geometry("g2-fp32", 65)["past"] == [1] and fc.geometry("plain-fp32", 65)["past"] == []
    assert fc.mlp_form(16, 4033, 0) == dict(inst="k_point_mlp<6, 2, false>", tpw=2, T=64, ntiles=1024, grid=512)
    assert fc.mlp_form(205, 320, 1)["grid"] == 513 and fc.mlp_form(205, 320, 1)["ntiles"] == 1025
    assert fc.mlp_form(3, 65, 1)["inst"] == "k_point_mlp<1, 1, false>"


def test_every_instantiation_is_reached():
    """Each k_conv4_max form and each non-gather k_point_mlp form by at least
    two rows; every row runs the form it names; S = 1, S = 2 and a reused
    buffer in every form."""
    rows = {f: [] for f in fc.CONV4_FORMS}
    for f, C, N, p in fc.CONV4_CASES:
        assert fc.conv4_form(C, N, p) == f
        rows[f].append((C, N))
    for C, N in W16_CASES:
        rows[fc.conv4_form(C, N, 0)].append((C, N))
    assert len(rows) == 9 and all(len(v) >= 2 for v in rows.values()), rows
    for f, v in rows.items():
        steps = {fc.geometry(f, N)["S"] for _, N in v}
        assert {1, 2} <= steps and max(steps) >= 3, (f, steps)
    for f, C, N, p in fc.RANDOM_CASES:
        assert fc.conv4_form(C, N, p) == f
    assert {f for f, *_ in fc.RANDOM_CASES} == set(fc.CONV4_FORMS)
    for C, N in fc.RELU_CASES:
        assert fc.conv4_form(C, N, 0) in ("plain-fp32", "g2-fp32")
    for N, p in fc.XCD_CASES:
        assert fc.conv4_form(64, N, p) == fc.conv4_form(65, N, p)
        assert fc.conv4_grid(64, N, p)[1] and not fc.conv4_grid(65, N, p)[1]
    mlp = {}
    for C, N in fc.MLP_CASES:
        for p in (0, 1):
            mlp.setdefault(fc.mlp_form(C, N, p)["inst"], []).append((C, N))
    assert set(mlp) == set(fc.MLP_FORMS.values()) and all(len(v) >= 2 for v in mlp.values())
    # the two-tile shapes: an even tile count, an odd one, tiles of two clouds
    # in one workgroup with a ragged tile per cloud, a ragged 64th tile
    f = lambda C, N: fc.mlp_form(C, N, 0)
    assert f(1024, 64)["ntiles"] == 1024 and f(205, 320)["ntiles"] % 2 == 1
    assert f(342, 130)["T"] == 3 and 130 % 64 == 2 and f(16, 4033)["T"] == 64 and 4033 % 64 == 1
    assert max(C * N for C, N in fc.MLP_CASES) * 128 * 4 <= 34e6


def test_every_pattern_is_planted():
    """Each pattern a form's geometry has a place for sits in at least one of
    the form's cases, and a wave group with no valid unit in the last step
    occurs in every wave-group form."""
    for form in UNIT_FORMS:
        want, have, past = set(), set(), False
        for f, C, N, _ in fc.CONV4_CASES:
            if f != form:
                continue
            want |= set(fc.applicable_patterns(form, N))
            d = fc.unit_integer_case(form, C, N)
            have |= {n for nm in d["names"] for n in nm.values()}
            past |= bool(d["geom"]["past"])
        assert want <= have, (form, want - have)
        ngrp = fc.CONV4_FORMS[form]["NGRP"]
        assert past == (ngrp > 1), form
        assert {"last", "first_last", "halves", "lane3", "steps_even", "steps_odd"} <= want
        assert ("units" in want) == (ngrp == 1)
        assert ({"groups_up", "groups_down", "own_g1"} <= want) == (ngrp > 1)
        assert ("own_g3" in want) == (ngrp == 4)
        if form_has_ragged(form):
            assert {"ragged_first", "full_last"} <= want


def form_has_ragged(form):
    return fc.form_kind(form) != "p128"


# ---------------------------------------------------------------------------
# the conv4 integer generator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", UNIT_CASES, ids=_id)
def test_conv4_integer_case_conditions(case):
    kind, C, N = case
    d = fc._unit_case(kind, C, N)
    x, W, b = d["x"], d["W"], d["b"]
    for a in (x, W, b):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= 4
        assert np.array_equal(fc.bf16_round(a), a)  # the bf16 forms round nothing away
        assert torch.equal(torch.from_numpy(a).bfloat16().float(), torch.from_numpy(a))
    v = fc.conv4_values(d)
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() < 2 ** 12 < 2 ** 17
    assert np.array_equal(v.max(1), d["gmax"]) and np.array_equal(v.argmax(1), d["gidx"])
    assert (d["gmax"] < 0).sum() > 100 and (d["gmax"] > 0).sum() > 100
    if (C, N) in fc.RELU_CASES:
        assert (d["gmax"] <= 0).sum() > 100
    pw = fc.pattern_of_winner(d)
    assert (pw != "").mean() >= 0.9, (pw != "").mean()
    # every tie pattern present decides channels: numpy's first and last argmax differ there
    decided = (N - 1 - v[:, ::-1].argmax(1)) != d["gidx"]
    for name in {n for nm in d["names"] for n in nm.values()} & set(fc.TIE_PATTERNS):
        assert ((pw == name) & decided).sum() >= 20, (name, ((pw == name) & decided).sum())
    # the planted unique winners win: point N - 1 in cloud 0, and a point of every other group
    for k, name in d["names"][0].items():
        if name == "last" or name.startswith("own_g"):
            p = int(np.flatnonzero(d["which"][0] == k)[0])
            assert (d["gidx"][0] == p).sum() >= 20, (name, p)


@pytest.mark.parametrize("N", [128, 256, 384])
def test_w16_integer_case_conditions(N):
    x, W, b, gmax, gidx = fc.w16_integer_case(N, 700 + N)
    v = x.astype(np.float64) @ W.astype(np.float64).T + b
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() < 2 ** 12
    assert np.array_equal(v.max(1), gmax) and np.array_equal(v.argmax(1), gidx)
    assert (gmax < 0).sum() > 100 and (gmax > 0).sum() > 100 and (gmax <= 0).sum() > 100


# ---------------------------------------------------------------------------
# sensitivity: each slip, applied to the reference, is noticed by every case
# that has a place for it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", UNIT_CASES, ids=_id)
def test_exact_comparison_notices_each_slip(case):
    kind, C, N = case
    d = fc._unit_case(kind, C, N)
    assert fc.mismatches(d["gmax"], d["gidx"], d["gmax"], d["gidx"]) == 0
    g = d["geom"]
    slips = [("drop_last", None), ("last_on_ties", None), ("empty_as_zero", None)]
    slips += [("drop_group", k) for k in range(1, g["NGRP"])]
    for how, k in slips:
        r = fc.corrupt(d, how, k)
        if how == "drop_last":
            assert r is not None
        if how == "last_on_ties":
            assert (r is None) == (N == 1)
        if how == "drop_group":
            assert (r is None) == (k >= g["U"])
        if how == "empty_as_zero":
            assert (r is None) == (not g["past"] and N >= 5)
        if r is not None:
            assert fc.mismatches(r[0], r[1], d["gmax"], d["gidx"]) >= 20, (how, k)
    if (C, N) in fc.RELU_CASES:  # the ReLU'd reference differs from the plain one
        rm, ri = fc.relu_reference(d["gmax"], d["gidx"])
        assert fc.mismatches(rm, ri, d["gmax"], d["gidx"]) > 100


# ---------------------------------------------------------------------------
# the k_point_mlp integer generator
# ---------------------------------------------------------------------------
def test_mlp_integer_generator_conditions():
    w = fc.mlp_weights()
    t = w["table"]
    for k in ("w1", "b1", "b2", "b3"):
        assert np.abs(w[k]).max() <= 1 and np.array_equal(w[k], np.round(w[k]))
    assert ((w["w2"] != 0).sum(1) == 4).all() and np.abs(w["w2"]).max() == 1
    assert ((w["w3"] != 0).sum(1) == 4).all() and np.abs(w["w3"]).max() == 2
    assert np.abs(w["w4"]).max() <= 2 and np.abs(w["b4"]).max() <= 2
    for k in ("x1", "x2", "x3", "v"):
        assert np.array_equal(t[k], np.round(t[k])) and np.abs(t[k]).max() <= fc.MLP_BOUNDS[k], k
    assert fc.MLP_BOUNDS["x3"] < 256 and fc.MLP_BOUNDS["v"] < 2 ** 17
    for k in ("x2", "x3"):  # what bf16 mode rounds
        a = t[k].astype(np.float32)
        assert np.array_equal(fc.bf16_round(a), a)
    for k in ("w3", "w4"):
        assert np.array_equal(fc.bf16_round(w[k]), w[k])
    print("largest x1, x2, x3, |v|:", [float(np.abs(t[k]).max()) for k in ("x1", "x2", "x3", "v")])
    assert (t["x3"] != 0).mean() >= 0.25
    for C, N in fc.MLP_CASES[:5] + [(342, 130)]:
        pts = fc.mlp_points(C, N, 40 + C + N)
        x3, gmax, gidx = fc.mlp_reference(pts, w)
        assert (x3 != 0).mean() >= 0.25
        assert (gmax < 0).sum() > 100 and (gmax > 0).sum() > 100, (C, N)
    # the table look-up is the plain computation
    pts = fc.mlp_points(3, 65, 108)
    x3, gmax, gidx = fc.mlp_reference(pts, w)
    f = {k: w[k].astype(np.float64) for k in ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")}
    h = np.maximum(pts.astype(np.float64) @ f["w1"].T + f["b1"], 0)
    h = np.maximum(h @ f["w2"].T + f["b2"], 0)
    h = np.maximum(h @ f["w3"].T + f["b3"], 0)
    v = h @ f["w4"].T + f["b4"]
    assert np.array_equal(h, x3) and np.array_equal(v.max(1), gmax) and np.array_equal(v.argmax(1), gidx)
    # integer points give few distinct rows: the first-index rule decides many channels
    assert ((65 - 1 - v[:, ::-1].argmax(1)) != gidx).mean() > 0.25


# ---------------------------------------------------------------------------
# random data: the cap on the pairs too close to call, from the reference alone
# ---------------------------------------------------------------------------
def test_bf16_round_is_torchs():
    a = np.random.default_rng(3).standard_normal(4096).astype(np.float32)
    a[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]  # ties: to even
    assert np.array_equal(fc.bf16_round(a), torch.from_numpy(a).bfloat16().float().numpy())


@pytest.mark.parametrize("case", fc.RANDOM_CASES, ids=_id)
def test_random_cases_stay_under_the_cap(case):
    form, C, N, p = case
    s = fc.random_stats(fc.random_case(C, N), p)
    print(f"{_id(case)}: {s['close']} of {s['pairs']} pairs too close ({100 * s['share']:.3f} %), "
          f"smallest gap {s['min_gap']:.3e}")
    assert s["share"] <= fc.GAP_CAP

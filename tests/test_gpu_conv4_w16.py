"""k_conv4_max<3, C4W16>: fp32 mode's conv4 + max at 64 clouds or more and
N % 128 == 0 (16 waves of 16 channels on 16x16x32 MFMAs, 128-point steps,
top-2 keys per 64-point span, four lanes per channel).  The
smallest shapes that reach every path are C = 64 with N = 128 (one step: the
prologue straight into the last screen), 256 (both LDS buffers) and 384 (a
buffer reused).

On small integers every split product and partial sum is exact and the key
truncation drops only zero bits, so gmax / gidx must equal numpy's max and
first argmax with no tolerance.  The generator of the integer case is
tests/feat_fwd_cases.py's (w16_integer_case), which also holds the cases of the
other eight forms (tests/test_gpu_feat_fwd_edges.py).  Runs on an MI355X only."""
import numpy as np
import pytest
import torch

import feat_fwd_cases as fc
from oracle import pointnet_np as onp

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from adversarial_learning_on_pointclouds_amd import ops

DEV = "cuda"
C = 64  # the fewest clouds that run 256-channel workgroups


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# the integer case (five distinct rows per cloud, equal values planted by
# structural position) lives with the other forms' generators
_integer_case = fc.w16_integer_case


@pytest.fixture(scope="module", params=[128, 256, 384])
def integer_case(request):
    return _integer_case(request.param, 700 + request.param)


def test_integers_exact(integer_case):
    """gmax and gidx equal numpy's max and first argmax on every channel:
    equal winners within a 16-point tile (rows of different lane quarters),
    across the tiles of a 64-point span, across the spans of a step and across
    steps; channels with a negative maximum included (the key order below
    zero)."""
    x, W, b, rg, ri = integer_case
    assert (rg < 0).sum() > 100 and (rg > 0).sum() > 100  # both signs are exercised
    gmax, gidx = ops.conv4_max(_t(x), _t(W), _t(b))
    gmax, gidx = gmax.cpu().numpy(), gidx.cpu().numpy()
    bad = np.argwhere((gidx != ri) | (gmax != rg))
    print(f"N={x.shape[1]}: {len(bad)} of {gidx.size} channels differ")
    assert len(bad) == 0, [(c, o, gidx[c, o], ri[c, o], gmax[c, o], rg[c, o]) for c, o in bad[:8]]


def test_integers_relu_all_nonpositive_rows(integer_case):
    """conv_max_fwd at K = 128, O = 1024 runs k_conv4_max with the ReLU before
    the max: channels whose values are all <= 0 give gmax 0 at index 0, the
    others are unchanged."""
    x, W, b, rg, ri = integer_case
    dead = rg <= 0
    assert dead.sum() > 100
    gmax, gidx = ops.conv_max_fwd(_t(x), _t(W), _t(b), relu_before_max=True)
    gmax, gidx = gmax.cpu().numpy(), gidx.cpu().numpy()
    assert (gmax[dead] == 0).all() and (gidx[dead] == 0).all()
    assert (gmax[~dead] == rg[~dead]).all() and (gidx[~dead] == ri[~dead]).all()


@pytest.mark.parametrize("N", [128, 384])
def test_bitwise_against_two_group_form(N):
    """Clouds 0..31 of a 64-cloud launch (the 128-point-step form) equal a
    32-cloud launch of the same clouds, and cloud 5 alone (the two-group form):
    the exact re-evaluation of the same top two gives the same bits whatever
    screened them."""
    g = torch.Generator().manual_seed(4100 + N)
    x3 = torch.randn(C, N, 128, generator=g).relu().to(DEV)
    x3[5, N // 2:] = x3[5, 0]  # ties across spans and steps
    W = (torch.randn(1024, 128, generator=g) * 0.1).to(DEV)
    b = (torch.randn(1024, generator=g) * 0.1).to(DEV)
    g64, i64 = ops.conv4_max(x3, W, b)
    g32, i32 = ops.conv4_max(x3[:32].contiguous(), W, b)
    print(f"N={N}: {(i64[:32] != i32).sum().item()} gidx, "
          f"{(g64[:32] != g32).sum().item()} gmax of {i32.numel()} differ")
    assert torch.equal(i64[:32], i32) and torch.equal(g64[:32], g32)
    g1, i1 = ops.conv4_max(x3[5:6].contiguous(), W, b)
    assert torch.equal(i64[5:6], i1) and torch.equal(g64[5:6], g1)


def test_conv4_max_alone_equals_feat_fwd():
    """conv4_max on feat_fwd's own x3 at (C, N) = (64, 128) gives feat_fwd's
    gmax / gidx bitwise."""
    G = onp.make_params(onp.cls_spec(40), seed=61)
    names = ["feat.conv1.weight", "feat.conv1.bias", "feat.conv2.weight", "feat.conv2.bias",
             "feat.conv3.weight", "feat.conv3.bias", "feat.conv4.weight", "feat.conv4.bias"]
    w = [_t(G[n]) for n in names]
    pts = np.random.default_rng(77).uniform(-1, 1, (C, 128, 3)).astype(np.float32)
    gmax, gidx, x3 = ops.feat_fwd(_t(pts), *w)
    g2, i2 = ops.conv4_max(x3, w[6], w[7])
    assert torch.equal(gmax, g2) and torch.equal(gidx, i2)

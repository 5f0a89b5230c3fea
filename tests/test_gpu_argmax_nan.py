"""The NaN half of the argmax order (csrc/prims.h, ranks_before): a NaN ranks
above every number, +inf included, and among NaNs the first index wins, as
np.argmax and torch.max give.  Checked on the two kernels that turn logits into
labels, pcadv_row_eval (pred) and pcadv_row_semi_ce (labels); the tie half is
test_ties_take_the_first_index in their own files.  MI355X only."""
import numpy as np
import pytest

from test_gpu_row_eval import _call as _eval_call
from test_gpu_row_semi import _call as _semi_call

pytestmark = pytest.mark.gpu

# sixteen lanes hold four classes each: 7 leaves lane 1 a partial group, 48
# floats per row of 40 classes is a stride wider than the row, 64 fills all lanes
SHAPES = [(7, 7), (40, 48), (50, 50), (64, 64)]
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _rows(ncls, ld):
    rng = np.random.default_rng(ncls + ld)
    x = rng.uniform(-4, 4, (8, ld)).astype(np.float32)
    x[:, ncls:] = 1e30  # columns past ncls are not the row's
    mid = ncls // 2
    x[0, 0] = NAN                          # the first class
    x[1, ncls - 1] = NAN                   # the last class
    x[2, mid], x[2, mid + 1] = NAN, 9.0    # the middle, a larger finite value after it
    x[3, 2], x[3, ncls - 2] = NAN, NAN     # two lanes' groups
    x[4, 4], x[4, 6] = NAN, NAN            # one group of four
    x[5, 1], x[5, 5] = INF, NAN            # +inf before the NaN
    x[6, :ncls] = NAN                      # nothing but NaN
    want = [0, ncls - 1, mid, 2, 4, 5, 0]  # row 7: no NaN
    ref = np.argmax(x[:, :ncls], axis=1)
    assert ref[:7].tolist() == want and not np.isnan(x[7]).any()
    return x, ref


@pytest.mark.parametrize("ncls,ld", SHAPES)
def test_row_eval_pred_takes_the_first_nan(ncls, ld):
    x, ref = _rows(ncls, ld)
    y = np.where(np.arange(8) % 2 == 0, ref, (ref + 1) % ncls)  # half right, half wrong
    pred, acc, _, _, _ = _eval_call(x, y, ncls)
    print(f"ncls={ncls} ld={ld}: pred {pred.tolist()} np.argmax {ref.tolist()} right {acc[0]}")
    assert np.array_equal(pred, ref)
    assert acc[0] == float(np.sum(ref == y)) == 4.0


@pytest.mark.parametrize("ncls,ld", SHAPES)
def test_row_semi_labels_take_the_first_nan(ncls, ld):
    x, ref = _rows(ncls, ld)
    _, lab, _, K = _semi_call(x, np.ones(8, np.float32), 0.5, 1.0, ncls)  # every row kept
    print(f"ncls={ncls} ld={ld}: labels {lab.tolist()} np.argmax {ref.tolist()} kept {K}")
    assert K == 8
    assert np.array_equal(lab, ref)

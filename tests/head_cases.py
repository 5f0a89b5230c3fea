"""The cases of tests/test_gpu_head_edges.py (the fused step's head and
discriminator tail on given pooled features), shared with the CPU checks of
tests/test_head_ref.py: batch sizes, parameters and inputs."""
import functools

import numpy as np

from oracle import pointnet_np as onp

# B: C = 2B generator rows, R = 3B discriminator rows, 16-row blocks
#   1   one partial block everywhere; means over one row
#   3
#   6   2B = 12 splits a block; R = 18 leaves a two-row block
#   8   chained conv1 input gradient (2B % 16 == 0), an eight-row last tile
#   9   a two-row second head block
#   24  chained; 72 rows end mid-tile
#   33  66 weight-gradient rows: the 64 / 65 switch of wgrad.h
#   65  130 rows: a second 128-row slab of two rows
#   256 the ABI's maximum (chained)
ADV_B = (1, 3, 6, 8, 9, 24, 33, 65, 256)
CLS_B = (1, 15, 17, 64, 65, 129, 256)
SEMI_B = (6, 24)       # one unchained and one chained batch
DRAWN_B = (9, 24)
MAX_B = 256
HP = dict(lambda_cls=1.0, lambda_adv=0.001, lambda_semi=1.0, semi_th=0.8)


@functools.lru_cache(maxsize=None)
def params():
    """(G, D): the oracle's generator and discriminator parameters."""
    return (onp.make_params(onp.cls_spec(40), seed=1),
            onp.make_params(onp.disc_spec(40, 1), seed=2, init="xavier"))


def adv_inputs(B, p):
    """Pooled features of the 2B clouds, labels, explicit dropout masks and
    soft D labels (make_D_label's ranges)."""
    rng = np.random.default_rng(1000 + B)
    return dict(gmax=(0.5 * rng.standard_normal((2 * B, 1024))).astype(np.float32),
                labels=rng.integers(0, 40, B).astype(np.int64),
                mask=(rng.random((2 * B, 256)) >= p).astype(np.float32),
                soft_gt=rng.uniform(0.7, 1.05, B).astype(np.float32),
                soft_nogt=rng.uniform(0.0, 0.305, B).astype(np.float32))


def cls_inputs(B, p):
    rng = np.random.default_rng(2000 + B)
    return dict(gmax=(0.5 * rng.standard_normal((B, 1024))).astype(np.float32),
                labels=rng.integers(0, 40, B).astype(np.int64),
                mask=(rng.random((B, 256)) >= p).astype(np.float32))

"""Inputs shared by tests/test_stackdisc_ref.py (CPU) and
tests/test_gpu_stackdisc.py: the kernel shapes and their seeded weights, logits,
soft labels and shape labels."""
import numpy as np

import stackdisc_ref as ref

# (GT rows, no-GT rows, ncls, row stride, max workgroups, points per cloud): one
# row, a tile less one + one, two full tiles, a ragged tile that straddles the
# ranges with clouds of 13 points straddling a 64-row tile, several tiles per
# persistent workgroup, narrow inputs, a padded row stride
SHAPES = [(1, 0, 50, 50, 0, 1), (0, 1, 50, 50, 0, 1), (63, 1, 50, 50, 0, 9), (64, 64, 50, 50, 0, 32),
          (65, 200, 50, 50, 0, 13), (300, 700, 50, 50, 3, 50), (65, 200, 16, 16, 0, 13),
          (65, 200, 3, 3, 0, 13), (65, 200, 50, 56, 2, 13)]
# (shape, num_shapes): every shape with the reference's 16, one with 5
CASES = [(s, 16) for s in SHAPES] + [((65, 200, 50, 50, 0, 13), 5)]
LAMBDA_SHAPE, LAMBDA_ADV = 0.5, 0.37


def _xavier(rng, o, k):
    return (rng.standard_normal((o, k, 1)) * np.sqrt(2.0 / (o + k))).astype(np.float32)


def make_params(rng, ncls, num_shapes=16, bias_std=0.0):
    """init_type "xavier" of the reference (utils/model_utils.py:27-58)."""
    p = []
    for o, k in ((64, ncls), (64, 64), (64, 64), (128, 64), (num_shapes, 1)):
        p += [_xavier(rng, o, k), (rng.standard_normal(o) * bias_std).astype(np.float32)]
    return p


def make_inputs(shape, num_shapes=16):
    """One case's inputs: logits 2 randn, xavier weights with zero biases, soft
    labels up to 1.05 (one exactly 1.05), one shape label per GT cloud."""
    n0, n1, ncls, ld, _, ppc = shape
    rng = np.random.default_rng(2000 + 7 * n0 + n1 + 31 * ncls + ld + 1000 * num_shapes)
    lg = (2.0 * rng.standard_normal((n0 + n1, ncls))).astype(np.float32)
    params = make_params(rng, ncls, num_shapes)
    soft0 = rng.uniform(0.7, 1.05, n0).astype(np.float32)
    if n0:
        soft0[n0 // 2] = np.float32(1.05)
    soft1 = rng.uniform(0.0, 0.305, n1).astype(np.float32)
    labels = rng.integers(0, num_shapes, n0 // ppc).astype(np.int32)
    x0 = np.concatenate([ref.transform(lg[:n0], ref.SOFTMAX), ref.transform(lg[n0:], ref.LOG_SOFTMAX)])
    return dict(lg=lg, params=params, soft0=soft0, soft1=soft1, labels=labels, x0=x0)

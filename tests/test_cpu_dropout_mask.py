"""The numpy restatement of the dropout hash (tests/dropout_util.py) on the CPU: it agrees with a scalar, plain-integer
statement of csrc/common.h's dropout_keep, and for the seeds the attention-softmax tests use its own drop rate over
the L x L scores lies within 0.02 of p (a condition on those tests' inputs, not on the kernel)."""
import numpy as np
import pytest

from dropout_util import keep_mask, row_keep, score_keep
from test_gpu_bert_kernels import EMB_SEED, LN_SEED, SOFTMAX_CASES, SOFTMAX_P, softmax_drop_rate

M32 = 0xFFFFFFFF


def keep_scalar(seed, idx, p):
    if p <= 0:
        return True
    h = ((idx & M32) * 0x9E3779B1 & M32) ^ (seed & M32)
    h = (h + (seed >> 32)) & M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return np.float32(h >> 8) * np.float32(1.0 / 16777216.0) >= np.float32(p)


@pytest.mark.parametrize("seed", [0, 1234, EMB_SEED, LN_SEED, 2**64 - 1])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_keep_mask_matches_scalar_hash(seed, p):
    idx = np.concatenate([np.arange(300), np.array([2**31 - 1, 2**31, 2**32 - 1, 2**32 + 5])])
    want = np.array([keep_scalar(seed, int(i), p) for i in idx])
    assert np.array_equal(keep_mask(seed, idx, p), want)


def test_index_spaces():
    assert np.array_equal(row_keep(7, 5, 12, 0.5).ravel(), keep_mask(7, np.arange(60), 0.5))
    assert np.array_equal(score_keep(7, 2, 3, 4, 0.5)[1, 2, 3], keep_mask(7, np.array([(1 * 3 + 2) * 4 + 3]), 0.5)[0])


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: str(c[:4]))
def test_softmax_seeds_drop_rate(case):
    assert abs(softmax_drop_rate(case) - SOFTMAX_P) < 0.02


@pytest.mark.parametrize("seed,p", [(EMB_SEED, 0.1), (LN_SEED, 0.1), (LN_SEED, 0.5)])
def test_hidden_dropout_seeds_drop_rate(seed, p):
    assert abs(1.0 - row_keep(seed, 37, 768, p).mean() - p) < 0.02

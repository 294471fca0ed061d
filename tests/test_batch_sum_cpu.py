"""The shared batch sum without a GPU: the float32 emulation of tests/batch_sum_ref.py (the order tests/test_batch_sum_gpu.py
holds the kernels of tf-mpc_amd/csrc/batch_sum.h to, bit for bit) against the fp64 sum and a hand-worked case, and the
workspace layout of the two entry points that use it against its formula."""
import numpy as np
import pytest

import batch_sum_ref as ref
from tfmpc import _hip

U32 = 2.0 ** -24                  # fp32 unit roundoff


@pytest.mark.parametrize("B", [1, 3, 4, 63, 64, 65, 131, 259, 300, 64 * 257 + 1])
@pytest.mark.parametrize("order", ["steady state", "riccati"])
def test_emulated_orders_are_sums(order, B):
    """Any fp32 order of B terms is within the sequential sum's bound (B - 1) u sum|x| of the exact sum."""
    x = np.random.default_rng(B).normal(size=(B, 7)).astype(np.float32)
    got = (ref.steady_state_sum if order == "steady state" else ref.riccati_sum)(x)
    assert got.dtype == np.float32 and got.shape == (7,)
    exact = x.astype(np.float64).sum(0)
    bound = (B - 1) * U32 * np.abs(x.astype(np.float64)).sum(0)
    assert (np.abs(got - exact) <= bound).all(), (order, B, np.abs(got - exact).max(), bound.min())


def test_more_chunks_than_tree_threads_take_the_strided_sums():
    """259 chunks: threads 0, 1, 2 of the tree add two chunks each (k and k + 256) before the tree."""
    partial = np.zeros((259, 1), np.float32)
    partial[0], partial[256], partial[1] = 2.0 ** 24, 1.0, 1.0
    # thread 0: (0 + 2^24) + 1 = 2^24 (the tie rounds to even); thread 1: 1; the tree adds them at w = 1: 2^24 + 1 = 2^24
    assert ref.stage2_tree(partial)[0] == np.float32(16777216.0)
    # in order: ((2^24 + 1) -> 2^24, ... then chunk 256: + 1 -> 2^24
    assert ref.stage2_in_order(partial)[0] == np.float32(16777216.0)
    partial[1], partial[257] = 1.0, 1.0
    # thread 1: 1 + 1 = 2, and 2^24 + 2 is exact; in order every + 1 is lost to 2^24
    assert ref.stage2_tree(partial)[0] == np.float32(16777218.0)
    assert ref.stage2_in_order(partial)[0] == np.float32(16777216.0)


def test_hand_worked_eleven_records_in_chunks_of_four():
    """Chunks [0, 4), [4, 8), [8, 11).  With H = 2^24, where H + 1 rounds back to H:
      chunk 0: s = [H, 1, 1, -H]          -> (H + 1) + (1 - H) = H - (H - 1) = 1          (one after the other: 0; exactly: 2)
      chunk 1: s = [1, H, -H, 1]          -> (1 + H) + (-H + 1) = H - (H - 1) = 1
      chunk 2: the tail of three goes to s[0], s[1], s[2]: s = [1, 1, H, 0]
                                          -> (1 + 1) + (H + 0) = H + 2, exact             (s[0] = 1 + H, s[1] = 1: H)
    Stage 2 in order: ((0 + 1) + 1) + (H + 2) = H + 4, exact.  The tree adds t[0] + t[2] = 1 + (H + 2) = H + 3 -> H + 4
    (tie to even) at w = 2, then + t[1] = H + 5 -> H + 4 at w = 1."""
    H = 2.0 ** 24
    rec = np.array([H, 1, 1, -H, 1, H, -H, 1, 1, 1, H], np.float32).reshape(11, 1)
    partial = ref.stage1(rec, 4)
    assert partial.shape == (3, 1)
    assert partial[:, 0].tolist() == [1.0, 1.0, 16777218.0]
    assert ref.stage2_in_order(partial)[0] == np.float32(16777220.0)
    assert ref.stage2_tree(partial)[0] == np.float32(16777220.0)
    # two columns keep their own sums
    both = ref.stage1(np.concatenate([rec, rec[::-1]], axis=1), 4)
    assert both[:, 0].tolist() == [1.0, 1.0, 16777218.0]
    # reversed: [H, 1, 1, 1] -> (H + 1) + 2 = H + 2; [-H, H, 1, -H] -> 0 + (1 - H) = 1 - H; [1, 1, H, 0] -> H + 2
    assert both[:, 1].tolist() == [16777218.0, -16777215.0, 16777218.0]


SHAPES = [(5, 3), (16, 8), (20, 10)]


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("B", [2, 64, 65, 300])
def test_steady_state_vjp_workspace_is_the_plan(B, n, m):
    assert _hip.load().tfmpc_lqr_steady_state_vjp_workspace_bytes(B, n, m) == ref.steady_state_workspace_bytes(B, n, m)


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("B", [2, 256, 257])
def test_riccati_vjp_workspace_is_the_plan(B, n, m):
    T = 3
    assert _hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes(B, n, m, T) == ref.riccati_workspace_bytes(B, n, m, T)

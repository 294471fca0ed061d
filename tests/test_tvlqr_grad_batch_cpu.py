"""The oracles of tests/test_tvlqr_grad_batch_gpu.py without a GPU (tests/tvlqr_grad_batch_ref.py): for every case of
that file the reference alone must sit comfortably inside what the kernels are held to, and the budget must tell a
one-instance error from rounding.

* the fp32 closed form, summed over the batch in fp32 (plain sequential order, and the order of the matrix-core
  reduction's df / dc lane sums: chunks of 256, four interleaved running sums), has ratio <= 1 under the project budget;
* dropping (or doubling) a single instance of the fp64 sum misses that budget by at least 100x for the typical (median)
  instance and for the instances at the chunk edges (first, last, either side of the last chunk's start), and by at
  least 25x -- ten times the 2.5 the GPU file allows a sum -- for EVERY instance, so a reduction that loses, repeats
  or misplaces one instance cannot pass the GPU file.  (The budget is the host's own fp32 error: between two hosts it
  moved by 3x on one case, so the all-instance minimum is not held to the 100x of the typical one.);
* both fp32 orders differ from the fp64 sum of the same fp32 terms by at most half of (B + 8) 2^-24 M, M the summed
  magnitudes of the terms: the consistency bound of the GPU file, 2 (B + 8) 2^-24 M, leaves a factor four;
* the control-limited cases hold every control at some instance and free it at another, and the all-held rollout stays
  bounded.
"""
import numpy as np
import pytest
import torch

import tvlqr_grad_batch_ref as batch

SEPARATION = 100.0           # the typical instance and the chunk-edge instances
EVERY_INSTANCE = 25.0        # ten times the median <= 2.5 a summed gradient is held to


@pytest.mark.parametrize("case", batch.CASES, ids=batch.case_id)
def test_the_fp32_reference_is_inside_the_budget_and_one_instance_is_far_outside(case):
    n, m, T, B, sharing = case
    user, full, w = batch.problem(*case)
    g64, budget = batch.oracle(*case)
    names = batch.summed_names(user, full)
    assert names, case
    t32 = batch.per_instance(user, full, w, torch.float32)
    t64 = batch.per_instance(user, full, w, torch.float64)
    M = batch.term_magnitudes(user, full, w)
    for k in names:
        ref, err = g64[k], budget[k]
        assert t32[k].dtype == torch.float32
        terms32 = t32[k].reshape((B,) + tuple(ref.shape))
        terms64 = t64[k].reshape((B,) + tuple(ref.shape))
        assert float((terms64.sum(0) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k
        exact = terms32.double().sum(0)                                  # the fp64 sum of the same fp32 terms
        bound = 0.5 * (B + 8) * batch.U32 * M[k]
        assert M[k].shape == ref.shape and float(M[k].min()) > 0.0, k
        for order, fn in (("sequential", batch.sum_sequential), ("kernel", batch.sum_kernel_order)):
            s = fn(terms32)
            assert s.dtype == torch.float32
            r = batch.ratio(s.double(), ref, err)
            c = float(((s.double() - exact).abs() / bound).max())
            print(batch.case_id(case), k, order, "budget ratio", r, "consistency ratio (of the half bound)", c)
            assert r <= 1.0, (case, k, order, r)
            assert c <= 1.0, (case, k, order, c)
        # one instance dropped: ref - g_b (doubled: ref + g_b, the same distance), for every b
        scale = max(1.0, float(ref.abs().max()))
        floor = max(float(err.max()), 1e-6 * scale)
        per = terms64.abs().reshape(B, -1).max(1).values / floor
        last = (B - 1) // batch.CHUNK * batch.CHUNK
        edges = sorted({0, B - 1, last, max(0, last - 1)})
        print(batch.case_id(case), k, "one instance dropped: ratio min", float(per.min()), "median", float(per.median()),
              "edges", [float(per[b]) for b in edges])
        assert float(per.median()) >= SEPARATION and all(float(per[b]) >= SEPARATION for b in edges), (case, k, per.median())
        assert float(per.min()) >= EVERY_INSTANCE, (case, k, float(per.min()))


def test_the_consistency_cases_are_cases_of_the_matrix():
    assert set(batch.CONSISTENCY_CASES) <= set(batch.CASES)
    # chunks: a second one, an exactly full one, a one-instance last one, three with a tail of 4 + 3
    assert [(-(-B // batch.CHUNK), B % batch.CHUNK) for B in batch.EDGE_BATCHES] == [(1, 17), (1, 0), (2, 1), (3, 7)]
    assert {n + m for n, m in batch.MFMA_SHAPES} == {32, 17, 16, 8, 25} and all(n <= 16 and n + m <= 32 for n, m in batch.MFMA_SHAPES)
    assert all(n > 16 or n + m > 32 for n, m in batch.GENERIC_SHAPES + [(20, 10)])


@pytest.mark.parametrize("n,m", batch.BOX_SHAPES)
def test_the_box_cases_hold_and_free_every_control(n, m):
    _, own = batch.box_problem(n, m)
    sols = [("tv_case", own)] + [(f"shared, bounds {'[T, m]' if timed else '[m]'}", batch.box_shared(n, m, timed)[1])
                                 for timed in (False, True)]
    for what, sol in sols:
        cl = sol["clamped"]
        assert cl.shape == (batch.BOX_BATCH, batch.BOX_T, m)
        held = cl.sum(0)
        print(f"{n}x{m}", what, "held fraction", cl.mean(), "held per (t, i): min", held.min(), "max", held.max())
        assert 0.2 <= cl.mean() <= 0.8, (what, cl.mean())
        assert held.min() >= 1 and held.max() <= batch.BOX_BATCH - 1, (what, held)
        assert (cl & sol["at_low"]).any() and (cl & ~sol["at_low"]).any(), what      # both bounds occur


def test_the_all_held_rollout_stays_bounded():
    ops, xs, us, al, peak = batch.all_held_rollout()
    B, T, m = us.shape
    assert -(-B // batch.CHUNK) * T > 256          # box_reduce_final: more (chunk, step) partials than threads
    print("all-held rollout: max |x| in fp64", peak)
    assert peak < 1.0e4
    assert np.array_equal(us, np.where(al, ops["low"], ops["high"]))

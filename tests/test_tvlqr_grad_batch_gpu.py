"""The batch-summed gradients of the time-varying LQR on the MI355X past one reduction chunk: the reductions of
tfmpc_tvlqr_vjp_f32 and tfmpc_tvlqr_box_vjp_f32 (vjp_reduce_steps_mfma16 for n <= 16, n + m <= 32, vjp_reduce_steps
otherwise, vjp_reduce_steps_stage2, vjp_reduce_final, box_reduce_bounds / box_reduce_final) against the fp64
closed form summed over the batch (tests/tvlqr_grad_batch_ref.py), at batches of 17, 256, 257 and 519 instances -- a
second LDS tile, an exactly full chunk of 256, a one-instance last chunk, three chunks with a tail of 4 + 3 -- and at
the shape edges of the two per-step reductions.

Budget, the project's rule (tests/test_tvlqr_grad_gpu.py): kernel error against fp64 over the fp32 restatements' own
error, floor 1e-6 max(1, |ref|); median <= 2.5 and max <= 10 over instances.  A gradient summed over the batch counts
as ONE instance, and its fp32 error is the sum over the batch of the per-instance absolute fp32 errors (C, c: fp32
autograd; F, f, x0: elementwise the larger of that and the fp32 closed form).  tests/test_tvlqr_grad_batch_cpu.py shows
that the fp32 closed form summed in fp32 sits at 0.01 - 0.63 of that budget on every case here, and that losing or
repeating any single instance misses it by 290x or more.

Consistency with the per-instance path: the same problem with the shared operands materialised per instance goes through
the costate sweep's own stores; the fp64 sum of those per-instance gradients and the shared gradient add up the same
products, so they differ by summation and product rounding only: |shared - sum| <= 2 (B + 8) 2^-24 M elementwise, M the
summed magnitudes of the products (B u bounds any fp32 summation order, a few u per term the fma / matrix-core
roundings of one product, 2 the use of fp64 magnitudes for the kernel's fp32 ones).  Independent of the adjoint solve's
accuracy.

Every test prints its ratios: case, gradient, ratio."""
import numpy as np
import pytest
import torch

import tvlqr_grad_batch_ref as batch
from test_lqr_box_grad_gpu import _call, _f32_trajectory, _reference, _rename, _upstream
from test_lqr_box_grad_gpu import _check as _box_check
from test_tvlqr_grad_gpu import MODEL, _check, _kernel_grads, _loss
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR

pytestmark = pytest.mark.gpu


def _supported(n, m, T):
    assert _hip.load().tfmpc_tvlqr_kernel_name(n, m, T).decode() not in ("unsupported", "invalid"), (n, m, T)


def _run(case):
    """One case of the matrix: every gradient under the project rule -- the batch sums as one instance each (printed),
    the rest per instance."""
    n, m, T, B, _ = case
    _supported(n, m, T)
    user, full, w = batch.problem(*case)
    g64, budget = batch.oracle(*case)
    got = _kernel_grads(user, w)
    names = batch.summed_names(user, full)
    assert names, case
    for k in names:
        assert got[k].shape == g64[k].shape, (case, k, got[k].shape, g64[k].shape)
        assert bool(torch.isfinite(got[k]).all()), (case, k)
        ratios = np.array([batch.ratio(got[k], g64[k], budget[k])])          # one instance: median and max coincide
        print(batch.case_id(case), k, "ratio", ratios.max())
        assert np.median(ratios) <= 2.5 and ratios.max() <= 10.0, (case, k, ratios.max())
    _check(got, g64, budget, user, what=case)                                # ... and the per-instance gradients
    return got


@pytest.mark.parametrize("case", batch.BATCH_EDGE_CASES, ids=batch.case_id)
def test_batch_edges(case):
    _run(case)


@pytest.mark.parametrize("case", batch.NEED_CASES, ids=batch.case_id)
def test_subsets_of_shared_operands(case):
    got = _run(case)
    assert got["x0"].shape[0] == case[3]


@pytest.mark.parametrize("case", batch.SHAPE_EDGE_CASES, ids=batch.case_id)
def test_shape_edges_of_the_two_reductions(case):
    _run(case)


@pytest.mark.parametrize("case", batch.FINAL_CASES, ids=batch.case_id)
def test_shared_final_cost_and_x0(case):
    got = _run(case)
    n = case[0]
    assert got["Cfin"].shape == (n, n) and got["cfin"].shape == (n,) and got["x0"].shape == (n,)


@pytest.mark.parametrize("case", batch.CONSISTENCY_CASES, ids=batch.case_id)
def test_shared_sums_are_the_sums_of_the_per_instance_path(case):
    n, m, T, B, _ = case
    _supported(n, m, T)
    user, full, w = batch.problem(*case)
    shared = _kernel_grads(user, w)
    per = _kernel_grads({k: np.ascontiguousarray(v) for k, v in full.items()}, w)     # batch stride != 0: the sweep's own stores
    M = batch.term_magnitudes(user, full, w)
    for k in MODEL:
        assert per[k].shape == (B,) + tuple(shared[k].shape), (k, per[k].shape)
        total = per[k].sum(0)
        bound = 2.0 * (B + 8) * batch.U32 * M[k]
        worst = float(((shared[k] - total).abs() / bound).max())
        print(batch.case_id(case), k, "consistency ratio", worst)
        assert worst <= 1.0, (case, k, worst)


@pytest.mark.parametrize("n,m", batch.EDGE_SHAPES)
def test_flagged_instance_in_a_later_chunk(n, m):
    B, T, bad = 519, 3, 300
    user, _, w = batch.problem(n, m, T, B, "Ffc")
    C = user["C"].copy()
    C[bad, 1, n:, n:] = -1.0e4 * np.eye(m, dtype=np.float32)
    ops = {k: torch.as_tensor(C if k == "C" else v, device="cuda").requires_grad_() for k, v in user.items()}
    tv = TimeVaryingLQR(ops["F"], ops["f"], ops["C"], ops["c"], device="cuda")
    traj = tv.solve(ops["x0"])
    _loss(traj.states[..., None], traj.actions[..., None], traj.costs[..., None, None], w).backward()
    torch.cuda.synchronize()
    st = tv.last_grad_status.cpu().numpy()
    assert st[bad] & _hip.ST_NOT_PD and (np.delete(st, bad) == 0).all(), np.nonzero(st)
    others = torch.as_tensor(np.delete(np.arange(B), bad), device="cuda")
    for k in ("F", "f", "c"):                       # every batch sum contains it
        assert ops[k].grad.shape == ops[k].shape and bool(torch.isnan(ops[k].grad).all()), k
    for k in ("x0", "C"):                           # per instance: its own rows only
        assert bool(torch.isnan(ops[k].grad[bad]).all()), k
        assert bool(torch.isfinite(ops[k].grad[others]).all()), k


@pytest.mark.parametrize("timed", [False, True], ids=["bounds[m]", "bounds[T,m]"])
@pytest.mark.parametrize("n,m", batch.BOX_SHAPES)
def test_box_vjp_shared_model_and_bounds(n, m, timed):
    """One model, final cost and pair of bounds shared by 261 instances (a second chunk of five): every gradient but
    x0's is a batch sum; the bounds' also a sum over time when they are passed as [m]."""
    B, T = batch.BOX_BATCH, batch.BOX_T
    _supported(n, m, T)
    sh, sol = batch.box_shared(n, m, timed)          # F is shared: the optimum of the shared problem, re-solved
    xs, us = _f32_trajectory(sh, sol)
    g = _upstream(B, T, n, m, "mixed")
    ref, r32 = _reference(sh, xs, us, sol["clamped"], sol["at_low"], g)
    t = lambda a: torch.as_tensor(a[0], dtype=torch.float32, device="cuda")      # noqa: E731
    over = {k: t(sh[k]) for k in ("F", "f", "C", "c", "Cfin", "cfin")}
    over.update(low=t(sh["low"]) if timed else t(sh["low"])[0], high=t(sh["high"]) if timed else t(sh["high"])[0])
    assert over["low"].shape == ((T, m) if timed else (m,))
    got = _rename(_call(sh, xs, us, g, **over))
    assert int(got["status"].abs().sum()) == 0
    assert np.array_equal(got["clamped"].cpu().numpy(), sol["clamped"])
    assert got["low"].numel() == (T if timed else 1) * m and got["F"].shape == over["F"].shape      # ([m] comes back as [1, m])
    bsum = (0,) if timed else (0, 1)
    sums = [(k, (0,)) for k in ("F", "f", "C", "c", "Cfin", "cfin")] + [("low", bsum), ("high", bsum)]
    _box_check(got, ref, r32, f"box shared {n}x{m} B={B} {'[T, m]' if timed else '[m]'}", sums=sums)


def test_box_reduce_final_past_one_pass_of_its_threads():
    """chunks * T = 3 * 86 = 258 > 256 partial sums per bound: the strided loop of box_reduce_final.  Every control held
    (the trajectory is the rollout of the bounds), one model and one pair of bounds [m] shared by 513 instances."""
    n, m, B, T = (batch.STRIDED[k] for k in ("n", "m", "B", "T"))
    _supported(n, m, T)
    ops, xs, us, at_low, _ = batch.all_held_rollout()
    g = _upstream(B, T, n, m, "mixed")
    t = lambda a: torch.as_tensor(a[0], dtype=torch.float32, device="cuda")      # noqa: E731
    over = {k: t(ops[k]) for k in ("F", "f", "C", "c")}
    over.update(low=t(ops["low"])[0], high=t(ops["high"])[0])
    got = _rename(_call(ops, xs, us, g, **over))
    assert int(got["status"].abs().sum()) == 0 and bool(got["clamped"].all())
    assert got["low"].numel() == m and got["high"].numel() == m
    ref, r32 = _reference(ops, xs, us, np.ones((B, T, m), bool), at_low, g)
    sums = [(k, (0,)) for k in ("F", "f", "C", "c")] + [("low", (0, 1)), ("high", (0, 1))]
    _box_check(got, ref, r32, f"all held {n}x{m} B={B} T={T}", sums=sums)

"""The time-parallel double-precision time-varying LQR on the MI355X (tfmpc_tvlqr_solve_time_parallel_f64 through
TimeVaryingLQR.solve_time_parallel).

Accuracy is the project's double rule with the time-parallel fp64 restatement's own error as the budget
(tests/tvlqr_time_parallel_ref.py): per output and instance, the kernel's error against the longdouble sequential recursion
(tvlqr_f64_ref.solve_ld) over max(the restatement's error against it, 2^-48 max(1, |ref|)); median over instances <= 2.5
and every instance <= 10, on states, actions, costs, K, k, V and v, no instance left out.  Everything else -- forwarding,
strides, batch position, repetition -- is asserted bit for bit."""
import functools

import numpy as np
import pytest
import torch

import tvlqr_f64_ref as ref64
import tvlqr_ref
import tvlqr_time_parallel_ref as tp
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR, tvlqr_solve_time_parallel
from tfmpc.utils.trajectory import Trajectory

pytestmark = pytest.mark.gpu

FIELDS = tp.FIELDS
F64 = torch.float64


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _tv(F, f, C, c, *final):
    """(f and c as columns: [B, 1, 1] alone would read as [T, n, 1] at n = T = 1)"""
    F, f, C, c, *final = (np.asarray(a, dtype=np.float64) for a in (F, f, C, c, *final))
    return TimeVaryingLQR(F, f[..., None], C, c[..., None], *final, device="cuda", dtype=F64)


def _solve(tv, x0, segments):
    """The public call with every output: a dict of numpy arrays [B, ...] plus the status."""
    x0 = np.asarray(x0, dtype=np.float64)
    traj, K, k, V, v = tv.solve_time_parallel(x0[..., None], segments, want_policy=True, want_value=True)
    torch.cuda.synchronize()
    assert isinstance(traj, Trajectory) and all(t.dtype == F64 for t in (K, k, V, v))
    got = dict(states=traj.states, actions=traj.actions, costs=traj.costs, K=K.cpu().numpy(), k=k.cpu().numpy()[..., 0],
               V=V.cpu().numpy(), v=v.cpu().numpy()[..., 0])
    if x0.ndim == 1:
        got = {name: a[None] for name, a in got.items()}
    got["status"] = tv.last_status.cpu().numpy()
    return got


def _same_bits(a, b, what="", fields=FIELDS):
    for name in fields:
        assert np.array_equal(a[name], b[name], equal_nan=True), (what, name)


@functools.lru_cache(maxsize=None)
def _case(n, m, T, segments, B, unscaled=False, final=False):
    """Operands, the longdouble sequential reference and the fp64 time-parallel restatement, computed once."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = tp.perturbed(make, n, m, T, B, seed=n * 100 + m)
    x0 = tvlqr_ref.make_x0(n, B, seed=T).astype(np.float64)
    Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B)) if final else (None, None)
    rld, _ = ref64.references(F, f, C, c, x0, Cf, cf)
    rtp = tp.solve_batch(F, f, C, c, x0, segments, Cf, cf)
    return F, f, C, c, x0, Cf, cf, rld, rtp


# the issue's shapes (n, m, T, segments, B), then T = 1, wide controls, an explicit final cost, an unscaled model
CASES = [(3, 2, 8, 4, 4), (5, 3, 7, 3, 4), (16, 8, 50, 5, 4), (16, 8, 64, 64, 3), (17, 8, 12, 3, 3), (32, 32, 8, 2, 2),
         (16, 8, 200, 8, 3), (1, 1, 1, 1, 3), (16, 17, 8, 2, 3), (8, 32, 8, 2, 3)]


@pytest.mark.parametrize("n,m,T,segments,B", CASES)
def test_accuracy_against_the_longdouble_recursion(n, m, T, segments, B):
    F, f, C, c, x0, _, _, rld, rtp = _case(n, m, T, segments, B)
    got = _solve(_tv(F, f, C, c), x0, segments)
    assert (got["status"] == 0).all(), got["status"]
    ref64.check(got, rld, rtp, fields=FIELDS, what=(n, m, T, segments))


@pytest.mark.parametrize("unscaled,final", [(False, True), (True, False)])
def test_accuracy_with_an_explicit_final_cost_and_on_an_unscaled_model(unscaled, final):
    n, m, T, segments, B = 16, 8, 50, 5, 4
    F, f, C, c, x0, Cf, cf, rld, rtp = _case(n, m, T, segments, B, unscaled, final)
    tv = _tv(F, f, C, c, Cf, cf) if final else _tv(F, f, C, c)
    got = _solve(tv, x0, segments)
    assert (got["status"] == 0).all(), got["status"]
    ref64.check(got, rld, rtp, fields=FIELDS, what=("unscaled" if unscaled else "final cost", n, m, T, segments))


@pytest.mark.parametrize("n,m,T,segments,B", [(16, 8, 50, 5, 4), (5, 3, 7, 3, 4), (17, 8, 12, 3, 3)])
def test_seams_the_rollout_meets_the_stitched_boundary_state(n, m, T, segments, B):
    """states[s_i] is the stitch's boundary state (segment i starts from it); F z + f from states[s_i - 1] and
    actions[s_i - 1] is where segment i - 1's rollout arrives.  A wrong offset at a seam breaks their agreement."""
    F, f, C, c, x0, _, _, rld, rtp = _case(n, m, T, segments, B)
    got = _solve(_tv(F, f, C, c), x0, segments)
    _, table = tp.segment_table(T, segments)
    assert len(table) > 1
    arrived = {"states": np.stack([np.stack([
        F[b, t0 - 1] @ np.concatenate([got["states"][b, t0 - 1], got["actions"][b, t0 - 1]]) + f[b, t0 - 1]
        for t0, _ in table[1:]]) for b in range(B)])}
    pick = lambda r: [{"states": x["states"][[t0 for t0, _ in table[1:]]]} for x in r]     # noqa: E731
    ref64.check(arrived, pick(rld), pick(rtp), fields=("states",), what=("seam", n, m, T, segments))
    # ... and the restatement's boundary states are the ones the kernel started the segments from
    stitched = {"states": got["states"][:, [t0 for t0, _ in table[1:]]]}
    ref64.check(stitched, pick(rld), pick(rtp), fields=("states",), what=("boundary", n, m, T, segments))
    # ... and the two agree WITH EACH OTHER within the same budget: the restatement's error at the seams or the floor
    ratio = []
    for b in range(B):
        ref = pick(rld)[b]["states"]
        budget = max(ref64.error(pick(rtp)[b]["states"], ref), ref64.FLOOR * max(1.0, float(np.abs(ref).max())))
        ratio.append(float(np.abs(arrived["states"][b] - stitched["states"][b]).max()) / budget)
    print(f"budget ('arrived - stitched', {n}, {m}, {T}, {segments}): median {np.median(ratio):.3g} max {max(ratio):.3g}")
    assert np.median(ratio) <= ref64.MEDIAN_BOUND and max(ratio) <= ref64.MAX_BOUND, ratio


# ---- bits ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,T,segments", [(16, 8, 9, 1), (17, 8, 1, 5), (3, 2, 1, 1)])
def test_one_segment_forwards_to_the_sequential_solve(n, m, T, segments):
    B = 3
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, B, seed=21)
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    tv = _tv(F, f, C, c)
    got = _solve(tv, x0, segments)
    seq = tv.solve_device(_dev(x0[..., None]), want_policy=True, want_value=True)
    torch.cuda.synchronize()
    for name in FIELDS:
        a = seq[name].cpu().numpy()
        a = a[..., 0] if name in ("states", "actions", "k", "v") else a.reshape(B, -1) if name == "costs" else a
        assert np.array_equal(got[name], a), name
    assert _hip.load().tfmpc_tvlqr_time_parallel_kernel_name_f64(n, m, T, segments) == _hip.load().tfmpc_tvlqr_kernel_name_f64(n, m, T)


def test_strides_shared_unbatched_numpy_and_noncontiguous_operands_give_the_materialised_bits():
    n, m, T, B, segments = 12, 5, 11, 3, 4
    d = n + m
    # time stride 0: a time-invariant model against its materialised copy
    F1, f1, C1, c1 = tp.perturbed(tvlqr_ref.make_models, n, m, 1, B, seed=22)
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    views = [_dev(a).expand(B, T, *a.shape[2:]) for a in (F1, f1, C1, c1)]
    tv0 = TimeVaryingLQR(*views, device="cuda", dtype=F64)
    assert tv0._model_args()[2] == 0 and tv0.F.data_ptr() == views[0].data_ptr()
    rep = lambda a: np.repeat(a, T, axis=1)                # noqa: E731
    _same_bits(_solve(tv0, x0, segments), _solve(_tv(rep(F1), rep(f1), rep(C1), rep(c1)), x0, segments), "time stride 0")
    # batch stride 0: one model shared by the batch, and one x0 for a batched model
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, B, seed=23)
    shared = _tv(F[0], f[0], C[0], c[0])
    assert shared.batch_size is None and shared._model_args()[1] == 0
    tile = lambda a: np.repeat(a[:1], B, axis=0)           # noqa: E731
    _same_bits(_solve(shared, x0, segments), _solve(_tv(tile(F), tile(f), tile(C), tile(c)), x0, segments), "shared model")
    ref = _solve(_tv(F, f, C, c), np.repeat(x0[:1], B, axis=0), segments)
    traj, K, k, V, v = _tv(F, f, C, c).solve_time_parallel(x0[0][:, None], segments, want_policy=True, want_value=True)
    assert traj.states.shape == (B, T + 1, n) and np.array_equal(traj.states, ref["states"]) and np.array_equal(K.cpu().numpy(), ref["K"])
    # unbatched problem and x0: the shapes lose the batch axis, the bits are instance 0's
    one = _solve(_tv(F[:1], f[:1], C[:1], c[:1]), x0[:1], segments)
    traj, K, k, V, v = shared.solve_time_parallel(x0[0], segments, want_policy=True, want_value=True)
    assert traj.states.shape == (T + 1, n) and K.shape == (T, m, n) and v.shape == (T, n, 1)
    assert np.array_equal(traj.states, one["states"][0]) and np.array_equal(V.cpu().numpy(), one["V"][0])
    # numpy against non-contiguous tensor views of the same numbers, and the functional form
    full = _solve(_tv(F, f, C, c), x0, segments)
    Ft = _dev(np.swapaxes(F, -1, -2)).transpose(-1, -2)
    Cw = torch.zeros((B, T, d, 2 * d), dtype=F64, device="cuda")
    Cw[..., ::2] = _dev(C)
    xw = torch.zeros((B, 2 * n, 1), dtype=F64, device="cuda")
    xw[:, ::2] = _dev(x0[..., None])
    assert not Ft.is_contiguous() and not Cw[..., ::2].is_contiguous()
    tv2 = TimeVaryingLQR(Ft, _dev(f), Cw[..., ::2], _dev(c), device="cuda", dtype=F64)
    traj, K, k, V, v = tv2.solve_time_parallel(xw[:, ::2], segments, want_policy=True, want_value=True)
    assert np.array_equal(traj.states, full["states"]) and np.array_equal(traj.costs, full["costs"])
    assert np.array_equal(k.cpu().numpy()[..., 0], full["k"]) and np.array_equal(V.cpu().numpy(), full["V"])
    states, actions, costs = tvlqr_solve_time_parallel(F, f, C, c, x0[..., None], segments)
    assert states.dtype == F64 and states.shape == (B, T + 1, n, 1) and costs.shape == (B, T + 1, 1, 1)
    assert np.array_equal(states.cpu().numpy()[..., 0], full["states"]) and np.array_equal(actions.cpu().numpy()[..., 0], full["actions"])


@pytest.mark.parametrize("n,m,T,segments", [(16, 8, 23, 4), (20, 10, 9, 9)])
def test_an_instance_alone_gives_its_bits_in_a_batch_and_two_calls_agree(n, m, T, segments):
    B = 3
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, B, seed=24)
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    tv = _tv(F, f, C, c)
    batch, again = _solve(tv, x0, segments), _solve(tv, x0, segments)
    _same_bits(batch, again, "two calls")
    for b in range(B):
        alone = _solve(_tv(F[b:b + 1], f[b:b + 1], C[b:b + 1], c[b:b + 1]), x0[b:b + 1], segments)
        for name in FIELDS:
            assert np.array_equal(alone[name][0], batch[name][b]), (name, b)
    # without gain or value outputs the trajectory is the same
    lean = tv.solve_time_parallel(x0[..., None], segments)
    assert isinstance(lean, Trajectory) and np.array_equal(lean.states, batch["states"]) and np.array_equal(lean.costs, batch["costs"])


def test_the_default_segment_count_is_accepted_and_valid():
    n, m, T, B = 5, 3, 200, 2
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, B, seed=25)
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    tv = _tv(F, f, C, c)
    segments = tv.default_segments(B)
    assert 1 <= segments <= T
    _same_bits(_solve(tv, x0, None), _solve(tv, x0, segments), "default")
    assert (tv.last_status.cpu().numpy() == 0).all()


# ---- status ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_an_indefinite_step_flags_its_instance_alone(n, m):
    B, T, segments = 3, 12, 3
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, B, seed=26)
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    clean = _solve(_tv(F, f, C, c), x0, segments)
    assert (clean["status"] == 0).all()
    C_bad = C.copy()
    C_bad[1, 6, n:, n:] = -1e3 * np.eye(m)                  # R_6 of instance 1: the middle of segment 1 (steps 4 .. 7)
    got = _solve(_tv(F, f, C_bad, c), x0, segments)
    assert got["status"][1] & _hip.ST_NOT_PD and (got["status"][[0, 2]] == 0).all(), got["status"]
    for name in FIELDS:
        assert np.isnan(got[name][1]).all(), name
        for b in (0, 2):
            assert np.array_equal(got[name][b], clean[name][b]), (name, b)

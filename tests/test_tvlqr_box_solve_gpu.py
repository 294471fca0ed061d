"""The control-limited time-varying LQR forward on the MI355X: tfmpc_tvlqr_box_solve_f32 (tfmpc.solvers.tvlqr_box_solve,
DESIGN.md 3.17) against the exact fp64 optimum of tests/lqr_box_grad_ref.py.

Budget, the project's rule: per instance and per output (states, actions, costs), the kernel's error against the fp64
optimum divided by max(the fp32 restatement's error on that instance, 1e-6 max(1, |ref|_inf)); median <= 2.5 and every
instance <= 10.  The restatement is tests/tvlqr_box_solve_ref.py (pinned without a GPU by
tests/test_tvlqr_box_solve_cpu.py)."""
import numpy as np
import pytest
import torch

import lqr_box_grad_ref as bref
import tvlqr_box_solve_ref as sref
import tvlqr_ref
from test_lqr_box_grad_cpu import GPU_TV_BATCH, GPU_TV_HORIZONS, GPU_TV_SHAPES, tv_final
from test_lqr_box_grad_gpu import _check, _f32_trajectory, _reference, _upstream

pytestmark = pytest.mark.gpu

OUTPUTS = ("states", "actions", "costs")
ST_NOT_PD, ST_MAX_ATTEMPTS = 2, 16
TIGHT = 1e-3            # the width of bounds so tight that every control of the test problem is held


def _t(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def _solve(ops, **kw):
    """ops: a dict of numpy arrays (F f C c x0 low high Cfin cfin) or tensors -> numpy outputs with the batch axis kept."""
    from tfmpc.solvers import tvlqr_box_solve
    p = {k: (v if isinstance(v, torch.Tensor) else _t(v)) for k, v in ops.items()}
    kw = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    res = tvlqr_box_solve(p["F"], p["f"], p["C"], p["c"], p["x0"], p["low"], p["high"], C_final=p.get("Cfin"),
                          c_final=p.get("cfin"), **kw)
    info = res.info
    out = dict(states=res[0][..., 0], actions=res[1][..., 0], costs=res[2][..., 0, 0], iterations=info.last_iterations,
               status=info.last_status, reason=info.last_reason, clamped=info.last_clamped)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _rule(got, r32, sol, what, pick=None):
    for name in OUTPUTS:
        ratios = sref.budget_ratios(got[name], r32[name], sol[name])
        if pick is not None:
            ratios = ratios[pick]
        print(what, name, "median %.3f max %.3f" % (np.median(ratios), ratios.max()))
        assert np.median(ratios) <= 2.5 and ratios.max() <= 10.0, (what, name, np.median(ratios), ratios.max())


def _feasible(got, ops):
    lo = np.broadcast_to(np.asarray(ops["low"], dtype=np.float32), got["actions"].shape)
    hi = np.broadcast_to(np.asarray(ops["high"], dtype=np.float32), got["actions"].shape)
    return bool((got["actions"] >= lo).all() and (got["actions"] <= hi).all())


def _rollout64(ops, actions, dtype=np.float64):
    F, f, x0 = (np.asarray(ops[k]).astype(dtype) for k in ("F", "f", "x0"))
    B, T = actions.shape[:2]
    xs = np.empty((B, T + 1, F.shape[2]), dtype)
    xs[:, 0] = x0
    u = actions.astype(dtype)
    for t in range(T):
        z = np.concatenate([xs[:, t], u[:, t]], -1)
        xs[:, t + 1] = (np.einsum("bij,bj->bi", F[:, t], z).astype(dtype) + f[:, t]).astype(dtype)
    return xs


def _converged(got, cap=sref.DEFAULT_PASSES):
    assert not got["status"].any(), got["status"]
    assert not got["reason"].any(), got["reason"]
    assert (got["iterations"] < cap).all(), got["iterations"]


def _same_held_sets(got, ops, sol, max_unclear=0.25):
    held = sref.held_from_actions(got["actions"], ops["low"], ops["high"])
    clear = sol["clear"]
    assert (~clear).mean() <= max_unclear, (~clear).mean()
    assert np.array_equal(held[clear], sol["clamped"][clear])
    return held


@pytest.mark.parametrize("T", GPU_TV_HORIZONS)
@pytest.mark.parametrize("n,m", GPU_TV_SHAPES)
def test_the_time_varying_workload(n, m, T):
    ops, sol, r32 = sref.case(n, m, T, GPU_TV_BATCH, tv_final(T))
    got = _solve(ops)
    print(f"tv {n}x{m} T={T} sweeps", got["iterations"].tolist(), "restatement", r32["iterations"].tolist())
    _converged(got)
    _rule(got, r32, sol, f"tv {n}x{m} T={T}")
    assert _feasible(got, ops)
    held = _same_held_sets(got, ops, sol)
    assert np.array_equal(got["clamped"], held)                      # clamp_mask: the last sweep's sets are the held set
    # the states are the rollout of the kernel's own actions, to the rounding of an fp32 rollout
    xs64 = _rollout64(ops, got["actions"])
    ratios = sref.budget_ratios(got["states"], _rollout64(ops, got["actions"], np.float32), xs64)
    print(f"tv {n}x{m} T={T} own rollout median %.3f max %.3f" % (np.median(ratios), ratios.max()))
    assert np.median(ratios) <= 2.5 and ratios.max() <= 10.0


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 20)])
def test_without_bounds_it_is_the_tvlqr_solve(n, m, T):
    """The rule with tfmpc_tvlqr_solve_f32 itself as the budget: this kernel's error against the fp64 TV-LQR optimum over
    max(the plain kernel's error on that instance, floor), median <= 2.5 and every instance <= 10.  Each kernel also
    meets the rule with its own fp32 restatement as the budget."""
    from tfmpc.solvers import tvlqr_solve
    B = GPU_TV_BATCH
    ops, _ = bref.tv_case(n, m, T, B)
    free = dict(ops, low=-np.inf, high=np.inf)
    got = _solve(free)
    _converged(got)
    assert (got["iterations"] <= 2).all() and not got["clamped"].any()
    ref, p32 = ({k: np.stack([tvlqr_ref.solve(ops["F"][b], ops["f"][b], ops["C"][b], ops["c"][b], ops["x0"][b][:, None], dtype=dt)[k]
                              for b in range(B)]) for k in OUTPUTS} for dt in (np.float64, np.float32))
    r32 = sref.solve_batch(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], -np.inf, np.inf)
    xs, us, cs = tvlqr_solve(*(_t(ops[k]) for k in ("F", "f", "C", "c", "x0")))
    plain = dict(states=xs[..., 0].cpu().numpy(), actions=us[..., 0].cpu().numpy(), costs=cs[..., 0, 0].cpu().numpy())
    _rule(got, r32, ref, f"unbounded {n}x{m} T={T}")
    _rule(plain, p32, ref, f"tfmpc_tvlqr_solve_f32 {n}x{m} T={T}")
    _rule(got, plain, ref, f"unbounded {n}x{m} T={T} against tfmpc_tvlqr_solve_f32")
    # bounds so wide that nothing clamps: the same optimum
    wide = _solve(dict(ops, low=-1e4, high=1e4))
    _converged(wide)
    assert not wide["clamped"].any()
    _rule(wide, r32, ref, f"wide {n}x{m} T={T}")


def test_a_pinned_box_and_a_tight_box():
    n, m, T, B = 12, 6, 8, GPU_TV_BATCH
    ops, _ = bref.tv_case(n, m, T, B)
    got = _solve(dict(ops, high=ops["low"]))
    assert not got["iterations"].any() and not got["status"].any() and not got["reason"].any()
    assert np.array_equal(got["actions"], ops["low"].astype(np.float32))
    assert np.allclose(got["states"], _rollout64(ops, got["actions"]), rtol=0, atol=1e-4 * max(1.0, np.abs(got["states"]).max()))
    # so tight that every control is held
    ops, sol, r32 = sref.case(n, m, T, B, False, TIGHT)
    assert sol["clamped"].all()
    got = _solve(ops)
    _converged(got)
    _rule(got, r32, sol, "tight")
    assert got["clamped"].all() and sref.held_from_actions(got["actions"], ops["low"], ops["high"]).all()


@pytest.mark.parametrize("n,m,T,B,final", [(3, 5, 10, 8, False), (5, 3, 1, 8, True), (5, 3, 200, 4, False), (32, 32, 4, 2, False)])
def test_edge_shapes(n, m, T, B, final):
    """More controls than states, one step, a horizon past the matrix-core box kernel's 148 (clear share 0.75), and the
    largest shape served, which needs more than 64 KiB of LDS."""
    ops, sol, r32 = sref.case(n, m, T, B, final)
    got = _solve(ops)
    print(f"edge {n}x{m} T={T} sweeps", got["iterations"].tolist(), "clear", sol["clear"].tolist())
    _converged(got)
    _rule(got, r32, sol, f"edge {n}x{m} T={T}")
    assert _feasible(got, ops)
    _same_held_sets(got, ops, sol)


@pytest.mark.parametrize("which", ["batch", "time", "both"])
def test_stride_zero_operands_give_the_bits_of_materialised_copies(which):
    n, m, T, B = 12, 6, 8, GPU_TV_BATCH
    ops, _ = bref.tv_case(n, m, T, B)
    names = ("F", "f", "C", "c", "low", "high")
    full = {k: _t(ops[k]) for k in names}
    full["F"] = 0.6 * full["F"]                                      # (one step's draw held for T steps: keep it stable)
    if which in ("batch", "both"):
        full = {k: v[:1].expand(B, *v.shape[1:]) for k, v in full.items()}
    if which in ("time", "both"):
        full = {k: v[:, :1].expand(v.shape[0], T, *v.shape[2:]) for k, v in full.items()}
    thin = {k: v for k, v in full.items()}
    if which in ("time", "both"):
        thin = {k: (v if k == "high" else v[:, :1]) for k, v in thin.items()}     # a time axis of 1 (one operand carries T)
    if which in ("batch", "both"):
        thin = {k: v[0] for k, v in thin.items()}                     # no batch axis
    a = _solve(dict(thin, x0=ops["x0"]))
    b = _solve(dict({k: v.contiguous() for k, v in full.items()}, x0=ops["x0"]))
    c = _solve(dict(full, x0=ops["x0"]))                              # expanded views: stride 0, no copy
    assert not a["status"].any() and a["iterations"].max() > 1
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


def test_an_instance_does_not_depend_on_its_batch():
    n, m, T = 16, 8, 50
    ops, _, _ = sref.case(n, m, T, GPU_TV_BATCH, tv_final(T))
    take = lambda idx: {k: (None if v is None else v[idx]) for k, v in ops.items()}      # noqa: E731
    base = _solve(ops)
    for b in (0, 5):
        one = _solve(take([b]))
        for k in base:
            assert np.array_equal(one[k][0], base[k][b]), (k, b)
    idx = np.random.default_rng(3).permutation(257) % GPU_TV_BATCH
    big = _solve(take(idx))
    for k in base:
        assert np.array_equal(big[k], base[k][idx]), k


def test_a_flagged_instance_and_the_pass_cap():
    n, m, T, B = 5, 3, 6, 4
    ops, sol, _ = sref.case(n, m, T, B)
    bad = {k: (None if v is None else v.copy()) for k, v in ops.items()}
    s, i = np.argwhere(~sol["clamped"][2])[0]
    bad["C"][2, s, n + i, n + i] = -50.0                              # an indefinite C_uu at one step
    got = _solve(bad)
    assert got["status"][2] & ST_NOT_PD and not got["status"][[0, 1, 3]].any() and got["reason"][2] == sref.REASON_FAILED
    for k in OUTPUTS:
        assert np.isnan(got[k][2]).all() and np.isfinite(got[k][[0, 1, 3]]).all(), k
    rest = _solve({k: (None if v is None else v[[0, 1, 3]]) for k, v in ops.items()})
    for k in rest:
        assert np.array_equal(got[k][[0, 1, 3]], rest[k]), k
    # one pass: the cap is reported and the trajectory is feasible and consistent
    got = _solve(ops, max_iter=1)
    assert (got["status"] == ST_MAX_ATTEMPTS).all() and (got["reason"] == sref.REASON_PASS_CAP).all() and (got["iterations"] == 1).all()
    assert _feasible(got, ops) and all(np.isfinite(got[k]).all() for k in OUTPUTS)
    assert np.allclose(got["states"], _rollout64(ops, got["actions"]), rtol=0, atol=1e-4 * max(1.0, np.abs(got["states"]).max()))


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 50)])
def test_warm_start(n, m, T):
    ops, sol, r32 = sref.case(n, m, T, GPU_TV_BATCH, tv_final(T))
    _, us = _f32_trajectory(ops, sol)
    got = _solve(ops, u_init=us)
    print(f"warm {n}x{m} sweeps", got["iterations"].tolist())
    _converged(got)
    assert (got["iterations"] <= 2).all()
    _same_held_sets(got, ops, sol)
    shared = _solve(ops, u_init=us[0])                                # one start for the batch: [T, m]
    assert np.array_equal(shared["actions"][0], got["actions"][0])
    # a start outside the box is clipped into it
    out = _solve(ops, u_init=np.full_like(us, 100.0))
    _converged(out)
    assert _feasible(out, ops)
    _same_held_sets(out, ops, sol)
    _rule(out, r32, sol, f"start outside the box {n}x{m}")


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 50)])
def test_autograd_is_the_box_vjp_on_the_returned_trajectory(n, m, T):
    from tfmpc.solvers import tvlqr_box_solve, tvlqr_box_vjp
    B = GPU_TV_BATCH
    ops, sol, _ = sref.case(n, m, T, B, tv_final(T))
    leaves = {k: _t(ops[k]).requires_grad_() for k in ("F", "f", "C", "c", "x0", "low", "high")}
    xs, us, cs = tvlqr_box_solve(*leaves.values())
    g = _upstream(B, T, n, m, "mixed")
    loss = (xs[..., 0] * _t(g[0])).sum() + (us[..., 0] * _t(g[1])).sum() + (cs[..., 0, 0] * _t(g[2])).sum()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items()}
    direct = tvlqr_box_vjp(*(leaves[k].detach() for k in ("F", "f", "C", "c", "low", "high")), xs.detach()[..., 0],
                           us.detach()[..., 0], *(_t(a) for a in g))
    for k in grads:
        assert torch.equal(grads[k], direct[k].reshape(grads[k].shape)), k
    # clear instances against the closed form at the fp64 optimum, the budget widened by the closed form's sensitivity to
    # the measured forward error (tests/test_lqr_box_grad_gpu.py::test_box_lqr_solve_end_to_end)
    xd, ud = xs.detach()[..., 0].double().cpu().numpy(), us.detach()[..., 0].double().cpu().numpy()
    lo, hi = ops["low"].astype(np.float32).astype(np.float64), ops["high"].astype(np.float32).astype(np.float64)
    cld, ald = (ud == lo) | (ud == hi), ud == lo
    ref, r32 = _reference(ops, xd, ud, cld, ald, g)
    opt, _ = _reference(ops, sol["states"], sol["actions"], sol["clamped"], sol["at_low"], g)
    pick = np.nonzero(sol["clear"])[0]
    wide = {k: r32[k] + (ref[k] - opt[k]).abs() for k in ref}
    sub = lambda d_: {k: v[pick] for k, v in d_.items()}      # noqa: E731
    _check({k: v[pick] for k, v in grads.items()}, sub(opt), sub(wide), f"autograd at the fp64 optimum {n}x{m}")


def test_autograd_returns_gradients_in_the_operands_own_shapes():
    """Shared, unbatched and time-constant operands, a scalar and an [m] bound and an explicit final cost: each gradient
    has its operand's shape and is the sum of the materialised problem's gradients over the axes the operand lacks.
    Both runs solve the same bits, so the terms are the same and only the order of an fp32 sum of N terms differs:
    |difference| <= N 2^-23 sum |term| (N - 1 roundings of the sum, one more for a fused term)."""
    from tfmpc.solvers import tvlqr_box_solve
    n, m, T, B = 5, 3, 8, 4
    ops, _ = bref.tv_case(n, m, T, B, final=True)
    thin = dict(F=0.6 * ops["F"][0], f=ops["f"][:, :1], C=ops["C"][0, :1], c=ops["c"], x0=ops["x0"][0],
                low=np.float64(ops["low"].mean()), high=ops["high"][0, 0], C_final=ops["Cfin"][0], c_final=ops["cfin"])
    full_shape = dict(F=(B, T, n, n + m), f=(B, T, n), C=(B, T, n + m, n + m), c=(B, T, n + m), x0=(B, n), low=(B, T, m),
                      high=(B, T, m), C_final=(B, n, n), c_final=(B, n))
    g = _upstream(B, T, n, m, "mixed")

    def run(leaves):
        xs, us, cs = tvlqr_box_solve(**leaves)
        loss = (xs[..., 0] * _t(g[0])).sum() + (us[..., 0] * _t(g[1])).sum() + (cs[..., 0, 0] * _t(g[2])).sum()
        loss.backward()
        return xs.detach(), us.detach()

    a = {k: _t(v).requires_grad_() for k, v in thin.items()}
    b = {k: _t(np.broadcast_to(v, full_shape[k]).copy()).requires_grad_() for k, v in thin.items()}
    (xa, ua), (xb, ub) = run(a), run(b)
    assert torch.equal(xa, xb) and torch.equal(ua, ub)
    held = (ua[..., 0] == b["low"].detach()) | (ua[..., 0] == b["high"].detach())
    assert held.any() and not held.all()                              # the bounds take part
    for k in thin:
        assert a[k].grad.shape == a[k].shape, k
        terms = b[k].grad.double()
        lead = terms.dim() - a[k].dim()
        dims = tuple(range(lead)) + tuple(lead + i for i, s_ in enumerate(a[k].shape) if s_ != terms.shape[lead + i])
        count = terms.numel() // max(a[k].numel(), 1)
        want = terms.sum(dims).reshape(a[k].shape) if dims else terms
        allow = count * 2.0 ** -23 * (terms.abs().sum(dims).reshape(a[k].shape) if dims else terms.abs())
        diff = (a[k].grad.double() - want).abs()
        print("own shapes", k, tuple(a[k].shape), "terms", count, "worst difference over its allowance",
              float((diff / allow.clamp_min(1e-300)).max()))
        assert bool((diff <= allow).all()), k


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 20)])
def test_against_the_ilqr_forward(n, m, T):
    from tfmpc.solvers import box_lqr_solve
    B = 64
    F, f, C, c, x0, lo, hi = bref.workload_numbers(B, n, m)
    F, f, C, c, x0 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (F, f, C, c, x0))
    x0 = x0.reshape(B, n)
    tile = lambda a: bref.tile_time(a, T)      # noqa: E731
    ops = dict(F=tile(F), f=tile(f), C=tile(C), c=tile(c), x0=x0, low=np.full((B, T, m), lo), high=np.full((B, T, m), hi))
    sol = bref.solve_box_batch(ops["F"], ops["f"], ops["C"], ops["c"], x0, ops["low"], ops["high"])
    r32 = sref.solve_batch(ops["F"], ops["f"], ops["C"], ops["c"], x0, ops["low"], ops["high"])
    # the time-invariant model through stride-0 views
    view = lambda a: _t(a).unsqueeze(1).expand(B, T, *a.shape[1:])      # noqa: E731
    got = _solve(dict(F=view(F), f=view(f), C=view(C), c=view(c), x0=x0, low=lo, high=hi))
    res = box_lqr_solve(_t(F), _t(f), _t(C), _t(c), _t(x0).unsqueeze(-1), lo, hi, T, atol=1e-6)
    ilqr = dict(states=res[0][..., 0].cpu().numpy(), actions=res[1][..., 0].cpu().numpy(), costs=res[2][..., 0, 0].cpu().numpy())
    print(f"workload {n}x{m} T={T} newton sweeps", np.bincount(got["iterations"]).tolist(), "iLQR iterations",
          np.bincount(res.info.last_iterations.cpu().numpy()).tolist())
    _converged(got)
    _same_held_sets(got, ops, sol)
    _same_held_sets(ilqr, ops, sol)
    _rule(got, r32, sol, f"workload {n}x{m} newton")
    _rule(ilqr, r32, sol, f"workload {n}x{m} iLQR")

"""Gradients of the control-limited LQR on the MI355X: tfmpc_tvlqr_box_vjp_f32 (tfmpc.solvers.tvlqr_box_vjp) and
tfmpc.solvers.box_lqr_solve against the fp64 closed form of tests/lqr_box_grad_ref.py.

Budget, the project's rule: per instance, kernel error against fp64 divided by the error of the closed form restated in
fp32 on the same trajectory and held set (floor 1e-6 max(1, |ref|)); median <= 2.5, max <= 10.  A gradient summed over
the batch or over time counts as one instance, its budget the sum of its terms' absolute errors.

``dc[b, t, n + i] == 0`` for a held control holds for losses on states and actions: a loss on the costs adds the direct
term ``gcost_t u_t`` (the cost is linear in c), which is not zero on a bound.  Of ``dC`` the kernels emit the symmetric
gradient ``(dz z^T + z dz^T) / 2``: its entry (n + i, j) is ``(dz_i z_j + u_i dz_j) / 2``, so row n + i of the ``dz z^T``
term is zero but the symmetric sum is exactly zero only where BOTH indices are held controls; that is what is asserted."""
import numpy as np
import pytest
import torch

import lqr_box_grad_ref as bref
from test_lqr_box_grad_cpu import GPU_TV_BATCH, GPU_TV_HORIZONS, GPU_TV_SHAPES, tv_final

pytestmark = pytest.mark.gpu

NAMES = ("F", "f", "C", "c", "x0", "low", "high", "Cfin", "cfin")
KEY = dict(Cfin="C_final", cfin="c_final")


def _upstream(B, T, n, m, loss, seed=11):
    rng = np.random.default_rng(seed)
    g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    return tuple(a.astype(np.float32).astype(np.float64) if loss in (name, "mixed") else None
                 for a, name in zip(g, ("states", "actions", "costs")))


def _f32_trajectory(ops, sol):
    """The fp64 optimum as the kernel sees it: rounded to fp32, held controls carrying the bound's fp32 bits."""
    xs = sol["states"].astype(np.float32)
    us = sol["actions"].astype(np.float32)
    lo = np.broadcast_to(ops["low"], us.shape).astype(np.float32)
    hi = np.broadcast_to(ops["high"], us.shape).astype(np.float32)
    cl, al = sol["clamped"], sol["at_low"]
    us = np.where(cl & al, lo, np.where(cl, hi, us))
    free_on_bound = ~cl & ((us == lo) | (us == hi))
    assert not free_on_bound.any()
    return xs, us


def _check(kern, ref, r32, what, sums=()):
    """kern / ref / r32: dicts of [B, T, ...] tensors (r32: the fp32 restatement's absolute error).  ``sums``: names whose
    kernel value is already summed -- (name, dims) -- compared as one instance."""
    sums = dict(sums)
    for name in ref:
        if name not in kern:
            continue
        k, want, e32 = kern[name].double().cpu(), ref[name], r32[name]
        if name in sums:
            want, e32 = want.sum(sums[name], keepdim=True), e32.sum(sums[name], keepdim=True)
            k = k.reshape(want.shape)
            items = [None] if 0 in sums[name] else range(want.shape[0])      # a batch sum counts as one instance
        else:
            k = k.reshape(want.shape)
            items = range(want.shape[0])
        ratios = []
        for b in items:
            sel = (lambda t: t) if b is None else (lambda t, b=b: t[b])   # noqa: E731
            scale = max(1.0, float(sel(want).abs().max()))
            budget = max(float(sel(e32).max()), 1e-6 * scale)
            ratios.append(float((sel(k) - sel(want)).abs().max()) / budget)
        ratios = np.array(ratios)
        print(what, name, "median", np.median(ratios), "max", ratios.max())
        assert np.median(ratios) <= 2.5 and ratios.max() <= 10.0, (what, name, np.median(ratios), ratios.max())


def _reference(ops, xs, us, cl, al, g):
    args = (ops["F"], ops["f"], ops["C"], ops["c"], ops["low"], ops["high"], xs, us, cl, al, ops["Cfin"], ops["cfin"], *g)
    ref = bref.closed_form(*args)
    r32 = bref.closed_form(*args, dtype=torch.float32)
    return ref, {k: (r32[k].double() - ref[k]).abs() for k in ref}


def _call(ops, xs, us, g, **over):
    from tfmpc.solvers import tvlqr_box_vjp
    dev = "cuda"
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)      # noqa: E731
    p = {k: t(v) for k, v in ops.items()}
    p.update(over)
    return tvlqr_box_vjp(p["F"], p["f"], p["C"], p["c"], p["low"], p["high"], t(xs), t(us), *(t(a) for a in g),
                         C_final=p["Cfin"], c_final=p["cfin"])


def _rename(got):
    out = dict(got)
    for k, v in KEY.items():
        if v in out:
            out[k] = out.pop(v)
    return out


# every shape and horizon under the mixed loss; the single-output losses on the exact matrix-core shape and the generic one
TV_CASES = [(n, m, T, loss) for (n, m) in GPU_TV_SHAPES for T in GPU_TV_HORIZONS for loss in ("mixed", "states", "actions", "costs")
            if loss == "mixed" or (n, m) in ((16, 8), (20, 10))]


@pytest.mark.parametrize("n,m,T,loss", TV_CASES)
def test_box_vjp_on_the_fp64_optimum(n, m, T, loss):
    B = GPU_TV_BATCH
    ops, sol = bref.tv_case(n, m, T, B, final=tv_final(T))
    xs, us = _f32_trajectory(ops, sol)
    g = _upstream(B, T, n, m, loss)
    got = _rename(_call(ops, xs, us, g))
    assert int(got["status"].abs().sum()) == 0
    assert np.array_equal(got["clamped"].cpu().numpy(), sol["clamped"])          # read off the same bits
    ref, r32 = _reference(ops, xs, us, sol["clamped"], sol["at_low"], g)
    _check(got, ref, r32, f"tv {n}x{m} T={T} {loss}")
    # held controls: exactly zero where the math says zero
    cl = torch.as_tensor(sol["clamped"], device="cuda")
    al = torch.as_tensor(sol["at_low"], device="cuda")
    assert bool((got["low"][~(cl & al)] == 0.0).all()) and bool((got["high"][~(cl & ~al)] == 0.0).all())
    if g[2] is None:
        assert bool((got["c"][..., n:][cl] == 0.0).all())
        dC = got["C"].clone()
        if not tv_final(T):
            dC[:, T - 1, :n, :n] = 0.0                                           # (the default final cost's part: x rows only)
        held = torch.cat([torch.zeros(B, T, n, dtype=torch.bool, device="cuda"), cl], -1)
        both = held[..., :, None] & held[..., None, :]
        assert bool((dC[both] == 0.0).all())


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 2), (20, 10, 50)])
def test_shared_operands_and_summed_gradients(n, m, T):
    """One model and one pair of bounds shared by the batch (the gradients are batch sums), and a time axis of 1."""
    B = GPU_TV_BATCH
    ops, _ = bref.tv_case(n, m, T, B, final=tv_final(T))
    sh = {k: (None if v is None else np.repeat(v[:1], B, axis=0)) for k, v in ops.items() if k != "x0"}
    sh["x0"] = ops["x0"]
    sh["low"], sh["high"] = sh["low"][:, :1].repeat(T, axis=1), sh["high"][:, :1].repeat(T, axis=1)     # constant in time
    sol = bref.solve_box_batch(sh["F"], sh["f"], sh["C"], sh["c"], sh["x0"], sh["low"], sh["high"], sh["Cfin"], sh["cfin"])
    xs, us = _f32_trajectory(sh, sol)
    g = _upstream(B, T, n, m, "mixed")
    ref, r32 = _reference(sh, xs, us, sol["clamped"], sol["at_low"], g)
    t = lambda a: torch.as_tensor(a[0], dtype=torch.float32, device="cuda")      # noqa: E731
    over = {k: t(sh[k]) for k in ("F", "f", "C", "c")}
    over.update(low=t(sh["low"])[:1], high=t(sh["high"])[0, :])                   # [1, m] and [m]
    if sh["Cfin"] is not None:
        over.update(Cfin=t(sh["Cfin"]), cfin=t(sh["cfin"]))
    got = _rename(_call(sh, xs, us, g, **over))
    assert np.array_equal(got["clamped"].cpu().numpy(), sol["clamped"])
    sums = [(k, (0,)) for k in ("F", "f", "C", "c", "Cfin", "cfin")] + [("low", (0, 1)), ("high", (0, 1))]
    _check(got, ref, r32, f"shared {n}x{m} T={T}", sums=sums)
    again = _rename(_call(sh, xs, us, g, **over))                                  # fixed-order sums: the same bits
    for k in ref:
        assert torch.equal(got[k], again[k]), k
    # a time axis of 1 on a per-instance model: sums over time
    if T > 1:
        ti = {k: np.repeat(v[:, :1], T, axis=1) for k, v in ops.items() if k in ("F", "f", "C", "c", "low", "high")}
        ti.update(x0=ops["x0"], Cfin=ops["Cfin"], cfin=ops["cfin"])
        ti["F"] = (0.6 * ti["F"]).astype(np.float32).astype(np.float64)      # one step's draw held for T steps: keep it stable
        sol = bref.solve_box_batch(ti["F"], ti["f"], ti["C"], ti["c"], ti["x0"], ti["low"], ti["high"], ti["Cfin"], ti["cfin"])
        xs, us = _f32_trajectory(ti, sol)
        ref, r32 = _reference(ti, xs, us, sol["clamped"], sol["at_low"], g)
        t1 = lambda a: torch.as_tensor(a[:, :1], dtype=torch.float32, device="cuda")      # noqa: E731
        got = _rename(_call(ti, xs, us, g, **{k: t1(ti[k]) for k in ("F", "f", "C", "c", "low", "high")}))
        _check(got, ref, r32, f"time-1 {n}x{m} T={T}", sums=[(k, (1,)) for k in ("F", "f", "C", "c", "low", "high")])


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 20), (20, 10, 10)])
def test_no_control_held_is_the_plain_vjp_and_all_held_is_finite(n, m, T):
    from tfmpc.solvers import tvlqr_solve
    B = GPU_TV_BATCH
    ops, _ = bref.tv_case(n, m, T, B)
    g = _upstream(B, T, n, m, "mixed")
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")      # noqa: E731
    leaves = {k: t(ops[k]).requires_grad_() for k in ("F", "f", "C", "c", "x0")}
    xs, us, cs = tvlqr_solve(leaves["F"], leaves["f"], leaves["C"], leaves["c"], leaves["x0"])
    loss = (xs[..., 0] * t(g[0])).sum() + (us[..., 0] * t(g[1])).sum() + (cs[..., 0, 0] * t(g[2])).sum()
    plain = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    xs64, us64 = xs.detach()[..., 0].double().cpu().numpy(), us.detach()[..., 0].double().cpu().numpy()
    none = np.zeros((B, T, m), bool)
    for lo, hi in ((-np.inf, np.inf), (-1e6, 1e6)):
        un = dict(ops, low=np.full((B, T, m), lo), high=np.full((B, T, m), hi))
        got = _rename(_call(un, xs64, us64, g))
        assert not bool(got["clamped"].any())
        ref, r32 = _reference(un, xs64, us64, none, none, g)
        _check(got, ref, r32, f"free {n}x{m} T={T}")
        _check(plain, ref, r32, f"plain {n}x{m} T={T}")
        print("same bits as tfmpc_tvlqr_vjp_f32:", {k: bool(torch.equal(plain[k].reshape(got[k].shape), got[k])) for k in plain})
        assert float(got["low"].abs().max()) == 0.0 and float(got["high"].abs().max()) == 0.0
    # every control held at every step: the trajectory is the rollout of the bound
    lo = np.full((B, T, m), -0.25)
    al = np.ones((B, T, m), bool)
    al[:, ::2] = False
    hi = np.full((B, T, m), 0.25)
    us_all = np.where(al, lo, hi)
    xs_all = np.empty((B, T + 1, n))
    xs_all[:, 0] = ops["x0"]
    for s in range(T):
        z = np.concatenate([xs_all[:, s], us_all[:, s]], -1)
        xs_all[:, s + 1] = np.einsum("bij,bj->bi", ops["F"][:, s], z) + ops["f"][:, s]
    xs_all = xs_all.astype(np.float32).astype(np.float64)
    held = dict(ops, low=lo, high=hi)
    got = _rename(_call(held, xs_all, us_all, g))
    assert bool(got["clamped"].all()) and all(bool(torch.isfinite(got[k]).all()) for k in NAMES if k in got)
    ref, r32 = _reference(held, xs_all, us_all, np.ones((B, T, m), bool), al, g)
    _check(got, ref, r32, f"all held {n}x{m} T={T}")


def test_empty_and_single_batches_and_a_flagged_instance():
    n, m, T, B = 5, 3, 6, 4
    ops, sol = bref.tv_case(n, m, T, B)
    xs, us = _f32_trajectory(ops, sol)
    g = _upstream(B, T, n, m, "mixed")
    one = {k: (None if v is None else v[:1]) for k, v in ops.items()}
    got1 = _rename(_call(one, xs[:1], us[:1], tuple(a[:1] for a in g)))
    full = _rename(_call(ops, xs, us, g))
    for k in ("F", "c", "x0", "low", "high"):
        assert torch.equal(got1[k][0], full[k][0]), k
    empty = {k: (None if v is None else v[:0]) for k, v in ops.items()}
    got0 = _call(empty, xs[:0], us[:0], tuple(a[:0] for a in g))
    assert got0["F"].shape[0] == 0 and got0["clamped"].shape == (0, T, m)
    # an adjoint that is not positive definite: NaN in the instance's own rows only, and the status says so
    bad = {k: (None if v is None else v.copy()) for k, v in ops.items()}
    free = np.argwhere(~sol["clamped"][2])
    s, i = free[0]
    bad["C"][2, s, n + i, n + i] = -50.0
    got = _rename(_call(bad, xs, us, g))
    from tfmpc import _hip
    st = got["status"].cpu().numpy()
    assert st[2] & (_hip.ST_NOT_PD | getattr(_hip, "ST_SINGULAR", 0)) and not st[[0, 1, 3]].any()
    for k in ("F", "f", "C", "c", "x0", "low", "high"):
        assert bool(torch.isnan(got[k][2]).all()) and bool(torch.isfinite(got[k][[0, 1, 3]]).all()), k
    shared = _rename(_call(bad, xs, us, g, low=torch.as_tensor(bad["low"][0, 0], dtype=torch.float32, device="cuda")))
    assert bool(torch.isnan(shared["low"]).all())      # a batch sum that contains the flagged instance


def _workload(n, m, T, B=64):
    import workloads
    w = workloads.control_limited_stable(B, n, m, T, 0.5)
    u0 = torch.zeros(T, m, device="cuda")
    return w, u0


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 20)])
def test_box_lqr_solve_end_to_end(n, m, T):
    from tfmpc.envs.lq import LQEnv
    from tfmpc.solvers import box_lqr_solve
    from tfmpc.solvers.ilqr import iLQR
    B = 64
    w, u0 = _workload(n, m, T, B)
    F64, f64, C64, c64 = (np.asarray(w[k], dtype=np.float32).astype(np.float64) for k in ("F", "f", "C", "c"))
    x064 = w["x0"][..., 0].double().cpu().numpy()
    tt = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")      # noqa: E731
    leaves = dict(F=tt(F64), f=tt(f64), C=tt(C64), c=tt(c64), x0=w["x0"].clone(), low=tt(np.full(m, -0.5)), high=tt(np.full(m, 0.5)))
    # without grad: the plain path, bit for bit iLQR(LQEnv).solve's
    res = box_lqr_solve(*(leaves[k] for k in ("F", "f", "C", "c", "x0", "low", "high")), T, atol=1e-6)
    assert not any(t.requires_grad for t in res)
    traj, _ = iLQR(LQEnv(F64, f64, C64, c64, -0.5, 0.5), atol=1e-6).solve(w["x0"], T, show_progress=False, u_init=u0)
    for lf in leaves.values():
        lf.requires_grad_()
    xs, us, cs = box_lqr_solve(*(leaves[k] for k in ("F", "f", "C", "c", "x0", "low", "high")), T, atol=1e-6)
    for a, b_ in ((xs, res[0]), (us, res[1]), (cs, res[2])):
        assert a.requires_grad and torch.equal(a.detach(), b_)
    assert np.array_equal(np.asarray(traj.states).reshape(B, T + 1, n), xs.detach()[..., 0].cpu().numpy())
    assert np.array_equal(np.asarray(traj.actions).reshape(B, T, m), us.detach()[..., 0].cpu().numpy())
    assert np.array_equal(np.asarray(traj.costs).reshape(B, T + 1), cs.detach()[..., 0, 0].cpu().numpy())
    g = _upstream(B, T, n, m, "mixed")
    loss = (xs[..., 0] * tt(g[0])).sum() + (us[..., 0] * tt(g[1])).sum() + (cs[..., 0, 0] * tt(g[2])).sum()
    grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    info = xs.grad_fn is not None and res.info
    assert info.last_status is not None
    # fp64 optimum
    tile = lambda a: bref.tile_time(a, T)      # noqa: E731
    ops = dict(F=tile(F64), f=tile(f64), C=tile(C64), c=tile(c64), x0=x064, low=np.full((B, T, m), -0.5), high=np.full((B, T, m), 0.5),
               Cfin=None, cfin=None)
    sol = bref.solve_box_batch(ops["F"], ops["f"], ops["C"], ops["c"], x064, ops["low"], ops["high"])
    clear = sol["clear"]
    assert (~clear).mean() <= 0.25, (~clear).mean()
    xd, ud = xs.detach()[..., 0].double().cpu().numpy(), us.detach()[..., 0].double().cpu().numpy()
    cld = (ud == -0.5) | (ud == 0.5)
    ald = ud == -0.5
    assert np.array_equal(cld[clear], sol["clamped"][clear])
    scale = max(1.0, np.abs(sol["states"]).max())
    assert np.abs(xd[clear] - sol["states"][clear]).max() <= 2e-3 * scale, np.abs(xd[clear] - sol["states"][clear]).max()
    # (a) against the closed form on the device's own trajectory and held set
    ref, r32 = _reference(ops, xd, ud, cld, ald, g)
    time_sums = [(k, (1,)) for k in ("F", "f", "C", "c")] + [("low", (0, 1)), ("high", (0, 1))]
    _check(grads, ref, r32, f"e2e own trajectory {n}x{m}", sums=time_sums)
    # (b) clear instances against the gradient at the fp64 optimum, the budget widened by the closed form's sensitivity
    # to the measured forward error
    opt, _ = _reference(ops, sol["states"], sol["actions"], sol["clamped"], sol["at_low"], g)
    pick = np.nonzero(clear)[0]
    sub = lambda d_: {k: v[pick] for k, v in d_.items()}      # noqa: E731
    wide = {k: r32[k] + (ref[k] - opt[k]).abs() for k in ref}
    per_instance = {k: grads[k][pick] for k in ("F", "f", "C", "c", "x0")}
    _check(per_instance, sub(opt), sub(wide), f"e2e fp64 optimum {n}x{m}", sums=[(k, (1,)) for k in ("F", "f", "C", "c")])


def test_three_descent_steps_lower_a_tracking_loss():
    from tfmpc.solvers import box_lqr_solve
    n, m, T, B = 5, 3, 20, 16
    w, _ = _workload(n, m, T, B)
    tt = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")      # noqa: E731
    F, f, C = tt(w["F"]), tt(w["f"]), tt(w["C"])
    c = tt(w["c"]).requires_grad_()
    target = torch.zeros(B, T + 1, n, 1, device="cuda")
    losses = []
    for _ in range(4):
        xs, us, _ = box_lqr_solve(F, f, C, c, w["x0"], -0.5, 0.5, T, atol=1e-6)
        loss = ((xs - target) ** 2).mean()
        losses.append(float(loss.detach()))
        grad, = torch.autograd.grad(loss, c)
        with torch.no_grad():
            c -= 0.5 * grad / grad.abs().max()
    print("tracking losses", losses)
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2], losses

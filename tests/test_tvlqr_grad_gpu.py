"""Gradients of the time-varying LQR on the MI355X (tfmpc_tvlqr_vjp_f32 through tfmpc.solvers.tvlqr_solve, LQR.solve and
TimeVaryingLQR.solve) against the fp64 closed form of tests/tvlqr_grad_ref.py.  Budget: the fp32 restatements' own error
against fp64 -- per instance, the median over instances of (kernel error / fp32 error) <= 2.5 and every instance <= 10,
the rule of test_tvlqr_gpu.py.  The fp32 error is the error of fp32 autograd through the recursion -- except for the
costate-built gradients F, f and x0, where it is, elementwise, the larger of that and the error of the closed-form
adjoint the kernels run, restated in fp32.  On the seeded workloads of these tests (T = 2 / 20 / 50) that algorithm is
itself less accurate than autograd there: median 0.9 - 1.9x, up to 16.6x (dF), 16.4x (df) and 19.1x (dx0); for C and
c it is at most 1.8x, so they keep the autograd budget (tests/tvlqr_grad_ref.py).  A gradient summed over the batch or
over time counts as one instance, and its fp32 error is the sum of the absolute errors of the terms it adds up."""
import numpy as np
import pytest
import torch

import tvlqr_grad_ref as gref
import tvlqr_ref
from tfmpc import _hip
from tfmpc.envs import make_lqr
from tfmpc.solvers import TimeVaryingLQR, tvlqr_solve

pytestmark = pytest.mark.gpu

MODEL = ("F", "f", "C", "c")
WIDENED = ("F", "f", "x0")       # the costate-built gradients: budget widened to the fp32 closed form's error


def _weights(B, T, n, m, loss, seed=0):
    rng = np.random.default_rng(seed)
    gx, gu, gc = rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1))
    return tuple(g if loss in (name, "mixed") else None for g, name in ((gx, "states"), (gu, "actions"), (gc, "costs")))


def _loss(states, actions, costs, w):
    total = 0
    for out, g in zip((states[..., 0], actions[..., 0], costs.reshape(costs.shape[:-2])), w):
        if g is not None:
            total = total + (out * torch.as_tensor(g, dtype=torch.float32, device=out.device).reshape(out.shape)).sum()
    return total


def _case(n, m, T, B, shared=(), const=(), final=None, x0_shared=False, loss="mixed", seed=0):
    """Operands as the user passes them (numpy, fp32): 'shared' drop the batch axis, 'const' keep a time axis of 1;
    final None / 'per' / 'shared'.  Also the [B, T, ...] broadcasts the oracle reads."""
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=seed)
    full = dict(F=F, f=f, C=C, c=c)
    user = {}
    for k, a in full.items():
        a = a[:, :1] if k in const else a
        a = a[0] if k in shared else a
        user[k] = np.ascontiguousarray(a)
        b = a if k not in shared else a[None]
        full[k] = np.broadcast_to(b, (B, T) + a.shape[(1 if k in shared else 2):]).copy()
    x0 = tvlqr_ref.make_x0(n, B, seed=seed + 1)
    user["x0"] = x0[0].copy() if x0_shared else x0
    full["x0"] = np.broadcast_to(x0[:1], x0.shape).copy() if x0_shared else x0
    if final is not None:
        Cf, cf = tvlqr_ref.make_final(n, B, seed=seed + 2)
        if final == "shared":
            Cf, cf = np.repeat(Cf[:1], B, 0), np.repeat(cf[:1], B, 0)
            user.update(Cfin=Cf[0].copy(), cfin=cf[0].copy())
        else:
            user.update(Cfin=Cf, cfin=cf)
        full.update(Cfin=Cf, cfin=cf)
    return user, full, _weights(B, T, n, m, loss, seed=seed + 3)


def _reduce(g, name, user, B):
    """Per-instance [B, T, ...] oracle gradient -> the user's operand shape (sum over a missing batch axis and over a
    time axis of 1)."""
    shape = user[name].shape
    if len(shape) < g.dim():
        g = g.sum(0)
    if name in MODEL:
        tdim = 1 if len(shape) == (4 if name in ("F", "C") else 3) else 0
        if shape[tdim] == 1 and g.shape[tdim] != 1:
            g = g.sum(tdim, keepdim=True)
    return g


def _oracles(user, full, w):
    B = full["x0"].shape[0]
    args = [full[k] for k in ("F", "f", "C", "c", "x0")] + [full.get("Cfin"), full.get("cfin")]
    g64 = gref.closed_form(*args, *w)
    a32 = gref.autograd_grads(*args, *w, dtype=torch.float32)
    c32 = gref.closed_form(*args, *w, dtype=torch.float32)
    # the fp32 error of a summed gradient is bounded by the sum of the per-instance (per-step) errors it adds up:
    # cancellation in one restatement's sum is luck, not accuracy
    err = {k: (a32[k].double() - g64[k]).abs() for k in g64}
    for k in WIDENED:
        err[k] = torch.maximum(err[k], (c32[k].double() - g64[k]).abs())
    return {k: _reduce(g64[k], k, user, B) for k in g64}, {k: _reduce(err[k], k, user, B) for k in g64}


def _kernel_grads(user, w, solver="functional"):
    ops = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in user.items()}
    if solver == "functional":
        states, actions, costs = tvlqr_solve(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops.get("Cfin"), ops.get("cfin"))
    else:
        tv = TimeVaryingLQR(ops["F"], ops["f"], ops["C"], ops["c"], ops.get("Cfin"), ops.get("cfin"), device="cuda")
        traj = tv.solve(ops["x0"])
        states, actions, costs = traj.states[..., None], traj.actions[..., None], traj.costs[..., None, None]
    assert states.requires_grad
    _loss(states, actions, costs, w).backward()
    torch.cuda.synchronize()
    return {k: t.grad.double().cpu() for k, t in ops.items()}


def _check(got, g64, e32, user, what=""):
    B = np.asarray(user["x0"]).shape[0] if np.asarray(user["x0"]).ndim == 2 else None
    for name in g64:
        ref, r32, k = g64[name], e32[name], got[name]
        assert k.shape == ref.shape, (what, name, k.shape, ref.shape)
        assert bool(torch.isfinite(k).all()), (what, name)
        per = name in ("x0", "Cfin", "cfin") and k.dim() == (2 if name in ("x0", "cfin") else 3) or \
            name in MODEL and k.dim() == (4 if name in ("F", "C") else 3)
        items = range(k.shape[0]) if per and B is not None else [None]
        ratios = []
        for b in items:
            sel = (lambda t: t) if b is None else (lambda t, b=b: t[b])   # noqa: E731
            scale = max(1.0, float(sel(ref).abs().max()))
            budget = max(float(sel(r32).max()), 1e-6 * scale)
            ratios.append(float((sel(k) - sel(ref)).abs().max()) / budget)
        ratios = np.array(ratios)
        assert np.median(ratios) <= 2.5 and ratios.max() <= 10.0, (what, name, np.median(ratios), ratios.max())


@pytest.mark.parametrize("T", [1, 2, 50])
@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (12, 6), (20, 10)])
def test_per_instance_shapes_and_horizons(n, m, T):
    user, full, w = _case(n, m, T, 5, seed=n + m + T)
    got = _kernel_grads(user, w)
    _check(got, *_oracles(user, full, w), user, what=(n, m, T))


@pytest.mark.parametrize("loss", ["states", "actions", "costs", "mixed"])
@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
@pytest.mark.parametrize("sharing", ["batch", "time", "both", "mixed"])
def test_shared_operands_and_losses(n, m, sharing, loss):
    kw = dict(batch=dict(shared=MODEL), time=dict(const=("F", "f", "C")), both=dict(shared=MODEL, const=("F", "C", "c")),
              mixed=dict(shared=("C", "c"), const=("f", "C"), x0_shared=True))[sharing]
    user, full, w = _case(n, m, 20, 6, loss=loss, seed=7, **kw)
    got = _kernel_grads(user, w)
    _check(got, *_oracles(user, full, w), user, what=(sharing, loss))


@pytest.mark.parametrize("final", ["per", "shared"])
@pytest.mark.parametrize("T", [1, 50])
@pytest.mark.parametrize("n,m", [(16, 8), (12, 6), (20, 10)])
def test_explicit_final_cost(n, m, T, final):
    user, full, w = _case(n, m, T, 4, final=final, seed=11)
    got = _kernel_grads(user, w, solver="class")
    g64, g32 = _oracles(user, full, w)
    assert "Cfin" in g64 and "Cfin" in got
    _check(got, g64, g32, user, what=("final", final))
    user, full, w = _case(n, m, T, 4, final=final, x0_shared=True, shared=("F",), seed=12)
    _check(_kernel_grads(user, w), *_oracles(user, full, w), user, what=("final, shared x0", final))


@pytest.mark.parametrize("n,m", [(16, 8), (12, 6)])
def test_lqr_solve_gradients_match_from_lqr_and_the_oracle(n, m):
    B, T = 6, 30
    np.random.seed(3)
    lqr = make_lqr(n, m, batch_size=B)
    sym = 0.5 * (lqr.C + lqr.C.transpose(-1, -2))
    base = dict(F=lqr.F.cpu().numpy(), f=lqr.f.cpu().numpy()[..., 0], C=sym.cpu().numpy(), c=lqr.c.cpu().numpy()[..., 0])
    x0 = tvlqr_ref.make_x0(n, B)
    w = _weights(B, T, n, m, "mixed", seed=4)
    from tfmpc.solvers.lqr import LQR
    ops = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in base.items()}
    x0t = torch.as_tensor(x0, device="cuda").requires_grad_()
    traj = LQR(ops["F"], ops["f"], ops["C"], ops["c"], device="cuda").solve(x0t, T)
    _loss(traj.states[..., None], traj.actions[..., None], traj.costs[..., None, None], w).backward()
    got = {k: t.grad.double().cpu() for k, t in ops.items()}
    got["x0"] = x0t.grad.double().cpu()
    # the same problem as TimeVaryingLQR.from_lqr poses it: views with time stride 0 (autograd sums their gradients)
    leaves = {k: torch.as_tensor(v[:, None], device="cuda").requires_grad_() for k, v in base.items()}
    views = [leaves[k].expand(B, T, *leaves[k].shape[2:]) for k in MODEL]
    s, a, cs = tvlqr_solve(*views, torch.as_tensor(x0, device="cuda"))
    _loss(s, a, cs, w).backward()
    user = {k: v[:, None] for k, v in base.items()}
    user["x0"] = x0
    full = {k: np.repeat(v[:, None], T, axis=1) for k, v in base.items()}
    full["x0"] = x0
    g64, g32 = _oracles(user, full, w)
    tvg = {k: leaves[k].grad.double().cpu() for k in MODEL}
    got_tv = dict(got, **{k: got[k][:, None] for k in MODEL})
    _check(got_tv, g64, g32, user, what="LQR")
    _check(dict(got_tv, **tvg), g64, g32, user, what="from_lqr")
    # LQR's forward is its own kernel: the same bits as without grad
    with torch.no_grad():
        plain = LQR(base["F"], base["f"], base["C"], base["c"], device="cuda").solve_device(torch.as_tensor(x0, device="cuda"), T)
    assert torch.equal(plain["states"][..., 0], traj.states.detach())


def test_shared_gradients_are_bitwise_reproducible():
    user, full, w = _case(16, 8, 50, 700, shared=MODEL, final="shared", seed=5)
    a, b = _kernel_grads(user, w), _kernel_grads(user, w)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    user, _, w = _case(20, 10, 9, 300, shared=("F", "C"), const=("c",), seed=6)
    a, b = _kernel_grads(user, w), _kernel_grads(user, w)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_batch_zero_and_one(n, m):
    T = 9
    user, full, w = _case(n, m, T, 1, seed=29)
    got = _kernel_grads(user, w)
    _check(got, *_oracles(user, full, w), user, what="B=1")
    # unbatched operands and x0: gradients without the batch axis, equal to the B = 1 ones
    un = {k: v[0] for k, v in user.items()}
    w1 = tuple(None if g is None else g[0] for g in w)
    ops = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in un.items()}
    s, a, c = tvlqr_solve(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"])
    assert s.shape == (T + 1, n, 1)
    _loss(s, a, c, w1).backward()
    # unbatched operands take the batch reduction (matrix cores for n <= 16), B = 1 the per-instance sweep: the same
    # sums, rounded differently (about one ulp)
    for k in ops:
        assert ops[k].grad.shape == ops[k].shape
        torch.testing.assert_close(ops[k].grad.double().cpu(), got[k][0], rtol=1e-5, atol=1e-5 * max(1.0, float(got[k].abs().max())))
    # B = 0
    F, f, C, c = (torch.as_tensor(v[:0], device="cuda").requires_grad_() for v in (user["F"], user["f"], user["C"], user["c"]))
    x0 = torch.zeros((0, n), device="cuda", requires_grad=True)
    s, a, cs = tvlqr_solve(F, f, C, c, x0)
    assert s.shape == (0, T + 1, n, 1)
    (s.sum() + a.sum() + cs.sum()).backward()
    assert F.grad.shape == F.shape and x0.grad.shape == x0.shape


@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_not_pd_instance_gets_nan_in_its_own_rows(n, m):
    B, T = 4, 20
    user, _, w = _case(n, m, T, B, seed=23)
    user["C"] = user["C"].copy()
    user["C"][2, 7, n:, n:] = -1.0e4 * np.eye(m, dtype=np.float32)
    ops = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in user.items()}
    tv = TimeVaryingLQR(ops["F"], ops["f"], ops["C"], ops["c"], device="cuda")
    traj = tv.solve(ops["x0"])
    _loss(traj.states[..., None], traj.actions[..., None], traj.costs[..., None, None], w).backward()
    torch.cuda.synchronize()
    st = tv.last_grad_status.cpu().numpy()
    assert st[2] & _hip.ST_NOT_PD and (st[[0, 1, 3]] == 0).all(), st
    for k, t in ops.items():
        g = t.grad
        assert bool(torch.isnan(g[2]).all()), k
        assert bool(torch.isfinite(g[[0, 1, 3]]).all()), k
    # a gradient summed over the batch includes it: NaN
    Fs = torch.as_tensor(user["F"][0], device="cuda").requires_grad_()
    traj = TimeVaryingLQR(Fs, *(torch.as_tensor(user[k], device="cuda") for k in ("f", "C", "c")), device="cuda").solve(
        torch.as_tensor(user["x0"], device="cuda"))
    traj.total_cost.sum().backward()
    assert bool(torch.isnan(Fs.grad).all())


@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_outputs_without_grad_are_the_plain_path(n, m):
    user, _, w = _case(n, m, 30, 5, shared=("C",), seed=31)
    plain = TimeVaryingLQR(*(user[k] for k in MODEL), device="cuda").solve_device(torch.as_tensor(user["x0"], device="cuda"))
    ops = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in user.items()}
    traj = TimeVaryingLQR(*(ops[k] for k in MODEL), device="cuda").solve(ops["x0"])
    with torch.no_grad():
        ng = TimeVaryingLQR(*(ops[k] for k in MODEL), device="cuda").solve(ops["x0"])
    torch.cuda.synchronize()
    assert isinstance(ng.states, np.ndarray)
    np.testing.assert_array_equal(ng.states, plain["states"][..., 0].cpu().numpy())
    assert torch.equal(traj.states.detach(), plain["states"][..., 0])
    assert torch.equal(traj.actions.detach(), plain["actions"][..., 0])
    assert torch.equal(traj.costs.detach(), plain["costs"][..., 0, 0])
    # a dtype / device conversion goes through autograd: fp64 CPU operands get fp64 CPU gradients
    F64 = torch.as_tensor(user["F"], dtype=torch.float64).requires_grad_()
    s, a, c = tvlqr_solve(F64, user["f"], user["C"], user["c"], torch.as_tensor(user["x0"], device="cuda"))   # numpy f, C, c
    c.sum().backward()
    assert F64.grad.dtype == torch.float64 and F64.grad.device.type == "cpu"
    with pytest.raises(RuntimeError):               # double backward
        F2 = torch.as_tensor(user["F"], device="cuda").requires_grad_()
        s, a, c = tvlqr_solve(F2, *(torch.as_tensor(user[k], device="cuda") for k in ("f", "C", "c", "x0")))
        (g,) = torch.autograd.grad(c.sum(), F2, create_graph=True)
        g.sum().backward()


def _full_size(sample):
    B, n, m, T, P = 65536, 16, 8, 50, 64
    user, full, w = _case(n, m, T, P, seed=37)
    rep = lambda a: torch.as_tensor(a, device="cuda").repeat(B // P, *([1] * (a.ndim - 1)))     # noqa: E731
    ops = {k: rep(v).requires_grad_() for k, v in user.items()}
    wt = tuple(None if g is None else rep(g.astype(np.float32)) for g in w)
    s, a, c = tvlqr_solve(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"])
    _loss(s, a, c, [None if g is None else g.cpu().numpy() for g in wt]).backward()
    torch.cuda.synchronize()
    for k, t in ops.items():
        assert bool(torch.isfinite(t.grad).all()), k
    g64, g32 = _oracles(user, full, w)
    idx = np.arange(B) if sample is None else np.random.default_rng(0).choice(B, size=sample, replace=False)
    for k, t in ops.items():
        got = t.grad[torch.as_tensor(idx, device="cuda")].double().cpu()
        pool = torch.as_tensor(idx % P)
        sub = {kk: vv[pool] for kk, vv in g64.items()}, {kk: vv[pool] for kk, vv in g32.items()}
        _check({k: got}, {k: sub[0][k]}, {k: sub[1][k]}, {"x0": np.zeros((len(idx), n))}, what=("full", k))


def test_full_size_sampled():
    _full_size(96)


@pytest.mark.slow
def test_full_size_every_instance():
    _full_size(None)

"""Gradients of the finite-horizon Riccati recursion on the MI355X (tfmpc.solvers.tvlqr_backward:
tfmpc_tvlqr_backward_f32 forward, tfmpc_tvlqr_backward_vjp_f32 backward) against the fp64 closed form of
tests/tvlqr_backward_grad_ref.py, which tests/test_tvlqr_backward_grad_cpu.py pins to fp64 autograd through the
recursion.  Budget (the project's rule, as tests/test_lqr_steady_state_grad_gpu.py): the larger of two fp32 errors of the
restatement against fp64 -- its own fp32 forward and sweep, and its fp32 sweep started from the kernel's K, k, V, v (the
sweep cannot undo the error of the outputs it is handed) -- with a floor of 1e-6 of the gradient's scale; the median over
instances of (kernel error / budget) <= 2.5 and every instance <= 10.  A gradient summed over the batch or over time has
as budget the sum of its terms' budgets.  Every case prints its measured ratios (DESIGN.md 3.12 quotes them)."""

import numpy as np
import pytest
import torch

import tvlqr_backward_grad_ref as bref
import tvlqr_grad_ref
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR, tvlqr_backward, tvlqr_solve
from tfmpc.solvers.lqr import LQR

pytestmark = pytest.mark.gpu

OPS = ("F", "f", "C", "c", "Cfin", "cfin")
GRAD_OF = dict(F="dF", f="df", C="dC", c="dc", Cfin="dCfin", cfin="dcfin")
OUTS = ("K", "k", "V", "v", "const")


def _leaves(**ops):
    return {name: (None if a is None else torch.as_tensor(a, device="cuda").requires_grad_()) for name, a in ops.items()}


def _loss(outs, up):
    total = 0
    for out, g in zip(outs, (up[name] for name in bref.UPS)):
        if g is not None:
            total = total + (out * torch.as_tensor(g, device=out.device).reshape(out.shape)).sum()
    return total


def _kernel(leaves, up):
    """leaves: name -> cuda tensor requiring grad (or None).  Returns (grads by operand name as float64 numpy, the
    kernel's forward outputs as the restatement's fp32 ``fwd`` dict)."""
    outs = tvlqr_backward(*(leaves[name] for name in OPS))
    _loss(outs, up).backward()
    torch.cuda.synchronize()
    got = {name: t.grad.double().cpu().numpy() for name, t in leaves.items() if t is not None}
    fwd = {name: o.detach().float().cpu().numpy() for name, o in zip(OUTS, outs)}
    B, T, m, n = fwd["K"].shape
    fwd.update(k=fwd["k"].reshape(B, T, m), v=fwd["v"].reshape(B, T, n), status=np.zeros(B, np.int32))
    return got, fwd


def _refs(F, f, C, c, Cf, cf, up, fwd=None):
    """Fully expanded [B, T, ...] model -> (fp64 gradients, the fp32 budget's elementwise absolute errors)."""
    g64 = bref.closed_form(F, f, C, c, Cf, cf, **up)
    assert (g64["status"] == 0).all()
    runs = [bref.closed_form(F, f, C, c, Cf, cf, **up, dtype=np.float32)]
    if fwd is not None:
        runs.append(bref.closed_form(F, f, C, c, Cf, cf, **up, dtype=np.float32, fwd=fwd))
    err = {}
    for name in bref.GRADS:
        if g64[name] is not None:
            err[name] = np.max([np.abs(r[name].astype(np.float64) - g64[name]) for r in runs], axis=0)
    return g64, err


def _ratios(got, ref, err):
    """Per leading (instance) index: max error / budget."""
    out = []
    for b in range(ref.shape[0]):
        budget = max(float(err[b].max()), 1e-6 * max(1.0, float(np.abs(ref[b]).max())))
        g = got[b].reshape(ref[b].shape)
        assert np.isfinite(g).all(), b
        out.append(float(np.abs(g - ref[b]).max()) / budget)
    return np.array(out)


def _check(got, g64, err, names, what):
    for name in names:
        key = GRAD_OF[name]
        r = _ratios(got[name], g64[key], err[key])
        print(what, key, "error / budget: median %.2f max %.2f" % (np.median(r), r.max()))
        assert np.median(r) <= 2.5 and r.max() <= 10.0, (what, name, np.median(r), r.max())


def _check_summed(got, ref, err, what):
    """One summed gradient: ``ref`` and ``err`` already summed over the shared axes (budget = the sum of the terms')."""
    budget = max(float(err.max()), 1e-6 * max(1.0, float(np.abs(ref).max())))
    g = got.reshape(ref.shape)
    assert np.isfinite(g).all(), what
    ratio = float(np.abs(g - ref).max()) / budget
    print(what, "summed error / budget: %.2f" % ratio)
    assert ratio <= 10.0, (what, ratio)


SHAPES = [(16, 8, 1, "tvb_vjp_mfma_16"), (16, 8, 2, "tvb_vjp_mfma_16"), (16, 8, 20, "tvb_vjp_mfma_16"),
          (5, 3, 7, "tvb_vjp_mfma_16 (padded)"), (1, 1, 3, "tvb_vjp_mfma_16 (padded)"), (16, 16, 3, "tvb_vjp_mfma_16"),
          (17, 8, 3, "tvb_vjp_mfma_32"), (32, 16, 4, "tvb_vjp_mfma_32")]


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("n,m,T,kernel", SHAPES)
def test_gradients_per_instance_and_step(n, m, T, kernel, final):
    assert _hip.load().tfmpc_tvlqr_backward_vjp_kernel_name(n, m, T).decode() == kernel
    B = 3
    F, f, C, c, Cf, cf = bref.problem(n, m, T, B, seed=n + m + T, final=final)
    up = bref.upstream(n, m, T, B, seed=n)
    leaves = _leaves(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf)
    got, fwd = _kernel(leaves, up)
    g64, err = _refs(F, f, C, c, Cf, cf, up, fwd)
    _check(got, g64, err, [name for name in OPS if leaves[name] is not None], (n, m, T, final))


STRIDE_SHAPES = [(16, 8, 4), (5, 3, 4)]


@pytest.mark.parametrize("n,m,T", STRIDE_SHAPES)
def test_time_stride_zero_sums_over_time(n, m, T):
    """F, f, C with a time axis of size 1: held in time, their gradients accumulated inside the sweep (c keeps its T
    steps, which set the horizon).  Held to the fp64 time sum, and to the time sum of the per-step run of the same
    (expanded) model, within the summed budget."""
    B = 3
    F, f, C, _, Cf, cf = bref.problem(n, m, 1, B, seed=3 + n, final=True)
    c = np.random.default_rng(n).normal(size=(B, T, n + m)).astype(np.float32)
    up = bref.upstream(n, m, T, B, seed=7)
    got, fwd = _kernel(_leaves(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf), up)
    rep = lambda a: np.repeat(a, T, axis=1)          # noqa: E731
    g64, err = _refs(rep(F), rep(f), rep(C), c, Cf, cf, up, fwd)
    steps, _ = _kernel(_leaves(F=rep(F), f=rep(f), C=rep(C), c=c, Cfin=Cf, cfin=cf), up)
    for name in ("F", "f", "C"):
        key = GRAD_OF[name]
        assert got[name].shape[1] == 1
        r = _ratios(got[name][:, 0], g64[key].sum(1), err[key].sum(1))
        print((n, m, T), key, "time-summed error / budget: median %.2f max %.2f" % (np.median(r), r.max()))
        assert np.median(r) <= 2.5 and r.max() <= 10.0, (name, r)
        r2 = _ratios(got[name][:, 0], steps[name].sum(1), 2.0 * err[key].sum(1))
        assert r2.max() <= 10.0, (name, r2)
    _check(got, g64, err, ("c", "Cfin", "cfin"), (n, m, T, "time stride 0"))


@pytest.mark.parametrize("B", [3, 257])
@pytest.mark.parametrize("n,m,T", STRIDE_SHAPES)
def test_batch_stride_zero_sums_over_the_batch(n, m, T, B):
    """F, f, C (and an explicit C_final) shared by the batch, c and c_final per instance; 257 instances are one past
    the reduction's 256-instance chunk."""
    final = n == 5
    F, f, C, _, Cf, _ = bref.problem(n, m, T, 1, seed=5 + n, final=final)
    rng = np.random.default_rng(B)
    c = rng.normal(size=(B, T, n + m)).astype(np.float32)
    cf = rng.normal(size=(B, n)).astype(np.float32) if final else None
    up = bref.upstream(n, m, T, B, seed=9)
    leaves = _leaves(F=F[0], f=f[0], C=C[0], c=c, Cfin=Cf[0] if final else None, cfin=cf)
    got, fwd = _kernel(leaves, up)
    assert got["F"].shape == (T, n, n + m) and got["c"].shape == (B, T, n + m)
    rep = lambda a: np.repeat(a, B, axis=0)          # noqa: E731
    g64, err = _refs(rep(F), rep(f), rep(C), c, rep(Cf) if final else None, cf, up, fwd)
    for name in ("F", "f", "C") + (("Cfin",) if final else ()):
        key = GRAD_OF[name]
        _check_summed(got[name], g64[key].sum(0), err[key].sum(0), (n, m, T, B, key))
    _check(got, g64, err, ("c",) + (("cfin",) if final else ()), (n, m, T, B))
    again, _ = _kernel(_leaves(F=F[0], f=f[0], C=C[0], c=c, Cfin=Cf[0] if final else None, cfin=cf), up)
    for name in got:
        assert np.array_equal(got[name], again[name]), name                       # the same bits on every call


@pytest.mark.parametrize("n,m,T", STRIDE_SHAPES)
def test_default_against_explicit_final_cost(n, m, T):
    """The default final cost is C_{T-1}[:n,:n], c_{T-1}[:n]: its gradient lands in dC[T-1][:n,:n] and dc[T-1][:n]."""
    B = 3
    F, f, C, c, _, _ = bref.problem(n, m, T, B, seed=11 + n)
    up = bref.upstream(n, m, T, B, seed=2)
    dflt, fwd = _kernel(_leaves(F=F, f=f, C=C, c=c, Cfin=None, cfin=None), up)
    Cf, cf = C[:, T - 1, :n, :n].copy(), c[:, T - 1, :n].copy()
    expl, fwd_e = _kernel(_leaves(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf), up)
    g64, err = _refs(F, f, C, c, None, None, up, fwd)
    e64, err_e = _refs(F, f, C, c, Cf, cf, up, fwd_e)
    _check(dflt, g64, err, ("F", "f", "C", "c"), (n, m, T, "default"))
    _check(expl, e64, err_e, OPS, (n, m, T, "explicit"))
    # the two runs differ by where the final cost's gradient goes
    moved_C, moved_c = expl["C"].copy(), expl["c"].copy()
    moved_C[:, T - 1, :n, :n] += expl["Cfin"]
    moved_c[:, T - 1, :n] += expl["cfin"]
    assert np.abs(e64["dCfin"]).max() > 1e-3
    for name, moved in (("C", moved_C), ("c", moved_c)):
        key = GRAD_OF[name]
        both = err[key] + err_e[key]
        if name == "C":
            both[:, T - 1, :n, :n] += err_e["dCfin"]
        else:
            both[:, T - 1, :n] += err_e["dcfin"]
        assert _ratios(dflt[name], moved, both).max() <= 10.0, name
    for name in ("F", "f"):
        assert _ratios(dflt[name], expl[name], err[GRAD_OF[name]] + err_e[GRAD_OF[name]]).max() <= 10.0, name


@pytest.mark.parametrize("subset", ["gK", "value at t = 0"])
def test_upstream_subsets(subset):
    n, m, T, B = 16, 8, 4, 3
    F, f, C, c, Cf, cf = bref.problem(n, m, T, B, seed=21, final=True)
    if subset == "gK":
        up = bref.upstream(n, m, T, B, seed=4, only=("gK",))
    else:
        up = bref.upstream(n, m, T, B, seed=4, only=("gV", "gv", "gconst"))
        for name in ("gV", "gv", "gconst"):
            up[name][:, 1:] = 0.0
    leaves = _leaves(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf)
    got, fwd = _kernel(leaves, up)
    g64, err = _refs(F, f, C, c, Cf, cf, up, fwd)
    _check(got, g64, err, OPS, subset)
    if subset != "gK":           # only step 0 depends on nothing later: every later step's adjoint is carried from it
        assert np.abs(got["F"][:, T - 1]).max() > 0


def _abi_call(lib, B, n, m, T, model, fwd, ups, outs, status, ws=None):
    """tfmpc_tvlqr_backward_vjp_f32 on contiguous per-instance, per-step tensors (default final cost)."""
    d = n + m
    args = []
    for t, size in zip(model, (n * d, n, d * d, d)):
        args += [_hip.ptr(t), T * size, size]
    args += [None, 0, None, 0]
    out_args = []
    for t, size in zip(outs, (n * d, n, d * d, d)):
        out_args += [_hip.ptr(t), T * size, size]
    rc = lib.tfmpc_tvlqr_backward_vjp_f32(B, n, m, T, *args, *(_hip.ptr(t) for t in fwd), *(_hip.ptr(t) for t in ups),
                                          *out_args, None, 0, None, 0, _hip.ptr(status), _hip.ptr(ws),
                                          0 if ws is None else ws.numel() * 4, _hip.stream())
    torch.cuda.synchronize()
    return rc


def test_all_upstream_null_gives_exact_zeros():
    n, m, T, B = 5, 3, 4, 3
    d = n + m
    F, f, C, c, _, _ = bref.problem(n, m, T, B, seed=31)
    tv = TimeVaryingLQR(F, f, C, c, device="cuda")
    pol, val = tv.backward()
    model = [tv.F, tv.f, tv.C, tv.c]
    outs = [torch.full((B, T, size), 7.0, device="cuda") for size in (n * d, n, d * d, d)]
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rc = _abi_call(_hip.load(), B, n, m, T, model, [pol.K, pol.k, val.V, val.v, tv.last_status], [None] * 5, outs, status)
    assert rc == 0 and (status.cpu().numpy() == 0).all()
    for t in outs:
        assert (t == 0).all()


def test_flagged_instance_is_isolated():
    """Instance 1 of 3 has an indefinite C_uu at one step: NaN in its own rows and in the batch sums, its status set,
    its neighbours' gradients the bits of a run without it."""
    n, m, T, B = 16, 8, 4, 3
    F, f, C, c, _, _ = bref.problem(n, m, T, B, seed=41)
    Cb = C.copy()
    Cb[1, 2, n:, n:] = -np.eye(m, dtype=np.float32)
    up = bref.upstream(n, m, T, B, seed=6)
    keep = [0, 2]

    def run(F, f, C, c, up, mask):
        leaves = _leaves(F=F, f=f, C=C, c=c)
        tv = TimeVaryingLQR(*leaves.values(), device="cuda")
        pol, val = tv.backward(differentiable=True)
        outs = [torch.nan_to_num(o, nan=0.0) * mask.reshape(-1, 1, 1, 1) for o in (pol.K, pol.k, val.V, val.v, val.const)]
        _loss(outs, up).backward()
        torch.cuda.synchronize()
        return {name: t.grad.double().cpu().numpy() for name, t in leaves.items()}, tv

    mask = torch.tensor([1.0, 0.0, 1.0], device="cuda")
    got, tv = run(F, f, Cb, c, up, mask)
    assert tv.last_status.cpu().numpy()[1] != 0
    st = tv.last_grad_status.cpu().numpy()
    assert st[1] & _hip.ST_NOT_PD and st[0] == 0 and st[2] == 0, st
    clean, _ = run(F[keep], f[keep], C[keep], c[keep], {k: v[keep] for k, v in up.items()}, torch.ones(2, device="cuda"))
    for name in ("F", "f", "C", "c"):
        assert np.isnan(got[name][1]).all(), name
        assert np.array_equal(got[name][keep], clean[name]), name
    # a flagged instance poisons every gradient summed over its batch
    Fs = torch.as_tensor(F[0], device="cuda").requires_grad_()
    tv2 = TimeVaryingLQR(Fs, f, Cb, c, device="cuda")
    pol, val = tv2.backward(differentiable=True)
    (torch.nan_to_num(val.V, nan=0.0) * mask.reshape(-1, 1, 1, 1)).sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(Fs.grad).all()
    st2 = tv2.last_grad_status.cpu().numpy()
    assert st2[1] != 0 and st2[0] == 0 and st2[2] == 0, st2


def test_bits_and_the_lqr_front_end():
    n, m, T, B = 16, 8, 4, 3
    F, f, C, c, _, _ = bref.problem(n, m, 1, B, seed=51)
    F, f, C, c = F[:, 0], f[:, 0], C[:, 0], c[:, 0]
    up = bref.upstream(n, m, T, B, seed=8)

    def via_lqr():
        leaves = _leaves(F=F, f=f, C=C, c=c)
        lqr = LQR(*leaves.values(), device="cuda")
        pol, val = lqr.backward(T, differentiable=True)
        outs = (pol.K, pol.k, val.V, val.v, val.const)
        _loss(outs, up).backward()
        torch.cuda.synchronize()
        return {name: t.grad.double().cpu().numpy() for name, t in leaves.items()}, outs, lqr

    a, outs, lqr = via_lqr()
    b, _, _ = via_lqr()
    for name in a:
        assert np.array_equal(a[name], b[name]), name                 # two calls: identical bits
    assert (lqr.last_grad_status.cpu().numpy() == 0).all()
    # the forward is LQR's own kernel: the same bits as without the keyword, which returns no graph
    plain_pol, plain_val = LQR(*_leaves(F=F, f=f, C=C, c=c).values(), device="cuda").backward(T)
    plain = (plain_pol.K, plain_pol.k, plain_val.V, plain_val.v, plain_val.const)
    for o, p in zip(outs, plain):
        assert o.grad_fn is not None and p.grad_fn is None and not p.requires_grad
        assert torch.equal(o.detach(), p)
    tv_pol, _ = TimeVaryingLQR(*(t.unsqueeze(1) for t in _leaves(F=F, f=f, C=C, c=c).values()), device="cuda").backward()
    assert tv_pol.K.grad_fn is None
    # the same gradients through tvlqr_backward on expanded (time stride 0) operands, and against fp64
    leaves = _leaves(F=F, f=f, C=C, c=c)
    ex = [t.unsqueeze(1).expand(B, T, *t.shape[1:]) for t in leaves.values()]
    _loss(tvlqr_backward(*ex), up).backward()
    torch.cuda.synchronize()
    rep = lambda x: np.repeat(x[:, None], T, axis=1)          # noqa: E731
    fwd = {name: o.detach().cpu().numpy() for name, o in zip(OUTS, outs)}
    fwd.update(k=fwd["k"].reshape(B, T, m), v=fwd["v"].reshape(B, T, n), status=np.zeros(B, np.int32))
    g64, err = _refs(rep(F), rep(f), rep(C), rep(c), None, None, up, fwd)
    for name, t in leaves.items():
        key = GRAD_OF[name]
        ref, bud = g64[key].sum(1), err[key].sum(1)
        r = _ratios(a[name], ref, bud)
        print("LQR front end", key, "error / budget: median %.2f max %.2f" % (np.median(r), r.max()))
        assert np.median(r) <= 2.5 and r.max() <= 10.0, (name, r)
        assert _ratios(a[name], t.grad.double().cpu().numpy().reshape(ref.shape), 2.0 * bud).max() <= 10.0, name


def test_envelope_cross_check_with_the_trajectory_vjp():
    """The optimal cost from x0 is both V_0's quadratic (this path) and the sum of the solved trajectory's costs
    (tfmpc_tvlqr_vjp_f32): two kernels, one gradient.  Tolerance: the sum of both paths' fp32 budgets (10 x)."""
    n, m, T, B = 16, 8, 4, 3
    F, f, C, c, Cf, cf = bref.problem(n, m, T, B, seed=61, final=True)
    x0 = np.random.default_rng(3).normal(size=(B, n)).astype(np.float32)
    la = _leaves(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf)
    K, k, V, v, const = tvlqr_backward(*la.values())
    x = torch.as_tensor(x0, device="cuda").unsqueeze(-1)
    cost = 0.5 * (x.transpose(-1, -2) @ V[:, 0] @ x) + v[:, 0].transpose(-1, -2) @ x + const[:, 0]
    cost.sum().backward()
    lb = _leaves(F=F, f=f, C=C, c=c, Cfin=Cf, cfin=cf)
    states, actions, costs = tvlqr_solve(lb["F"], lb["f"], lb["C"], lb["c"], torch.as_tensor(x0, device="cuda"), lb["Cfin"], lb["cfin"])
    assert np.allclose(costs.sum().item(), cost.sum().item(), rtol=1e-4)
    costs.sum().backward()
    torch.cuda.synchronize()
    # budgets: each path's fp32 restatement against its fp64
    # (the loss's upstream gradients in fp64 from the fp32 x0, as the trajectory path's oracle sees x0)
    up = dict(gK=None, gk=None, gV=np.zeros((B, T, n, n)), gv=np.zeros((B, T, n)), gconst=np.zeros((B, T)))
    x64 = x0.astype(np.float64)
    up["gV"][:, 0], up["gv"][:, 0], up["gconst"][:, 0] = 0.5 * x64[:, :, None] * x64[:, None, :], x64, 1.0
    g64, err_a = _refs(F, f, C, c, Cf, cf, up)
    t64 = lambda *a: [None if x is None else torch.as_tensor(x, dtype=torch.float64) for x in a]      # noqa: E731
    gc = np.ones((B, T + 1))
    args = t64(F, f, C, c, x0, Cf, cf, None, None, gc)
    s64 = tvlqr_grad_ref.closed_form(*args, dtype=torch.float64)
    s32 = tvlqr_grad_ref.closed_form(*args, dtype=torch.float32)
    a32 = tvlqr_grad_ref.autograd_grads(*args, dtype=torch.float32)      # (the TV-LQR tests' rule: the larger of the two)
    for name in OPS:
        key = GRAD_OF[name]
        ref = g64[key]
        assert np.abs(s64[name].double().numpy().reshape(ref.shape) - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), name
        err_b = np.maximum(*(np.abs(r[name].double().numpy() - s64[name].double().numpy()).reshape(ref.shape) for r in (s32, a32)))
        ga, gb = la[name].grad.double().cpu().numpy(), lb[name].grad.double().cpu().numpy()
        r = _ratios(ga, gb.reshape(ga.shape), err_a[key] + err_b)
        print("envelope", key, "difference / summed budget: max %.2f" % r.max())
        assert r.max() <= 10.0, (name, r)

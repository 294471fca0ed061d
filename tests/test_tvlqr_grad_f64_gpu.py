"""Gradients of the double-precision time-varying LQR on the MI355X (tfmpc_tvlqr_vjp_f64 through
tfmpc.solvers.tvlqr_solve(dtype=torch.float64) and TimeVaryingLQR.solve(x0, differentiable=True)) against the 80-bit
value-function reference of tests/tvlqr_grad_f64_ref.py, all seven gradients, under its budget rule: per output and
instance, kernel error over max(error of the fp64 value-function restatement, error of fp64 autograd, 2^-48 max(1, |ref|));
the median over instances <= 2.5 and every instance <= 10; a batch- or time-summed gradient's budget is the sum of its
terms' budgets and its reference the 80-bit sum."""
import numpy as np
import pytest
import torch

import tvlqr_f64_ref as ref64
import tvlqr_grad_f64_ref as g64
import tvlqr_ref
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR, tvlqr_solve

pytestmark = pytest.mark.gpu

F64 = torch.float64
MODEL = ("F", "f", "C", "c")
NAMES = ("F", "f", "C", "c", "x0", "Cfin", "cfin")
LOSSES = ("states", "actions", "costs", "mixed")
_CACHE = {}


def _case(n, m, T, B, shared=(), const=(), final=False, loss="mixed", seed=0, unscaled=False):
    """A seeded problem and its references, computed once.  ``shared``: operands without a batch axis (every instance
    then has instance 0's), ``const``: model operands with a time axis of 1 (every step has step 0's).  -> (user: what
    the caller passes, fp64 numpy; w: the loss weights; refs: tvlqr_grad_f64_ref.references of the replicated problem)."""
    key = (n, m, T, B, tuple(shared), tuple(const), final, loss, seed, unscaled)
    if key in _CACHE:
        return _CACHE[key]
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    full = dict(zip(MODEL, (a.astype(np.float64) for a in make(n, m, T, B, seed=seed))))
    full["x0"] = tvlqr_ref.make_x0(n, B, seed=seed + 1).astype(np.float64)
    if final:
        full["Cfin"], full["cfin"] = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B, seed=seed + 2))
    user = {}
    for k in list(full):
        a = full[k]
        if k in const:
            a = np.repeat(a[:, :1], T, axis=1)
        if k in shared:
            a = np.repeat(a[:1], B, axis=0)
        full[k] = a
        u = a[:, :1] if k in const else a
        user[k] = np.ascontiguousarray(u[0] if k in shared else u)
    rng = np.random.default_rng(seed + 3)
    w = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    w = tuple(g if loss in (name, "mixed") else None for g, name in zip(w, LOSSES))
    refs = g64.references(full["F"], full["f"], full["C"], full["c"], full["x0"], full.get("Cfin"), full.get("cfin"), *w)
    _CACHE[key] = (user, w, refs)
    return _CACHE[key]


def _loss(states, actions, costs, w):
    total = 0
    for out, g in zip((states[..., 0], actions[..., 0], costs.reshape(costs.shape[:-2])), w):
        if g is not None:
            total = total + (out * torch.as_tensor(g, dtype=out.dtype, device=out.device).reshape(out.shape)).sum()
    return total


def _grads(user, w, dtype=F64, solver="functional"):
    """-> (gradients as numpy, the solver when one was built)."""
    ops = {k: torch.as_tensor(v, device="cuda", dtype=dtype).requires_grad_() for k, v in user.items()}
    tv = None
    if solver == "functional":
        out = tvlqr_solve(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops.get("Cfin"), ops.get("cfin"), dtype=dtype)
    else:
        tv = TimeVaryingLQR(ops["F"], ops["f"], ops["C"], ops["c"], ops.get("Cfin"), ops.get("cfin"), device="cuda", dtype=dtype)
        traj = tv.solve(ops["x0"], differentiable=True)          # a TensorTrajectory: the vectors without their last axis
        out = (traj.states[..., None], traj.actions[..., None], traj.costs[..., None, None])
    assert all(t.dtype == dtype and t.requires_grad for t in out)
    _loss(*out, w).backward()
    torch.cuda.synchronize()
    for k, t in ops.items():
        assert t.grad.dtype == dtype and t.grad.shape == t.shape, (k, t.grad.dtype, t.grad.shape)
    return {k: t.grad.cpu().numpy() for k, t in ops.items()}, tv


def _check(got, refs, what, shared=(), const=(), idx=None):
    assert set(got) == set(refs[0]), (set(got), set(refs[0]))
    g64.check({k: got[k] for k in NAMES if k in got}, refs, what=what, shared=shared, time_shared=const, idx=idx)


# ---- shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,T", [(1, 1, 20), (3, 2, 20), (16, 8, 20), (16, 16, 20), (17, 8, 20), (16, 17, 20), (5, 20, 20),
                                   (32, 32, 6)])
def test_shapes_per_instance(n, m, T):
    user, w, refs = _case(n, m, T, 6, seed=n * 100 + m)
    got, _ = _grads(user, w)
    _check(got, refs, f"shapes ({n}, {m}, {T})")


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("n,m", [(16, 8), (12, 5)])
def test_short_horizons(n, m, T):
    """T = 1 has only the final-cost step: V_1 = C_fin, and the default final cost's gradient lands in dC[0], dc[0]."""
    user, w, refs = _case(n, m, T, 6, seed=T)
    got, _ = _grads(user, w)
    _check(got, refs, f"horizons ({n}, {m}, {T})")


# ---- sharing ------------------------------------------------------------------------------------------------------------

# (shared by the batch, time axis of 1).  The horizon is read off the operands' time axes, so one operand keeps its own:
# "time" and "both" leave c with T steps.
TIME = ("F", "f", "C")
SHARING = {"batch": (MODEL, ()), "time": ((), TIME), "both": (MODEL, TIME), "only F": (("F",), ("F",)),
           "only C, c": (("C", "c"), ()), "only f": ((), ("f",))}


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("sharing", list(SHARING))
@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_shared_operands_and_losses(n, m, sharing, loss):
    shared, const = SHARING[sharing]
    user, w, refs = _case(n, m, 5, 6, shared=shared, const=const, loss=loss, seed=n + len(sharing))
    got, _ = _grads(user, w)
    _check(got, refs, f"sharing ({n}, {m}) {sharing} {loss}", shared, const)


@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_shared_final_cost_and_shared_x0(n, m):
    shared = ("Cfin", "cfin", "x0")
    user, w, refs = _case(n, m, 5, 6, shared=shared, final=True, seed=41)
    got, _ = _grads(user, w)
    _check(got, refs, f"final ({n}, {m}) shared final cost and x0", shared)
    user, w, refs = _case(n, m, 5, 6, final=True, seed=42)
    got, _ = _grads(user, w)
    _check(got, refs, f"final ({n}, {m}) per-instance final cost")


@pytest.mark.parametrize("B", [1, 3, 257])
def test_batch_sums_across_chunk_edges(B):
    """257: a second chunk of one instance; 1, 3: a k-step of the matrix-core sum with fewer than four live instances.
    (Some operand has to carry the batch axis: x0 for the model's sums, C and c for x0's.)"""
    for shared in (MODEL, ("F", "f", "x0")):
        user, w, refs = _case(4, 2, 3, B, shared=shared, seed=B)
        got, _ = _grads(user, w)
        _check(got, refs, f"chunks (4, 2, 3) B={B} {'+'.join(shared)}", shared)


@pytest.mark.parametrize("n,m,T,shared,final", [(17, 2, 2, MODEL, False), (17, 2, 2, ("Cfin", "cfin", "x0"), True),
                                                (4, 2, 3, ("Cfin", "cfin", "x0"), True)])
def test_scalar_and_final_sums_across_chunk_edges(n, m, T, shared, final):
    """B = 257 is sixteen full LDS tiles plus a second chunk of one instance.  n = 17 is the smallest shape off the
    matrix-core sum: the scalar per-step sums, with the default final cost's second pass at t = T - 1 (T = 2 has a step with
    and a step without it); the shared final cost and x0 are the one-record-per-instance sums."""
    user, w, refs = _case(n, m, T, 257, shared=shared, final=final, seed=257)
    got, _ = _grads(user, w)
    _check(got, refs, f"chunk edges ({n}, {m}, {T}) B=257 {'+'.join(shared)}", shared)


# ---- what the value-function costates buy -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_unscaled_models_at_the_headline_horizon(seed):
    """rho(F_x) ~ 5 over T = 50: no recursion-based kernel can pass this, and the fp32 path's gradients are at least four
    digits worse on every output of every instance."""
    user, w, refs = _case(16, 8, 50, 4, seed=seed, unscaled=True)
    got, _ = _grads(user, w)
    _check(got, refs, f"unscaled (16, 8, 50) seed {seed}")
    got32, _ = _grads(user, w, dtype=torch.float32)
    for k in got:
        for b in range(4):
            e64, e32 = g64._err(got[k][b], refs[0][k][b]), g64._err(got32[k][b], refs[0][k][b])
            e32 = e32 if np.isfinite(e32) else np.inf              # an overflowed fp32 gradient is as wrong as it gets
            print(f"unscaled seed {seed} d{k}[{b}]: fp64 error {e64:.3g}, fp32 error {e32:.3g}, gain {e32 / max(e64, 1e-300):.3g}")
            assert e64 * 1e4 <= e32, (k, b, e64, e32)


@pytest.mark.parametrize("final", [False, True])
def test_gradcheck(final):
    n, m, T, B = 3, 2, 3, 2
    user, _, _ = _case(n, m, T, B, final=final, seed=7)
    dev = lambda a: torch.as_tensor(a, device="cuda", dtype=F64).requires_grad_()      # noqa: E731
    sym = lambda A: 0.5 * (A + A.transpose(-1, -2))                                      # noqa: E731
    ops = [dev(user[k]) for k in ("F", "f", "c", "x0", "C")] + ([dev(user["Cfin"]), dev(user["cfin"])] if final else [])

    def fn(F, f, c, x0, A, *fin):
        fin = (sym(fin[0]), fin[1]) if fin else ()
        return tvlqr_solve(F, f, sym(A), c, x0, *fin, dtype=F64)       # the solver accepts symmetric costs only

    assert torch.autograd.gradcheck(fn, ops)


# ---- the Python surface ---------------------------------------------------------------------------------------------------

def test_time_invariant_and_unbatched_problems():
    n, m, T, B = 12, 5, 7, 3
    user, w, refs = _case(n, m, T, B, shared=MODEL, const=MODEL, seed=51)
    ops = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in user.items()}
    tv = TimeVaryingLQR.time_invariant(ops["F"][0], ops["f"][0], ops["C"][0], ops["c"][0], T, device="cuda", dtype=F64)
    out = tv.solve_tensors(ops["x0"], differentiable=True)
    _loss(*out, w).backward()
    got = {k: t.grad.cpu().numpy() for k, t in ops.items()}
    for k, t in ops.items():
        assert t.grad.dtype == F64 and t.grad.shape == t.shape, k
    _check(got, refs, "surface time_invariant", MODEL, MODEL)
    # an un-batched problem: no batch axis anywhere, B = 1 for the kernels
    user, w, refs = _case(n, m, T, 1, seed=52)
    un = {k: v[0] for k, v in user.items()}
    w1 = tuple(g[0] for g in w)
    got, tv = _grads(un, w1, solver="class")
    assert tv.batch_size is None
    _check(got, refs, "surface unbatched")


def test_shared_gradients_are_bitwise_reproducible():
    for args, kw in (((16, 8, 5, 300), dict(shared=MODEL + ("Cfin", "cfin"), final=True, seed=5)),
                     ((20, 10, 4, 300), dict(shared=("F", "C"), const=("c", "F"), seed=6))):
        make = tvlqr_ref.make_models
        n, m, T, B = args
        user = dict(zip(MODEL, (a.astype(np.float64) for a in make(n, m, T, B, seed=kw["seed"]))))
        user["x0"] = tvlqr_ref.make_x0(n, B).astype(np.float64)
        if kw.get("final"):
            user["Cfin"], user["cfin"] = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B))
        for k in kw.get("const", ()):
            user[k] = user[k][:, :1]
        for k in kw["shared"]:
            user[k] = user[k][0]
        rng = np.random.default_rng(3)
        w = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
        a, b = _grads(user, w)[0], _grads(user, w)[0]
        for k in a:
            assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_the_trajectory_with_grad_is_the_trajectory_without(n, m):
    user, w, _ = _case(n, m, 5, 6, seed=n + len("only C, c"), shared=("C", "c"))
    ops = {k: torch.as_tensor(v, device="cuda") for k, v in user.items()}
    tv = TimeVaryingLQR(*(ops[k] for k in MODEL), device="cuda", dtype=F64)
    with torch.no_grad():
        plain = tv.solve_tensors(ops["x0"])
    lean = tv.solve_device(ops["x0"])
    ops["F"].requires_grad_()
    with_grad = TimeVaryingLQR(*(ops[k] for k in MODEL), device="cuda", dtype=F64).solve_tensors(ops["x0"], differentiable=True)
    assert with_grad[0].requires_grad and not plain[0].requires_grad and "v" not in lean
    for a, b, c in zip(plain, with_grad, (lean["states"], lean["actions"], lean["costs"])):
        assert torch.equal(a, b.detach()) and torch.equal(a, c)


@pytest.mark.parametrize("n,m,T,B,bad", [(16, 8, 5, 3, 1), (4, 2, 2, 519, 300)])
def test_not_pd_instance(n, m, T, B, bad):
    """C per instance (one indefinite), F, f and x0 shared: NaN in the instance's own rows of dC, dc and in every batch sum;
    the other rows finite and within the rule; last_grad_status flags it alone."""
    shared = ("F", "f", "x0")
    user, w, refs = _case(n, m, T, B, shared=shared, seed=23)
    user = dict(user, C=user["C"].copy())
    user["C"][bad, T - 1, n:, n:] = -1.0e4 * np.eye(m)
    got, tv = _grads(user, w, solver="class")
    st = tv.last_grad_status.cpu().numpy()
    others = [b for b in range(B) if b != bad]
    assert st[bad] & _hip.ST_NOT_PD and (st[others] == 0).all(), st[bad]
    for k in shared:
        assert np.isnan(got[k]).all(), k
    for k in ("C", "c"):
        assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][others]).all(), k
    g64.check({k: got[k] for k in ("C", "c")}, refs, what=f"not_pd ({n}, {m}, {T}) B={B}", idx=others)


def test_an_empty_batch():
    n, m, T = 16, 8, 4
    F, f, C, c = (torch.as_tensor(a[:0], device="cuda", dtype=F64).requires_grad_() for a in tvlqr_ref.make_models(n, m, T, 1))
    x0 = torch.zeros((0, n), device="cuda", dtype=F64, requires_grad=True)
    s, a, cs = tvlqr_solve(F, f, C, c, x0, dtype=F64)
    assert s.shape == (0, T + 1, n, 1) and s.dtype == F64
    (s.sum() + a.sum() + cs.sum()).backward()
    torch.cuda.synchronize()
    assert F.grad.shape == F.shape and x0.grad.shape == x0.shape and F.grad.dtype == F64
    # operands shared by an empty batch: the sum over nothing
    Fs = torch.as_tensor(tvlqr_ref.make_models(n, m, T, 1)[0][0], device="cuda", dtype=F64).requires_grad_()
    s, a, cs = tvlqr_solve(Fs, f.detach(), C.detach(), c.detach(), x0.detach(), dtype=F64)
    (s.sum() + cs.sum()).backward()
    assert Fs.grad.shape == Fs.shape and float(Fs.grad.abs().sum()) == 0.0

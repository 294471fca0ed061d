"""Double-precision gradients of the infinite-horizon LQR on the MI355X:
``lqr_steady_state(..., dtype=torch.float64, differentiable=True)`` (``tfmpc_lqr_steady_state_f64`` forward,
``tfmpc_lqr_steady_state_vjp_f64`` backward) and ``lqr_steady_state_vjp`` against the 80-bit restatement of
tests/lqr_steady_state_grad_f64_ref.py under the project's budget rule (its docstring; the restatements themselves are
pinned by tests/test_lqr_steady_state_grad_f64_cpu.py), and the batch sums against the float64 emulation of
tests/batch_sum_f64_ref.py bit for bit.

Ratios measured on the MI355X are tabled in DESIGN.md 3.22."""

import functools

import numpy as np
import pytest
import torch

import batch_sum_f64_ref as sum64
import lqr_steady_state_f64_ref as ref64
import lqr_steady_state_grad_f64_ref as g64
import tvlqr_grad_f64_ref as tvg64
import tvlqr_grad_ref
from stale_memory import PATTERNS, StaleMemory, same
from tfmpc import _hip
from tfmpc.solvers import lqr_steady_state, lqr_steady_state_vjp, tvlqr_solve

# (the shared problems are read-only numpy arrays; every conversion of one to a tensor is a copy to the device)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

F64 = torch.float64
OPS = ("F", "f", "C", "c")
OUTS = ("K", "k", "P", "p")
GRADS = g64.GRADS
WAVE16, WAVE32 = "ss_vjp_f64_wave16", "ss_vjp_f64_wave32"


def _kernel(n, m):
    return _hip.load().tfmpc_lqr_steady_state_vjp_kernel_name_f64(n, m).decode()


def _weights(B, n, m, loss="all", seed=0):
    """Upstream gradients [B, ...] of sum(w_K K) + sum(w_k k) + sum(w_P P) + sum(w_p p) ('all') or of one output (the
    others None: a NULL pointer at the kernel)."""
    rng = np.random.default_rng(seed)
    w = dict(K=rng.normal(size=(B, m, n)), k=rng.normal(size=(B, m)), P=rng.normal(size=(B, n, n)), p=rng.normal(size=(B, n)))
    return {name: (g if loss in ("all", name) else None) for name, g in w.items()}


def _ups(w):
    return {"g" + name: w[name] for name in OUTS}


def _leaves(F, f, C, c):
    return {name: torch.tensor(a, device="cuda", dtype=F64).requires_grad_() for name, a in zip(OPS, (F, f, C, c))}


def _loss(ss, w, mask=None):
    total = 0
    for name in OUTS:
        if w[name] is not None:
            out = getattr(ss, name)
            wt = torch.tensor(w[name], device=out.device).reshape(out.shape)
            if mask is not None:
                out, wt = torch.nan_to_num(out, nan=0.0), wt * mask.reshape(-1, *[1] * (out.dim() - 1))
            total = total + (out * wt).sum()
    return total


def _grads(ops, w, mask=None, **kw):
    """ops: name -> numpy (no grad) or a leaf on the device.  Returns (dF, df, dC, dc of the leaves as numpy, ss)."""
    ss = lqr_steady_state(*(ops[name] for name in OPS), dtype=F64, differentiable=True, **kw)
    assert ss.K.dtype == F64 and ss.status.dtype == torch.int32 and not ss.status.requires_grad and not ss.iterations.requires_grad
    _loss(ss, w, mask).backward()
    torch.cuda.synchronize()
    got = {}
    for name, t in ops.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            assert t.grad.dtype == F64 and t.grad.shape == t.shape, name
            got["d" + name] = t.grad.cpu().numpy()
    return got, ss


def _forward_of(ss):
    return {name: getattr(ss, name).detach().cpu().numpy() for name in OUTS}


@functools.lru_cache(maxsize=None)
def _problem(kind, n, m, B=6, loss="all", shared=False):
    """Operands, upstream gradients and the three references of one case, computed once and read-only.  ``shared``: every
    instance has instance 0's F, f and C (its own c)."""
    F, f, C, c = ref64.operands(kind, n, m, B, seed=100 * n + m)
    if shared:
        F, f, C = (np.repeat(a[:1], B, axis=0) for a in (F, f, C))
    w = _weights(B, n, m, loss, seed=n + m)
    refs = g64.references(F, f, C, c, _ups(w))
    for a in (F, f, C, c) + tuple(v for v in w.values() if v is not None):
        a.setflags(write=False)
    return (F, f, C, c), w, refs


# ---- per-instance gradients -----------------------------------------------------------------------------------------------

SHAPES = [(1, 1, WAVE16), (3, 2, WAVE16), (3, 5, WAVE16), (12, 6, WAVE16), (16, 8, WAVE16), (16, 16, WAVE16), (17, 8, WAVE32),
          (16, 17, WAVE32), (20, 10, WAVE32), (32, 16, WAVE32), (32, 32, WAVE32)]
CASES = [(kind, *s) for s in SHAPES for kind in ("make_lqr", "damped")] + [("damped", 22, 3, WAVE32)]


@pytest.mark.parametrize("kind,n,m,kernel", CASES)
def test_gradients_per_instance(kind, n, m, kernel):
    assert _kernel(n, m) == kernel
    ops, w, refs = _problem(kind, n, m)
    got, ss = _grads(_leaves(*ops), w)
    assert (ss.status.cpu().numpy() == 0).all()
    own = g64.own_forward(*ops, _ups(w), _forward_of(ss))
    g64.check(got, refs, own=own, what=f"{kind} ({n}, {m})")          # no exception granted: not even dc on the damped workload needs one


@pytest.mark.parametrize("loss", OUTS)
@pytest.mark.parametrize("n,m", [(16, 8), (5, 3)])
def test_losses_on_each_single_output(n, m, loss):
    """The other three upstream pointers are NULL."""
    ops, w, refs = _problem("make_lqr", n, m, loss=loss)
    got, ss = _grads(_leaves(*ops), w)
    own = g64.own_forward(*ops, _ups(w), _forward_of(ss))
    g64.check(got, refs, own=own, what=f"loss on {loss} ({n}, {m})")


def test_all_upstream_null_gives_exact_zeros():
    (F, f, C, c), _, _ = _problem("make_lqr", 16, 8)
    ss = lqr_steady_state(F, f, C, c, dtype=F64)
    *grads, status = lqr_steady_state_vjp(F, f, C, c, ss.K, ss.k, ss.P, ss.p, ss.status)
    torch.cuda.synchronize()
    assert not status.any()
    for g, a in zip(grads, (F, f, C, c)):
        assert g.dtype == F64 and g.shape[:a.ndim] == a.shape and bool((g == 0).all())


# ---- batch sums, bit for bit -----------------------------------------------------------------------------------------------

def _tiled(kind, n, m, B):
    """A batch of B from the case's six instances (instance b is instance b % 6), with its own upstream gradients."""
    (F, f, C, c), _, _ = _problem(kind, n, m)
    idx = np.arange(B) % F.shape[0]
    return (F[idx], f[idx], C[idx], c[idx]), _weights(B, n, m, seed=B)


@pytest.mark.parametrize("n,m,B", [(16, 8, 131), (20, 10, 65), (3, 2, 16449)])
def test_batch_sums_are_the_emulated_order(n, m, B):
    """131: two chunks and a tail of 3; 65: one chunk and one instance; 16 449: 258 chunks, the strided part of the tree.
    Shared F, f, C with per-instance c, then a fully shared model: once with the shared operands replicated (the
    per-instance bits), once shared (the summed bits)."""
    (F, f, C, c), w = _tiled("make_lqr", n, m, B)
    rep = lambda a: np.repeat(a[:1], B, axis=0)        # noqa: E731
    per, ss = _grads(_leaves(rep(F), rep(f), rep(C), c), w)
    assert not ss.status.any()
    summed, _ = _grads(_leaves(F[0], f[0], C[0], c), w)
    again, _ = _grads(_leaves(F[0], f[0], C[0], c), w)
    for name in ("dF", "df", "dC"):
        assert summed[name].shape == per[name].shape[1:]
        assert np.array_equal(summed[name], sum64.steady_state_sum(per[name])), name
        assert np.array_equal(summed[name], again[name]), name
    assert np.array_equal(summed["dc"], per["dc"]) and np.array_equal(again["dc"], per["dc"])
    # the fully shared model: every operand without a batch axis, per-instance upstream gradients
    per, ss = _grads(_leaves(rep(F), rep(f), rep(C), rep(c)), w)
    out = lqr_steady_state_vjp(F[0], f[0], C[0], c[0], ss.K.detach(), ss.k.detach(), ss.P.detach(), ss.p.detach(), ss.status,
                               **{k: torch.as_tensor(v, device="cuda") for k, v in _ups(w).items()})
    torch.cuda.synchronize()
    assert not out[4].any() and tuple(out[4].shape) == (B,)
    for name, g in zip(GRADS, out[:4]):
        assert np.array_equal(g.cpu().numpy().reshape(per[name].shape[1:]), sum64.steady_state_sum(per[name])), name


@pytest.mark.parametrize("kind", ["make_lqr", "damped"])
@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_summed_gradients_under_the_budget_rule(n, m, kind):
    """F, f and C shared by the batch: their gradients against the 80-bit sum, the budget the sum of the terms' budgets."""
    (F, f, C, c), w, refs = _problem(kind, n, m, shared=True)
    got, ss = _grads(_leaves(F[0], f[0], C[0], c), w)
    assert not ss.status.any() and got["dF"].shape == F[0].shape and got["dC"].shape == C[0].shape
    own = g64.own_forward(F, f, C, c, _ups(w), _forward_of(ss))
    for name in ("dF", "df", "dC"):
        g64.check_summed(got[name], refs, name, own=own, what=f"{kind} ({n}, {m})")
    g64.check(got, refs, own=own, names=("dc",), what=f"{kind} ({n}, {m}) shared")


def test_unbatched_and_mixed_operands():
    n, m = 12, 6
    (F, f, C, c), w, refs = _problem("make_lqr", n, m)
    w1 = {k: v[0] for k, v in w.items()}
    got, ss = _grads(_leaves(F[0], f[0], C[0], c[0]), w1)            # a batch of one, in place, no workspace
    assert tuple(ss.K.shape) == (m, n) and tuple(ss.p.shape) == (n, 1) and ss.status.dim() == 0
    assert got["dF"].shape == (n, n + m) and got["df"].shape == (n,) and got["dc"].shape == (n + m,)
    full, _ = _grads(_leaves(F, f, C, c), w)
    for name in GRADS:
        assert np.array_equal(got[name], full[name][0]), name
    # shared operands over a batch of one: the sum is the instance's own gradient
    shared, _ = _grads(_leaves(F[0], f[0], C[0], c[:1]), {k: v[:1] for k, v in w.items()})
    for name in ("dF", "df", "dC"):
        assert np.array_equal(shared[name], full[name][0]), name
    # numpy F and f (no grad), tensors C and c: the same gradients as all-tensor operands
    ops = dict(F=F, f=f, C=torch.as_tensor(C, device="cuda").requires_grad_(), c=torch.as_tensor(c, device="cuda").requires_grad_())
    mixed, _ = _grads(ops, w)
    assert set(mixed) == {"dC", "dc"}
    for name in ("dC", "dc"):
        assert np.array_equal(mixed[name], full[name]), name


def test_independent_of_the_batch():
    n, m, B, at = 16, 8, 4096, 4000
    (F, f, C, c), w = _tiled("damped", n, m, B)
    big, _ = _grads(_leaves(F, f, C, c), w)
    one, _ = _grads(_leaves(*(a[at:at + 1] for a in (F, f, C, c))), {k: v[at:at + 1] for k, v in w.items()})
    for name in GRADS:
        assert np.array_equal(one[name][0], big[name][at]), name


# ---- flagged instances -----------------------------------------------------------------------------------------------------

def _flagged(F, C, n, m):
    F, C = F.copy(), C.copy()
    F[1, 0, :] = 0.0           # instance 1: an unstable mode no input reaches
    F[1, :, 0] = 0.0
    F[1, 0, 0] = 1.5
    C[1, 0, 1:] = 0.0
    C[1, 1:, 0] = 0.0
    C[4, n:, n:] = -1e3 * np.eye(m)          # instance 4: R not positive definite
    return F, C


@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (20, 10)])
def test_status_isolation(n, m):
    (F, f, C, c), w, _ = _problem("make_lqr", n, m)
    B, keep = 6, [0, 2, 3, 5]
    Fb, Cb = _flagged(F, C, n, m)
    mask = torch.zeros(B, device="cuda", dtype=F64)
    mask[keep] = 1.0
    got, ss = _grads(_leaves(Fb, f, Cb, c), w, mask=mask)
    st = ss.status.cpu().numpy()
    assert st[1] == _hip.ST_NOT_STABILISING and st[4] == _hip.ST_NOT_PD and not st[keep].any(), st
    for name in GRADS:
        assert np.isnan(got[name][[1, 4]]).all(), name
    clean, _ = _grads(_leaves(*(a[keep] for a in (F, f, C, c))), {k: v[keep] for k, v in w.items()})
    for name in GRADS:
        assert np.array_equal(got[name][keep], clean[name]), name
    # the backward's status: the forward's where that was flagged
    ups = {k: torch.as_tensor(v, device="cuda") * mask.reshape(-1, *[1] * (v.ndim - 1)) for k, v in _ups(w).items()}
    out = lqr_steady_state_vjp(Fb, f, Cb, c, ss.K.detach(), ss.k.detach(), ss.P.detach(), ss.p.detach(), ss.status, **ups)
    torch.cuda.synchronize()
    assert np.array_equal(out[4].cpu().numpy(), st)
    for name, g in zip(GRADS, out[:4]):
        assert np.array_equal(g.cpu().numpy().reshape(got[name].shape), got[name], equal_nan=True), name
    # a flagged instance poisons every gradient summed over its batch
    rep = lambda a: np.repeat(a[:1], B, axis=0)        # noqa: E731
    Cs = rep(C)
    Cs[4, n:, n:] = -1e3 * np.eye(m)
    shared, ss2 = _grads(dict(_leaves(F[0], f[0], C[0], c), C=Cs), w, mask=mask)
    assert ss2.status.cpu().numpy().tolist() == [0, 0, 0, 0, _hip.ST_NOT_PD, 0]
    for name in ("dF", "df"):
        assert np.isnan(shared[name]).all(), name
    assert np.isnan(shared["dc"][4]).all() and np.isfinite(shared["dc"][keep]).all()


def test_a_capped_smith_loop_flags_the_backward_alone():
    """The damped workload needs 13 - 15 Smith steps: max_iter = 1 stops the backward with a clean forward status."""
    (F, f, C, c), w, _ = _problem("damped", 16, 8)
    ss = lqr_steady_state(F, f, C, c, dtype=F64)
    assert not ss.status.any()
    ups = {k: torch.as_tensor(v, device="cuda") for k, v in _ups(w).items()}
    *grads, status = lqr_steady_state_vjp(F, f, C, c, ss.K, ss.k, ss.P, ss.p, ss.status, **ups, max_iter=1)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == _hip.ST_NOT_STABILISING).all()
    assert all(bool(torch.isnan(g).all()) for g in grads)
    *grads, status = lqr_steady_state_vjp(F, f, C, c, ss.K, ss.k, ss.P, ss.p, ss.status, **ups)
    assert not status.any() and all(bool(torch.isfinite(g).all()) for g in grads)


# ---- the front end ---------------------------------------------------------------------------------------------------------

def test_forward_bits_are_the_plain_double_call():
    (F, f, C, c), _, _ = _problem("damped", 16, 8)
    ops = _leaves(F, f, C, c)
    ss = lqr_steady_state(*ops.values(), dtype=F64, differentiable=True, max_iter=30, tol=1e-14)
    plain = lqr_steady_state(F, f, C, c, dtype=F64, max_iter=30, tol=1e-14)
    assert all(getattr(ss, name).requires_grad for name in OUTS)
    for name in OUTS + ("iterations", "status"):
        assert torch.equal(getattr(ss, name).detach(), getattr(plain, name)), name
    with pytest.raises(NotImplementedError, match="differentiable=True"):
        lqr_steady_state(*ops.values(), dtype=F64)


def test_gradcheck():
    n, m, B = 3, 2, 2
    F, f, C, c = ref64.operands("make_lqr", n, m, B, seed=7)
    ops = [torch.as_tensor(a, device="cuda", dtype=F64).requires_grad_() for a in (F, f, c, C)]

    def fn(F, f, c, A):
        ss = lqr_steady_state(F, f, 0.5 * (A + A.transpose(-1, -2)), c, dtype=F64, differentiable=True)   # symmetric costs only
        return ss.K, ss.k, ss.P, ss.p

    assert torch.autograd.gradcheck(fn, ops)


@pytest.mark.parametrize("n,m", [(16, 8), (12, 6)])
def test_end_to_end_with_a_stationary_terminal_cost(n, m):
    """Receding-horizon MPC over T steps whose terminal cost is the stationary value function, every operand shared
    between the horizon (a time-expanded view) and the steady state, all in double.  Reference: the 80-bit gradients of
    tests/tvlqr_grad_f64_ref.py summed over time, plus the 80-bit vjp_gj fed their Cfin, cfin gradients as gP, gp.  Budget:
    the sum of the two stages' budgets -- the horizon's (time-summed) and the steady state's for that upstream gradient."""
    T, B = 12, 4
    F, f, C, c = (a[:B] for a in _problem("damped", n, m)[0])
    rng = np.random.default_rng(n)
    x0 = rng.normal(size=(B, n))
    gx, gu, gc = rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1))
    leaves = _leaves(F, f, C, c)
    ss = lqr_steady_state(*leaves.values(), dtype=F64, differentiable=True)
    rep = lambda t: t.unsqueeze(1).expand(t.shape[0], T, *t.shape[1:])      # noqa: E731
    states, actions, costs = tvlqr_solve(*(rep(t) for t in leaves.values()), torch.as_tensor(x0, device="cuda"), ss.P, ss.p, dtype=F64)
    dev = lambda a: torch.as_tensor(a, device="cuda")                       # noqa: E731
    loss = (states[..., 0] * dev(gx)).sum() + (actions[..., 0] * dev(gu)).sum() + (costs.reshape(B, T + 1) * dev(gc)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {"d" + k: t.grad.cpu().numpy() for k, t in leaves.items()}

    fwd_ld = [ref64.steady_state_ld(F[b], f[b], C[b], c[b]) for b in range(B)]
    repT = lambda a: np.repeat(a[:, None], T, axis=1)                       # noqa: E731
    Pld, pld = np.stack([r["P"] for r in fwd_ld]), np.stack([r["p"] for r in fwd_ld])
    horizon = lambda Cf, cf: (repT(F), repT(f), repT(C), repT(c), x0, Cf, cf, gx, gu, gc)      # noqa: E731
    auto = tvlqr_grad_ref.autograd_grads(*horizon(Pld.astype(np.float64), pld.astype(np.float64)), dtype=F64)
    tv_refs = (tvg64.grads(*horizon(Pld, pld), dtype=tvg64.LD), tvg64.grads(*horizon(Pld, pld), dtype=np.float64),
               {k: v.numpy() for k, v in auto.items()})
    ups = dict(gP=tv_refs[0]["Cfin"], gp=tv_refs[0]["cfin"])
    ss_refs = g64.references(F, f, C, c, ups)
    own = g64.own_forward(F, f, C, c, ups, _forward_of(ss))
    total = [{"d" + k: tv_refs[0][k][b].sum(0) + ss_refs[0][b]["d" + k] for k in OPS} for b in range(B)]
    extra = [{} for _ in range(B)]
    for k in OPS:
        bud = tvg64.term_budgets(tv_refs, k, time_summed=True) + g64.budgets(ss_refs, "d" + k, own)
        for b in range(B):
            extra[b]["d" + k] = float(bud[b])
    ref64.check(got, (total, total, total), fields=GRADS, what=f"end to end ({n}, {m})", extra=extra)


@pytest.mark.parametrize("kind", ["make_lqr", "damped"])
def test_against_the_fp32_path(kind):
    """Per instance at (16, 8): the fp32 path's error (fp32 forward and fp32 VJP on the rounded operands) against the 80-bit
    result is at least 1e4 times the double path's (floored at 2^-48 of the gradient's scale) on dF and dC -- the bar of
    tests/test_lqr_steady_state_f64_gpu.py on K and P.  df and dc are printed, not asserted."""
    n, m = 16, 8
    ops, w, refs = _problem(kind, n, m)
    got64, _ = _grads(_leaves(*ops), w)
    leaves32 = {k: torch.as_tensor(a, device="cuda", dtype=torch.float32).requires_grad_() for k, a in zip(OPS, ops)}
    ss32 = lqr_steady_state(*leaves32.values())
    w32 = {k: v.astype(np.float32) for k, v in w.items()}
    _loss(ss32, w32).backward()
    torch.cuda.synchronize()
    assert not ss32.status.any()
    got32 = {"d" + k: t.grad.double().cpu().numpy() for k, t in leaves32.items()}
    for name in GRADS:
        gain = []
        for b, ld in enumerate(refs[0]):
            err64 = max(ref64.error(got64[name][b], ld[name]), ref64.FLOOR * ref64.scale_of(ld[name]))
            gain.append(ref64.error(got32[name][b], ld[name]) / err64)
        print(f"fp32 error / fp64 error, {kind} {name}: min {min(gain):.3g} median {np.median(gain):.3g}")
        if name in ("dF", "dC"):
            assert min(gain) >= 1e4, (kind, name, gain)


# ---- stale memory (tests/stale_memory.py) -----------------------------------------------------------------------------------

def _run_under_every_fill(call, workspace_bytes, what):
    """``call()`` -> (tensors by name, the names the front end creates with ``torch.empty``), under the four fills and
    once unpatched: the patch was hit (the check against vacuity) and every tensor is the same under all five."""
    runs = []
    for i, pattern in enumerate(PATTERNS):
        with StaleMemory(pattern, seed=17 * i) as mem:
            tensors, made = call()
            torch.cuda.synchronize()
        mem.check({k: tensors[k] for k in made}, workspace_bytes)
        runs.append({k: v.detach().clone() for k, v in tensors.items()})
    tensors, _ = call()
    torch.cuda.synchronize()
    runs.append({k: v.detach().clone() for k, v in tensors.items()})
    for label, other in zip(PATTERNS[1:] + ("unpatched",), runs[1:]):
        assert other.keys() == runs[0].keys()
        for k in runs[0]:
            assert same(runs[0][k], other[k]), (what, k, label)
    return runs[0]


MODEL = OPS


@pytest.mark.parametrize("shared,unstable", [((), False), ((), True), (("F", "C"), False), (MODEL, False)],
                         ids=["per", "not-stabilising", "shared-F-C", "unbatched"])
@pytest.mark.parametrize("n,m", [(1, 1), (16, 8), (20, 10)])
def test_no_stale_memory_is_read_or_left(n, m, shared, unstable):
    B = 3
    F, f, C, c = (a[:B] for a in _problem("make_lqr", n, m)[0])
    if unstable:
        F, C = _flagged(np.concatenate([F, F]), np.concatenate([C, C]), n, m)
        F, C = F[:B], C[:B]
    unbatched = shared == MODEL
    ops = {k: (v[0] if k in shared else v) for k, v in zip(OPS, (F, f, C, c))}
    Bk = 1 if unbatched else B
    w = _weights(Bk, n, m, seed=6)
    mask = torch.ones(Bk, device="cuda", dtype=F64)
    if unstable:
        mask[1] = 0.0
    ws_bytes = int(_hip.load().tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(B, n, m)) if shared and not unbatched else 0

    def call():
        leaves = {k: torch.as_tensor(v, device="cuda").requires_grad_() for k, v in ops.items()}
        ss = lqr_steady_state(*leaves.values(), dtype=F64, differentiable=True)
        ssb = ss if not unbatched else type(ss)(*(t[None] for t in (ss.K, ss.k, ss.P, ss.p, ss.iterations, ss.status)))
        grads = torch.autograd.grad(_loss(ssb, w, mask), list(leaves.values()))
        tensors = dict(K=ss.K, k=ss.k, P=ss.P, p=ss.p, iterations=ss.iterations, status=ss.status)
        tensors.update({"d" + k: g for k, g in zip(leaves, grads)})
        return tensors, OUTS + GRADS

    first = _run_under_every_fill(call, ws_bytes, what=(n, m, shared, unstable))
    if unstable:
        st = first["status"].cpu().numpy()
        assert st[1] & _hip.ST_NOT_STABILISING and not st[[0, 2]].any(), st
        for k in ("K", "P", "dF", "dC"):
            assert bool(torch.isnan(first[k][1]).all()) and bool(torch.isfinite(first[k][[0, 2]]).all()), k
    else:
        assert not first["status"].any() and all(bool(torch.isfinite(v).all()) for v in first.values())

"""Gradients of the periodic infinite-horizon LQR in double on the MI355X (tfmpc_tvlqr_periodic_vjp_f64 through
``periodic_steady_state(differentiable=True)`` and ``tfmpc.solvers.tvlqr_periodic_vjp``).

Accuracy is the project's budget rule: per gradient and instance, the kernel's error against the
longdouble restatement of tests/tvlqr_periodic_grad_ref.py over max(the fp64 restatement's error, the error of the fp64
restatement started from the kernel's own K, k, V, v, 2^-48 max(1, |ref|)); median <= 2.5 and every instance <= 10
(tests/test_tvlqr_periodic_grad_cpu.py shows on the host that the rule is attainable on these inputs).  Summed gradients,
repetition, batch position, status isolation and stale memory are asserted bit for bit."""
import functools

import numpy as np
import pytest
import torch

import batch_sum_f64_ref as sum64
import tvlqr_f64_ref as ref64
import tvlqr_periodic_grad_ref as pg
import tvlqr_periodic_ref as pr
import tvlqr_ref
import tvlqr_time_parallel_ref as tp
from stale_memory import PATTERNS, StaleMemory, same
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR, tvlqr_backward_vjp, tvlqr_periodic_steady_state, tvlqr_periodic_vjp

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
GRADS, UPS, FWD = pg.GRADS, pg.UPS, pg.FWD


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _cols(F, f, C, c):
    """(f and c as columns: [B, 1, 1] alone would read as [T, n, 1] at n = T = 1)"""
    return F, f[..., None], C, c[..., None]


def _forward(F, f, C, c, segments):
    """The periodic forward's batched K, k, V, v, residual, iterations, status (cuda tensors)."""
    tv = TimeVaryingLQR(*_cols(*(np.asarray(a, dtype=np.float64) for a in (F, f, C, c))), device="cuda", dtype=F64)
    return tv._periodic_launch(segments, 0, 0.0)


def _host_fwd(fwd):
    out = {name: t.detach().cpu().numpy() for name, t in zip(FWD, fwd[:4])}
    out["k"], out["v"] = out["k"][..., 0], out["v"][..., 0]
    return out


def _vjp(F, f, C, c, fwd, ups, segments, **kw):
    """``tvlqr_periodic_vjp``: a dict of cuda tensors (dF, df, dC, dc in the operands' shapes, residual, iterations,
    status)."""
    out = tvlqr_periodic_vjp(*_cols(F, f, C, c), *fwd[:4], fwd[6], **{k: v for k, v in ups.items() if v is not None},
                             segments=segments, **kw)
    torch.cuda.synchronize()
    assert all(g.dtype == F64 for g in out[:5])
    return dict(zip(GRADS + ("residual", "iterations", "status"), out))


def _flat(got):
    """Gradients as numpy with the vectors flat, as the restatement holds them."""
    out = {name: got[name].cpu().numpy() for name in GRADS}
    out["df"], out["dc"] = out["df"][..., 0], out["dc"][..., 0]
    return out


@functools.lru_cache(maxsize=None)
def _case(n, m, N, segments, B, unscaled=False):
    """Operands, all four upstream gradients and the references, computed once; no test writes to them."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = tp.perturbed(make, n, m, N, B, seed=n * 100 + m)
    ups = pg.upstream(n, m, N, B, seed=n + m)
    refs = pg.references(F, f, C, c, ups, segments, pr.solve_batch(F, f, C, c, segments, dtype=LD),
                         pr.solve_batch(F, f, C, c, segments))
    return F, f, C, c, ups, refs


# (n, m, N, segments, B, unscaled): both instantiations, a one-step period, a short last segment ((17, 8, 5, 2)), a lane
# with two columns of [Q_uu | gK | gk] ((16, 17, 3, 1)), len = 1 ((8, 32, 4, 4))
CASES = [(3, 2, 4, 2, 4, False), (5, 3, 7, 3, 4, False), (16, 8, 6, 3, 4, False), (16, 8, 1, 1, 4, False),
         (17, 8, 5, 2, 3, False), (16, 17, 3, 1, 3, False), (8, 32, 4, 4, 3, False), (32, 32, 3, 2, 3, False),
         (16, 8, 50, 5, 3, False), (17, 8, 5, 2, 3, True), (16, 8, 6, 3, 4, True)]


@pytest.mark.parametrize("n,m,N,segments,B,unscaled", CASES)
def test_accuracy_against_the_longdouble_restatement(n, m, N, segments, B, unscaled):
    kernel = "tvp_vjp_f64_wave16" if n <= 16 and m <= 16 else "tvp_vjp_f64_wave32"
    assert _hip.load().tfmpc_tvlqr_periodic_vjp_kernel_name_f64(n, m, N, segments).decode() == kernel
    F, f, C, c, ups, refs = _case(n, m, N, segments, B, unscaled)
    fwd = _forward(F, f, C, c, segments)
    got = _vjp(F, f, C, c, fwd, ups, segments)
    assert not got["status"].any(), got["status"]
    what = (n, m, N, segments, "unscaled" if unscaled else "scaled")
    own = pg.own_forward(F, f, C, c, ups, segments, _host_fwd(fwd))
    pg.check(_flat(got), refs, own=own, what=what)
    r64 = refs[1]
    res, its = got["residual"].cpu().numpy(), got["iterations"].cpu().numpy()
    for b in range(B):
        print(f"residual {what} [{b}]: kernel {res[b]:.3g} restatement {r64['residual'][b]:.3g}; Smith steps {its[b]} / "
              f"{r64['iterations'][b]}")
    for b in range(B):
        assert 0.0 <= res[b] <= 64 * r64["residual"][b], (b, res[b], r64["residual"][b])
        assert abs(int(its[b]) - int(r64["iterations"][b])) <= 1, (b, its[b], r64["iterations"][b])


def _leaves(F, f, C, c):
    return [_dev(a).requires_grad_() for a in _cols(F, f, C, c)]


def _loss(ss, ups):
    total = 0
    for name, g in zip(FWD, UPS):
        if ups[g] is not None:
            out = getattr(ss, name)
            total = total + (out * _dev(ups[g]).reshape(out.shape)).sum()
    return total


@pytest.mark.parametrize("only", UPS)
def test_each_upstream_gradient_alone(only):
    """Through autograd: the loss uses one output, the other three upstream pointers are NULL."""
    n, m, N, segments, B = 5, 3, 7, 3, 4
    F, f, C, c, _, _ = _case(n, m, N, segments, B)
    ups = pg.upstream(n, m, N, B, seed=3, names=(only,))
    leaves = _leaves(F, f, C, c)
    ss = tvlqr_periodic_steady_state(*leaves, segments=segments, differentiable=True)
    plain = tvlqr_periodic_steady_state(*(t.detach() for t in leaves), segments=segments)
    assert all(same(a.detach(), b) for a, b in zip(ss, plain))            # the forward keeps its bits
    _loss(ss, ups).backward()
    torch.cuda.synchronize()
    assert all(t.grad.dtype == F64 and t.grad.shape == t.shape for t in leaves)
    got = _flat(dict(zip(GRADS, (t.grad for t in leaves))))
    refs = pg.references(F, f, C, c, ups, segments, pr.solve_batch(F, f, C, c, segments, dtype=LD),
                         pr.solve_batch(F, f, C, c, segments))
    own = pg.own_forward(F, f, C, c, ups, segments, _host_fwd(tuple(t.detach() for t in ss)))
    pg.check(got, refs, own=own, what=f"{only} alone")


def test_gradcheck():
    """torch's defaults, through the real forward kernel.  C enters as a symmetric matrix (an asymmetric one is
    refused), so it is differentiated through (A + A') / 2."""
    F, f, C, c, _, _ = _case(3, 2, 3, 2, 2)
    F, f, A, c = _leaves(F, f, C, c)

    def fn(F, f, A, c):
        return tuple(tvlqr_periodic_steady_state(F, f, 0.5 * (A + A.transpose(-1, -2)), c, segments=2, differentiable=True)[:4])

    assert torch.autograd.gradcheck(fn, (F, f, A, c))


# ---- sharing -------------------------------------------------------------------------------------------------------------

def _share(ops, mode):
    """``ops`` ([B, N, ...] by name) with the operands of ``mode`` shared: (operands, names summed over the batch, over
    time)."""
    o = dict(ops)
    if mode == "batch":
        o.update(F=ops["F"][0], f=ops["f"][0], C=ops["C"][0])
        return o, ("F", "f", "C"), ()
    if mode == "time":
        o.update(F=ops["F"][:, :1], f=ops["f"][:, :1], C=ops["C"][:, :1])
        return o, (), ("F", "f", "C")
    if mode == "both":
        o.update(F=ops["F"][0, :1], f=ops["f"][0, :1], C=ops["C"][0, :1])
        return o, ("F", "f", "C"), ("F", "f", "C")
    if mode == "F":
        o.update(F=ops["F"][0])
        return o, ("F",), ()
    assert mode == "Cc"
    o.update(C=ops["C"][0], c=ops["c"][0])
    return o, ("C", "c"), ()


def _expanded(ops, B, N):
    out = {}
    for name, a in ops.items():
        if a.ndim < (4 if name in ("F", "C") else 3):
            a = np.repeat(a[None], B, axis=0)
        if a.shape[1] == 1:
            a = np.repeat(a, N, axis=1)
        out[name] = np.ascontiguousarray(a)
    return out


@functools.lru_cache(maxsize=None)
def _shared_case(n, m, N, B, mode):
    full = dict(zip("FfCc", tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=n * 100 + m)))
    ops, over_b, over_t = _share(full, mode)
    ops = {k: np.ascontiguousarray(a) for k, a in ops.items()}
    ex = _expanded(ops, B, N)
    ups = pg.upstream(n, m, N, B, seed=B)
    segments = 1 if over_t else 2
    exo = [ex[k] for k in "FfCc"]
    refs = pg.references(*exo, ups, segments, pr.solve_batch(*exo, segments, dtype=LD), pr.solve_batch(*exo, segments))
    return ops, ex, ups, refs, over_b, over_t, segments


@pytest.mark.parametrize("mode", ["batch", "time", "both", "F", "Cc"])
@pytest.mark.parametrize("n,m,B", [(16, 8, 131), (20, 10, 65)])
def test_shared_operands_get_summed_gradients(n, m, B, mode):
    """A summed gradient is, bit for bit, tests/batch_sum_f64_ref.py's emulated order (time: the sequential sum in time
    order, one segment; batch: chunks of 64, then the tree) applied to the per-instance, per-step bits of a call on the
    expanded operands with the same forward; it also meets the summed budget."""
    N = 3
    ops, ex, ups, refs, over_b, over_t, segments = _shared_case(n, m, N, B, mode)
    o, e = [ops[k] for k in "FfCc"], [ex[k] for k in "FfCc"]
    fwd = _forward(*o, 2)
    got = _vjp(*o, fwd, ups, 2)                                           # (a time-shared gradient: the call takes one segment)
    per = _vjp(*e, fwd, ups, segments)
    assert not got["status"].any() and not per["status"].any()
    own = pg.own_forward(*e, ups, segments, _host_fwd(fwd))
    flat = _flat(got)
    for name, key in zip("FfCc", GRADS):
        assert tuple(got[key].shape[:-2]) == ops[name].shape[:got[key].dim() - 2], key
        want = per[key].cpu().numpy()
        if name in over_t:
            acc = want[:, 0].copy()
            for t in range(1, N):
                acc = want[:, t] + acc
            want = acc[:, None]
        if name in over_b:
            want = sum64.steady_state_sum(want)
        assert np.array_equal(got[key].cpu().numpy().reshape(want.shape), want), (key, mode)
        if name in over_b or name in over_t:
            pg.check_summed(flat[key], refs, key, own, batch=name in over_b, time=name in over_t, what=f"({n},{m}) {mode}")
    again = _vjp(*o, fwd, ups, 2)
    assert all(same(got[key], again[key]) for key in got)


def test_repeated_calls_and_batch_position():
    n, m, N, segments, B, at = 16, 8, 6, 3, 128, 100
    F, f, C, c, ups, _ = _case(n, m, N, segments, 4)
    tile = lambda a: np.tile(a, (B // 4,) + (1,) * (a.ndim - 1))         # noqa: E731
    Fb, fb, Cb, cb = (tile(a) for a in (F, f, C, c))
    upb = {k: tile(g) for k, g in ups.items()}
    fwd = _forward(Fb, fb, Cb, cb, segments)
    big, again = _vjp(Fb, fb, Cb, cb, fwd, upb, segments), _vjp(Fb, fb, Cb, cb, fwd, upb, segments)
    assert not big["status"].any()
    assert all(same(big[key], again[key]) for key in big)
    one = slice(at, at + 1)
    alone = _vjp(Fb[one], fb[one], Cb[one], cb[one], tuple(t[one].contiguous() for t in fwd), {k: g[one] for k, g in upb.items()},
                 segments)
    for key in big:
        assert same(big[key][one], alone[key]), key


def test_one_more_lap_of_the_finite_kernel_reproduces_the_gradients():
    """The wrap adjoint (X*, y*) is in the kernel's own output: dC_0[:n, :n] = X* + sym(gV_0), dc_0[:n] = y* + gv_0.  Fed
    back once into tfmpc_tvlqr_backward_vjp_f64 with C_final = V[0], c_final = v[0], one lap of the finite kernel
    reproduces dF, df, dC, dc within the rule; its dCfin, dcfin are (X*, y*) again."""
    n, m, N, segments, B = 16, 8, 6, 3, 4
    F, f, C, c, ups, refs = _case(n, m, N, segments, B)
    fwd = _forward(F, f, C, c, segments)
    got = _vjp(F, f, C, c, fwd, ups, segments)
    K, k, V, v = fwd[:4]
    gV, gv = _dev(ups["gV"]).clone(), _dev(ups["gv"]).clone()
    X = got["dC"][:, 0, :n, :n] - 0.5 * (gV[:, 0] + gV[:, 0].transpose(-1, -2))
    y = got["dc"][:, 0, :n, 0] - gv[:, 0]
    gV[:, 0] += X
    gv[:, 0] += y
    out = tvlqr_backward_vjp(*_cols(F, f, C, c), K, k, V, v, fwd[6], gK=_dev(ups["gK"]), gk=_dev(ups["gk"]), gV=gV, gv=gv,
                             C_final=V[:, 0].contiguous(), c_final=v[:, 0].contiguous())
    torch.cuda.synchronize()
    assert not out[6].any()
    lap = _flat(dict(zip(GRADS, out[:4])))
    own = pg.own_forward(F, f, C, c, ups, segments, _host_fwd(fwd))
    pg.check(lap, refs, own=own, what="one more lap")
    print("wrap adjoint after one more lap (printed, not asserted: the residual test holds it):",
          float((out[4] - X).abs().max()), float((out[5][..., 0] - y).abs().max()))


# ---- status --------------------------------------------------------------------------------------------------------------

def test_a_forward_flagged_instance_is_isolated():
    n, m, N, segments, B, bad = 16, 8, 6, 3, 4, 1
    F, f, C, c, ups, _ = _case(n, m, N, segments, B)
    C = C.copy()
    C[bad, :, n:, n:] = -1e3 * np.eye(m)
    fwd = _forward(F, f, C, c, segments)
    assert fwd[6].tolist() == [0, pr.ST_NOT_PD, 0, 0]
    got = _vjp(F, f, C, c, fwd, ups, segments)
    assert got["status"].tolist() == [0, pr.ST_NOT_PD, 0, 0]
    keep = [b for b in range(B) if b != bad]
    clean = _vjp(F[keep], f[keep], C[keep], c[keep], tuple(t[keep].contiguous() for t in fwd), {k: g[keep] for k, g in ups.items()},
                 segments)
    assert not clean["status"].any()
    for key in GRADS + ("residual",):
        assert torch.isnan(got[key][bad]).all(), key
        assert same(got[key][keep], clean[key]), key                      # the neighbours' bits: those of a run without it
    fwd_s = _forward(F[0], f[0], C, c, segments)                          # F, f shared: every sum that contains it is NaN
    assert fwd_s[6].tolist() == [0, pr.ST_NOT_PD, 0, 0]
    sums = _vjp(F[0], f[0], C, c, fwd_s, ups, segments)
    assert sums["status"].tolist() == [0, pr.ST_NOT_PD, 0, 0]
    assert torch.isnan(sums["dF"]).all() and torch.isnan(sums["df"]).all()
    assert torch.isnan(sums["dC"][bad]).all() and not torch.isnan(sums["dC"][keep]).any()


def test_a_gain_that_does_not_stabilise_is_flagged_alone():
    n, m, N, segments, B, bad = 16, 8, 6, 3, 4, 2
    F, f, C, c, ups, _ = _case(n, m, N, segments, B)
    fwd = _forward(F, f, C, c, segments)
    ok = _vjp(F, f, C, c, fwd, ups, segments)
    F = F.copy()
    F[bad, :, :, :n] = 1.3 * np.eye(n)
    K = fwd[0].clone()
    K[bad] = 0.0
    got = _vjp(F, f, C, c, (K,) + tuple(fwd[1:]), ups, segments)
    assert got["status"].tolist() == [0, 0, _hip.ST_NOT_STABILISING, 0]
    keep = [b for b in range(B) if b != bad]
    for key in GRADS + ("residual",):
        assert torch.isnan(got[key][bad]).all() and same(got[key][keep], ok[key][keep]), key


# ---- stale memory (tests/stale_memory.py) -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shared", [(), ("F", "C"), ("F", "f", "C", "c")], ids=["per", "shared-F-C", "unbatched"])
@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_no_stale_memory_is_read_or_left(n, m, shared):
    N, segments, B = 5, 2, 3
    F, f, C, c, ups, _ = _case(n, m, N, segments, B)
    ops = {k: (a[0] if k in shared else a) for k, a in zip("FfCc", (F, f, C, c))}
    Bk = 1 if len(shared) == 4 else B
    ups = {k: g[:Bk] if Bk == B else g[0] for k, g in ups.items()}
    workspace_bytes = int(_hip.load().tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(Bk, n, m, N, segments))

    def call():
        args = _cols(*ops.values())
        ss = tvlqr_periodic_steady_state(*args, segments=segments)
        out = tvlqr_periodic_vjp(*args, ss.K, ss.k, ss.V, ss.v, ss.status, **ups, segments=segments)
        tensors = dict(zip(GRADS + ("residual", "iterations", "status"), out))
        if Bk == 1:
            return tensors, list(GRADS)                                    # (the scalars are views of one-element buffers)
        return tensors, list(tensors)

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
        for k in runs[0]:
            assert same(runs[0][k], other[k]), (k, label)
    assert all(torch.isfinite(v).all() for k, v in runs[0].items() if k in GRADS + ("residual",))
    assert not runs[0]["status"].any()


def test_without_the_flag_the_refusal_stands():
    F, f, C, c, _, _ = _case(3, 2, 4, 2, 4)
    leaves = _leaves(F, f, C, c)
    with pytest.raises(NotImplementedError, match="gradients") as err:
        tvlqr_periodic_steady_state(*leaves)
    assert "differentiable=True" in str(err.value)
    with pytest.raises(NotImplementedError, match="differentiable=True"):
        TimeVaryingLQR(*leaves, device="cuda", dtype=F64).periodic_steady_state(2)
    with torch.no_grad():                                                 # nothing records: nothing to refuse
        assert not tvlqr_periodic_steady_state(*leaves, segments=2).status.any()

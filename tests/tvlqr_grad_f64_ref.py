"""TEST INFRASTRUCTURE ONLY -- the gradients of the double-precision time-varying LQR solve (``tfmpc_tvlqr_vjp_f64``,
``tvlqr_solve(dtype=torch.float64)``) restated in numpy, generic in dtype, and the budget rule of their
tests.

``closed_form`` is the adjoint of DESIGN.md §3.8 -- fold, adjoint solve, costates, outer products -- with the costates of
steps 3 - 4 taken from the VALUE FUNCTION on the optimal trajectory,

    lam_t = V_t x_t + v_t,   dlam_t = V_t dx_t + v~_t,   V_T = C_fin, v_T = c_fin, v~_T = g_T,

where ``v~`` is the adjoint solve's own ``v`` and ``V`` is shared by both solves (same ``F, C, C_fin``; ``V`` does not
depend on linear terms).  ``costates="recursion"`` is §3.8's open-loop recursion
``lam_t = (C_t z_t + c_t)[:n] + F_t[:, :n]^T lam_{t+1}`` in the same dtype, kept to pin that the two agree where the
recursion is usable and by how much it fails where it is not.

THE REFERENCE is the value-function form in ``np.longdouble`` (80-bit).  The 80-bit RECURSION is not a reference past
T ~ 15 on unscaled models (``tvlqr_f64_ref.make_unscaled``, spectral radius of F_x ~ 5): it multiplies rounding error by
that radius per step and is off by 2e-5 at T = 20 and by 1e13 at T = 50 (gradient scale 1e2), while the value-function
form is closed-loop and keeps the error of the solve itself.  ``np.float64`` is the restatement whose error, next to fp64
autograd's, is the budget.

Budget rule (the project's own, one precision up, as ``tvlqr_f64_ref.ratios``): per output and instance,
``|got - ref_ld|_inf / max(err of the fp64 value-function form, err of tvlqr_grad_ref.autograd_grads(dtype=float64),
2^-48 max(1, |ref_ld|_inf))``; the median over instances <= 2.5 and every instance <= 10.  A batch- or time-summed
gradient's budget is the sum of its terms' budgets (per instance, per step).
"""

import numpy as np
import torch

import tvlqr_f64_ref as ref64
import tvlqr_grad_ref as gref
import tvlqr_ref

LD = np.longdouble
FLOOR = ref64.FLOOR
MEDIAN_BOUND, MAX_BOUND = ref64.MEDIAN_BOUND, ref64.MAX_BOUND
TIMED = ("F", "f", "C", "c")


def _solve(dtype, *args):
    if dtype == LD:
        return ref64.solve_ld(*args)
    return tvlqr_ref.solve(*args, dtype=dtype)


def _mv(A, x, reverse):
    """A x; ``reverse``: the row sums taken from the last column to the first."""
    if not reverse:
        return A @ x
    s = np.zeros(A.shape[0], dtype=A.dtype)
    for j in reversed(range(A.shape[1])):
        s = s + A[:, j] * x[j]
    return s


def closed_form(F, f, C, c, x0, Cfin=None, cfin=None, gx=None, gu=None, gcost=None, dtype=LD, costates="value",
                reverse=False):
    """ONE instance: F[T,n,d], f[T,n], C[T,d,d], c[T,d], x0[n], optional Cfin[n,n], cfin[n]; upstream gx[T+1,n], gu[T,m],
    gcost[T+1] (None = zero) -> dict of gradients F, f, C, c, x0 (and Cfin, cfin) in ``dtype``, symmetric convention for
    C and Cfin, the default final cost's added into C[T-1][:n,:n], c[T-1][:n] (as ``tvlqr_grad_ref.closed_form``)."""
    F, f, C, c, x0 = (np.asarray(a, dtype=dtype) for a in (F, f, C, c, x0))
    T, n, d = F.shape
    m = d - n
    f, c, x0 = f.reshape(T, n), c.reshape(T, d), x0.reshape(n)
    z0 = lambda *s: np.zeros(s, dtype=dtype)                                         # noqa: E731
    gx = z0(T + 1, n) if gx is None else np.asarray(gx, dtype=dtype)
    gu = z0(T, m) if gu is None else np.asarray(gu, dtype=dtype)
    gcost = z0(T + 1) if gcost is None else np.asarray(gcost, dtype=dtype)
    default = Cfin is None
    Cf = C[T - 1][:n, :n] if default else np.asarray(Cfin, dtype=dtype)
    cf = c[T - 1][:n] if default else np.asarray(cfin, dtype=dtype).reshape(n)
    fwd = _solve(dtype, F, f, C, c, x0, Cf, cf)
    xs, us = fwd["states"], fwd["actions"]
    z = np.concatenate([xs[:T], us], axis=-1)
    xT = xs[T]
    r = np.stack([C[t] @ z[t] for t in range(T)]) + c                                # C_t z_t + c_t
    rT = Cf @ xT + cf
    g = np.concatenate([gx[:T], gu], axis=-1) + gcost[:T, None] * r                  # 1. fold
    gT = gx[T] + gcost[T] * rT
    adj = _solve(dtype, F, z0(T, n), C, g, z0(n), Cf, gT)                            # 2. adjoint solve
    dxs, dus = adj["states"], adj["actions"]
    dz = np.concatenate([dxs[:T], dus], axis=-1)
    dxT = dxs[T]
    lam1, dlam1 = [None] * T, [None] * T                                             # 3. costates of step t + 1
    if costates == "value":
        V = adj["V"]
        for t in range(T):
            last = t == T - 1
            Vn = Cf if last else V[t + 1]
            lam1[t] = _mv(Vn, xs[t + 1], reverse) + (cf if last else fwd["v"][t + 1])
            dlam1[t] = _mv(Vn, dxs[t + 1], reverse) + (gT if last else adj["v"][t + 1])
        dlam0 = adj["v"][0]                                                          # V_0 dx_0 + v~_0 with dx_0 = 0
    else:
        lam, dlam = rT, Cf @ dxT + gT
        for t in reversed(range(T)):
            lam1[t], dlam1[t] = lam, dlam
            FxT = F[t][:, :n].T
            lam = r[t][:n] + FxT @ lam
            dlam = (C[t] @ dz[t] + g[t])[:n] + FxT @ dlam
        dlam0 = dlam
    lam1, dlam1 = np.stack(lam1), np.stack(dlam1)
    outer = lambda a, b: a[..., :, None] * b[..., None, :]                           # noqa: E731
    half = dtype(0.5)
    out = dict(F=outer(dlam1, z) + outer(lam1, dz), f=dlam1,                         # 4. gradients
               C=half * (outer(dz, z) + outer(z, dz)) + half * gcost[:T, None, None] * outer(z, z),
               c=dz + gcost[:T, None] * z, x0=dlam0)
    dCf = half * (outer(dxT, xT) + outer(xT, dxT)) + half * gcost[T] * outer(xT, xT)
    dcf = dxT + gcost[T] * xT
    if default:
        out["C"][T - 1][:n, :n] += dCf
        out["c"][T - 1][:n] += dcf
    else:
        out.update(Cfin=dCf, cfin=dcf)
    return out


def grads(F, f, C, c, x0, Cfin, cfin, gx, gu, gcost, **kw):
    """``closed_form`` per instance of a batch (operands [B, T, ...], Cfin / cfin [B, ...] or None) -> dict of [B, ...]."""
    pick = lambda a, b: None if a is None else a[b]                                  # noqa: E731
    per = [closed_form(F[b], f[b], C[b], c[b], x0[b], pick(Cfin, b), pick(cfin, b), pick(gx, b), pick(gu, b),
                       pick(gcost, b), **kw) for b in range(F.shape[0])]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def references(F, f, C, c, x0, Cfin, cfin, gx, gu, gcost):
    """(the 80-bit value-function reference, the fp64 value-function restatement, fp64 autograd): dicts of [B, ...]."""
    ops = (F, f, C, c, x0, Cfin, cfin, gx, gu, gcost)
    auto = gref.autograd_grads(*ops, dtype=torch.float64)
    return grads(*ops, dtype=LD), grads(*ops, dtype=np.float64), {k: v.numpy() for k, v in auto.items()}


def _err(a, ref):
    return float(np.abs(np.asarray(a, dtype=LD) - ref).max())


def term_budgets(refs, name, time_summed=False):
    """Budget per instance of output ``name``: max(error of either fp64 restatement, floor); for a gradient summed over
    time, the sum over the steps of the per-step budgets."""
    rld, r64, auto = refs

    def one(ref, a, b):
        return max(_err(a, ref), _err(b, ref), FLOOR * max(1.0, float(np.abs(ref).max())))
    out = []
    for b in range(rld[name].shape[0]):
        if time_summed and name in TIMED:
            out.append(sum(one(rld[name][b, t], r64[name][b, t], auto[name][b, t]) for t in range(rld[name].shape[1])))
        else:
            out.append(one(rld[name][b], r64[name][b], auto[name][b]))
    return np.array(out)


def ratios(got, refs, name, batch_summed=False, time_summed=False, idx=None):
    """The rule's ratio(s) for ``got`` (an array shaped like the operand of output ``name``): one per instance, or one in
    all for a batch-summed gradient.  The reference is summed in 80-bit over the axes ``got`` is summed over.  ``idx``:
    the instances to judge (the others are left out of per-instance ratios; a batch sum takes all)."""
    ref = refs[0][name]
    budgets = term_budgets(refs, name, time_summed)
    if time_summed and name in TIMED:
        ref = ref.sum(axis=1, keepdims=True)
    got = np.asarray(got, dtype=LD).reshape((-1,) + ref.shape[1:])
    if batch_summed:
        err = _err(got[0], ref.sum(axis=0))
        assert np.isfinite(err), name
        return np.array([err / budgets.sum()])
    idx = range(ref.shape[0]) if idx is None else idx
    out = []
    for b in idx:
        err = _err(got[b], ref[b])
        assert np.isfinite(err), (name, b)
        out.append(err / budgets[b])
    return np.array(out)


def check(got, refs, what="", shared=(), time_shared=(), idx=None, log=None):
    """Every gradient of ``got`` (dict name -> array) under the rule; ``shared`` / ``time_shared``: the names summed over the
    batch / over time.  ``log``: a dict that collects (median, max) per name."""
    for name in got:
        r = ratios(got[name], refs, name, name in shared, name in time_shared, idx)
        print(f"budget {what} d{name}: median {np.median(r):.3g} max {r.max():.3g}")
        if log is not None:
            log[name] = (float(np.median(r)), float(r.max()))
        assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))

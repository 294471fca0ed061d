"""TEST INFRASTRUCTURE ONLY -- restatements for the double-precision gradients of the infinite-horizon LQR
(``tfmpc_lqr_steady_state_vjp_f64``), and the budget rule of its tests.

``vjp_gj``       DESIGN.md 3.10's backward in the KERNEL's grouping (csrc/lqr_steady_state_vjp_f64.hip), for
                 ``np.float64`` or ``np.longdouble``: both eliminations through
                 ``lqr_steady_state_f64_ref.gauss_jordan`` (pivot-free for ``[G | I | gk]``, partial pivoting for
                 ``[I - A_cl | pbar]``, whose row exchanges it counts), the products grouped as the kernel groups them.
                 The forward defaults to ``steady_state_gj`` in the same ``dtype`` (so the 80-bit run starts from
                 ``steady_state_ld``).
``references``   per instance: the 80-bit result, the fp64 ``vjp_gj`` end to end, and the fp64 LAPACK restatement
                 (``lqr_steady_state_grad_ref.vjp(dtype=np.float64)``).
``own_forward``  the fp64 ``vjp_gj`` started from the kernel's own K, k, P, p (DESIGN.md 3.10's second budget term: the
                 backward cannot undo the error of the forward it is handed).
``ratios`` / ``check``  the one-precision-up budget rule per gradient and instance: the error
                 against the 80-bit result over max(error of the fp64 ``vjp_gj``, error of the LAPACK restatement, error
                 of ``own_forward``, 2^-48 max(1, |ref|_inf)); median over instances <= 2.5 and every instance <= 10.
                 No exception is granted: the fp32 gradients' ``LOOSE`` for ``dc`` on the damped workload (DESIGN.md
                 3.10) is not needed in double.
``check_summed`` a batch-summed gradient against the 80-bit sum; its budget is the sum of its terms' budgets.
"""

import numpy as np

import lqr_steady_state_f64_ref as ref64
import lqr_steady_state_grad_ref as gref
import lqr_steady_state_ref as ssref

LD = np.longdouble
GRADS = ("dF", "df", "dC", "dc")
OUTS = ("K", "k", "P", "p")
FLOOR = ref64.FLOOR
MEDIAN_BOUND, MAX_BOUND = ref64.MEDIAN_BOUND, ref64.MAX_BOUND


def _sym(X):
    return X.dtype.type(0.5) * (X + X.T)


def vjp_gj(F, f, C, c, gK=None, gk=None, gP=None, gp=None, dtype=np.float64, fwd=None, max_iter=gref.MAX_ITER, tol=None):
    """dict(dF [n,d], df [n], dC [d,d], dc [d], status, iterations, exchanges) of one instance.  ``fwd``: the forward's
    dict (default: ``steady_state_gj`` in ``dtype``).  A flagged forward or backward has NaN gradients."""
    F = np.asarray(F, dtype=dtype)
    f = np.asarray(f, dtype=dtype).reshape(-1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(-1)
    n = F.shape[0]
    m = F.shape[1] - n
    tol = dtype(4.0) * np.finfo(dtype).eps if tol is None else dtype(tol)
    if fwd is None:
        fwd = ref64.steady_state_gj(F, f, C, c, dtype=dtype)

    def flagged(status, it=0, exchanges=0):
        return dict(gref._nan(n, m, dtype), status=int(status), iterations=it, exchanges=exchanges)

    if fwd["status"]:
        return flagged(fwd["status"])
    K, k, P, p = (np.asarray(fwd[name], dtype=dtype) for name in OUTS)
    k, p = k.reshape(-1), p.reshape(-1)
    zeros = lambda *s: np.zeros(s, dtype)     # noqa: E731
    gK = zeros(m, n) if gK is None else np.asarray(gK, dtype).reshape(m, n)
    gk = zeros(m) if gk is None else np.asarray(gk, dtype).reshape(-1)
    gP = zeros(n, n) if gP is None else np.asarray(gP, dtype).reshape(n, n)
    gp = zeros(n) if gp is None else np.asarray(gp, dtype).reshape(-1)
    A, Bm = F[:, :n], F[:, n:]
    R = C[n:, n:]
    cu = c[n:]
    two = dtype(2.0)

    with np.errstate(all="ignore"):
        PB = P @ Bm
        Acl = A + Bm @ K
        w = P @ f + p
        aug = np.concatenate([_sym(R + Bm.T @ PB), np.eye(m, dtype=dtype), gk[:, None]], axis=1)
        if ref64.gauss_jordan(aug, m, False)[0]:
            return flagged(ssref.ST_NOT_PD)
        Gi, kappa = aug[:, m:2 * m], aug[:, 2 * m].copy()
        Bk = Bm @ kappa
        wbar = -Bk
        aug = np.concatenate([np.eye(n, dtype=dtype) - Acl, (gp - Bk)[:, None]], axis=1)
        bad, exchanges = ref64.gauss_jordan(aug, n, True)
        if bad:
            return flagged(ssref.ST_SINGULAR, exchanges=exchanges)
        rho = aug[:, n].copy()
        Krho = K @ rho
        v = wbar + Acl @ rho
        y = cu + Bm.T @ w
        Kbar = gK + np.outer(y, rho)
        L = (-Gi) @ Kbar
        Gbar = -np.outer(kappa, k) + L @ K.T
        U = np.concatenate([L, Gbar], axis=1) @ F.T
        Pbar = (gP + np.outer(v, f)) + Bm @ U
        Y, it, ok = gref.smith(Acl, _sym(Pbar), max_iter, tol)
        if not ok:
            return flagged(ssref.ST_NOT_STABILISING, it, exchanges)
        KY = K @ Y
        PA = P @ A
        W1 = PA + PB @ K
        Rbar = Gbar + KY @ K.T
        Sbar = L.T + two * KY.T
        dA = np.outer(w, rho) + np.concatenate([PB, W1], axis=1) @ np.concatenate([L, two * Y], axis=0)
        dB = np.outer(w, Krho - kappa) + np.concatenate([PA, PB, W1], axis=1) @ np.concatenate([L.T, Gbar + Gbar.T, two * KY.T], axis=0)
        dC = np.empty((n + m, n + m), dtype)
        dC[:n, :n] = _sym(Y)
        dC[:n, n:] = dtype(0.5) * Sbar
        dC[n:, :n] = dtype(0.5) * Sbar.T
        dC[n:, n:] = _sym(Rbar)
        out = dict(dF=np.concatenate([dA, dB], axis=1), df=P @ v, dC=dC, dc=np.concatenate([rho, Krho - kappa]), status=0,
                   iterations=it, exchanges=exchanges)
    assert all(out[name].dtype == dtype for name in GRADS)
    return out


def upstream_of(ups, b):
    """Instance b's gK, gk, gP, gp of ``ups`` (name -> [B, ...] array or None)."""
    return {name: (None if ups.get(name) is None else ups[name][b]) for name in ("gK", "gk", "gP", "gp")}


def references(F, f, C, c, ups, idx=None):
    """Per instance of ``idx``: (80-bit ``vjp_gj`` from ``steady_state_ld``, fp64 ``vjp_gj`` end to end, fp64 LAPACK
    restatement)."""
    idx = range(F.shape[0]) if idx is None else idx
    rld = [vjp_gj(F[b], f[b], C[b], c[b], **upstream_of(ups, b), dtype=LD) for b in idx]
    rgj = [vjp_gj(F[b], f[b], C[b], c[b], **upstream_of(ups, b)) for b in idx]
    rla = [gref.vjp(F[b], f[b], C[b], c[b], **upstream_of(ups, b), dtype=np.float64) for b in idx]
    for r in rld + rgj + rla:
        assert r["status"] == 0, r["status"]
    return rld, rgj, rla


def own_forward(F, f, C, c, ups, fwd, idx=None, fwd_index=None):
    """Per instance of ``idx``: the fp64 ``vjp_gj`` started from the kernel's forward outputs ``fwd[name][fwd_index[j]]``
    (name in K, k, P, p; numpy float64)."""
    idx = list(range(F.shape[0]) if idx is None else idx)
    fwd_index = idx if fwd_index is None else fwd_index
    out = []
    for j, b in enumerate(idx):
        own = {name: np.asarray(fwd[name][fwd_index[j]], dtype=np.float64) for name in OUTS}
        out.append(vjp_gj(F[b], f[b], C[b], c[b], **upstream_of(ups, b), fwd=dict(own, status=0)))
        assert out[-1]["status"] == 0
    return out


def budgets(refs, name, own=None, extra=None):
    """Instance j's budget for gradient ``name``."""
    rld, rgj, rla = refs
    out = []
    for j in range(len(rld)):
        ref = rld[j][name]
        budget = max(ref64.error(rgj[j][name], ref), ref64.error(rla[j][name], ref), FLOOR * ref64.scale_of(ref))
        if own is not None:
            budget = max(budget, ref64.error(own[j][name], ref))
        if extra is not None:
            budget = max(budget, extra[j][name])
        out.append(budget)
    return np.array(out)


def ratios(got, refs, name, idx=None, own=None, extra=None):
    """The budget rule's ratio per instance for gradient ``name``; ``got[name][b]`` is instance ``idx[j]``'s."""
    rld = refs[0]
    idx = list(range(len(rld))) if idx is None else list(idx)
    bud = budgets(refs, name, own, extra)
    out = []
    for j, b in enumerate(idx):
        ref = rld[j][name]
        err = ref64.error(np.asarray(got[name][b]).reshape(ref.shape), ref)
        assert np.isfinite(err), (name, b)
        out.append(err / bud[j])
    return np.array(out)


def check(got, refs, idx=None, own=None, names=GRADS, what="", extra=None):
    for name in names:
        r = ratios(got, refs, name, idx, own, extra)
        print(f"budget {what} {name}: median {np.median(r):.3g} max {r.max():.3g}")
        assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))


def check_summed(got, refs, name, own=None, what=""):
    """``got``: the batch-summed gradient ``name`` over exactly the instances of ``refs``."""
    ref = sum(r[name] for r in refs[0])
    budget = float(budgets(refs, name, own).sum())
    ratio = ref64.error(np.asarray(got).reshape(ref.shape), ref) / budget
    print(f"budget {what} sum {name}: {ratio:.3g}")
    assert ratio <= MEDIAN_BOUND, (what, name, ratio)

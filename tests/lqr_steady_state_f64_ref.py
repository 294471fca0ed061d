"""TEST INFRASTRUCTURE ONLY -- restatements for the double-precision infinite-horizon LQR
(``tfmpc_lqr_steady_state_f64``), and the budget rule of its tests.

``steady_state_gj``  the KERNEL's operation order in numpy, for ``np.float64`` or ``np.longdouble``: Gauss-Jordan with
                     partial pivoting (first row of maximal |entry|, pivot row scaled by the reciprocal of the pivot) for
                     ``[I + GH | A_k | G_k]`` and ``I - A_cl'``, pivot-free elimination of the definite systems ``R`` and
                     ``R + B'PB``, sums in plain order, row operations vectorised.  Also counts the row exchanges of the
                     pivoted solves (``exchanges_sda``, ``exchanges_p``).
``steady_state_ld``  the same in ``np.longdouble`` (80-bit on x86-64): the reference the fp64 results are measured
                     against.
``operands``         the two workloads of tests/lqr_steady_state_ref.py in float64, F multiplied by 1 + 1e-9 N(0, 1) so
                     that no entry is representable in fp32.
``ratios`` / ``check``  the one-precision-up budget rule: per output and instance, the error against
                     ``steady_state_ld`` over max(error of the fp64 ``steady_state_gj``, error of the fp64
                     ``lqr_steady_state_ref.steady_state`` (LAPACK), 2^-48 max(1, |ref|_inf)); median over instances
                     <= 2.5 and every instance <= 10.
"""

import numpy as np

import lqr_steady_state_ref as ssref

LD = np.longdouble
FIELDS = ("K", "k", "P", "p")
FLOOR = 2.0 ** -48
MEDIAN_BOUND, MAX_BOUND = 2.5, 10.0


def gauss_jordan(aug, rows, pivot):
    """In-place elimination of ``aug[rows][width]`` as csrc/wave_ops.h wave_gauss_jordan does it.  Returns
    (bad, row exchanges): bad is a zero pivot (``pivot``) or a non-positive / NaN one (pivot-free)."""
    one = aug.dtype.type(1)
    bad, exchanges = False, 0
    for p in range(rows):
        fac = aug[:rows, p].copy()
        piv = p + int(np.argmax(np.abs(fac[p:]))) if pivot else p          # (argmax: the first of equal maxima)
        pv = fac[piv]
        if (pv == 0) if pivot else not (pv > 0):
            bad = True
        pr = aug[piv] * (one / pv)
        if piv != p:
            exchanges += 1
            aug[piv] = aug[p]
            fac[piv] = fac[p]
        fac[p] = 0
        aug[:rows] -= fac[:, None] * pr[None, :]
        aug[p] = pr
    return bad, exchanges


def _sym(X):
    return X.dtype.type(0.5) * (X + X.T)


def steady_state_gj(F, f, C, c, dtype=np.float64, max_iter=ssref.MAX_ITER, tol=None):
    """dict(K [m,n], k [m], P [n,n], p [n], iterations, status, exchanges_sda, exchanges_p) of one instance; a flagged
    instance has NaN outputs.  ``tol`` defaults to 4 ulp of ``dtype``."""
    F = np.asarray(F, dtype=dtype)
    f = np.asarray(f, dtype=dtype).reshape(-1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(-1)
    n = F.shape[0]
    m = F.shape[1] - n
    tol = dtype(4.0) * np.finfo(dtype).eps if tol is None else dtype(tol)
    a_zero = dtype(ssref.A_ZERO)
    A, Bm = F[:, :n], F[:, n:]
    Q, S, R = C[:n, :n], C[:n, n:], C[n:, n:]
    cx, cu = c[:n], c[n:]
    eye = np.eye(n, dtype=dtype)
    count = dict(exchanges_sda=0, exchanges_p=0)

    def flagged(status, it):
        return dict(K=np.full((m, n), np.nan, dtype), k=np.full(m, np.nan, dtype), P=np.full((n, n), np.nan, dtype),
                    p=np.full(n, np.nan, dtype), iterations=it, status=status, **count)

    with np.errstate(all="ignore"):
        aug = np.concatenate([R, S.T, Bm.T], axis=1)
        if gauss_jordan(aug, m, False)[0]:
            return flagged(ssref.ST_NOT_PD, 0)
        RiSt, RiBt = aug[:, m:m + n], aug[:, m + n:]
        Ak = A - Bm @ RiSt
        G = _sym(Bm @ RiBt)
        H = _sym(Q - S @ RiSt)
        it, converged = 0, False
        while it < max_iter:
            it += 1
            aug = np.concatenate([eye + G @ H, Ak, G], axis=1)
            bad, ex = gauss_jordan(aug, n, True)
            count["exchanges_sda"] += ex
            if bad:
                return flagged(ssref.ST_SINGULAR, it)
            Y1, Y2 = aug[:, n:2 * n], aug[:, 2 * n:]
            G = G + _sym((Ak @ Y2) @ Ak.T)
            inc = _sym(Ak.T @ (H @ Y1))
            H = H + inc
            Ak = Ak @ Y1
            if not (np.isfinite(H).all() and np.isfinite(inc).all() and np.isfinite(Ak).all()):
                break
            if np.abs(inc).max() <= tol * np.abs(H).max() and np.abs(Ak).max() <= a_zero:
                converged = True
                break
        if not converged:
            return flagged(ssref.ST_NOT_STABILISING, it)
        P = H
        Pf = P @ f
        aug = np.concatenate([Bm.T @ (P @ Bm) + R, Bm.T @ (P @ A) + S.T, cu[:, None], Bm.T], axis=1)
        aug[:, :m] = _sym(aug[:, :m])
        if gauss_jordan(aug, m, False)[0]:
            return flagged(ssref.ST_NOT_PD, it)
        K, kc, Z = -aug[:, m:m + n], -aug[:, m + n], aug[:, m + n + 1:]
        Acl = A + Bm @ K
        aug = np.concatenate([eye - Acl.T, ((cx + K.T @ cu) + Acl.T @ Pf)[:, None]], axis=1)
        bad, count["exchanges_p"] = gauss_jordan(aug, n, True)
        if bad:
            return flagged(ssref.ST_SINGULAR, it)
        p = aug[:, n]
        k = kc - Z @ (Pf + p)
        out = dict(K=K, k=k, P=P, p=p, iterations=it, status=0, **count)
        if not all(np.isfinite(out[name]).all() for name in FIELDS) or not ssref._certified(Acl, max_iter):
            return flagged(ssref.ST_NOT_STABILISING, it)
    return out


def steady_state_ld(F, f, C, c, max_iter=ssref.MAX_ITER):
    return steady_state_gj(F, f, C, c, dtype=LD, max_iter=max_iter)


def operands(kind, n, m, B, seed=0):
    """F [B,n,n+m], f [B,n], C [B,d,d], c [B,d] of workload ``kind`` ("make_lqr" or "damped") in float64, no entry of F
    representable in fp32."""
    make = ssref.make_lqr_batch if kind == "make_lqr" else ssref.damped_workload
    F, f, C, c = (a.astype(np.float64) for a in make(n, m, B, seed=seed))
    F = F * (1.0 + 1e-9 * np.random.default_rng(seed + 1000).normal(size=F.shape))
    return F, f, C, c


def references(F, f, C, c, idx=None):
    """Per instance of ``idx``: (``steady_state_ld``, fp64 ``steady_state_gj``, fp64 ``ssref.steady_state``)."""
    idx = range(F.shape[0]) if idx is None else idx
    rld = [steady_state_ld(F[b], f[b], C[b], c[b]) for b in idx]
    rgj = [steady_state_gj(F[b], f[b], C[b], c[b]) for b in idx]
    rla = [ssref.steady_state(F[b], f[b], C[b], c[b], dtype=np.float64) for b in idx]
    return rld, rgj, rla


def error(got, ref):
    """Largest absolute deviation of an fp64 array from a longdouble reference, taken in longdouble."""
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max())


def scale_of(ref):
    return max(1.0, float(np.abs(ref).max()))


def ratios(got, refs, name, idx=None, extra=None):
    """The budget rule's ratio per instance for output ``name``; ``got[name][b]`` is instance ``idx[j]``'s result and
    ``refs`` what ``references`` returned for those instances.  ``extra[j][name]``: a further error that widens
    instance j's budget (a test that composes two kernels)."""
    rld, rgj, rla = refs
    idx = list(range(len(rld))) if idx is None else list(idx)
    out = []
    for j, b in enumerate(idx):
        ref = rld[j][name]
        budget = max(error(rgj[j][name], ref), error(rla[j][name], ref), FLOOR * scale_of(ref))
        if extra is not None:
            budget = max(budget, extra[j][name])
        err = error(got[name][b], ref)
        assert np.isfinite(err), (name, b)
        out.append(err / budget)
    return np.array(out)


def check(got, refs, idx=None, fields=FIELDS, what="", extra=None):
    for name in fields:
        r = ratios(got, refs, name, idx, extra)
        print(f"budget {what} {name}: median {np.median(r):.3g} max {r.max():.3g}")
        assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))

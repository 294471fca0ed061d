"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the steady state's vector-Jacobian product
(``tfmpc_lqr_steady_state_vjp_f32``): given the forward's K, k, P, p and upstream gradients gK, gk, gP,
gp, the gradients of ``<gK, K> + <gk, k> + <gP, P> + <gp, p>`` with respect to F, f, C, c.

The explicit formulas are reversed first (k, p, A_cl, K, G = R + B'PB), then P's implicit dependence through the
Riccati equation is one Stein solve ``Y = A_cl Y A_cl' + sym(Pbar)`` by Smith doubling.  The grouping of the products
is the kernel's (csrc/lqr_steady_state_vjp.hip), single instance, ``dtype`` float32 (the fp32 error budget, started
from the fp32 forward of tests/lqr_steady_state_ref.py) or float64 (the truth, itself checked against central
differences and against autograd through the finite recursion by tests/test_lqr_steady_state_grad_cpu.py).

``dC`` is the symmetric gradient: C enters only as a symmetric matrix, so ``dC = sym([[Qbar, Sbar], [0, Rbar]])``.
"""

import numpy as np

import lqr_steady_state_ref as ssref

ST_SINGULAR, ST_NOT_PD, ST_NOT_STABILISING = ssref.ST_SINGULAR, ssref.ST_NOT_PD, ssref.ST_NOT_STABILISING
MAX_ITER = ssref.MAX_ITER
PHI_ZERO = ssref.A_ZERO          # Smith doubling stops once max|Phi^2| <= PHI_ZERO (and the increment is below tol)


def _sym(X):
    return 0.5 * (X + X.T)


def _nan(n, m, dtype):
    d = n + m
    return dict(dF=np.full((n, d), np.nan, dtype), df=np.full(n, np.nan, dtype), dC=np.full((d, d), np.nan, dtype),
                dc=np.full(d, np.nan, dtype))


def smith(Acl, X, max_iter, tol):
    """Y = sum_j Acl^j X Acl'^j by doubling: (Y, iterations, converged)."""
    Y, Phi = X.copy(), Acl.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(1, max_iter + 1):
            inc = (Phi @ Y) @ Phi.T
            Y = Y + _sym(inc)
            Phi = Phi @ Phi
            if not (np.isfinite(inc).all() and np.isfinite(Y).all() and np.isfinite(Phi).all()):
                return Y, it, False
            if np.abs(inc).max() <= tol * np.abs(Y).max() and np.abs(Phi).max() <= PHI_ZERO:
                return Y, it, True
    return Y, max_iter, False


def vjp(F, f, C, c, gK=None, gk=None, gP=None, gp=None, dtype=np.float64, fwd=None, max_iter=MAX_ITER, tol=None):
    """Returns dict(dF [n,d], df [n], dC [d,d], dc [d], status, iterations).  ``fwd``: the forward's dict (default: the
    restatement's own steady state in ``dtype``).  A flagged forward or backward instance has NaN gradients."""
    F = np.asarray(F, dtype=dtype)
    f = np.asarray(f, dtype=dtype).reshape(-1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(-1)
    n = F.shape[0]
    m = F.shape[1] - n
    if tol is None:
        tol = ssref.TOL_F32 if dtype == np.float32 else 4.0 * float(np.finfo(np.float64).eps)
    if fwd is None:
        fwd = ssref.steady_state(F, f, C, c, dtype=dtype)
    if fwd["status"]:
        return dict(_nan(n, m, dtype), status=int(fwd["status"]), iterations=0)
    K, k, P, p = (np.asarray(fwd[name], dtype=dtype) for name in ("K", "k", "P", "p"))
    k, p = k.reshape(-1), p.reshape(-1)
    zeros = lambda *s: np.zeros(s, dtype)     # noqa: E731
    gK = zeros(m, n) if gK is None else np.asarray(gK, dtype).reshape(m, n)
    gk = zeros(m) if gk is None else np.asarray(gk, dtype).reshape(-1)
    gP = zeros(n, n) if gP is None else np.asarray(gP, dtype).reshape(n, n)
    gp = zeros(n) if gp is None else np.asarray(gp, dtype).reshape(-1)
    A, Bm = F[:, :n], F[:, n:]
    R = C[n:, n:]
    cx, cu = c[:n], c[n:]

    # recomputed forward quantities
    PB = P @ Bm
    G = R + Bm.T @ PB
    Acl = A + Bm @ K
    Pf = P @ f
    # 1. k: kappa = G^-1 gk (and G^-1 itself, for L below: one elimination without pivoting)
    try:
        np.linalg.cholesky(_sym(G))
    except np.linalg.LinAlgError:
        return dict(_nan(n, m, dtype), status=ST_NOT_PD, iterations=0)
    X = np.linalg.solve(G, np.concatenate([np.eye(m, dtype=dtype), gk[:, None]], axis=1))
    Gi, kappa = X[:, :m], X[:, m]
    w = Pf + p
    wbar = -(Bm @ kappa)
    pbar = gp + wbar
    # 2. p: rho = (I - A_cl)^-1 pbar
    try:
        rho = np.linalg.solve(np.eye(n, dtype=dtype) - Acl, pbar)
    except np.linalg.LinAlgError:
        return dict(_nan(n, m, dtype), status=ST_SINGULAR, iterations=0)
    Krho = K @ rho
    v = wbar + Acl @ rho                    # Pbar += v f',  fbar = P v
    df = P @ v
    dcx, dcu = rho, Krho - kappa
    y = cu + Bm.T @ w
    # 3, 4. A_cl is rank one here (w rho'); Kbar = gK + y rho'; L = -G^-1 Kbar; Gbar = -kappa k' + L K'
    Kbar = gK + np.outer(y, rho)
    L = -(Gi @ Kbar)
    Gbar = -np.outer(kappa, k) + L @ K.T
    # Pbar = gP + v f' + B (L A' + Gbar B')
    U = np.concatenate([L, Gbar], axis=1) @ F.T
    Pbar = gP + np.outer(v, f) + Bm @ U
    # 6. Stein solve
    Y, it, ok = smith(Acl, _sym(Pbar), max_iter, tol)
    if not ok:
        return dict(_nan(n, m, dtype), status=ST_NOT_STABILISING, iterations=it)
    KY = K @ Y
    Rbar = Gbar + KY @ K.T
    Sbar = L.T + 2.0 * KY.T
    PA = P @ A
    W1 = PA + PB @ K                        # P A_cl
    dA = np.outer(w, rho) + np.concatenate([PB, W1], axis=1) @ np.concatenate([L, 2.0 * Y], axis=0)
    dB = np.outer(w, Krho - kappa) + np.concatenate([PA, PB, W1], axis=1) @ np.concatenate([L.T, Gbar + Gbar.T, 2.0 * KY.T], axis=0)
    dC = np.empty((n + m, n + m), dtype)
    dC[:n, :n] = _sym(Y)
    dC[:n, n:] = 0.5 * Sbar
    dC[n:, :n] = 0.5 * Sbar.T
    dC[n:, n:] = _sym(Rbar)
    out = dict(dF=np.concatenate([dA, dB], axis=1), df=df, dC=dC, dc=np.concatenate([dcx, dcu]), status=0, iterations=it)
    if not all(np.isfinite(out[name]).all() for name in ("dF", "df", "dC", "dc")):
        return dict(_nan(n, m, dtype), status=ST_NOT_STABILISING, iterations=it)
    return out


def steady_state_grad_fd(F, f, C, c, gK, gk, gP, gp, eps=1e-6):
    """Central differences of the fp64 steady state's loss <gK, K> + <gk, k> + <gP, P> + <gp, p> (C perturbed as a
    symmetric pair), for the CPU tests."""
    def loss(F_, f_, C_, c_):
        r = ssref.steady_state(F_, f_, C_, c_)
        assert r["status"] == 0
        return (gK * r["K"]).sum() + (gk * r["k"]).sum() + (gP * r["P"]).sum() + (gp * r["p"]).sum()

    ops = [np.array(a, dtype=np.float64) for a in (F, f, C, c)]
    out = []
    for i, a in enumerate(ops):
        g = np.zeros_like(a)
        for idx in np.ndindex(a.shape):
            if i == 2 and idx[0] > idx[1]:
                continue
            plus, minus = [o.copy() for o in ops], [o.copy() for o in ops]
            for o, s in ((plus, eps), (minus, -eps)):
                o[i][idx] += s
                if i == 2 and idx[0] != idx[1]:
                    o[i][idx[::-1]] += s
            g[idx] = (loss(*plus) - loss(*minus)) / (2 * eps)
        if i == 2:          # a symmetric pair moved together: split the derivative half and half
            off = ~np.eye(a.shape[0], dtype=bool)
            g = np.triu(g)
            g = g + np.triu(g, 1).T
            g[off] *= 0.5
        out.append(g)
    return dict(zip(("dF", "df", "dC", "dc"), out))

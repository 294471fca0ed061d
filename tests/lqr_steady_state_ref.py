"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the infinite-horizon LQR of ``tfmpc_lqr_steady_state_f32``
(DESIGN.md 3.9): the structure-preserving doubling algorithm (SDA) for P, then the gains, the affine terms and the
closed-loop certificate.

Same operation order as the kernel (csrc/lqr_steady_state.hip), single instance, ``dtype`` float32 (the fp32 error
budget) or float64 (the truth, itself checked against scipy and against the finite recursion of oracle/lqr_ref.py).
"""

import numpy as np

ST_SINGULAR, ST_NOT_PD, ST_NOT_STABILISING = 0x1, 0x2, 0x80
MAX_ITER = 40
TOL_F32 = 4.0 * float(np.finfo(np.float32).eps)      # the kernel's default: |H_{k+1} - H_k| <= tol |H_{k+1}| (max norms)
A_ZERO = 1e-3                                        # ... and max |A_{k+1}| <= A_ZERO: the closed loop's doubling went to zero


def _chol_solve(R, rhs):
    """R^-1 rhs for a symmetric R, or None if R is not positive definite (the kernel: elimination without pivoting)."""
    try:
        np.linalg.cholesky(R)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(R, rhs)


def _sym(X):
    return 0.5 * (X + X.T)


def steady_state(F, f, C, c, max_iter=MAX_ITER, tol=None, dtype=np.float64):
    """Returns dict(K [m,n], k [m], P [n,n], p [n], iterations, status).  A flagged instance has NaN outputs."""
    F = np.asarray(F, dtype=dtype)
    f = np.asarray(f, dtype=dtype).reshape(-1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(-1)
    n = F.shape[0]
    m = F.shape[1] - n
    if tol is None:
        tol = TOL_F32 if dtype == np.float32 else 4.0 * float(np.finfo(np.float64).eps)
    A, Bm = F[:, :n], F[:, n:]
    Q, S, R = C[:n, :n], C[:n, n:], C[n:, n:]
    cx, cu = c[:n], c[n:]
    nan = dict(K=np.full((m, n), np.nan, dtype), k=np.full(m, np.nan, dtype), P=np.full((n, n), np.nan, dtype),
               p=np.full(n, np.nan, dtype))

    X = _chol_solve(R, np.concatenate([S.T, Bm.T], axis=1))
    if X is None:
        return dict(nan, iterations=0, status=ST_NOT_PD)
    RiSt, RiBt = X[:, :n], X[:, n:]
    Ak = A - Bm @ RiSt
    G = _sym(Bm @ RiBt)
    H = _sym(Q - S @ RiSt)
    eye = np.eye(n, dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        status, it, converged, G, H, Ak = _doubling(Ak, G, H, eye, max_iter, tol)
    if status:
        return dict(nan, iterations=it, status=status)
    if not converged:
        return dict(nan, iterations=it, status=ST_NOT_STABILISING)
    P = H
    W = P @ Bm
    Muu = _sym(R + Bm.T @ W)
    X = _chol_solve(Muu, np.concatenate([Bm.T @ (P @ A) + S.T, cu[:, None], Bm.T], axis=1))
    if X is None:
        return dict(nan, iterations=it, status=ST_NOT_PD)
    K, kc, Z = -X[:, :n], -X[:, n], X[:, n + 1:]
    Acl = A + Bm @ K
    try:
        p = np.linalg.solve(eye - Acl.T, cx + K.T @ cu + Acl.T @ (P @ f))
    except np.linalg.LinAlgError:
        return dict(nan, iterations=it, status=ST_SINGULAR)
    k = kc - Z @ (P @ f + p)
    out = dict(K=K, k=k, P=P, p=p, iterations=it, status=0)
    if not all(np.isfinite(out[name]).all() for name in ("K", "k", "P", "p")) or not _certified(Acl, max_iter):
        return dict(nan, iterations=it, status=ST_NOT_STABILISING)
    return out


def _doubling(Ak, G, H, eye, max_iter, tol):
    """The SDA loop: (status, iterations, converged, G, H, A_k)."""
    n = eye.shape[0]
    status, it, converged = 0, 0, False
    while it < max_iter:
        it += 1
        M = eye + G @ H
        try:
            Y = np.linalg.solve(M, np.concatenate([Ak, G], axis=1))
        except np.linalg.LinAlgError:
            status |= ST_SINGULAR
            break
        Y1, Y2 = Y[:, :n], Y[:, n:]
        G = G + _sym((Ak @ Y2) @ Ak.T)
        incH = _sym(Ak.T @ (H @ Y1))
        H = H + incH
        Ak = Ak @ Y1
        dH, Hmax, Amax = np.abs(incH).max(), np.abs(H).max(), np.abs(Ak).max()
        if not (np.isfinite(dH) and np.isfinite(Hmax) and np.isfinite(Amax)):
            break
        if dH <= tol * Hmax and Amax <= A_ZERO:
            converged = True
            break
    return status, it, converged, G, H, Ak


def _certified(Acl, max_iter):
    """A_cl^(2^j) -> 0 within max_iter squarings: the closed loop is stable."""
    M = Acl
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(max_iter):
            M = M @ M
            if not np.isfinite(M).all():
                return False
            if np.abs(M).max() <= A_ZERO:
                return True
    return False


def damped_workload(n, m, B, seed=0, dtype=np.float32):
    """Lightly damped plants: A orthogonal, B = 0.05 N(0, 1), C = diag(1e-3 I, I), c ~ N(0, 1) -- closed-loop spectral
    radius about 0.997 at n = 16, m = 8.  Returns F [B,n,n+m], f [B,n], C [B,d,d], c [B,d]."""
    rng = np.random.default_rng(seed)
    d = n + m
    F = np.empty((B, n, d))
    for b in range(B):
        q, r = np.linalg.qr(rng.normal(size=(n, n)))
        F[b, :, :n] = q * np.sign(np.diag(r))
        F[b, :, n:] = 0.05 * rng.normal(size=(n, m))
    f = rng.normal(size=(B, n))
    C = np.broadcast_to(np.diag(np.r_[np.full(n, 1e-3), np.ones(m)]), (B, d, d)).copy()
    c = rng.normal(size=(B, d))
    return tuple(a.astype(dtype) for a in (F, f, C, c))


def make_lqr_batch(n, m, B, seed=0):
    """``tfmpc.envs.make_lqr``'s draws (global numpy RNG, the reference's order) as float32 arrays, C symmetrised."""
    from sklearn.datasets import make_spd_matrix
    np.random.seed(seed)
    d = n + m
    out = []
    for _ in range(B):
        F = np.random.normal(size=(n, d))
        f = np.random.normal(size=(n,))
        C = make_spd_matrix(d)
        c = np.random.normal(size=(d,))
        out.append((F, f, 0.5 * (C + C.T), c))
    return tuple(np.stack(a).astype(np.float32) for a in zip(*out))

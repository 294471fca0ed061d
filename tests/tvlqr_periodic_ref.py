"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the periodic infinite-horizon LQR in double
(``tfmpc_tvlqr_periodic_steady_state_f64``), built on ``tvlqr_time_parallel_ref``'s ``condense`` /
``combine`` / ``close`` in the kernels' operation order.

The model's time axis is ONE PERIOD of N steps.  ``solve`` condenses every segment of the period into a segment element,
folds them (serially, from the last) into the one-period element ``E1``, doubles it -- ``E <- combine(E, E)``, the
element of 2^k periods, whose ``H -> P_0`` and ``h -> p_0`` (the periodic stabilising value function at phase 0) while
``A -> 0`` -- under the stop rule of DESIGN.md 3.16 extended to ``h``, certifies the closed-loop monodromy
``(I + G1 P_0)^-1 A1`` by squaring, closes over the seams and expands every segment with the sequential recursion in the
kernel's (Schur) form.  ``V[t], v[t]`` is the value function AT step t, so ``V[0] = P_0``.

``dtype=np.float64`` solves with ``np.linalg.solve``; ``dtype=np.longdouble`` with ``tvlqr_f64_ref.inv_ld``.
``brute`` is the longdouble sequential recursion over tiled periods, run until it is periodic.
"""

import numpy as np

import tvlqr_f64_ref as ref64
import tvlqr_time_parallel_ref as tp

LD = np.longdouble
FIELDS = ("K", "k", "V", "v")
ST_SINGULAR, ST_NOT_PD, ST_NAN, ST_NOT_STABILISING = 0x1, 0x2, 0x4, 0x80
MAX_ITER = 40
TOL = 4.0 * float(np.finfo(np.float64).eps)
A_ZERO = 1e-3
BRUTE_TOL = 2.0 ** -60
BRUTE_MAX_PERIODS = 1 << 14


def workspace_bytes(B, n, m, N, segments):
    """The C ABI's formula: with w = B P, the w segment elements and the B one-period elements (3 n n + 2 n doubles
    each), the value function at every segment's end (n n + n), the gains B N m (n + 1), then 2 w + B status words."""
    if min(B, n, m, N) <= 0 or segments < 1:
        return 0
    w = B * len(tp.segment_table(N, segments)[1])
    return 8 * ((w + B) * (3 * n * n + 2 * n) + w * (n * n + n) + B * N * m * (n + 1)) + (4 * (2 * w + B) + 7) // 8 * 8


class _Flag(Exception):
    def __init__(self, status, iterations=0):
        super().__init__(status)
        self.status, self.iterations = status, iterations


def _lin(dtype):
    """``solve(A, rhs)`` that raises ``_Flag(ST_SINGULAR)`` where the kernel's pivoted elimination meets a zero pivot."""
    inner = tp._solver(dtype)

    def solve(A, rhs):
        try:
            with np.errstate(all="ignore"):
                return inner(A, rhs)
        except (np.linalg.LinAlgError, ZeroDivisionError, FloatingPointError):
            raise _Flag(ST_SINGULAR) from None
    return solve


def _require_pd(M):
    """The kernel eliminates R_t and Q_uu without pivoting: a non-positive pivot <=> not positive definite."""
    try:
        np.linalg.cholesky(np.asarray(M, dtype=np.float64))
    except np.linalg.LinAlgError:
        raise _Flag(ST_NOT_PD) from None


def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in arrays)


def _amax(X):
    return float(np.abs(X).max())


def stitch(elems, lin, max_iter, tol):
    """The stitch kernel on the period's segment elements: ``(E1, P0, p0, Vend, vend, residual, iterations)``; raises
    ``_Flag``."""
    P = len(elems)
    E = elems[P - 1]
    for i in reversed(range(P - 1)):
        E = tp.combine(elems[i], E, lin)
    E1 = E
    it, converged = 0, False
    with np.errstate(all="ignore"):
        while it < max_iter:
            it += 1
            En = tp.combine(E, E, lin)
            dH, dh = _amax(En[3] - E[3]), _amax(En[4] - E[4])
            E = En
            if not _finite(*E):
                break
            if dH <= tol * _amax(E[3]) and dh <= tol * max(1.0, _amax(E[4])) and _amax(E[0]) <= A_ZERO:
                converged = True
                break
    if not converged:
        raise _Flag(ST_NOT_STABILISING, it)
    P0, p0 = E[3], E[4]
    n = P0.shape[0]
    # the closed-loop monodromy of one period, squared until it is small
    Phi = lin(np.eye(n, dtype=P0.dtype) + E1[2] @ P0, E1[0])
    certified = False
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            Phi = Phi @ Phi
            if not _finite(Phi):
                break
            if _amax(Phi) <= A_ZERO:
                certified = True
                break
    if not certified:
        raise _Flag(ST_NOT_STABILISING, it)
    Vend, vend = [None] * P, [None] * P
    V, v = P0, p0
    for i in reversed(range(P)):
        Vend[i], vend[i] = V, v
        V, v = tp.close(elems[i], V, v, lin)       # (i == 0: once around, back at phase 0)
    residual = max(_amax(V - P0) / _amax(P0), _amax(v - p0) / max(1.0, _amax(p0)))
    return E1, P0, p0, Vend, vend, residual, it


def solve(F, f, C, c, segments, max_iter=0, tol=0.0, dtype=np.float64):
    """One instance, one period: F[N,n,d], f[N,n], C[N,d,d], c[N,d] -> dict(K[N,m,n], k[N,m], V[N,n,n], v[N,n], residual,
    iterations, status); a flagged instance has NaN in K, k, V, v and residual."""
    dtype = np.dtype(dtype).type
    F = np.asarray(F, dtype=dtype)
    N, n = F.shape[0], F.shape[1]
    m = F.shape[2] - n
    f = np.asarray(f, dtype=dtype).reshape(N, n, 1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(N, n + m, 1)
    max_iter = max_iter or MAX_ITER
    tol = tol or TOL
    lin = _lin(dtype)
    _, table = tp.segment_table(N, segments)
    it = 0
    try:
        for t in range(N):
            _require_pd(C[t][n:, n:])
        elems = [tp.condense(F, f, C, c, t0, t1, n, lin) for t0, t1 in table]
        _, _, _, Vend, vend, residual, it = stitch(elems, lin, max_iter, tol)
        Ks, ks, Vs, vs = [None] * N, [None] * N, [None] * N, [None] * N
        for i, (t0, t1) in enumerate(table):
            V, v = Vend[i], vend[i]
            for t in reversed(range(t0, t1)):
                Ft, ft, Ct, ct = F[t], f[t], C[t], c[t]
                W = Ft.T @ V
                Q = Ct + W @ Ft
                q = ct + W @ ft + Ft.T @ v
                _require_pd(Q[n:, n:])
                sol = -lin(Q[n:, n:], np.concatenate([q[n:], Q[n:, :n]], axis=1))
                ks[t], Ks[t] = sol[:, :1], sol[:, 1:]
                V, v = tp._sym(Q[:n, :n] + Q[:n, n:] @ Ks[t]), q[:n] + Q[:n, n:] @ ks[t]
                Vs[t], vs[t] = V, v
        out = dict(K=np.stack(Ks), k=np.stack(ks)[..., 0], V=np.stack(Vs), v=np.stack(vs)[..., 0], residual=residual,
                   iterations=it, status=0)
        if not _finite(*(out[name] for name in FIELDS)):
            raise _Flag(ST_NAN)
        return out
    except _Flag as flag:
        nan = lambda *shape: np.full(shape, np.nan, dtype=dtype)          # noqa: E731
        return dict(K=nan(N, m, n), k=nan(N, m), V=nan(N, n, n), v=nan(N, n), residual=float("nan"),
                    iterations=max(it, flag.iterations), status=flag.status)


def solve_batch(F, f, C, c, segments, max_iter=0, tol=0.0, dtype=np.float64):
    """Per instance ``solve``: operands [B, N, ...] -> a list of dicts."""
    return [solve(F[b], f[b], C[b], c[b], segments, max_iter, tol, dtype) for b in range(F.shape[0])]


def brute(F, f, C, c, max_periods=BRUTE_MAX_PERIODS):
    """The longdouble sequential recursion (``tvlqr_f64_ref.solve_ld``) over tiled periods from a zero final cost, the
    period count doubled until ``V_0, v_0`` and ``V_N, v_N`` agree to 2^-60 relative: dict(K, k, V, v, periods) of the
    first period.  The recursion is continued from its own front, which is the same as starting over with more periods."""
    F = np.asarray(F, dtype=LD)
    N, n = F.shape[0], F.shape[1]
    f, C, c = np.asarray(f, dtype=LD).reshape(N, n), np.asarray(C, dtype=LD), np.asarray(c, dtype=LD).reshape(N, -1)
    Vf, vf = np.zeros((n, n), dtype=LD), np.zeros(n, dtype=LD)
    x0 = np.zeros(n, dtype=LD)
    count, total = 1, 0
    while total + count <= max_periods:
        tile = lambda a: np.concatenate([a] * count, axis=0)               # noqa: E731
        r = ref64.solve_ld(tile(F), tile(f), tile(C), tile(c), x0, Vf, vf)
        total += count
        VN, vN = (r["V"][N], r["v"][N]) if count > 1 else (Vf, vf)
        V0, v0 = r["V"][0], r["v"][0]
        if (np.abs(V0 - VN).max() <= BRUTE_TOL * max(1.0, float(np.abs(V0).max())) and
                np.abs(v0 - vN).max() <= BRUTE_TOL * max(1.0, float(np.abs(v0).max()))):
            return dict(K=r["K"][:N], k=r["k"][:N], V=r["V"][:N], v=r["v"][:N], periods=total)
        Vf, vf = V0, v0
        count *= 2
    raise RuntimeError(f"the recursion is not periodic to 2^-60 after {total} periods")


def error(got, ref):
    return ref64.error(got, ref)


def ratios(got, rld, r64, name, idx=None):
    """``tvlqr_f64_ref.ratios`` (the budget rule) for arrays or scalars (``residual``)."""
    wrap = lambda r: [{name: np.atleast_1d(np.asarray(x[name]))} for x in r]      # noqa: E731
    return ref64.ratios({name: [np.atleast_1d(np.asarray(a)) for a in got[name]]}, wrap(rld), wrap(r64), name, idx)


def check(got, rld, r64, idx=None, fields=FIELDS, what=""):
    """The budget rule of ``tvlqr_f64_ref``: per output and instance, error against the longdouble restatement over
    max(the fp64 restatement's error, 2^-48 max(1, |ref|)); median <= 2.5, max <= 10."""
    for name in fields:
        r = ratios(got, rld, r64, name, idx)
        print(f"budget {what} {name}: median {np.median(r):.3g} max {r.max():.3g}")
        assert np.median(r) <= ref64.MEDIAN_BOUND and r.max() <= ref64.MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))

"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the double-precision gradients of the periodic infinite-horizon LQR
(``tfmpc_tvlqr_periodic_vjp_f64``): the wrap-around adjoint, for ONE instance.

``vjp``      the three sweeps and two stitches in the kernel's order, stop rule and status words, parametric in ``dtype``
             (``np.float64`` / ``np.longdouble``, whose solves go through ``tvlqr_f64_ref.inv_ld``) and in ``segments``.
             A sweep over a segment ``[t0, t1)`` is DESIGN.md 3.23's step, ``tvlqr_backward_grad_f64_ref.closed_form``, on
             the segment's slice with ``Cfin = V[t1 % N]``, ``cfin = v[t1 % N]`` and the incoming adjoint ``(X, y)`` added
             to ``gV[t0], gv[t0]``; its ``dCfin, dcfin`` are the outgoing adjoint.  ``reverse=True`` takes every product's
             k-sum in reversed order: another admissible fp64 evaluation, for the attainability test.
``brute``    independent of the solve and of the Stein algebra: the longdouble ``closed_form`` over R tiled periods with
             the default final cost and the upstream gradients on the first tile only, the tiles' gradients added, R
             doubled until the change is <= 2^-60 relative.
``references`` / ``own_forward`` / ``check``   the budget rule of DESIGN.md 3.14 / 3.23 through
             ``tvlqr_backward_grad_f64_ref``: the kernel's error against the longdouble restatement over max(the fp64
             restatement's error, the error of the fp64 restatement started from the kernel's own K, k, V, v,
             2^-48 max(1, |ref|)); median <= 2.5 and every instance <= 10.
"""

import numpy as np

import tvlqr_backward_grad_f64_ref as gr64
import tvlqr_periodic_ref as pr
import tvlqr_time_parallel_ref as tp

LD = np.longdouble
GRADS = ("dF", "df", "dC", "dc")
UPS = ("gK", "gk", "gV", "gv")
FWD = ("K", "k", "V", "v")
ST_SINGULAR, ST_NOT_PD, ST_NAN, ST_NOT_STABILISING = pr.ST_SINGULAR, pr.ST_NOT_PD, pr.ST_NAN, pr.ST_NOT_STABILISING
MAX_ITER = 40
TOL = 4.0 * float(np.finfo(np.float64).eps)
PHI_ZERO = 1e-3
BRUTE_TOL = 2.0 ** -60
BRUTE_MAX_TILES = 1 << 12


def _up64(x):
    return (x + 63) // 64 * 64


def workspace_bytes(B, n, m, N, segments):
    """The C ABI's formula (include/tfmpc_hip.h), in doubles with every array rounded up to 64 and w = B P: Psi_s, W_s,
    X_s (w n n each), s_s, y_s (w n each), Phi (B n n); for B > 1 the batch sum's records of dF, df, dC, dc (B N size
    each) and its partial sums (ceil(B / 64) N d d); then the 3 w + 2 B status words."""
    if min(B, n, m, N) <= 0 or segments < 1 or n > 32 or m > 32:
        return 0
    d = n + m
    w = B * len(tp.segment_table(N, segments)[1])
    doubles = 3 * _up64(w * n * n) + 2 * _up64(w * n) + _up64(B * n * n)
    if B > 1:
        doubles += sum(_up64(B * N * size) for size in (n * d, n, d * d, d)) + _up64(-(-B // 64) * N * d * d)
    doubles += _up64((3 * w + 2 * B + 1) // 2)
    return 8 * doubles


def _amax(X):
    return float(np.abs(X).max())


def _finite(*arrays):
    return all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in arrays)


def _sym(X):
    return X.dtype.type(0.5) * (X + X.T)


class _Sweep:
    """One instance's operands and forward in ``dtype``, and the sweep over a segment."""

    def __init__(self, F, f, C, c, fwd, ups, dtype, reverse):
        self.dtype, self.reverse = dtype, reverse
        self.F = np.asarray(F, dtype=dtype)
        self.N, self.n = self.F.shape[0], self.F.shape[1]
        self.m = self.F.shape[2] - self.n
        N, n, m = self.N, self.n, self.m
        self.f = np.asarray(f, dtype=dtype).reshape(N, n)
        self.C = np.asarray(C, dtype=dtype)
        self.c = np.asarray(c, dtype=dtype).reshape(N, n + m)
        shapes = dict(K=(N, m, n), k=(N, m), V=(N, n, n), v=(N, n))
        self.fwd = {name: np.asarray(fwd[name], dtype=dtype).reshape(shapes[name]) for name in FWD}
        ups = ups or {}
        self.ups = {g: (None if ups.get(g) is None else np.asarray(ups[g], dtype=dtype).reshape(shapes[o]))
                    for g, o in zip(UPS, FWD)}
        self.mm = gr64._mm(reverse)

    def lap(self, t0, t1, X=None, y=None):
        """``closed_form`` over [t0, t1) from the incoming adjoint: (its dict, X_out [n, n], y_out [n, 1])."""
        n, dtype = self.n, self.dtype
        sl, nx, L = slice(t0, t1), t1 % self.N, t1 - t0
        g = {name: (None if a is None else a[sl][None].copy()) for name, a in self.ups.items()}
        if X is not None:
            if g["gV"] is None:
                g["gV"] = np.zeros((1, L, n, n), dtype)
            g["gV"][0, 0] += X
        if y is not None:
            if g["gv"] is None:
                g["gv"] = np.zeros((1, L, n), dtype)
            g["gv"][0, 0] += y[:, 0]
        sub = dict({name: a[sl][None] for name, a in self.fwd.items()}, status=np.zeros(1, np.int32))
        with np.errstate(all="ignore"):
            out = gr64.closed_form(self.F[sl][None], self.f[sl][None], self.C[sl][None], self.c[sl][None],
                                   self.fwd["V"][nx][None], self.fwd["v"][nx][None], **g, dtype=dtype, fwd=sub,
                                   reverse=self.reverse)
        if out["status"][0]:
            raise pr._Flag(int(out["status"][0]))
        return out, out["dCfin"][0], out["dcfin"][0][:, None]

    def psi(self, t0, t1):
        """prod A_cl,t over the segment, A_cl,t = F_t,x + F_t,u K_t, the later step on the left."""
        n = self.n
        Ps = np.eye(n, dtype=self.dtype)
        for t in range(t0, t1):
            Ps = self.mm(self.F[t][:, :n] + self.mm(self.F[t][:, n:], self.fwd["K"][t]), Ps)
        return Ps


def vjp(F, f, C, c, fwd, ups=None, segments=1, max_iter=0, tol=0.0, dtype=np.float64, reverse=False):
    """One instance, one period: F[N,n,d], f[N,n], C[N,d,d], c[N,d], the forward's dict (K, k, V, v, status) and ``ups``
    (gK, gk, gV, gv -> array or None) -> dict(dF[N,n,d], df[N,n], dC[N,d,d], dc[N,d], X[n,n], y[n] (the wrap adjoint),
    residual, iterations, status); a flagged instance has NaN gradients and residual."""
    dtype = np.dtype(dtype).type
    F = np.asarray(F, dtype=dtype)
    N, n, d = F.shape
    max_iter = max_iter or MAX_ITER
    tol = tol or TOL
    it = 0

    def flagged(status, it=0):
        nan = lambda *shape: np.full(shape, np.nan, dtype=dtype)          # noqa: E731
        return dict(dF=nan(N, n, d), df=nan(N, n), dC=nan(N, d, d), dc=nan(N, d), X=nan(n, n), y=nan(n),
                    residual=float("nan"), iterations=it, status=int(status))

    if int(fwd["status"]):
        return flagged(fwd["status"])
    sw = _Sweep(F, f, C, c, fwd, ups, dtype, reverse)
    mm, lin = sw.mm, pr._lin(dtype)
    _, table = tp.segment_table(N, segments)
    P = len(table)
    eye = np.eye(n, dtype=dtype)
    try:
        with np.errstate(all="ignore"):
            # pass A, stitch A
            Psi = [sw.psi(t0, t1) for t0, t1 in table]
            sv = [sw.lap(t0, t1)[2] for t0, t1 in table]
            Phi, sy = Psi[0], sv[0]
            for s in range(1, P):
                Phi, sy = mm(Psi[s], Phi), mm(Psi[s], sy) + sv[s]
            ys = [lin(eye - Phi, sy)]
            for s in range(P - 1):
                ys.append(mm(Psi[s], ys[s]) + sv[s])
            if not _finite(*ys):
                raise pr._Flag(ST_NAN)
            # pass B, stitch B
            Ws = [sw.lap(t0, t1, None, ys[s])[1] for s, (t0, t1) in enumerate(table)]
            X = Ws[0]
            for s in range(1, P):
                X = mm(mm(Psi[s], X), Psi[s].T) + Ws[s]
            Fk, converged = Phi, False
            while it < max_iter:
                it += 1
                inc = mm(mm(Fk, X), Fk.T)
                X = X + inc
                Fk = mm(Fk, Fk)
                if not _finite(inc, X, Fk):
                    break
                if _amax(inc) <= tol * max(1.0, _amax(X)) and _amax(Fk) <= PHI_ZERO:
                    converged = True
                    break
            if not converged:
                raise pr._Flag(ST_NOT_STABILISING, it)
            Xs = [_sym(X)]
            for s in range(P - 1):
                Xs.append(_sym(mm(mm(Psi[s], Xs[s]), Psi[s].T)) + Ws[s])
            # pass C, finish
            out = dict(dF=np.empty((N, n, d), dtype), df=np.empty((N, n), dtype), dC=np.empty((N, d, d), dtype),
                       dc=np.empty((N, d), dtype))
            for s, (t0, t1) in enumerate(table):
                r, Xo, yo = sw.lap(t0, t1, Xs[s], ys[s])
                for name in GRADS:
                    out[name][t0:t1] = r[name][0]
            if not _finite(Xo, yo):
                raise pr._Flag(ST_NAN, it)
            residual = max(_amax(Xo - Xs[0]) / max(1.0, _amax(Xs[0])), _amax(yo - ys[0]) / max(1.0, _amax(ys[0])))
        return dict(out, X=Xs[0], y=ys[0][:, 0], residual=float(residual), iterations=it, status=0)
    except pr._Flag as flag:
        return flagged(flag.status, max(it, flag.iterations))


def upstream_of(ups, b):
    return {name: (None if (ups or {}).get(name) is None else ups[name][b]) for name in UPS}


def vjp_batch(F, f, C, c, fwds, ups, segments, dtype=np.float64, reverse=False, **kw):
    """Per instance ``vjp``: operands [B, N, ...], ``fwds`` a list of forward dicts, ``ups`` name -> [B, N, ...] or None;
    a dict of stacked arrays (gradients [B, N, ...], X, y, residual, iterations, status)."""
    rs = [vjp(F[b], f[b], C[b], c[b], fwds[b], upstream_of(ups, b), segments, dtype=dtype, reverse=reverse, **kw)
          for b in range(F.shape[0])]
    out = {name: np.stack([r[name] for r in rs]) for name in GRADS + ("X", "y")}
    out.update(residual=np.array([r["residual"] for r in rs]), iterations=np.array([r["iterations"] for r in rs]),
               status=np.array([r["status"] for r in rs], np.int32), dCfin=None, dcfin=None)
    return out


def upstream(n, m, N, B, seed, names=UPS):
    """Upstream gradients of unit scale for ``names`` (the others None); gV is a general matrix: the kernel symmetrises."""
    rng = np.random.default_rng(seed)
    shapes = dict(gK=(B, N, m, n), gk=(B, N, m), gV=(B, N, n, n), gv=(B, N, n))
    full = {name: rng.normal(size=shapes[name]) for name in UPS}
    return {name: (full[name] if name in names else None) for name in UPS}


def brute(F, f, C, c, ups, max_tiles=BRUTE_MAX_TILES):
    """Batched: the longdouble ``closed_form`` (from its own longdouble recursion) over R tiled periods, the default final
    cost, the upstream gradients on the first tile, the tiles' gradients added; R doubled until no gradient changes by
    more than 2^-60 relative to max(1, |gradient|).  dict(dF, df, dC, dc [B, N, ...], tiles)."""
    F, f, C, c = (np.asarray(a, dtype=LD) for a in (F, f, C, c))
    B, N = F.shape[:2]
    prev, R = None, 2
    while R <= max_tiles:
        tile = lambda a: np.concatenate([a] * R, axis=1)                  # noqa: E731
        pad = lambda g: None if g is None else np.concatenate(            # noqa: E731
            [np.asarray(g, dtype=LD), np.zeros((B, (R - 1) * N) + np.shape(g)[2:], LD)], axis=1)
        r = gr64.closed_form(tile(F), tile(f), tile(C), tile(c), **{name: pad((ups or {}).get(name)) for name in UPS},
                             dtype=LD)
        assert not r["status"].any()
        cur = {name: r[name].reshape(B, R, N, *r[name].shape[2:]).sum(axis=1) for name in GRADS}
        if prev is not None and all(_amax(cur[name] - prev[name]) <= BRUTE_TOL * max(1.0, _amax(cur[name]))
                                    for name in GRADS):
            return dict(cur, tiles=R)
        prev, R = cur, 2 * R
    raise RuntimeError(f"the tiled gradients have not settled to 2^-60 at {R // 2} tiles")


def references(F, f, C, c, ups, segments, fwd_ld, fwd_64):
    """(longdouble restatement, fp64 restatement end to end, the same again) in ``tvlqr_backward_grad_f64_ref``'s
    ``refs`` form (its third entry is fp64 autograd there; the periodic rule has no such term)."""
    rld = vjp_batch(F, f, C, c, fwd_ld, ups, segments, dtype=LD)
    r64 = vjp_batch(F, f, C, c, fwd_64, ups, segments)
    assert not rld["status"].any() and not r64["status"].any()
    return rld, r64, r64


def own_forward(F, f, C, c, ups, segments, got_fwd):
    """The fp64 restatement started from the kernel's own K, k, V, v (``got_fwd``: name -> [B, N, ...] numpy)."""
    fwds = [dict({name: got_fwd[name][b] for name in FWD}, status=0) for b in range(F.shape[0])]
    out = vjp_batch(F, f, C, c, fwds, ups, segments)
    assert not out["status"].any()
    return out


def check(got, refs, own=None, names=GRADS, what=""):
    return gr64.check(got, refs, own, names=names, what=what)


def check_summed(got, refs, name, own=None, batch=False, time=False, what=""):
    return gr64.check_summed(got, refs, name, own, batch=batch, time=time, what=what)

"""TEST INFRASTRUCTURE ONLY -- the control-limited Newton sweep of ``tfmpc_tvlqr_box_solve_f32`` in
numpy, one instance at a time, with ``dtype`` a parameter.  The fp64 instance shows the algorithm exact (it meets
``lqr_box_grad_ref.solve_box``); the fp32 instance is the error budget of the GPU tests.

The restatement follows the kernel decision for decision: clipped start, backward sweep in delta form with a projected-
Newton box-QP per step (warm start 0, free block by elimination without pivoting, Armijo backtracking on the projection
arc with the decrease computed as ``g.d + 1/2 d^T Q d``), Schur-form value update, the stop rule on the step norm, eleven
step sizes, the trusted step, the converged sweep's step applied in full.  Only the order of the floating-point sums differs (numpy's products against the kernel's
matrix-core and fused multiply-add chains).
"""

import functools

import numpy as np

ST_NOT_PD, ST_NAN, ST_QP_MAXITER, ST_MAX_ATTEMPTS = 2, 4, 8, 16
REASON_CONVERGED, REASON_NO_DECREASE, REASON_PASS_CAP, REASON_FAILED = 0, 1, 2, 3
QP_ITERATIONS, QP_BACKTRACKS, ALPHAS, TRUSTED_IN_A_ROW = 100, 21, 11, 3
ARMIJO, TRUST_RATIO, DEFAULT_TOL, DEFAULT_PASSES = 1e-4, 1e-6, 4e-6, 100
F64_TOL = 1e-12            # the stop rule the fp64 instance is run with (4e-6 is sized for fp32 rounding)


def eliminate(A, rhs, dt):
    """Gauss-Jordan without pivoting on [A | rhs]; -> (A^-1 rhs, a pivot was not positive)."""
    m = A.shape[0]
    aug = np.concatenate([A, rhs], 1).astype(dt)
    bad = False
    for p in range(m):
        pv = aug[p, p]
        if not pv > 0:
            bad = True
        with np.errstate(all="ignore"):
            pr = aug[p] / pv
            fac = aug[:, p].copy()
            aug = aug - np.outer(fac, pr).astype(dt)
        aug[p] = pr
    return aug[:, m:], bad


def box_qp(H, q, G, lo, hi, dt):
    """min 1/2 x^T H x + q^T x, lo <= x <= hi from x = 0; G = Q_ux rides along in the elimination.
    -> (x, K [m, n] with held rows exactly 0, held [m] bool, status bits)."""
    m, n = G.shape
    x = np.zeros(m, dt)
    held = prev = np.zeros(m, bool)
    full = False
    sol = np.zeros((m, 1 + n), dt)
    status = ST_QP_MAXITER
    for it in range(QP_ITERATIONS):
        g = (q + H @ x).astype(dt)
        held = ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))
        if it > 0 and np.array_equal(held, prev) and full:
            status = 0
            break
        fr = ~held
        A = np.where(np.outer(fr, fr), H, np.eye(m, dtype=dt))
        rhs = np.where(fr[:, None], np.concatenate([g[:, None], G], 1), 0).astype(dt)
        sol, bad = eliminate(A, rhs, dt)
        if bad:
            return x, np.zeros((m, n), dt), held, ST_NOT_PD
        if held.all():
            status = 0
            break
        step = np.where(fr, -sol[:, 0], 0).astype(dt)
        alpha, accepted = dt(1), False
        for _ in range(QP_BACKTRACKS):
            xc = np.clip((x + alpha * step).astype(dt), lo, hi)
            dd = (xc - x).astype(dt)
            gd = dt(g @ dd)
            df = dt(gd + dt(0.5) * dt(dd @ (H @ dd).astype(dt)))
            if df < 0 and df <= dt(ARMIJO) * gd:
                accepted = True
                break
            alpha = dt(alpha * dt(0.5))
        if not accepted:
            status = 0
            break
        full = bool(alpha == 1 and np.array_equal(xc, (x + step).astype(dt)))
        x, prev = xc, held
    K = np.where(held[:, None], dt(0), -sol[:, 1:]).astype(dt)
    return x, K, held, status


def rollout(F, f, C, c, Cf, cf, x0, dt, u_of):
    """u_t = u_of(t, x_t); -> states, actions, costs[T+1], J (summed in time order)."""
    T, n, d = F.shape
    xs, us, cs = np.zeros((T + 1, n), dt), np.zeros((T, d - n), dt), np.zeros(T + 1, dt)
    xs[0] = x0
    J = dt(0)
    for t in range(T):
        us[t] = u_of(t, xs[t])
        z = np.concatenate([xs[t], us[t]])
        cs[t] = dt(z @ (dt(0.5) * (C[t] @ z) + c[t]).astype(dt))
        J = dt(J + cs[t])
        xs[t + 1] = (F[t] @ z + f[t]).astype(dt)
    cs[T] = dt(xs[T] @ (dt(0.5) * (Cf @ xs[T]) + cf).astype(dt))
    return xs, us, cs, dt(J + cs[T])


def solve(F, f, C, c, x0, low, high, Cfin=None, cfin=None, u_init=None, max_iter=0, tol=0.0, dtype=np.float32):
    """F[T,n,d] f[T,n] C[T,d,d] c[T,d] x0[n]; low, high broadcastable to [T,m].  -> dict: states, actions, costs,
    iterations (sweeps run), status, reason, clamped [T,m] (the last sweep's held sets; all False without a sweep)."""
    dt = np.dtype(dtype).type
    F, f, C, c, x0 = (np.asarray(a).astype(dt) for a in (F, f, C, c, x0))
    T, n, d = F.shape
    m = d - n
    with np.errstate(invalid="ignore"):
        low = np.broadcast_to(np.asarray(low).astype(dt), (T, m))
        high = np.broadcast_to(np.asarray(high).astype(dt), (T, m))
    Cf = (C[T - 1][:n, :n] if Cfin is None else np.asarray(Cfin)).astype(dt)
    cf = (c[T - 1][:n] if cfin is None else np.asarray(cfin)).astype(dt)
    max_iter = max_iter or DEFAULT_PASSES
    tol = dt(tol or (DEFAULT_TOL if dt == np.float32 else F64_TOL))
    u0 = np.zeros((T, m), dt) if u_init is None else np.asarray(u_init).astype(dt)
    xs, us, cs, J = rollout(F, f, C, c, Cf, cf, x0, dt, lambda t, x: np.clip(u0[t], low[t], high[t]))
    clamped = np.zeros((T, m), bool)
    status, reason, sweeps, trusted = 0, REASON_CONVERGED, 0, 0
    if np.isnan(J):
        status, reason = ST_NAN, REASON_FAILED
    elif (low != high).any():
        reason = REASON_PASS_CAP
        for _ in range(max_iter):
            # ---- backward sweep
            V, v = Cf.copy(), (Cf @ xs[T] + cf).astype(dt)
            K, k = np.zeros((T, m, n), dt), np.zeros((T, m), dt)
            dV, status = dt(0), 0
            for t in range(T - 1, -1, -1):
                z = np.concatenate([xs[t], us[t]])
                Q = (C[t] + (F[t].T @ V).astype(dt) @ F[t]).astype(dt)
                q = (C[t] @ z + c[t] + F[t].T @ v).astype(dt)
                with np.errstate(invalid="ignore"):
                    lo, hi = (low[t] - us[t]).astype(dt), (high[t] - us[t]).astype(dt)
                k[t], K[t], clamped[t], st = box_qp(Q[n:, n:], q[n:], Q[n:, :n], lo, hi, dt)
                status |= st
                if st & ST_NOT_PD:
                    break
                Vn = (Q[:n, :n] + Q[:n, n:] @ K[t]).astype(dt)
                V = (dt(0.5) * (Vn + Vn.T)).astype(dt)
                v = (q[:n] + Q[:n, n:] @ k[t]).astype(dt)
                dV = dt(dV + dt(k[t] @ (dt(0.5) * (Q[n:, n:] @ k[t]) + q[n:]).astype(dt)))
            sweeps += 1
            if np.isnan(dV):
                status |= ST_NAN
            if status & (ST_NOT_PD | ST_NAN):
                reason = REASON_FAILED
                break
            if np.abs(k).max() <= tol * max(dt(1), np.abs(us).max()):
                reason = REASON_CONVERGED
                if np.abs(k).max() > 0:            # the converged sweep's step is applied in full, untested
                    xs, us, cs, J = rollout(F, f, C, c, Cf, cf, x0, dt, lambda t, x: np.clip(
                        (us[t] + k[t] + K[t] @ (x - xs[t])).astype(dt), low[t], high[t]))
                    if np.isnan(J):
                        status, reason = status | ST_NAN, REASON_FAILED
                break
            # ---- line search
            trust = bool(-dV <= dt(TRUST_RATIO) * max(dt(1), abs(J))) and trusted < TRUSTED_IN_A_ROW
            trusted = trusted + 1 if trust else 0
            alpha, accepted = dt(1), False
            for _ls in range(ALPHAS):
                def u_of(t, x, alpha=alpha):
                    return np.clip((us[t] + alpha * k[t] + K[t] @ (x - xs[t])).astype(dt), low[t], high[t])
                xn, un, cn, Jn = rollout(F, f, C, c, Cf, cf, x0, dt, u_of)
                if trust or Jn < J:
                    accepted = True
                    break
                alpha = dt(alpha * dt(0.5))
            if not accepted:
                reason = REASON_NO_DECREASE
                break
            xs, us, cs, J = xn, un, cn, Jn
            if np.isnan(J):
                status, reason = status | ST_NAN, REASON_FAILED
                break
        if reason == REASON_PASS_CAP:
            status |= ST_MAX_ATTEMPTS
    if status & (ST_NOT_PD | ST_NAN):
        xs, us, cs = (np.full_like(a, np.nan) for a in (xs, us, cs))
    return dict(states=xs, actions=us, costs=cs, iterations=sweeps, status=status, reason=reason, clamped=clamped)


def solve_batch(F, f, C, c, x0, low, high, Cfin=None, cfin=None, u_init=None, dtype=np.float32, **kw):
    """Batched operands [B, ...] (low / high broadcastable to [B, T, m]) -> dict of stacked arrays."""
    B, T, n, d = F.shape
    lo = np.broadcast_to(np.asarray(low, dtype=np.float64), (B, T, d - n))
    hi = np.broadcast_to(np.asarray(high, dtype=np.float64), (B, T, d - n))
    outs = [solve(F[b], f[b], C[b], c[b], x0[b], lo[b], hi[b], None if Cfin is None else Cfin[b],
                  None if cfin is None else cfin[b], None if u_init is None else u_init[b], dtype=dtype, **kw) for b in range(B)]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}


def held_from_actions(actions, low, high):
    """The VJP's held-set rule: a control is held iff it carries a bound's bits."""
    a = np.asarray(actions, dtype=np.float32)
    return (a == np.asarray(low, dtype=np.float32)) | (a == np.asarray(high, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def case(n, m, T, B, final=False, width=1.0):
    """``lqr_box_grad_ref.tv_case`` with the fp32 restatement's solution next to the fp64 optimum, computed once per
    process: (operands, optimum, fp32 restatement).  Read-only."""
    import lqr_box_grad_ref as bref
    ops, sol = bref.tv_case(n, m, T, B, final=final, width=width)
    r32 = solve_batch(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["low"], ops["high"], ops["Cfin"], ops["cfin"])
    return ops, sol, r32


def instance_error(got, ref):
    """Per instance: max |got - ref| over everything behind the batch axis."""
    B = ref.shape[0]
    return np.abs(np.asarray(got, dtype=np.float64).reshape(B, -1) - ref.reshape(B, -1)).max(1)


def budget_ratios(got, r32, ref):
    """The project's budget rule per instance: the error of ``got`` against the fp64 ``ref`` over
    max(the fp32 restatement's error, 1e-6 max(1, |ref|_inf))."""
    B = ref.shape[0]
    floor = 1e-6 * np.maximum(1.0, np.abs(ref.reshape(B, -1)).max(1))
    return instance_error(got, ref) / np.maximum(instance_error(r32, ref), floor)

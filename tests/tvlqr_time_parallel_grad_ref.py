"""TEST INFRASTRUCTURE ONLY -- the segmented adjoint of the time-parallel double-precision TV-LQR
(``tfmpc_tvlqr_vjp_time_parallel_f64``) restated in numpy for ONE instance, generic in dtype and in
``segments``, in the kernels' phases.

The adjoint problem of ``tvlqr_grad_f64_ref.closed_form`` has the forward's ``F, C, C_fin`` and the linear terms
``c~_t = g_t``, ``c~_fin = g_T``, ``f~ = 0``, ``x~0 = 0``: it has the forward's gains ``K_t`` and value function ``V_t``
(``V_T = C_fin``), which are PASSED IN, and only its vector part is computed.  With ``L_t = [I; K_t]``,
``Phi_t = F_t L_t``, ``B_t = F_t[:, n:]``:

    backward   v~_T = g_T,  v~_t = L_t' g_t + Phi_t' v~_{t+1}
    per step   Q_uu,t = C_t[n:, n:] + B_t' V_{t+1} B_t,  k~_t = -Q_uu,t^-1 (g_t[n:] + B_t' v~_{t+1})
    forward    dx_0 = 0,  du_t = K_t dx_t + k~_t,  dx_{t+1} = Phi_t dx_t + B_t k~_t

A segment ``[s, e)`` condenses to ``M = Phi_{e-1} ... Phi_s`` and one offset per direction (``v~_s = M' v~_e + beta``,
``dx_e = M dx_s + gamma``); the boundaries are stitched with P matrix-vector products and the segments expanded.
Costates, outer products and the default final cost are ``tvlqr_grad_f64_ref.closed_form``'s, unchanged.
"""

import numpy as np

import tvlqr_f64_ref as ref64
import tvlqr_grad_f64_ref as g64
import tvlqr_ref
from tvlqr_time_parallel_ref import segment_table

LD = np.longdouble


def workspace_bytes(B, n, m, T, segments):
    """The C ABI's formula for P > 1 (include/tfmpc_hip.h); P == 1 is ``tfmpc_tvlqr_vjp_workspace_bytes_f64``'s."""
    if min(B, n, m, T) <= 0 or segments < 1:
        return 0
    up = lambda x: (x + 63) // 64 * 64                                                # noqa: E731
    d, chunks, P = n + m, (B + 255) // 256, len(segment_table(T, segments)[1])
    doubles = (up(B * T * d) + 2 * up(B * n) + up(B * n * n) + up(B * (T + 1) * n) + up(B * T * m) + up(B * (T + 1))
               + up(B * T * n * n) + up(B * T * n) + up(B * T * m) + up(B * T * n * m) + 2 * up(B * T * n) + up(2 * B * T * n)
               + up(chunks * T * (n * d + n + d * d + d)) + up(B * P * n * n) + 4 * up(B * P * n) + up((B * T + 1) // 2))
    return 8 * doubles


def adjoint(F, C, Cf, K, V, g, gT, segments, dtype=np.float64):
    """F[T,n,d], C[T,d,d], Cf[n,n], the forward's K[T,m,n], V[T,n,n], the fold's g[T,d], gT[n] ->
    (dx[T+1,n], du[T,m], v~[T+1,n]) of the adjoint problem, by the segmented recursions."""
    F, C, Cf, K, V, g, gT = (np.asarray(a, dtype=dtype) for a in (F, C, Cf, K, V, g, gT))
    T, n, d = F.shape
    m = d - n
    solve = (lambda A, rhs: ref64.inv_ld(A) @ rhs) if dtype == LD else np.linalg.solve
    _, table = segment_table(T, segments)
    P = len(table)
    # per step
    Phi, a, r, E = [None] * T, [None] * T, [None] * T, [None] * T
    for t in range(T):
        Bt = F[t][:, n:]
        Phi[t] = F[t][:, :n] + Bt @ K[t]
        a[t] = g[t][:n] + K[t].T @ g[t][n:]
        Vn = Cf if t == T - 1 else V[t + 1]
        Quu = C[t][n:, n:] + Bt.T @ (Vn @ Bt)
        sol = solve(Quu, np.concatenate([g[t][n:, None], Bt.T], axis=1))
        r[t], E[t] = sol[:, 0], sol[:, 1:]
    # condense
    M, beta = [None] * P, [None] * P
    for i, (t0, t1) in enumerate(table):
        M[i], beta[i] = Phi[t1 - 1], a[t1 - 1]
        for t in reversed(range(t0, t1 - 1)):
            M[i], beta[i] = M[i] @ Phi[t], a[t] + Phi[t].T @ beta[i]
    # backward stitch and expand
    vend = [None] * P
    vv = gT
    for i in reversed(range(P)):
        vend[i] = vv
        vv = beta[i] + M[i].T @ vv
    vt = np.zeros((T + 1, n), dtype=dtype)
    vt[T] = gT
    kt, w, gamma = np.zeros((T, m), dtype=dtype), np.zeros((T, n), dtype=dtype), [None] * P
    for i, (t0, t1) in enumerate(table):
        vv = vend[i]
        for t in reversed(range(t0, t1)):
            kt[t] = -(r[t] + E[t] @ vv)
            vv = a[t] + Phi[t].T @ vv
            vt[t] = vv
            w[t] = F[t][:, n:] @ kt[t]
        gm = np.zeros(n, dtype=dtype)
        for t in range(t0, t1):
            gm = w[t] + Phi[t] @ gm
        gamma[i] = gm
    # forward stitch and expand
    xstart = [np.zeros(n, dtype=dtype)]
    for i in range(P - 1):
        xstart.append(gamma[i] + M[i] @ xstart[i])
    dx, du = np.zeros((T + 1, n), dtype=dtype), np.zeros((T, m), dtype=dtype)
    for i, (t0, t1) in enumerate(table):
        x = xstart[i]
        for t in range(t0, t1):
            dx[t] = x
            du[t] = kt[t] + K[t] @ x
            x = w[t] + Phi[t] @ x
        if t1 == T:
            dx[T] = x
    return dx, du, vt


def closed_form(F, f, C, c, x0, Cfin, cfin, gx, gu, gcost, fwd, segments, dtype=np.float64):
    """``tvlqr_grad_f64_ref.closed_form`` for ONE instance with the adjoint solve replaced by ``adjoint``.  ``fwd``: the
    forward solve's dict (``states, actions, K, V, v``), which is used as given, cast to ``dtype``."""
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
    xs, us, K, V, v = (np.asarray(fwd[k], dtype=dtype) for k in ("states", "actions", "K", "V", "v"))
    z = np.concatenate([xs[:T], us], axis=-1)
    xT = xs[T]
    r = np.stack([C[t] @ z[t] for t in range(T)]) + c
    rT = Cf @ xT + cf
    g = np.concatenate([gx[:T], gu], axis=-1) + gcost[:T, None] * r                  # fold
    gT = gx[T] + gcost[T] * rT
    dxs, dus, vt = adjoint(F, C, Cf, K, V, g, gT, segments, dtype)
    dz = np.concatenate([dxs[:T], dus], axis=-1)
    dxT = dxs[T]
    lam1, dlam1 = [None] * T, [None] * T                                             # costates of step t + 1
    for t in range(T):
        last = t == T - 1
        Vn = Cf if last else V[t + 1]
        lam1[t] = Vn @ xs[t + 1] + (cf if last else v[t + 1])
        dlam1[t] = Vn @ dxs[t + 1] + vt[t + 1]
    lam1, dlam1 = np.stack(lam1), np.stack(dlam1)
    outer = lambda a, b: a[..., :, None] * b[..., None, :]                           # noqa: E731
    half = dtype(0.5)
    out = dict(F=outer(dlam1, z) + outer(lam1, dz), f=dlam1,
               C=half * (outer(dz, z) + outer(z, dz)) + half * gcost[:T, None, None] * outer(z, z),
               c=dz + gcost[:T, None] * z, x0=vt[0])
    dCf = half * (outer(dxT, xT) + outer(xT, dxT)) + half * gcost[T] * outer(xT, xT)
    dcf = dxT + gcost[T] * xT
    if default:
        out["C"][T - 1][:n, :n] += dCf
        out["c"][T - 1][:n] += dcf
    else:
        out.update(Cfin=dCf, cfin=dcf)
    return out


def forward_of(kind, F, f, C, c, x0, Cfin, cfin, segments):
    """The forward solve whose ``K, V, v`` the restatement takes: ``"ld"`` the 80-bit recursion, ``"sequential"`` the fp64
    sequential restatement, ``"time_parallel"`` the fp64 time-parallel restatement with the same ``segments``."""
    if kind == "ld":
        return ref64.solve_ld(F, f, C, c, x0, Cfin, cfin)
    if kind == "sequential":
        return tvlqr_ref.solve(F, f, C, c, x0, Cfin, cfin, dtype=np.float64)
    import tvlqr_time_parallel_ref as tp
    return tp.solve(F, f, C, c, x0, segments, Cfin, cfin)


def grads(F, f, C, c, x0, Cfin, cfin, gx, gu, gcost, segments, dtype=np.float64, forward="sequential"):
    """``closed_form`` per instance of a batch (operands [B, T, ...], Cfin / cfin [B, ...] or None) -> dict of [B, ...]."""
    pick = lambda a, b: None if a is None else a[b]                                  # noqa: E731
    per = []
    for b in range(F.shape[0]):
        fwd = forward_of("ld" if dtype == LD else forward, F[b], f[b], C[b], c[b], x0[b], pick(Cfin, b), pick(cfin, b), segments)
        per.append(closed_form(F[b], f[b], C[b], c[b], x0[b], pick(Cfin, b), pick(cfin, b), pick(gx, b), pick(gu, b),
                               pick(gcost, b), fwd, segments, dtype))
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def widened(refs, own):
    """``tvlqr_grad_f64_ref.references``' triple with the budget's fp64 terms joined by this restatement's fp64 error
    (DESIGN.md 3.19's precedent): ``term_budgets`` takes the max of the two fp64 entries' errors, so the larger of the
    value-function form's and ``own``'s error, element by element against 80-bit, stands in the first."""
    rld, r64, auto = refs
    worse = {k: np.where(np.abs(own[k].astype(LD) - rld[k]) > np.abs(r64[k].astype(LD) - rld[k]), own[k], r64[k]) for k in rld}
    return rld, worse, auto


__all__ = ["adjoint", "closed_form", "grads", "widened", "workspace_bytes", "segment_table", "g64"]

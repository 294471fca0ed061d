"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the time-varying LQR (``tfmpc_tvlqr_*_f32``,
``tfmpc.solvers.tvlqr.TimeVaryingLQR``) and the seeded workloads of its tests and of ``tools/tvlqr_rate.py``.

The recursion is ``oracle/lqr_ref.py``'s (the reference's ``lqr.py:59-166``, same operation order) with
``F, f, C, c`` replaced by ``F_t, f_t, C_t, c_t`` at step t, and the final cost ``C_fin, c_fin`` (default
``C_{T-1}[:n,:n]``, ``c_{T-1}[:n]``) as the terminal value function.  ``dtype=np.float64`` is the oracle of record;
``dtype=np.float32`` gives the fp32 error budget.  ``kkt_solve`` poses the same problem as one dense equality-constrained
QP, an independent check of the restatement.
"""

import numpy as np

from oracle import lqr_ref


def backward(F, f, C, c, Cfin=None, cfin=None, dtype=np.float64):
    """F[T,n,d], f[T,n(,1)], C[T,d,d], c[T,d(,1)] -> (policy, value_fn) as ``lqr_ref.backward``."""
    F = np.asarray(F, dtype=dtype)
    T, n = F.shape[0], F.shape[1]
    f = np.asarray(f, dtype=dtype).reshape(T, n, 1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(T, -1, 1)
    if Cfin is None:
        V, v = C[T - 1][:n, :n], c[T - 1][:n]
    else:
        V, v = np.asarray(Cfin, dtype=dtype), np.asarray(cfin, dtype=dtype).reshape(n, 1)
    const = np.zeros((1, 1), dtype=dtype)
    half = dtype(0.5)
    policy, value_fn = [], []
    for t in reversed(range(T)):
        Ft, ft, Ct, ct = F[t], f[t], C[t], c[t]
        Ft_V = Ft.T @ V
        Q = Ct + Ft_V @ Ft
        q = ct + Ft_V @ ft + Ft.T @ v
        Q_uu, Q_ux, q_u = Q[n:, n:], Q[n:, :n], q[n:]
        inv_Q_uu = np.linalg.inv(Q_uu)
        K = -(inv_Q_uu @ Q_ux)
        k = -(inv_Q_uu @ q_u)
        Q_xx, Q_xu, q_x = Q[:n, :n], Q[:n, n:], q[:n]
        Kt_Quu = K.T @ Q_uu
        V_new = Q_xx + Q_xu @ K + K.T @ Q_ux + Kt_Quu @ K
        v_new = q_x + Q_xu @ k + K.T @ q_u + Kt_Quu @ k
        V_f = V @ ft
        const = const + (half * (k.T @ (Q_uu @ k)) + k.T @ q_u + (half * (ft.T @ V_f) + ft.T @ v))
        V, v = V_new, v_new
        policy.append((K, k))
        value_fn.append((V, v, const))
    return list(reversed(policy)), list(reversed(value_fn))


def forward(F, f, C, c, policy, x0, Cfin=None, cfin=None, dtype=np.float64):
    """-> states[T+1,n,1], actions[T,m,1], costs[T+1,1,1]"""
    F = np.asarray(F, dtype=dtype)
    T, n = F.shape[0], F.shape[1]
    f = np.asarray(f, dtype=dtype).reshape(T, n, 1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(T, -1, 1)
    x = np.asarray(x0, dtype=dtype).reshape(-1, 1)
    states, actions, costs = [x], [], []
    for t in range(T):
        K, k = policy[t]
        u = K @ x + k
        nx = lqr_ref.transition(F[t], f[t], x, u)
        costs.append(lqr_ref.cost(C[t], c[t], x, u))
        x = nx
        states.append(x)
        actions.append(u)
    if Cfin is None:
        costs.append(lqr_ref.final_cost(C[T - 1], c[T - 1], x))
    else:
        Cf, cf = np.asarray(Cfin, dtype=dtype), np.asarray(cfin, dtype=dtype).reshape(n, 1)
        costs.append(0.5 * (x.T @ Cf) @ x + x.T @ cf)
    return np.stack(states), np.stack(actions), np.stack(costs)


def solve(F, f, C, c, x0, Cfin=None, cfin=None, dtype=np.float64):
    """-> dict(states[T+1,n], actions[T,m], costs[T+1], K[T,m,n], k[T,m], V[T,n,n], v[T,n], const[T])"""
    policy, value_fn = backward(F, f, C, c, Cfin, cfin, dtype=dtype)
    x, u, cs = forward(F, f, C, c, policy, x0, Cfin, cfin, dtype=dtype)
    return dict(states=x[..., 0], actions=u[..., 0], costs=cs.reshape(-1),
                K=np.stack([p[0] for p in policy]), k=np.stack([p[1][:, 0] for p in policy]),
                V=np.stack([w[0] for w in value_fn]), v=np.stack([w[1][:, 0] for w in value_fn]),
                const=np.array([w[2][0, 0] for w in value_fn]))


def kkt_solve(F, f, C, c, x0, Cfin=None, cfin=None):
    """The problem as ONE dense equality-constrained QP in fp64 (variables x_1..x_T, u_0..u_{T-1}; x_0 fixed), solved
    through its KKT system -> (states[T+1,n], actions[T,m], total cost)."""
    F = np.asarray(F, dtype=np.float64)
    T, n, d = F.shape
    m = d - n
    f = np.asarray(f, dtype=np.float64).reshape(T, n)
    C = np.asarray(C, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64).reshape(T, d)
    x0 = np.asarray(x0, dtype=np.float64).reshape(n)
    if Cfin is None:
        Cfin, cfin = C[T - 1][:n, :n], c[T - 1][:n]
    Cfin, cfin = np.asarray(Cfin, dtype=np.float64), np.asarray(cfin, dtype=np.float64).reshape(n)
    # full vector w = [x_0 .. x_T, u_0 .. u_{T-1}]; x_0 is pinned by an equality row
    nx, nw = (T + 1) * n, (T + 1) * n + T * m
    xi = lambda t: slice(t * n, (t + 1) * n)                   # noqa: E731
    ui = lambda t: slice(nx + t * m, nx + (t + 1) * m)          # noqa: E731
    H, g = np.zeros((nw, nw)), np.zeros(nw)
    for t in range(T):
        idx = np.r_[np.arange(nw)[xi(t)], np.arange(nw)[ui(t)]]
        H[np.ix_(idx, idx)] += C[t]
        g[idx] += c[t]
    H[xi(T), xi(T)] += Cfin
    g[xi(T)] += cfin
    A, r = np.zeros(((T + 1) * n, nw)), np.zeros((T + 1) * n)
    A[:n, xi(0)] = np.eye(n)
    r[:n] = x0
    for t in range(T):
        rows = slice((t + 1) * n, (t + 2) * n)
        A[rows, xi(t + 1)] = np.eye(n)
        A[rows, xi(t)] -= F[t][:, :n]
        A[rows, ui(t)] -= F[t][:, n:]
        r[rows] = f[t]
    kkt = np.block([[H, A.T], [A, np.zeros((A.shape[0], A.shape[0]))]])
    sol = np.linalg.solve(kkt, np.r_[-g, r])
    w = sol[:nw]
    return w[:nx].reshape(T + 1, n), w[nx:].reshape(T, m), 0.5 * w @ H @ w + g @ w


# ---- seeded workloads ---------------------------------------------------------------------------------------------------

def make_models(n, m, T, count, seed=0, f_scale=1.0):
    """``count`` independent time-varying models, every step drawn as ``oracle.lqr_ref.make_lqr`` draws an LQR problem
    (global numpy RNG seeded with ``seed``; sklearn's ``make_spd_matrix`` for C), then cast to fp32 as the reference does.
    F is scaled by 1 / sqrt(n) (spectral radius ~ 1) so that fp32 survives long horizons; C is symmetrised exactly.
    Returns fp32 arrays F[count,T,n,d], f[count,T,n], C[count,T,d,d], c[count,T,d]."""
    np.random.seed(seed)
    d = n + m
    F = np.empty((count, T, n, d), np.float32)
    f = np.empty((count, T, n), np.float32)
    C = np.empty((count, T, d, d), np.float32)
    c = np.empty((count, T, d), np.float32)
    for b in range(count):
        for t in range(T):
            Fs, fs, Cs, cs = lqr_ref.make_lqr(n, m)
            F[b, t] = Fs / np.sqrt(n)
            f[b, t] = f_scale * fs[:, 0]
            C[b, t] = Cs
            c[b, t] = cs[:, 0]
    C = 0.5 * (C + np.swapaxes(C, -1, -2))
    return F, f, C.astype(np.float32), c


def make_final(n, count, seed=1):
    """Explicit final costs: Cfin[count,n,n] symmetric positive definite, cfin[count,n] (fp32)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(count, n, n))
    Cf = A @ np.swapaxes(A, -1, -2) / n + np.eye(n)
    Cf = (0.5 * (Cf + np.swapaxes(Cf, -1, -2))).astype(np.float32)
    return Cf, rng.normal(size=(count, n)).astype(np.float32)


def make_x0(n, count, seed=2):
    return np.random.default_rng(seed).normal(size=(count, n)).astype(np.float32)

"""TEST INFRASTRUCTURE ONLY -- restatements one precision up for the double-precision time-varying LQR
(``tfmpc_tvlqr_*_f64``, ``TimeVaryingLQR(dtype=torch.float64)``), and the budget rule of its tests.

``solve_ld``     ``tvlqr_ref``'s recursion and rollout, same operation order, in ``np.longdouble`` (80-bit on x86-64): the
                 reference the fp64 results are measured against.  numpy has no ``linalg`` for that type, so the inverse of
                 ``Q_uu`` is a Gauss-Jordan elimination with partial pivoting written here.
``solve_schur``  fp64 numpy in the KERNEL's order (factor ``Q_uu`` once for ``K`` and ``k``, ``V' = Q_xx + Q_xu K``,
                 ``V'`` symmetrised): shows on the host that the budget is attainable by that formulation.
``make_unscaled``  ``tvlqr_ref.make_models`` without the ``1 / sqrt(n)`` on F: ``make_lqr``'s own spectrum.
``ratios`` / ``check``  the budget rule: per output and instance, error against ``solve_ld`` over
                 max(error of ``tvlqr_ref.solve(dtype=float64)`` against ``solve_ld``, 2^-48 max(1, |ref|_inf));
                 median over instances <= 2.5 and every instance <= 10.
"""

import numpy as np

import tvlqr_ref
from oracle import lqr_ref

LD = np.longdouble
FIELDS = ("states", "actions", "costs", "K", "k", "V", "v", "const")
FLOOR = 2.0 ** -48
MEDIAN_BOUND, MAX_BOUND = 2.5, 10.0


def inv_ld(A):
    """Inverse of a square longdouble matrix: Gauss-Jordan with partial pivoting."""
    A = np.array(A, dtype=LD)
    r = A.shape[0]
    aug = np.concatenate([A, np.eye(r, dtype=LD)], axis=1)
    for p in range(r):
        piv = p + int(np.argmax(np.abs(aug[p:, p])))
        if piv != p:
            aug[[p, piv]] = aug[[piv, p]]
        aug[p] = aug[p] / aug[p, p]
        for i in range(r):
            if i != p:
                aug[i] = aug[i] - aug[i, p] * aug[p]
    return aug[:, r:]


def _operands(F, f, C, c, x0, Cfin, cfin, dtype):
    F = np.asarray(F, dtype=dtype)
    T, n = F.shape[0], F.shape[1]
    f = np.asarray(f, dtype=dtype).reshape(T, n, 1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(T, -1, 1)
    x = np.asarray(x0, dtype=dtype).reshape(-1, 1)
    if Cfin is None:
        Cf, cf = C[T - 1][:n, :n], c[T - 1][:n]
    else:
        Cf, cf = np.asarray(Cfin, dtype=dtype), np.asarray(cfin, dtype=dtype).reshape(n, 1)
    return F, f, C, c, x, Cf, cf, T, n


def _rollout(F, f, C, c, x, Cf, cf, policy, T, half):
    states, actions, costs = [x], [], []
    for t in range(T):
        K, k = policy[t]
        u = K @ x + k
        nx = lqr_ref.transition(F[t], f[t], x, u)
        z = np.concatenate([x, u], axis=0)
        costs.append(half * (z.T @ C[t]) @ z + z.T @ c[t])
        x = nx
        states.append(x)
        actions.append(u)
    costs.append(half * (x.T @ Cf) @ x + x.T @ cf)
    return np.stack(states), np.stack(actions), np.stack(costs)


def _pack(x, u, cs, policy, value_fn):
    return dict(states=x[..., 0], actions=u[..., 0], costs=cs.reshape(-1),
                K=np.stack([p[0] for p in policy]), k=np.stack([p[1][:, 0] for p in policy]),
                V=np.stack([w[0] for w in value_fn]), v=np.stack([w[1][:, 0] for w in value_fn]),
                const=np.array([w[2][0, 0] for w in value_fn]))


def solve_ld(F, f, C, c, x0, Cfin=None, cfin=None):
    """``tvlqr_ref.solve`` in ``np.longdouble``: the same recursion, the same operation order."""
    F, f, C, c, x, V, v, T, n = _operands(F, f, C, c, x0, Cfin, cfin, LD)
    Cf, cf = V, v
    const = np.zeros((1, 1), dtype=LD)
    half = LD(0.5)
    policy, value_fn = [], []
    for t in reversed(range(T)):
        Ft, ft, Ct, ct = F[t], f[t], C[t], c[t]
        Ft_V = Ft.T @ V
        Q = Ct + Ft_V @ Ft
        q = ct + Ft_V @ ft + Ft.T @ v
        Q_uu, Q_ux, q_u = Q[n:, n:], Q[n:, :n], q[n:]
        inv_Q_uu = inv_ld(Q_uu)
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
    policy, value_fn = list(reversed(policy)), list(reversed(value_fn))
    return _pack(*_rollout(F, f, C, c, x, Cf, cf, policy, T, half), policy, value_fn)


def solve_schur(F, f, C, c, x0, Cfin=None, cfin=None):
    """fp64 numpy in the kernel's order: one factorisation of ``Q_uu`` gives ``K`` and ``k``, ``V' = Q_xx + Q_xu K``,
    ``v' = q_x + Q_xu k``, ``V'`` symmetrised."""
    F, f, C, c, x, V, v, T, n = _operands(F, f, C, c, x0, Cfin, cfin, np.float64)
    Cf, cf = V, v
    const = np.zeros((1, 1))
    policy, value_fn = [], []
    for t in reversed(range(T)):
        Ft, ft, Ct, ct = F[t], f[t], C[t], c[t]
        W = Ft.T @ V
        Q = Ct + W @ Ft
        q = ct + W @ ft + Ft.T @ v
        sol = -np.linalg.solve(Q[n:, n:], np.concatenate([q[n:], Q[n:, :n]], axis=1))
        k, K = sol[:, :1], sol[:, 1:]
        V_new = Q[:n, :n] + Q[:n, n:] @ K
        v_new = q[:n] + Q[:n, n:] @ k
        const = const + (0.5 * (k.T @ (Q[n:, n:] @ k)) + k.T @ q[n:] + (0.5 * (ft.T @ (V @ ft)) + ft.T @ v))
        V, v = 0.5 * (V_new + V_new.T), v_new
        policy.append((K, k))
        value_fn.append((V, v, const))
    policy, value_fn = list(reversed(policy)), list(reversed(value_fn))
    return _pack(*_rollout(F, f, C, c, x, Cf, cf, policy, T, 0.5), policy, value_fn)


def make_unscaled(n, m, T, count, seed=0):
    """``tvlqr_ref.make_models`` with F as ``make_lqr`` draws it (no 1 / sqrt(n)); same RNG draws, fp32 arrays."""
    F, f, C, c = tvlqr_ref.make_models(n, m, T, count, seed=seed)
    np.random.seed(seed)
    for b in range(count):
        for t in range(T):
            F[b, t] = lqr_ref.make_lqr(n, m)[0]
    return F, f, C, c


def references(F, f, C, c, x0, Cf=None, cf=None):
    """Per instance: (``solve_ld``, ``tvlqr_ref.solve(dtype=float64)``); operands [B, T, ...], Cf / cf [B, ...] or None."""
    rld, r64 = [], []
    for b in range(x0.shape[0]):
        args = (F[b], f[b], C[b], c[b], x0[b], None if Cf is None else Cf[b], None if cf is None else cf[b])
        rld.append(solve_ld(*args))
        r64.append(tvlqr_ref.solve(*args, dtype=np.float64))
    return rld, r64


def error(got, ref):
    """Largest absolute deviation of an fp64 array from a longdouble reference, taken in longdouble."""
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max())


def ratios(got, rld, r64, name, idx=None):
    """The budget rule's ratio per instance for output ``name``; ``got[name][b]`` is instance ``idx[j]``'s result."""
    idx = list(range(len(rld))) if idx is None else list(idx)
    out = []
    for j, b in enumerate(idx):
        ref = rld[j][name]
        scale = max(1.0, float(np.abs(ref).max()))
        budget = max(error(r64[j][name], ref), FLOOR * scale)
        err = error(got[name][b], ref)
        assert np.isfinite(err), (name, b)
        out.append(err / budget)
    return np.array(out)


def check(got, rld, r64, idx=None, fields=FIELDS, what=""):
    for name in fields:
        r = ratios(got, rld, r64, name, idx)
        print(f"budget {what} {name}: median {np.median(r):.3g} max {r.max():.3g}")
        assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))

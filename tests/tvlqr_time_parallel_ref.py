"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the time-parallel double-precision time-varying LQR
(``tfmpc_tvlqr_solve_time_parallel_f64``), its three phases in the kernels' operation order.

A segment element ``(A, b, G, H, h)`` stands for ``V_e(x_s, x_e) = max_lam 1/2 x_s'H x_s + h'x_s - 1/2 lam'G lam +
lam'(x_e - A x_s - b)``.  ``step_element`` eliminates ``R_t`` once with all right-hand sides, ``combine`` composes two
elements with one solve of ``I + G1 H2``, ``close`` carries a value function from a segment's end to its start and
``boundary`` a state from its start to its end.  ``solve`` condenses every segment, stitches the boundaries and expands
every segment with the sequential recursion in the kernel's (Schur) form between its boundary state and the value
function behind it.

``dtype=np.float64`` solves with ``np.linalg.solve``; ``dtype=np.longdouble`` with ``tvlqr_f64_ref.inv_ld`` (the variant
that shows the formulas themselves, not fp64 rounding, agree with the sequential recursion).
"""

import numpy as np

import tvlqr_f64_ref as ref64

LD = np.longdouble
FIELDS = ("states", "actions", "costs", "K", "k", "V", "v")


def segment_table(T, segments):
    """``(len, [(t0, t1), ...])``: ``segments`` clamped to T, every segment ``ceil(T / segments)`` steps but the last."""
    segments = min(int(segments), T)
    if segments < 1:
        raise ValueError("segments must be at least 1")
    length = -(-T // segments)
    count = -(-T // length)
    return length, [(i * length, min(T, (i + 1) * length)) for i in range(count)]


def workspace_bytes(B, n, m, T, segments):
    """The C ABI's formula: elements, boundary values and states, gains in doubles, then 2 w + B status words."""
    if min(B, n, m, T) <= 0 or segments < 1:
        return 0
    w = B * len(segment_table(T, segments)[1])
    return 8 * (w * (4 * n * n + 4 * n) + B * T * m * (n + 1)) + (4 * (2 * w + B) + 7) // 8 * 8


def _solver(dtype):
    if dtype == LD:
        return lambda A, rhs: ref64.inv_ld(A) @ rhs
    return np.linalg.solve


def _sym(X):
    return X.dtype.type(0.5) * (X + X.T)


def step_element(Ft, ft, Ct, ct, n, solve):
    A_t, B = Ft[:, :n], Ft[:, n:]
    Q, S, R = Ct[:n, :n], Ct[:n, n:], Ct[n:, n:]
    q, r = ct[:n], ct[n:]
    sol = solve(R, np.concatenate([S.T, r, B.T], axis=1))
    Ks, kr, Kb = sol[:, :n], sol[:, n:n + 1], sol[:, n + 1:]
    return (A_t + B @ (-Ks), ft - B @ kr, _sym(B @ Kb), _sym(Q + S @ (-Ks)), q - S @ kr)


def combine(e1, e2, solve):
    """Element 1 precedes element 2 in time."""
    A1, b1, G1, H1, h1 = e1
    A2, b2, G2, H2, h2 = e2
    n = A1.shape[0]
    Y = solve(np.eye(n, dtype=A1.dtype) + G1 @ H2, np.concatenate([A1, G1, b1 - G1 @ h2], axis=1))
    YA, YG, yb = Y[:, :n], Y[:, n:2 * n], Y[:, 2 * n:]
    H = H1 + _sym(A1.T @ (H2 @ YA))
    h = h1 + A1.T @ (h2 + H2 @ yb)
    G = G2 + _sym((A2 @ YG) @ A2.T)
    return (A2 @ YA, A2 @ yb + b2, G, H, h)


def close(e, P, p, solve):
    """The value function at the segment's start from the one at its end."""
    A, b, G, H, h = e
    n = A.shape[0]
    M = solve(np.eye(n, dtype=A.dtype) + P @ G, np.concatenate([P @ A, p + P @ b], axis=1))
    return H + _sym(A.T @ M[:, :n]), h + A.T @ M[:, n:]


def boundary(e, P, p, x, solve):
    """The state at the segment's end from the one at its start and the value function at its end."""
    A, b, G, _, _ = e
    n = A.shape[0]
    return solve(np.eye(n, dtype=A.dtype) + G @ P, (A @ x + b) - G @ p)


def condense(F, f, C, c, t0, t1, n, solve):
    e = None
    for t in reversed(range(t0, t1)):
        s = step_element(F[t], f[t], C[t], c[t], n, solve)
        e = s if e is None else combine(s, e, solve)
    return e


def solve(F, f, C, c, x0, segments, Cfin=None, cfin=None, dtype=np.float64):
    """One instance: F[T,n,d], f[T,n], C[T,d,d], c[T,d], x0[n] -> dict of FIELDS plus ``boundary_states[P,n]``,
    ``boundary_V[P,n,n]``, ``boundary_v[P,n]`` (the stitch's results at every segment's start / end)."""
    dtype = np.dtype(dtype).type
    F, f, C, c, x, Cf, cf, T, n = ref64._operands(F, f, C, c, x0, Cfin, cfin, dtype)
    lin = _solver(dtype)
    half = dtype(0.5)
    _, table = segment_table(T, segments)
    P = len(table)
    elems = [condense(F, f, C, c, t0, t1, n, lin) for t0, t1 in table]
    # stitch: the value function at every segment's end, backwards; the state at every segment's start, forwards
    Vend, vend = [None] * P, [None] * P
    V, v = Cf, cf
    for i in reversed(range(P)):
        Vend[i], vend[i] = V, v
        if i:
            V, v = close(elems[i], V, v, lin)
    xs = [x]
    for i in range(P - 1):
        xs.append(boundary(elems[i], Vend[i], vend[i], xs[i], lin))
    # expand: the sequential recursion (Schur form, V' symmetrised) and rollout on every segment
    states, actions, costs = [None] * (T + 1), [None] * T, [None] * (T + 1)
    Ks, ks, Vs, vs = [None] * T, [None] * T, [None] * T, [None] * T
    for i, (t0, t1) in enumerate(table):
        V, v = Vend[i], vend[i]
        for t in reversed(range(t0, t1)):
            Ft, ft, Ct, ct = F[t], f[t], C[t], c[t]
            W = Ft.T @ V
            Q = Ct + W @ Ft
            q = ct + W @ ft + Ft.T @ v
            sol = -lin(Q[n:, n:], np.concatenate([q[n:], Q[n:, :n]], axis=1))
            ks[t], Ks[t] = sol[:, :1], sol[:, 1:]
            V, v = _sym(Q[:n, :n] + Q[:n, n:] @ Ks[t]), q[:n] + Q[:n, n:] @ ks[t]
            Vs[t], vs[t] = V, v
        z = xs[i]
        for t in range(t0, t1):
            u = Ks[t] @ z + ks[t]
            zu = np.concatenate([z, u], axis=0)
            states[t], actions[t] = z, u
            costs[t] = half * (zu.T @ C[t]) @ zu + zu.T @ c[t]
            z = F[t] @ zu + f[t]
        if i == P - 1:
            states[T] = z
            costs[T] = half * (z.T @ Cf) @ z + z.T @ cf
    return dict(states=np.stack(states)[..., 0], actions=np.stack(actions)[..., 0], costs=np.stack(costs).reshape(-1),
                K=np.stack(Ks), k=np.stack(ks)[..., 0], V=np.stack(Vs), v=np.stack(vs)[..., 0],
                boundary_states=np.stack(xs)[..., 0], boundary_V=np.stack(Vend), boundary_v=np.stack(vend)[..., 0])


def solve_batch(F, f, C, c, x0, segments, Cf=None, cf=None, dtype=np.float64):
    """Per instance ``solve``: operands [B, T, ...], Cf / cf [B, ...] or None -> a list of dicts."""
    return [solve(F[b], f[b], C[b], c[b], x0[b], segments, None if Cf is None else Cf[b], None if cf is None else cf[b],
                  dtype=dtype) for b in range(x0.shape[0])]


def perturbed(make, n, m, T, count, seed, rel=1e-9):
    """``make``'s fp32 models as doubles, perturbed by a relative ``rel`` (not an fp32 problem), C kept symmetric."""
    F, f, C, c = (a.astype(np.float64) for a in make(n, m, T, count, seed=seed))
    rng = np.random.default_rng(seed + 1000)
    F = F * (1.0 + rel * rng.normal(size=F.shape))
    f = f * (1.0 + rel * rng.normal(size=f.shape))
    c = c * (1.0 + rel * rng.normal(size=c.shape))
    C = C * (1.0 + rel * rng.normal(size=C.shape))
    return F, f, 0.5 * (C + np.swapaxes(C, -1, -2)), c

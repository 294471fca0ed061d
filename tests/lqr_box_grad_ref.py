"""TEST INFRASTRUCTURE ONLY -- the control-limited time-varying LQ problem in fp64 and the closed-form gradient of its
optimum, the reference of ``tfmpc_tvlqr_box_vjp_f32``.

``solve_box``: one instance, numpy fp64.  The problem is condensed to a QP in ``U = [u_0; ...; u_{T-1}]`` (dense: T m <= 400
in the tests) and solved by projected Newton on the free set until the active set is a fixed point; the free block is
then solved exactly, so the result is the optimum to fp64 rounding, with controls on a bound carrying the bound's value.

``closed_form``: a batch, torch, any dtype.  Given ANY trajectory and held set: the adjoint of ``tvlqr_grad_ref.closed_form``
on the masked model (held control i at step t: column n + i of F_t zero, row / column n + i of C_t zero with a unit diagonal,
entry n + i of the linear term zero), then the costates and outer products with the UNMASKED model, and
``r_t = C_t dz_t + g_t + F_t^T dlam_{t+1}`` whose entry n + i is the gradient of the bound a held control sits on (``low``
when it equals both).  fp32 gives the error budget of the GPU tests.
"""

import numpy as np
import torch

import tvlqr_grad_ref as gref

CLEAR = 1e-3


def condense(F, f, C, c, x0, Cfin=None, cfin=None):
    """Z = A U + a0 with Z = [z_0; ...; z_{T-1}; x_T]; cost = 1/2 Z^T W Z + w^T Z.  Returns A, a0, W, w."""
    T, n, d = F.shape
    m = d - n
    A = np.zeros((T * d + n, T * m))
    a0 = np.zeros(T * d + n)
    Sx, sx = np.zeros((n, T * m)), x0.astype(np.float64).copy()
    for t in range(T):
        A[t * d:t * d + n] = Sx
        a0[t * d:t * d + n] = sx
        A[t * d + n:(t + 1) * d, t * m:(t + 1) * m] = np.eye(m)
        Sx = F[t] @ A[t * d:(t + 1) * d]
        sx = F[t] @ a0[t * d:(t + 1) * d] + f[t]
    A[T * d:], a0[T * d:] = Sx, sx
    W = np.zeros((T * d + n, T * d + n))
    w = np.zeros(T * d + n)
    for t in range(T):
        W[t * d:(t + 1) * d, t * d:(t + 1) * d] = C[t]
        w[t * d:(t + 1) * d] = c[t]
    W[T * d:, T * d:] = C[T - 1][:n, :n] if Cfin is None else Cfin
    w[T * d:] = c[T - 1][:n] if cfin is None else cfin
    return A, a0, W, w


def solve_box(F, f, C, c, x0, low, high, Cfin=None, cfin=None, max_iter=5000):
    """F[T,n,d] f[T,n] C[T,d,d] c[T,d] x0[n]; low, high broadcastable to [T,m] (±inf allowed).  Returns a dict: states[T+1,n],
    actions[T,m], costs[T+1], clamped[T,m] (bool), at_low[T,m], multiplier[T,m] (|gradient| on held controls, else inf),
    slack[T,m] (distance of a free control to its nearer bound, else inf), clear (bool)."""
    F, f, C, c = (np.asarray(a, dtype=np.float64) for a in (F, f, C, c))
    T, n, d = F.shape
    m = d - n
    lo = np.broadcast_to(np.asarray(low, dtype=np.float64), (T, m)).reshape(-1)
    hi = np.broadcast_to(np.asarray(high, dtype=np.float64), (T, m)).reshape(-1)
    A, a0, W, w = condense(F, f, C, c, np.asarray(x0, dtype=np.float64), Cfin, cfin)
    H = A.T @ W @ A
    H = 0.5 * (H + H.T)
    g0 = A.T @ (W @ a0 + w)
    obj = lambda U: 0.5 * U @ H @ U + g0 @ U                                         # noqa: E731
    U = np.clip(np.zeros(T * m), lo, hi)
    held = None
    for _ in range(max_iter):
        grad = H @ U + g0
        new_held = ((U <= lo) & (grad > 0)) | ((U >= hi) & (grad < 0))
        free = ~new_held
        if held is not None and np.array_equal(held, new_held) and np.abs(grad[free]).max(initial=0.0) <= 1e-8 * max(1.0, np.abs(g0).max()):
            break
        held = new_held
        step = np.zeros_like(U)
        if free.any():
            step[free] = -np.linalg.solve(H[np.ix_(free, free)], grad[free])
        alpha, J0 = 1.0, obj(U)
        while True:
            Un = np.clip(U + alpha * step, lo, hi)
            if obj(Un) <= J0 + 1e-4 * grad @ (Un - U) or alpha < 1e-10:
                break
            alpha *= 0.5
        U = Un
    else:
        raise RuntimeError("projected Newton did not reach a fixed point")
    at_low = held & (U <= lo)
    U[held] = np.where(at_low, lo, hi)[held]
    free = ~held
    if free.any():                      # the free block exactly, on the final active set
        U[free] = -np.linalg.solve(H[np.ix_(free, free)], g0[free] + H[np.ix_(free, held)] @ U[held])
    grad = H @ U + g0
    # the KKT conditions of the polished point: feasible, multipliers of the right sign
    assert (U >= lo).all() and (U <= hi).all() and (grad[at_low] >= 0).all() and (grad[held & ~at_low] <= 0).all()
    Z = A @ U + a0
    xs = np.concatenate([Z[:T * d].reshape(T, d)[:, :n], Z[None, T * d:]], 0)
    us = U.reshape(T, m)
    z = Z[:T * d].reshape(T, d)
    costs = np.array([0.5 * z[t] @ C[t] @ z[t] + c[t] @ z[t] for t in range(T)] + [0.0])
    xT = Z[T * d:]
    Cf = C[T - 1][:n, :n] if Cfin is None else Cfin
    cf = c[T - 1][:n] if cfin is None else cfin
    costs[T] = 0.5 * xT @ Cf @ xT + cf @ xT
    mult = np.where(held, np.abs(grad), np.inf)
    slack = np.where(held, np.inf, np.minimum(U - lo, hi - U))
    return dict(states=xs, actions=us, costs=costs, clamped=held.reshape(T, m), at_low=at_low.reshape(T, m),
                multiplier=mult.reshape(T, m), slack=slack.reshape(T, m),
                clear=bool(mult.min() > CLEAR and slack.min() > CLEAR))


def solve_box_batch(F, f, C, c, x0, low, high, Cfin=None, cfin=None):
    """Batched operands [B, ...] (low / high broadcastable to [B, T, m]) -> dict of stacked arrays."""
    B, T, n, d = F.shape
    lo = np.broadcast_to(np.asarray(low, dtype=np.float64), (B, T, d - n))
    hi = np.broadcast_to(np.asarray(high, dtype=np.float64), (B, T, d - n))
    outs = [solve_box(F[b], f[b], C[b], c[b], x0[b], lo[b], hi[b], None if Cfin is None else Cfin[b],
                      None if cfin is None else cfin[b]) for b in range(B)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def closed_form(F, f, C, c, low, high, states, actions, clamped, at_low, Cfin, cfin, gx, gu, gcost, dtype=torch.float64):
    """Gradients at the given trajectory and held set: a dict F f C c x0 low high (+ Cfin cfin) with [B, T, ...] shapes
    (low, high: [B, T, m]).  ``f``, ``low`` and ``high`` enter only through the trajectory and the held set."""
    del f, low, high
    cv = lambda a: None if a is None else torch.as_tensor(a).to(dtype)               # noqa: E731
    F, C, c, states, actions, Cfin, cfin = (cv(a) for a in (F, C, c, states, actions, Cfin, cfin))
    clamped, at_low = torch.as_tensor(clamped).bool(), torch.as_tensor(at_low).bool()
    B, T, n, d = F.shape
    m = d - n
    gx = torch.zeros(B, T + 1, n, dtype=dtype) if gx is None else cv(gx)
    gu = torch.zeros(B, T, m, dtype=dtype) if gu is None else cv(gu)
    gcost = torch.zeros(B, T + 1, dtype=dtype) if gcost is None else cv(gcost)
    default = Cfin is None
    Cf = C[:, T - 1, :n, :n] if default else Cfin
    cf = c[:, T - 1, :n] if default else cfin
    z = torch.cat([states[:, :T], actions], -1)
    xT = states[:, T]
    mv = lambda A, v: (A @ v.unsqueeze(-1))[..., 0]                                  # noqa: E731
    r = mv(C, z) + c
    rT = mv(Cf, xT) + cf
    g = torch.cat([gx[:, :T], gu], -1) + gcost[:, :T, None] * r                      # 1. fold
    gT = gx[:, T] + gcost[:, T, None] * rT
    held = torch.cat([torch.zeros(B, T, n, dtype=torch.bool), clamped], -1)          # 2. adjoint solve on the masked model
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    Fm = torch.where(held[:, :, None, :], zero, F)
    Cm = torch.where(held[:, :, None, :] | held[:, :, :, None], zero, C)
    Cm = torch.where(torch.diag_embed(held), one, Cm)
    gm = torch.where(held, zero, g)
    dxs, dus, _ = gref.solve(Fm, torch.zeros(B, T, n, dtype=dtype), Cm, gm, torch.zeros(B, n, dtype=dtype), Cf, gT)
    dus = torch.where(clamped, zero, dus)
    dz = torch.cat([dxs[:, :T], dus], -1)
    dxT = dxs[:, T]
    lam = [None] * (T + 1)                                                           # 3. costates, unmasked model
    dlam = [None] * (T + 1)
    rfull = [None] * T
    lam[T], dlam[T] = rT, mv(Cf, dxT) + gT
    for t in reversed(range(T)):
        FT = F[:, t].transpose(-1, -2)
        lam[t] = r[:, t, :n] + mv(FT[:, :n], lam[t + 1])
        rfull[t] = mv(C[:, t], dz[:, t]) + g[:, t] + mv(FT, dlam[t + 1])
        dlam[t] = rfull[t][:, :n]
    ru = torch.stack(rfull, 1)[:, :, n:]
    lam1, dlam1 = torch.stack(lam[1:], 1), torch.stack(dlam[1:], 1)                  # 4. gradients
    outer = lambda a, b: a.unsqueeze(-1) * b.unsqueeze(-2)                           # noqa: E731
    out = dict(F=outer(dlam1, z) + outer(lam1, dz), f=dlam1,
               C=0.5 * (outer(dz, z) + outer(z, dz)) + 0.5 * gcost[:, :T, None, None] * outer(z, z),
               c=dz + gcost[:, :T, None] * z, x0=dlam[0],
               low=torch.where(clamped & at_low, ru, zero), high=torch.where(clamped & ~at_low, ru, zero))
    dCf = 0.5 * (outer(dxT, xT) + outer(xT, dxT)) + 0.5 * gcost[:, T, None, None] * outer(xT, xT)
    dcf = dxT + gcost[:, T, None] * xT
    if default:
        out["C"][:, T - 1, :n, :n] += dCf
        out["c"][:, T - 1, :n] += dcf
    else:
        out.update(Cfin=dCf, cfin=dcf)
    return out


def workload_numbers(B, n, m, bound=0.5):
    """The numbers of ``workloads.control_limited_stable`` without a device: F x0.18, the generator's x0, zero actions to
    start from, actions in [-bound, bound].  -> F, f, C, c, x0, low, high."""
    import problems
    F, f, C, c, x0 = problems.make_lqr_batch_fast(B, n, m, seed=4321)
    return 0.25 * F * (0.18 / 0.25), f, C, c, x0, -bound, bound


def tile_time(a, T):
    """[B, ...] -> [B, T, ...] (a time-invariant model as a time-varying one)."""
    return np.repeat(np.asarray(a)[:, None], T, axis=1)


def tv_bounds(n, m, T, B, seed=1, width=1.0):
    """Bounds of the time-varying test workload (``tvlqr_ref.make_models`` with this seed): per instance and step, low in
    [-1.5 width, -0.5 width], high in [0.5 width, 1.5 width]."""
    rng = np.random.default_rng(seed + 77)
    low = -width * rng.uniform(0.5, 1.5, size=(B, T, m))
    high = width * rng.uniform(0.5, 1.5, size=(B, T, m))
    return low, high


def tv_case(n, m, T, B, final=False, seed=1, width=1.0):
    """The time-varying control-limited test problem: fp32-representable operands (as fp64 arrays) and its fp64 optimum.
    -> (ops dict: F f C c x0 low high Cfin cfin, solution dict of ``solve_box_batch``)."""
    import tvlqr_ref
    F, f, C, c = (a.astype(np.float64) for a in tvlqr_ref.make_models(n, m, T, B, seed=seed))
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B)) if final else (None, None)
    low, high = (a.astype(np.float32).astype(np.float64) for a in tv_bounds(n, m, T, B, seed, width))
    sol = solve_box_batch(F, f, C, c, x0, low, high, Cf, cf)
    return dict(F=F, f=f, C=C, c=c, x0=x0, low=low, high=high, Cfin=Cf, cfin=cf), sol


def mixed(sol):
    """Per instance: at least one held and one free control."""
    cl = sol["clamped"].reshape(sol["clamped"].shape[0], -1)
    return cl.any(1) & (~cl).any(1)

"""TEST INFRASTRUCTURE ONLY -- the time-varying LQR of ``tests/tvlqr_ref.py`` restated in torch (differentiable by
autograd, any dtype) and the closed-form adjoint of ``tfmpc_tvlqr_vjp_f32`` in fp64.

``solve`` follows ``tvlqr_ref.backward`` / ``forward`` operation for operation on a batch: operands ``F[B,T,n,d]``,
``f[B,T,n]``, ``C[B,T,d,d]``, ``c[B,T,d]``, ``x0[B,n]``, optional ``Cfin[B,n,n]``, ``cfin[B,n]``.  Outputs
``states[B,T+1,n]``, ``actions[B,T,m]``, ``costs[B,T+1]``.

``closed_form(..., dtype=torch.float32)`` restates the kernels' algorithm in fp32: with ``autograd_grads`` in fp32 it
gives the error budget of the GPU tests (the larger of the two for F, f, x0; autograd alone for C, c).

``C`` enters the kernels only as a symmetric matrix, so the gradients compared are symmetric: ``sym(G) = (G + G^T) / 2``
of what autograd gives for ``C`` and ``Cfin``.
"""

import torch


def solve(F, f, C, c, x0, Cfin=None, cfin=None):
    B, T, n, d = F.shape
    f, c, x0 = f.unsqueeze(-1), c.unsqueeze(-1), x0.unsqueeze(-1)
    if Cfin is None:
        V, v = C[:, T - 1, :n, :n], c[:, T - 1, :n]
    else:
        V, v = Cfin, cfin.unsqueeze(-1)
    Ks, ks = [None] * T, [None] * T
    for t in reversed(range(T)):
        Ft, ft, Ct, ct = F[:, t], f[:, t], C[:, t], c[:, t]
        FtT = Ft.transpose(-1, -2)
        Ft_V = FtT @ V
        Q = Ct + Ft_V @ Ft
        q = ct + Ft_V @ ft + FtT @ v
        Q_uu, Q_ux, q_u = Q[:, n:, n:], Q[:, n:, :n], q[:, n:]
        Q_xx, Q_xu, q_x = Q[:, :n, :n], Q[:, :n, n:], q[:, :n]
        inv_Q_uu = torch.linalg.inv(Q_uu)
        K = -(inv_Q_uu @ Q_ux)
        k = -(inv_Q_uu @ q_u)
        KT = K.transpose(-1, -2)
        Kt_Quu = KT @ Q_uu
        V = Q_xx + Q_xu @ K + KT @ Q_ux + Kt_Quu @ K
        v = q_x + Q_xu @ k + KT @ q_u + Kt_Quu @ k
        Ks[t], ks[t] = K, k
    x = x0
    states, actions, costs = [x], [], []
    for t in range(T):
        u = Ks[t] @ x + ks[t]
        z = torch.cat([x, u], dim=-2)
        zT = z.transpose(-1, -2)
        costs.append((0.5 * (zT @ C[:, t]) @ z + zT @ c[:, t])[:, 0, 0])
        x = F[:, t] @ z + f[:, t]
        states.append(x)
        actions.append(u)
    xT = x.transpose(-1, -2)
    if Cfin is None:
        Cf, cf = C[:, T - 1, :n, :n], c[:, T - 1, :n]
    else:
        Cf, cf = Cfin, cfin.unsqueeze(-1)
    costs.append((0.5 * (xT @ Cf) @ x + xT @ cf)[:, 0, 0])
    return torch.stack(states, 1)[..., 0], torch.stack(actions, 1)[..., 0], torch.stack(costs, 1)


def sym(G):
    return 0.5 * (G + G.transpose(-1, -2))


def autograd_grads(F, f, C, c, x0, Cfin, cfin, gx, gu, gcost, dtype=torch.float64):
    """Gradients by autograd through ``solve`` in ``dtype`` (symmetric convention for C, Cfin): a dict."""
    ops = dict(F=F, f=f, C=C, c=c, x0=x0)
    if Cfin is not None:
        ops.update(Cfin=Cfin, cfin=cfin)
    ops = {k: torch.as_tensor(v).to(dtype).detach().requires_grad_() for k, v in ops.items()}
    xs, us, cs = solve(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops.get("Cfin"), ops.get("cfin"))
    loss = 0
    for out, g in ((xs, gx), (us, gu), (cs, gcost)):
        if g is not None:
            loss = loss + (out * torch.as_tensor(g).to(dtype)).sum()
    grads = torch.autograd.grad(loss, list(ops.values()))
    got = dict(zip(ops.keys(), (g.detach() for g in grads)))
    got["C"] = sym(got["C"])
    if "Cfin" in got:
        got["Cfin"] = sym(got["Cfin"])
    return got


def closed_form(F, f, C, c, x0, Cfin, cfin, gx, gu, gcost, dtype=torch.float64, parts=False):
    """The adjoint of DESIGN.md §3.8 (fp64 is the oracle; fp32 is the error budget of the algorithm the kernels run):
    fold, adjoint solve, costates, outer products.  gx[B,T+1,n], gu[B,T,m], gcost[B,T+1] (each may be None = zero)
    -> dict of gradients with the operands' [B, T, ...] shapes.  ``parts=True`` -> (that dict, the factors the
    gradients are products of: z, dz [B,T,d]; lam, dlam [B,T,n] (of step t + 1); gcost [B,T+1]; x_T, dx_T, dlam_0 [B,n]).

    In fp32 this algorithm is less accurate than autograd through ``solve`` for the costate-built gradients F, f and
    x0: on the seeded workloads of tests/test_tvlqr_grad_gpu.py (T = 2 / 20 / 50) the median ratio of the errors is
    0.9 - 1.9 and the worst 16.6 (dF), 16.4 (df), 19.1 (dx0); the costates lam, dlam are long sums carried through T
    transposed transitions, while autograd differentiates every rounded step.  For dC, dc it is at most 1.8."""
    d64 = lambda a: None if a is None else torch.as_tensor(a).to(dtype)              # noqa: E731
    F, f, C, c, x0, Cfin, cfin = (d64(a) for a in (F, f, C, c, x0, Cfin, cfin))
    B, T, n, d = F.shape
    m = d - n
    gx = torch.zeros(B, T + 1, n, dtype=dtype) if gx is None else d64(gx)
    gu = torch.zeros(B, T, m, dtype=dtype) if gu is None else d64(gu)
    gcost = torch.zeros(B, T + 1, dtype=dtype) if gcost is None else d64(gcost)
    default = Cfin is None
    Cf = C[:, T - 1, :n, :n] if default else Cfin
    cf = c[:, T - 1, :n] if default else cfin
    xs, us, _ = solve(F, f, C, c, x0, Cf, cf)
    z = torch.cat([xs[:, :T], us], -1)
    xT = xs[:, T]
    mv = lambda A, v: (A @ v.unsqueeze(-1))[..., 0]                                  # noqa: E731
    r = mv(C, z) + c                                                                 # C_t z_t + c_t
    rT = mv(Cf, xT) + cf
    g = torch.cat([gx[:, :T], gu], -1) + gcost[:, :T, None] * r                      # 1. fold
    gT = gx[:, T] + gcost[:, T, None] * rT
    dxs, dus, _ = solve(F, torch.zeros_like(f), C, g, torch.zeros_like(x0), Cf, gT)  # 2. adjoint solve
    dz = torch.cat([dxs[:, :T], dus], -1)
    dxT = dxs[:, T]
    lam = [None] * (T + 1)                                                           # 3. costates
    dlam = [None] * (T + 1)
    lam[T], dlam[T] = rT, mv(Cf, dxT) + gT
    for t in reversed(range(T)):
        FxT = F[:, t, :, :n].transpose(-1, -2)
        lam[t] = r[:, t, :n] + mv(FxT, lam[t + 1])
        dlam[t] = (mv(C[:, t], dz[:, t]) + g[:, t])[:, :n] + mv(FxT, dlam[t + 1])
    lam1, dlam1 = torch.stack(lam[1:], 1), torch.stack(dlam[1:], 1)                  # 4. gradients
    outer = lambda a, b: a.unsqueeze(-1) * b.unsqueeze(-2)                           # noqa: E731
    out = dict(F=outer(dlam1, z) + outer(lam1, dz), f=dlam1,
               C=0.5 * (outer(dz, z) + outer(z, dz)) + 0.5 * gcost[:, :T, None, None] * outer(z, z),
               c=dz + gcost[:, :T, None] * z, x0=dlam[0])
    dCf = 0.5 * (outer(dxT, xT) + outer(xT, dxT)) + 0.5 * gcost[:, T, None, None] * outer(xT, xT)
    dcf = dxT + gcost[:, T, None] * xT
    if default:
        out["C"][:, T - 1, :n, :n] += dCf
        out["c"][:, T - 1, :n] += dcf
    else:
        out.update(Cfin=dCf, cfin=dcf)
    if parts:
        return out, dict(z=z, dz=dz, lam=lam1, dlam=dlam1, gcost=gcost, x_T=xT, dx_T=dxT, dlam_0=dlam[0])
    return out

"""TEST INFRASTRUCTURE ONLY -- the gradients of the finite-horizon Riccati recursion (``tfmpc_tvlqr_backward_f32``'s
``K_t, k_t, V_t, v_t, const_t``) with respect to the model, twice:

* ``closed_form``: the forward-in-time adjoint sweep of DESIGN.md 3.12 in numpy at a chosen dtype, batched, reading only
  the forward's ``K, k, V, v`` and the model (what ``tfmpc_tvlqr_backward_vjp_f32`` computes).  ``dtype=np.float64`` is
  the oracle of record, ``dtype=np.float32`` the fp32 error budget; ``fwd=`` starts the sweep from given forward
  outputs (the kernel's).
* ``autograd_grads``: ``torch.autograd`` through ``recursion_torch``, a restatement of tests/tvlqr_ref.py's recursion.

``C`` and ``C_final`` enter as symmetric matrices: both return the symmetric gradient.
"""

import numpy as np
import torch

import tvlqr_ref

ST_NOT_PD = 2
UPS = ("gK", "gk", "gV", "gv", "gconst")
GRADS = ("dF", "df", "dC", "dc", "dCfin", "dcfin")


def _t(a):
    return np.swapaxes(a, -1, -2)


def _sym(a):
    return 0.5 * (a + _t(a))


def _not_pd(Quu):
    """Per instance: is the symmetric part of Quu[B,m,m] not positive definite (or not finite)?"""
    bad = ~np.isfinite(Quu).all(axis=(-1, -2))
    ev = np.linalg.eigvalsh(np.where(bad[:, None, None], np.eye(Quu.shape[-1]), _sym(Quu)).astype(np.float64))
    return bad | (ev.min(axis=-1) <= 0)


def _model(F, f, C, c, Cfin, cfin, dtype):
    F = np.asarray(F, dtype=dtype)
    B, T, n, d = F.shape
    f = np.asarray(f, dtype=dtype).reshape(B, T, n, 1)
    C = np.asarray(C, dtype=dtype)
    c = np.asarray(c, dtype=dtype).reshape(B, T, d, 1)
    if Cfin is None:
        Cf, cf = C[:, T - 1, :n, :n], c[:, T - 1, :n]
    else:
        Cf, cf = np.asarray(Cfin, dtype=dtype), np.asarray(cfin, dtype=dtype).reshape(B, n, 1)
    return F, f, C, c, Cf, cf


def recursion_np(F, f, C, c, Cfin=None, cfin=None, dtype=np.float64):
    """tests/tvlqr_ref.py's backward recursion batched: F[B,T,n,d], f[B,T,n], C[B,T,d,d], c[B,T,d] (Cfin[B,n,n],
    cfin[B,n]) -> dict(K[B,T,m,n], k[B,T,m], V[B,T,n,n], v[B,T,n], const[B,T], status[B])."""
    F, f, C, c, V, v = _model(F, f, C, c, Cfin, cfin, dtype)
    B, T, n, d = F.shape
    m = d - n
    const = np.zeros((B, 1, 1), dtype=dtype)
    half = dtype(0.5)
    out = dict(K=np.empty((B, T, m, n), dtype), k=np.empty((B, T, m), dtype), V=np.empty((B, T, n, n), dtype),
               v=np.empty((B, T, n), dtype), const=np.empty((B, T), dtype), status=np.zeros(B, np.int32))
    for t in reversed(range(T)):
        Ft, ft, Ct, ct = F[:, t], f[:, t], C[:, t], c[:, t]
        FtV = _t(Ft) @ V
        Q = Ct + FtV @ Ft
        q = ct + FtV @ ft + _t(Ft) @ v
        Quu, Qux, qu = Q[:, n:, n:], Q[:, n:, :n], q[:, n:]
        bad = _not_pd(Quu)
        out["status"][bad] |= ST_NOT_PD
        Quu_s = np.where(bad[:, None, None], np.eye(m, dtype=dtype), Quu)
        K = -np.linalg.solve(Quu_s, Qux)
        k = -np.linalg.solve(Quu_s, qu)
        KtQuu = _t(K) @ Quu
        Vn = _sym(Q[:, :n, :n] + Q[:, :n, n:] @ K + _t(K) @ Qux + KtQuu @ K)
        vn = q[:, :n] + Q[:, :n, n:] @ k + _t(K) @ qu + KtQuu @ k
        const = const + (half * (_t(k) @ (Quu @ k)) + _t(k) @ qu + (half * (_t(ft) @ (V @ ft)) + _t(ft) @ v))
        V, v = Vn, vn
        out["K"][:, t], out["k"][:, t], out["V"][:, t], out["v"][:, t] = K, k[..., 0], V, v[..., 0]
        out["const"][:, t] = const[:, 0, 0]
    for name in ("K", "k", "V", "v", "const"):
        out[name][out["status"] != 0] = np.nan
    return out


def closed_form(F, f, C, c, Cfin=None, cfin=None, gK=None, gk=None, gV=None, gv=None, gconst=None, dtype=np.float64,
                fwd=None):
    """The adjoint sweep, forward in time.  Upstream gradients gK[B,T,m,n], gk[B,T,m], gV[B,T,n,n], gv[B,T,n],
    gconst[B,T] (None = zero).  Returns dict(dF[B,T,n,d], df[B,T,n], dC[B,T,d,d], dc[B,T,d], dCfin[B,n,n] / dcfin[B,n]
    (None with the default final cost, whose gradient is in dC[:, T-1, :n, :n], dc[:, T-1, :n]), status[B]); a flagged
    instance (the forward's status, or a Quu that is not positive definite here) has NaN rows."""
    F, f, C, c, Cf, cf = _model(F, f, C, c, Cfin, cfin, dtype)
    B, T, n, d = F.shape
    m = d - n
    if fwd is None:
        fwd = recursion_np(F, f, C, c, Cfin, cfin, dtype=dtype)
    status = np.array(fwd["status"], dtype=np.int32).copy()
    K, k, V, v = (np.nan_to_num(np.asarray(fwd[name], dtype=dtype)) for name in ("K", "k", "V", "v"))
    k, v = k.reshape(B, T, m, 1), v.reshape(B, T, n, 1)
    up = lambda g, shape: None if g is None else np.asarray(g, dtype=dtype).reshape(shape)      # noqa: E731
    gK, gk, gV = up(gK, (B, T, m, n)), up(gk, (B, T, m, 1)), up(gV, (B, T, n, n))
    gv, gconst = up(gv, (B, T, n, 1)), up(gconst, (B, T, 1, 1))
    Vb, vb, al = np.zeros((B, n, n), dtype), np.zeros((B, n, 1), dtype), np.zeros((B, 1, 1), dtype)
    out = dict(dF=np.empty((B, T, n, d), dtype), df=np.empty((B, T, n), dtype), dC=np.empty((B, T, d, d), dtype),
               dc=np.empty((B, T, d), dtype), dCfin=None, dcfin=None)
    half, two = dtype(0.5), dtype(2.0)
    eye = np.broadcast_to(np.eye(n, dtype=dtype), (B, n, n))
    E = np.concatenate([np.zeros((n, m), dtype), np.eye(m, dtype=dtype)], axis=0)
    zm1, zmn = np.zeros((B, m, 1), dtype), np.zeros((B, m, n), dtype)
    for t in range(T):
        if gV is not None:
            Vb = Vb + _sym(gV[:, t])
        if gv is not None:
            vb = vb + gv[:, t]
        if gconst is not None:
            al = al + gconst[:, t]
        Ft, ft, Ct = F[:, t], f[:, t], C[:, t]
        P, s = (V[:, t + 1], v[:, t + 1]) if t < T - 1 else (Cf, cf)
        Fu = Ft[:, :, n:]
        Quu = Ct[:, n:, n:] + _t(Fu) @ (P @ Fu)
        bad = _not_pd(Quu)
        status[bad] |= ST_NOT_PD
        Quu = np.where(bad[:, None, None], np.eye(m, dtype=dtype), Quu)
        Kt = -np.linalg.solve(Quu, gK[:, t]) if gK is not None else zmn
        kt = -np.linalg.solve(Quu, gk[:, t]) if gk is not None else zm1
        L = np.concatenate([eye, K[:, t]], axis=1)
        l = np.concatenate([np.zeros((B, n, 1), dtype), k[:, t]], axis=1)
        w = E @ kt + L @ vb
        Qb = _sym(L @ Vb @ _t(L) + E @ Kt @ _t(L) + (w + half * al * l) @ _t(l))
        qb = w + al * l
        r = P @ ft + s
        rb = Ft @ qb
        out["dC"][:, t], out["dc"][:, t] = Qb, qb[..., 0]
        out["dF"][:, t] = two * (P @ Ft) @ Qb + r @ _t(qb)
        out["df"][:, t] = (P @ rb + al * r)[..., 0]
        Vb = Ft @ Qb @ _t(Ft) + _sym(rb @ _t(ft)) + half * al * (ft @ _t(ft))
        vb = rb + al * ft
    if Cfin is None:
        out["dC"][:, T - 1, :n, :n] += Vb
        out["dc"][:, T - 1, :n] += vb[..., 0]
    else:
        out["dCfin"], out["dcfin"] = Vb.copy(), vb[..., 0].copy()
    for name in GRADS:
        if out[name] is not None:
            out[name][status != 0] = np.nan
    out["status"] = status
    return out


def recursion_torch(F, f, C, c, Cfin=None, cfin=None):
    """The same recursion in torch (any dtype, batched like ``recursion_np``), for autograd: C and Cfin enter as general
    matrices.  Returns K[B,T,m,n], k[B,T,m], V[B,T,n,n], v[B,T,n], const[B,T]."""
    B, T, n, d = F.shape
    f, c = f.reshape(B, T, n, 1), c.reshape(B, T, d, 1)
    if Cfin is None:
        V, v = C[:, T - 1, :n, :n], c[:, T - 1, :n]
    else:
        V, v = Cfin, cfin.reshape(B, n, 1)
    const = torch.zeros((B, 1, 1), dtype=F.dtype)
    tr = lambda a: a.transpose(-1, -2)          # noqa: E731
    Ks, ks, Vs, vs, cs = [], [], [], [], []
    for t in reversed(range(T)):
        Ft, ft, Ct, ct = F[:, t], f[:, t], C[:, t], c[:, t]
        FtV = tr(Ft) @ V
        Q = Ct + FtV @ Ft
        q = ct + FtV @ ft + tr(Ft) @ v
        Quu, Qux, qu = Q[:, n:, n:], Q[:, n:, :n], q[:, n:]
        K = -torch.linalg.solve(Quu, Qux)
        k = -torch.linalg.solve(Quu, qu)
        KtQuu = tr(K) @ Quu
        Vn = Q[:, :n, :n] + Q[:, :n, n:] @ K + tr(K) @ Qux + KtQuu @ K
        vn = q[:, :n] + Q[:, :n, n:] @ k + tr(K) @ qu + KtQuu @ k
        const = const + (0.5 * (tr(k) @ (Quu @ k)) + tr(k) @ qu + (0.5 * (tr(ft) @ (V @ ft)) + tr(ft) @ v))
        V, v = 0.5 * (Vn + tr(Vn)), vn
        Ks.append(K), ks.append(k[..., 0]), Vs.append(V), vs.append(v[..., 0]), cs.append(const[:, 0, 0])
    return tuple(torch.stack(x[::-1], dim=1) for x in (Ks, ks, Vs, vs, cs))


def autograd_grads(F, f, C, c, Cfin=None, cfin=None, gK=None, gk=None, gV=None, gv=None, gconst=None,
                   dtype=torch.float64):
    """``closed_form``'s gradients (numpy, dtype's precision) from torch.autograd through ``recursion_torch``."""
    ops = [None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (F, f, C, c, Cfin, cfin)]
    outs = recursion_torch(*ops)
    loss = 0
    for g, o in zip((gK, gk, gV, gv, gconst), outs):
        if g is not None:
            loss = loss + (torch.as_tensor(np.asarray(g), dtype=dtype).reshape(o.shape) * o).sum()
    live = [o for o in ops if o is not None]
    if not isinstance(loss, torch.Tensor):
        grads = [torch.zeros_like(o) for o in live]
    else:
        grads = [torch.zeros_like(o) if g is None else g for o, g in zip(live, torch.autograd.grad(loss, live, allow_unused=True))]
    g = dict(zip(GRADS, [x.numpy() for x in grads] + [None] * (6 - len(grads))))
    g["dC"] = _sym(g["dC"])
    if g["dCfin"] is not None:
        g["dCfin"] = _sym(g["dCfin"])
    return g


# ---- seeded workloads ------------------------------------------------------------------------------------------------

def problem(n, m, T, B, seed=0, final=False):
    """tests/tvlqr_ref.py's seeded models: F[B,T,n,d], f[B,T,n], C[B,T,d,d], c[B,T,d] and, with ``final``, an explicit
    Cfin[B,n,n], cfin[B,n] (else None, None): fp32."""
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=seed)
    Cf, cf = tvlqr_ref.make_final(n, B, seed=seed + 1) if final else (None, None)
    return F, f, C, c, Cf, cf


def upstream(n, m, T, B, seed=0, only=None):
    """Seeded upstream gradients as a dict over ``UPS`` (fp32); ``only``: the names that are not None."""
    rng = np.random.default_rng(1000 + seed)
    g = dict(gK=rng.normal(size=(B, T, m, n)), gk=rng.normal(size=(B, T, m)), gV=rng.normal(size=(B, T, n, n)),
             gv=rng.normal(size=(B, T, n)), gconst=rng.normal(size=(B, T)))
    return {name: (a.astype(np.float32) if only is None or name in only else None) for name, a in g.items()}

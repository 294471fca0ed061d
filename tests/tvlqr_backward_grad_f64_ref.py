"""TEST INFRASTRUCTURE ONLY -- restatements one precision up for the double-precision gradients of the finite-horizon
Riccati recursion (``tfmpc_tvlqr_backward_vjp_f64``), and the budget rule of its tests.

``recursion_np`` / ``closed_form``  those of tests/tvlqr_backward_grad_ref.py, the same operation order, with the linear
                 solves through ``solve`` (``np.linalg.solve`` for fp64, ``tvlqr_f64_ref.inv_ld`` for ``np.longdouble``,
                 for which numpy has no ``linalg``) and every matrix product through ``mm`` (``reverse=True`` takes each
                 product's k-sum in reversed order: another admissible fp64 evaluation, for the attainability test).
``references``   batched: the 80-bit closed form (from the 80-bit recursion), the fp64 closed form end to end, and fp64
                 ``autograd_grads``.
``own_forward``  the fp64 closed form started from the kernel's own K, k, V, v (the backward cannot undo the error of
                 the forward it is handed).
``ratios`` / ``check``  the budget rule (DESIGN.md 3.14 / 3.22's form) per gradient and instance: the error against the
                 80-bit closed form over max(error of the fp64 closed form, error of fp64 autograd, error of
                 ``own_forward``, 2^-48 max(1, |ref|_inf)); median over instances <= 2.5 and every instance <= 10.
``check_summed`` a batch- and / or time-summed gradient against the 80-bit sum; its budget is the sum of its terms'
                 budgets (a term: one instance for a batch sum, one step of one instance where time is summed).
"""

import numpy as np

import tvlqr_backward_grad_ref as gref
import tvlqr_f64_ref as ref64

LD = np.longdouble
GRADS = gref.GRADS
UPS = gref.UPS
FWD = ("K", "k", "V", "v")
FLOOR = ref64.FLOOR
MEDIAN_BOUND, MAX_BOUND = ref64.MEDIAN_BOUND, ref64.MAX_BOUND

_t, _sym = gref._t, gref._sym


def solve(A, B):
    """A^-1 B batched over the leading axis, in the operands' dtype."""
    if A.dtype == LD:
        return np.stack([ref64.inv_ld(a) @ b for a, b in zip(A, B)])
    return np.linalg.solve(A, B)


def _mm(reverse):
    if not reverse:
        return lambda a, b: a @ b
    return lambda a, b: np.ascontiguousarray(a[..., ::-1]) @ np.ascontiguousarray(b[..., ::-1, :])


def recursion_np(F, f, C, c, Cfin=None, cfin=None, dtype=np.float64):
    """``tvlqr_backward_grad_ref.recursion_np`` with the solves through ``solve``."""
    F, f, C, c, V, v = gref._model(F, f, C, c, Cfin, cfin, dtype)
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
        bad = gref._not_pd(Quu)
        out["status"][bad] |= gref.ST_NOT_PD
        Quu_s = np.where(bad[:, None, None], np.eye(m, dtype=dtype), Quu)
        K = -solve(Quu_s, Qux)
        k = -solve(Quu_s, qu)
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
                fwd=None, reverse=False):
    """``tvlqr_backward_grad_ref.closed_form`` with the solves through ``solve`` and the products through ``mm``."""
    mm = _mm(reverse)
    F, f, C, c, Cf, cf = gref._model(F, f, C, c, Cfin, cfin, dtype)
    B, T, n, d = F.shape
    m = d - n
    if fwd is None:
        fwd = recursion_np(F, f, C, c, Cfin, cfin, dtype=dtype)
    status = np.array(fwd["status"], dtype=np.int32).copy()
    K, k, V, v = (np.nan_to_num(np.asarray(fwd[name], dtype=dtype)) for name in FWD)
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
        Quu = Ct[:, n:, n:] + mm(_t(Fu), mm(P, Fu))
        bad = gref._not_pd(Quu)
        status[bad] |= gref.ST_NOT_PD
        Quu = np.where(bad[:, None, None], np.eye(m, dtype=dtype), Quu)
        Kt = -solve(Quu, gK[:, t]) if gK is not None else zmn
        kt = -solve(Quu, gk[:, t]) if gk is not None else zm1
        L = np.concatenate([eye, K[:, t]], axis=1)
        l = np.concatenate([np.zeros((B, n, 1), dtype), k[:, t]], axis=1)       # noqa: E741
        w = E @ kt + mm(L, vb)
        Qb = _sym(mm(mm(L, Vb), _t(L)) + mm(E @ Kt, _t(L)) + (w + half * al * l) @ _t(l))
        qb = w + al * l
        r = mm(P, ft) + s
        rb = mm(Ft, qb)
        out["dC"][:, t], out["dc"][:, t] = Qb, qb[..., 0]
        out["dF"][:, t] = mm(two * mm(P, Ft), Qb) + r @ _t(qb)
        out["df"][:, t] = (mm(P, rb) + al * r)[..., 0]
        Vb = mm(mm(Ft, Qb), _t(Ft)) + _sym(rb @ _t(ft)) + half * al * (ft @ _t(ft))
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


def as_f64(*arrays):
    """fp32 (or any) arrays as float64 copies, ``None`` kept."""
    return tuple(None if a is None else np.asarray(a, dtype=np.float64) for a in arrays)


def references(F, f, C, c, Cf=None, cf=None, ups=None):
    """(80-bit closed form from the 80-bit recursion, fp64 closed form end to end, fp64 ``autograd_grads``), batched."""
    ups = ups or {}
    rld = closed_form(F, f, C, c, Cf, cf, **ups, dtype=LD)
    r64 = closed_form(F, f, C, c, Cf, cf, **ups, dtype=np.float64)
    rag = gref.autograd_grads(F, f, C, c, Cf, cf, **ups)
    assert not rld["status"].any() and not r64["status"].any()
    return rld, r64, rag


def own_forward(F, f, C, c, Cf, cf, ups, fwd):
    """The fp64 closed form started from the kernel's forward outputs ``fwd`` (K, k, V, v as numpy float64, batched)."""
    B = np.asarray(F).shape[0]
    own = {name: np.asarray(fwd[name], dtype=np.float64) for name in FWD}
    out = closed_form(F, f, C, c, Cf, cf, **(ups or {}), fwd=dict(own, status=np.zeros(B, np.int32)))
    assert not out["status"].any()
    return out


def _err(got, ref, keep):
    """max |got - ref| in longdouble over every axis but the first ``keep``."""
    ref = np.asarray(ref)
    e = np.abs(np.asarray(got, dtype=LD).reshape(ref.shape) - ref)
    return e.reshape(*e.shape[:keep], -1).max(axis=-1).astype(np.float64)


def _scale(ref, keep):
    a = np.abs(np.asarray(ref))
    return np.maximum(1.0, a.reshape(*a.shape[:keep], -1).max(axis=-1).astype(np.float64))


def budgets(refs, name, own=None, keep=1):
    """The budget per term of gradient ``name``: per instance (``keep=1``) or per instance and step (``keep=2``)."""
    rld, r64, rag = refs
    ref = rld[name]
    terms = [_err(r64[name], ref, keep), _err(rag[name], ref, keep), FLOOR * _scale(ref, keep)]
    if own is not None:
        terms.append(_err(own[name], ref, keep))
    return np.max(np.stack(terms), axis=0)


def ratios(got, refs, name, own=None):
    """The budget rule's ratio per instance for gradient ``name`` (``got`` batched like the references)."""
    err = _err(got, refs[0][name], 1)
    assert np.isfinite(err).all(), name
    return err / budgets(refs, name, own)


def names_of(refs):
    return [name for name in GRADS if refs[0][name] is not None]


def check(got, refs, own=None, names=None, what=""):
    """``got``: name -> batched array.  Prints every ratio's median and maximum, asserts the rule, returns them."""
    out = {}
    for name in (names_of(refs) if names is None else names):
        r = ratios(got[name], refs, name, own)
        out[name] = [float(np.median(r)), float(r.max())]
        print(f"budget {what} {name}: median {np.median(r):.3g} max {r.max():.3g}")
        assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))
    return out


def check_summed(got, refs, name, own=None, batch=False, time=False, what=""):
    """``got``: gradient ``name`` summed over the batch and / or time (a time axis of 1 kept or dropped) over exactly the
    instances of ``refs``.  The budget is the sum of the terms' budgets."""
    ref = refs[0][name]
    timed = name in GRADS[:4]
    time = time and timed
    bud = budgets(refs, name, own, keep=2 if time else 1)
    if time:
        ref, bud = ref.sum(axis=1), bud.sum(axis=1)
    if batch:
        ref, bud = ref.sum(axis=0)[None], np.array([bud.sum()])
    err = _err(np.asarray(got).reshape(ref.shape), ref, 1)
    assert np.isfinite(err).all(), name
    r = err / bud
    print(f"budget {what} sum({'b' if batch else ''}{'t' if time else ''}) {name}: median {np.median(r):.3g} max {r.max():.3g}")
    assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))
    return [float(np.median(r)), float(r.max())]

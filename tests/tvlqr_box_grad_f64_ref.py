"""TEST INFRASTRUCTURE ONLY -- the gradients of the double-precision control-limited time-varying LQR optimum
(``tfmpc_tvlqr_box_vjp_f64``, ``tvlqr_box_vjp(dtype=torch.float64)``) restated in numpy, generic in
dtype, on a GIVEN trajectory and held set, and the budget rule of their tests.

``closed_form`` is DESIGN.md §3.11's adjoint -- fold, adjoint solve on the masked model, costates, outer products and the
bound gradient ``r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i]`` with the UNMASKED model -- with the costates taken
from the value function of the REDUCED problem (held controls fixed at their bounds, free ones optimised),

    lam_{t+1} = V^m_{t+1} x_{t+1} + v^m_{t+1},   dlam_{t+1} = V^m_{t+1} dx_{t+1} + v~_{t+1},

``V^m``, ``v~`` from the adjoint solve on the masked model (column n + i of F_t zero, row and column n + i of C_t zero with a
unit diagonal, entry n + i of the linear term zero; final cost ``(C_fin, g_T)``), ``v^m`` from the same masked model with the
forward's reduced linear terms ``f^_t = f_t + F_t[:, n + H_t] u_H``, ``c^_t = c_t + C_t[:, n + H_t] u_H`` and the true final
cost.  ``costates="recursion"`` is §3.11's open-loop recursion in the same dtype, kept to pin where it agrees and by how
much it fails where it cannot be used.

THE REFERENCE is the value form in ``np.longdouble``; the ``np.float64`` run of the same code sets the budget.  Budget rule
(§3.14 / §3.15's): per output and instance, ``|got - ref_ld|_inf / max(error of the fp64 restatement, 2^-48 max(1,
|ref_ld|_inf))``; the median over instances <= 2.5 and every instance <= 10; the budget of a batch- or time-summed gradient
is the sum of its terms' budgets.
"""

import functools

import numpy as np

import lqr_box_grad_ref as bref
import tvlqr_box_f64_ref as dref
import tvlqr_box_solve_ref as sref
import tvlqr_f64_ref as ref64
import tvlqr_ref
from tvlqr_grad_f64_ref import _mv

LD = np.longdouble
FLOOR = ref64.FLOOR
MEDIAN_BOUND, MAX_BOUND = ref64.MEDIAN_BOUND, ref64.MAX_BOUND
TIMED = ("F", "f", "C", "c", "low", "high")


def _solve(dtype, *args):
    if dtype == LD:
        return ref64.solve_ld(*args)
    return tvlqr_ref.solve(*args, dtype=dtype)


def masked_model(F, C, lin, held):
    """ONE instance, held[T, m] bool: the model with the held controls taken out (copies)."""
    F, C, lin = F.copy(), C.copy(), lin.copy()
    n = F.shape[1]
    for t in range(F.shape[0]):
        for i in np.nonzero(held[t])[0]:
            F[t][:, n + i] = 0
            C[t][n + i, :] = 0
            C[t][:, n + i] = 0
            C[t][n + i, n + i] = 1
            lin[t][n + i] = 0
    return F, C, lin


def closed_form(F, f, C, c, low, states, actions, clamped, Cfin=None, cfin=None, gx=None, gu=None, gcost=None, dtype=LD,
                costates="value", reverse=False):
    """ONE instance at the GIVEN trajectory states[T+1, n], actions[T, m] and held set clamped[T, m] (bool); ``low``
    broadcastable to [T, m] tells the two bounds apart: a held control whose value equals ``low`` sits on ``low``.
    -> dict of gradients F, f, C, c, x0, low, high (and Cfin, cfin) in ``dtype``; conventions as
    ``tvlqr_grad_f64_ref.closed_form``."""
    F, f, C, c, states, actions = (np.asarray(a, dtype=dtype) for a in (F, f, C, c, states, actions))
    T, n, d = F.shape
    m = d - n
    f, c = f.reshape(T, n), c.reshape(T, d)
    clamped = np.asarray(clamped, dtype=bool).reshape(T, m)
    at_low = clamped & (np.asarray(actions, dtype=np.float64) == np.broadcast_to(np.asarray(low, dtype=np.float64), (T, m)))
    z0 = lambda *s: np.zeros(s, dtype=dtype)                                         # noqa: E731
    gx = z0(T + 1, n) if gx is None else np.asarray(gx, dtype=dtype)
    gu = z0(T, m) if gu is None else np.asarray(gu, dtype=dtype)
    gcost = z0(T + 1) if gcost is None else np.asarray(gcost, dtype=dtype)
    default = Cfin is None
    Cf = C[T - 1][:n, :n] if default else np.asarray(Cfin, dtype=dtype)
    cf = c[T - 1][:n] if default else np.asarray(cfin, dtype=dtype).reshape(n)
    xs, us = states, actions
    z = np.concatenate([xs[:T], us], axis=-1)
    xT = xs[T]
    r = np.stack([C[t] @ z[t] for t in range(T)]) + c                                # C_t z_t + c_t
    rT = Cf @ xT + cf
    g = np.concatenate([gx[:T], gu], axis=-1) + gcost[:T, None] * r                  # 1. fold
    gT = gx[T] + gcost[T] * rT
    Fm, Cm, gm = masked_model(F, C, g, clamped)                                      # 2. adjoint solve, masked model
    adj = _solve(dtype, Fm, z0(T, n), Cm, gm, z0(n), Cf, gT)
    dxs = adj["states"]
    dus = np.where(clamped, dtype(0), adj["actions"])
    dz = np.concatenate([dxs[:T], dus], axis=-1)
    dxT = dxs[T]
    lam1, dlam1 = [None] * T, [None] * T                                             # 3. costates of step t + 1
    if costates == "value":
        uh = np.where(clamped, us, dtype(0))                                         # the reduced forward problem
        fhat = f + np.stack([F[t][:, n:] @ uh[t] for t in range(T)])
        chat = c + np.stack([C[t][:, n:] @ uh[t] for t in range(T)])
        _, _, chat = masked_model(F, C, chat, clamped)
        vm = _solve(dtype, Fm, fhat, Cm, chat, xs[0], Cf, cf)["v"]
        V = adj["V"]
        for t in range(T):
            last = t == T - 1
            Vn = Cf if last else V[t + 1]
            lam1[t] = _mv(Vn, xs[t + 1], reverse) + (cf if last else vm[t + 1])
            dlam1[t] = _mv(Vn, dxs[t + 1], reverse) + (gT if last else adj["v"][t + 1])
        dlam0 = adj["v"][0]                                                          # V_0 dx_0 + v~_0 with dx_0 = 0
    else:
        lam, dlam = rT, Cf @ dxT + gT
        for t in reversed(range(T)):
            lam1[t], dlam1[t] = lam, dlam
            FxT = F[t][:, :n].T
            lam = r[t][:n] + FxT @ lam
            dlam = (C[t] @ dz[t] + g[t])[:n] + FxT @ dlam
        dlam0 = dlam
    lam1, dlam1 = np.stack(lam1), np.stack(dlam1)
    ru = np.stack([(C[t] @ dz[t] + g[t] + F[t].T @ dlam1[t])[n:] for t in range(T)])  # the bounds' gradient, unmasked model
    outer = lambda a, b: a[..., :, None] * b[..., None, :]                           # noqa: E731
    half = dtype(0.5)
    out = dict(F=outer(dlam1, z) + outer(lam1, dz), f=dlam1,                         # 4. gradients
               C=half * (outer(dz, z) + outer(z, dz)) + half * gcost[:T, None, None] * outer(z, z),
               c=dz + gcost[:T, None] * z, x0=dlam0,
               low=np.where(at_low, ru, dtype(0)), high=np.where(clamped & ~at_low, ru, dtype(0)))
    dCf = half * (outer(dxT, xT) + outer(xT, dxT)) + half * gcost[T] * outer(xT, xT)
    dcf = dxT + gcost[T] * xT
    if default:
        out["C"][T - 1][:n, :n] += dCf
        out["c"][T - 1][:n] += dcf
    else:
        out.update(Cfin=dCf, cfin=dcf)
    return out


def grads(ops, states, actions, clamped, gx, gu, gcost, **kw):
    """``closed_form`` per instance of a batch: ops a dict F f C c low (Cfin cfin) of [B, ...] arrays (low broadcastable to
    [B, T, m]) -> dict of [B, ...]."""
    B, T = actions.shape[:2]
    low = np.broadcast_to(ops["low"], actions.shape)
    pick = lambda a, b: None if a is None else a[b]                                  # noqa: E731
    per = [closed_form(ops["F"][b], ops["f"][b], ops["C"][b], ops["c"][b], low[b], states[b], actions[b], clamped[b],
                       pick(ops.get("Cfin"), b), pick(ops.get("cfin"), b), pick(gx, b), pick(gu, b), pick(gcost, b), **kw)
           for b in range(B)]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def references(ops, states, actions, clamped, gx, gu, gcost):
    """(the 80-bit value-form reference, the fp64 value-form restatement): dicts of [B, ...]."""
    return tuple(grads(ops, states, actions, clamped, gx, gu, gcost, dtype=dt) for dt in (LD, np.float64))


def _err(a, ref):
    return float(np.abs(np.asarray(a, dtype=LD) - ref).max())


def term_budgets(refs, name, time_summed=False):
    """Budget per instance of output ``name``: max(error of the fp64 restatement, floor); for a gradient summed over time,
    the sum over the steps of the per-step budgets."""
    rld, r64 = refs

    def one(ref, a):
        return max(_err(a, ref), FLOOR * max(1.0, float(np.abs(ref).max())))
    out = []
    for b in range(rld[name].shape[0]):
        if time_summed and name in TIMED:
            out.append(sum(one(rld[name][b, t], r64[name][b, t]) for t in range(rld[name].shape[1])))
        else:
            out.append(one(rld[name][b], r64[name][b]))
    return np.array(out)


def ratios(got, refs, name, batch_summed=False, time_summed=False, idx=None):
    """The rule's ratio(s) for ``got`` (shaped like the operand of output ``name``): one per instance, or one in all for a
    batch-summed gradient.  The reference is summed in 80-bit over the axes ``got`` is summed over."""
    ref = refs[0][name]
    budgets = term_budgets(refs, name, time_summed)
    if time_summed and name in TIMED:
        ref = ref.sum(axis=1, keepdims=True)
    got = np.asarray(got, dtype=LD).reshape((-1,) + ref.shape[1:])
    if batch_summed:
        err = _err(got[0], ref.sum(axis=0))
        assert np.isfinite(err), name
        return np.array([err / budgets.sum()])
    idx = range(ref.shape[0]) if idx is None else idx
    out = []
    for b in idx:
        err = _err(got[b], ref[b])
        assert np.isfinite(err), (name, b)
        out.append(err / budgets[b])
    return np.array(out)


def check(got, refs, what="", shared=(), time_shared=(), idx=None, log=None):
    """Every gradient of ``got`` (dict name -> array) under the rule; ``shared`` / ``time_shared``: the names summed over the
    batch / over time.  ``log``: a dict that collects (median, max) per name."""
    for name in got:
        r = ratios(got[name], refs, name, name in shared, name in time_shared, idx)
        print(f"budget {what} d{name}: median {np.median(r):.3g} max {r.max():.3g}")
        if log is not None:
            log[name] = (float(np.median(r)), float(r.max()))
        assert np.median(r) <= MEDIAN_BOUND and r.max() <= MAX_BOUND, (what, name, float(np.median(r)), float(r.max()))


def exact_zeros(got, clamped, at_low, n, loss, summed=()):
    """What §3.11 makes exactly zero: dlow / dhigh off the held set and on the other bound; under a loss without a cost
    term, dc[n + i] of a held control and the dC entries between two held controls.  Every output of ``got`` that is per
    instance and per step (its name not in ``summed``) is checked on its own.  -> the names checked."""
    checked = set()
    if "low" not in summed:
        assert (got["low"][~at_low] == 0).all()
        checked.add("low")
    if "high" not in summed:
        assert (got["high"][~(clamped & ~at_low)] == 0).all()
        checked.add("high")
    if loss in ("states", "actions"):
        if "c" not in summed:
            assert (got["c"][..., n:][clamped] == 0).all()
            checked.add("c")
        if "C" not in summed:
            both = clamped[..., :, None] & clamped[..., None, :]
            assert (got["C"][..., n:, n:][both] == 0).all()
            checked.add("C")
    return checked


# ---- the cases of the GPU test -----------------------------------------------------------------------------------------
BATCH = 4
LOSSES = ("states", "actions", "costs", "mixed")
MODEL = ("F", "f", "C", "c")
BOUNDS = ("scalar", "m", "Tm", "B1m", "BTm")
INF = float("inf")


def snap(actions, clamped, low, high):
    """Held controls carry the bits of the bound they are nearer to."""
    low, high = np.broadcast_to(low, actions.shape), np.broadcast_to(high, actions.shape)
    nearer_low = np.abs(actions - low) <= np.abs(actions - high)
    return np.where(clamped, np.where(nearer_low, low, high), actions)


def weights(B, n, m, T, loss, seed=3):
    rng = np.random.default_rng(seed)
    w = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    return tuple(g if loss in (name, "mixed") else None for g, name in zip(w, LOSSES))


def _operands(n, m, T, B, final, seed, width, unscaled):
    """The operands of ``lqr_box_grad_ref.tv_case`` (without its dense exact solve); ``unscaled``: F as ``make_lqr``
    draws it (``tvlqr_f64_ref.make_unscaled``)."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = (a.astype(np.float64) for a in make(n, m, T, B, seed=seed))
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B)) if final else (None, None)
    low, high = (a.astype(np.float32).astype(np.float64) for a in bref.tv_bounds(n, m, T, B, seed, width))
    return dict(F=F, f=f, C=C, c=c, x0=x0, low=low, high=high, Cfin=Cf, cfin=cf)


def _bound_form(a, form):
    """-> (the full [B, T, m] array every instance and step sees, what the caller passes)."""
    B, T, m = a.shape
    user = {"scalar": a[0, 0, 0], "m": a[0, 0], "Tm": a[0], "B1m": a[:, :1], "BTm": a}[form]
    return np.ascontiguousarray(np.broadcast_to(user, (B, T, m))), np.array(user)      # (a scalar stays 0-d)


@functools.lru_cache(maxsize=None)
def forward_case(n, m, T, width=1.0, B=BATCH, final=False, seed=1, shared=(), const=(), bounds="BTm", held="some"):
    """``lqr_box_grad_ref.tv_case``'s operands perturbed (no fp32 numbers) and their fp64 optimum by
    ``tvlqr_box_solve_ref.solve_batch(dtype=np.float64)``, held controls snapped to the bounds' bits.  ``shared``: operands
    without a batch axis (every instance has instance 0's); ``const``: model operands with a time axis of 1; ``bounds``: the
    form low / high are passed in (BOUNDS); ``held``: "some", "all" (low == high: the clipped unconstrained optimum),
    "none-inf" (bounds at +-inf) or "none-wide" (+-1e6).
    -> (full: the replicated problem, [B, T, ...] arrays; user: what the caller passes; states, actions, held set)."""
    full = dref.perturb(_operands(n, m, T, B, final, seed, width, False))
    user = {}
    for k in ("F", "f", "C", "c", "x0", "Cfin", "cfin"):
        a = full[k]
        if a is None:
            continue
        if k in const:
            a = np.repeat(a[:, :1], T, axis=1)
        if k in shared:
            a = np.repeat(a[:1], B, axis=0)
        full[k] = a
        u = a[:, :1] if k in const else a
        user[k] = np.ascontiguousarray(u[0] if k in shared else u)
    if held == "none-inf":
        full["low"], full["high"] = np.full((B, T, m), -INF), np.full((B, T, m), INF)
    elif held == "none-wide":
        full["low"], full["high"] = np.full((B, T, m), -1.0e6), np.full((B, T, m), 1.0e6)
    elif held == "all":
        full["high"] = full["low"] = np.clip(full["low"] + 0.5 * width, full["low"], full["high"])
    for k in ("low", "high"):
        full[k], user[k] = _bound_form(full[k], bounds)
    sol = sref.solve_batch(full["F"], full["f"], full["C"], full["c"], full["x0"], full["low"], full["high"], full.get("Cfin"),
                           full.get("cfin"), dtype=np.float64)
    assert not sol["status"].any(), sol["status"]
    actions = snap(sol["actions"].astype(np.float64), sol["clamped"], full["low"], full["high"])
    return full, user, sol["states"].astype(np.float64), actions, dref.held_from_actions(actions, full["low"], full["high"])


@functools.lru_cache(maxsize=None)
def unscaled_case(n=16, m=8, T=50, B=BATCH, seed=0):
    """An UNSCALED model (``make_lqr``'s spectrum, rho(F_x) ~ 5), on which no rollout from u = 0 survives T = 50 and the
    control-limited forward restatement cannot start.  The trajectory is built from the held set instead: the unconstrained
    fp64 optimum is clipped to ``tv_bounds`` scaled to the median |u| (about half of the controls are held), the reduced
    problem -- held controls fixed at their bounds -- is solved exactly by the closed-loop fp64 recursion on the masked
    model, and a free control that left the box gets the box widened around it.  The result is the stationary point of
    the problem with that held set, which is all the VJP reads.  -> as ``forward_case``."""
    full = dref.perturb(_operands(n, m, T, B, False, seed, 1.0, True))
    d = n + m
    states, actions = np.empty((B, T + 1, n)), np.empty((B, T, m))
    low, high = full["low"].copy(), full["high"].copy()
    for b in range(B):
        F, f, C, c, x0 = (full[k][b] for k in ("F", "f", "C", "c", "x0"))
        u0 = tvlqr_ref.solve(F, f, C, c, x0, dtype=np.float64)["actions"]
        scale = np.median(np.abs(u0))
        low[b], high[b] = scale * low[b], scale * high[b]
        held = (u0 <= low[b]) | (u0 >= high[b])
        uh = np.where(held, np.clip(u0, low[b], high[b]), 0.0)
        fhat = f + np.stack([F[t][:, n:] @ uh[t] for t in range(T)])
        chat = c + np.stack([C[t][:, n:] @ uh[t] for t in range(T)])
        Fm, Cm, chat = masked_model(F, C, chat, held)
        red = tvlqr_ref.solve(Fm, fhat, Cm, chat, x0, C[T - 1][:n, :n], c[T - 1][:n], dtype=np.float64)
        actions[b] = np.where(held, uh, red["actions"])
        states[b] = red["states"]
        out = ~held & ((actions[b] <= low[b]) | (actions[b] >= high[b]))
        low[b] = np.where(out, actions[b] - scale, low[b])
        high[b] = np.where(out, actions[b] + scale, high[b])
    full["low"], full["high"] = low, high
    user = {k: full[k] for k in ("F", "f", "C", "c", "x0", "low", "high")}
    return full, user, states, actions, dref.held_from_actions(actions, low, high)


@functools.lru_cache(maxsize=None)
def case(loss="mixed", unscaled=False, **kw):
    """-> (full, user, states, actions, held, loss weights, references) of ``forward_case(**kw)``; computed once,
    read-only."""
    full, user, states, actions, held = unscaled_case(**kw) if unscaled else forward_case(**kw)
    B, T, m = actions.shape
    w = weights(B, states.shape[2], m, T, loss)
    return full, user, states, actions, held, w, references(full, states, actions, held, *w)


# (n, m, T, seed): width 1 of ``tv_bounds`` unless said otherwise
SHAPES = [dict(n=1, m=1, T=1, seed=5), dict(n=3, m=2, T=2), dict(n=5, m=3, T=20), dict(n=3, m=5, T=20), dict(n=16, m=8, T=20),
          dict(n=16, m=16, T=4), dict(n=17, m=8, T=4, width=1.3), dict(n=16, m=17, T=4), dict(n=8, m=32, T=4),
          dict(n=32, m=32, T=4)]
FINAL = [dict(n=5, m=3, T=20, final=True), dict(n=16, m=8, T=20, final=True, shared=("Cfin", "cfin"))]
ALL_HELD = [dict(n=8, m=32, T=4, held="all"), dict(n=5, m=3, T=5, held="all")]
NONE_HELD = [dict(n=16, m=8, T=20, held="none-inf"), dict(n=17, m=8, T=4, held="none-wide")]
TIME = ("F", "f", "C")
SHARING = {"batch": (MODEL, ()), "time": ((), TIME), "both": (MODEL, TIME)}
SHARED_BOUNDS = {(5, 3): ("scalar", "m", "B1m"), (20, 10): ("Tm", "BTm", "scalar")}   # the bounds' form per sharing
SHARED = [dict(n=n, m=m, T=5, shared=SHARING[s][0], const=SHARING[s][1], bounds=SHARED_BOUNDS[n, m][i])
          for n, m in SHARED_BOUNDS for i, s in enumerate(SHARING)]
BOUND_FORMS = [dict(n=5, m=3, T=5, bounds=form) for form in BOUNDS]
ZEROS = [dict(n=5, m=3, T=5), dict(n=20, m=10, T=5)]           # nothing shared: every exact zero of §3.11 is a per-step entry
CHUNKS = [dict(n=4, m=2, T=3, B=B, shared=MODEL, bounds="Tm") for B in (3, 257)]
NOT_PD = [dict(n=4, m=2, T=2, B=B, shared=("F", "f"), bounds="B1m") for B in (3, 519)]
END_TO_END = [dict(n=16, m=8, T=50), dict(n=5, m=3, T=20)]
GRADCHECK = dict(n=3, m=2, T=4, B=2, seed=3)


def gpu_cases():
    """Every ``forward_case`` the GPU test uses with held and free controls in it."""
    return SHAPES + FINAL + SHARED + BOUND_FORMS + ZEROS + CHUNKS + NOT_PD + END_TO_END + [GRADCHECK]

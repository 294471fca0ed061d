"""Gradients through a control-limited LQR solve: ``tfmpc_tvlqr_box_vjp_f32`` (include/tfmpc_hip.h).

At the optimum of a box-constrained LQ problem the controls that sit on a bound are held (``du = 0``) in the adjoint;
everything else is the adjoint of :mod:`tfmpc.solvers.tvlqr_grad`.  The held set is read off the trajectory: control
``i`` at step ``t`` is held iff ``actions[b, t, i]`` equals ``low`` or ``high`` bit for bit (every forward of this
package clips, so a control on its bound carries the bound's bits).  There is no multiplier test: a control on its bound
with a zero multiplier counts as held, as in Amos et al. 2018.

:func:`tvlqr_box_vjp` is the thin front of the ABI call and serves any forward (a user's own QP solver included);
:func:`box_lqr_solve` is the differentiable solve built on the control-limited iLQR launch.
"""

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from tfmpc import _hip
from tfmpc.solvers.tvlqr_grad import as_f32_graph, wants_grad

NAMES = ("F", "f", "C", "c", "C_final", "c_final", "x0", "low", "high")


def _cast(a, device, dtype=torch.float32):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=dtype)
    return torch.as_tensor(np.asarray(a, dtype=np.float64 if dtype == torch.float64 else np.float32), device=device)


def _timed(t, inner, name, B, T):
    """``[T|1, *inner]`` or ``[B, T|1, *inner]`` (a trailing column axis of 1 on vectors dropped) -> (contiguous tensor,
    batch stride, time stride)."""
    if len(inner) == 1 and t.dim() >= 3 and t.shape[-1] == 1 and t.shape[-2] == inner[0]:
        t = t.squeeze(-1)
    k = len(inner)
    if t.dim() not in (k + 1, k + 2) or tuple(t.shape[-k:]) != tuple(inner) or t.shape[-k - 1] not in (1, T) \
            or (t.dim() == k + 2 and t.shape[0] != B):
        raise ValueError(f"{name} must be [T|1, {', '.join(map(str, inner))}] with an optional leading batch axis of {B} "
                         f"(T = {T}), got {tuple(t.shape)}")
    t = t.contiguous()
    per = int(np.prod(inner))
    st = per if t.shape[-k - 1] == T and T > 1 else 0
    sb = t.shape[-k - 1] * per if t.dim() == k + 2 else 0
    return t, sb, st


def _bound(t, m, name, B, T):
    """``[m]``, ``[T|1, m]`` or ``[B, T|1, m]``."""
    if t.dim() == 0:
        t = t.expand(m)
    if t.dim() == 1:
        t = t.unsqueeze(0)
    return _timed(t, (m,), name, B, T)


def tvlqr_box_vjp(F, f, C, c, low, high, states, actions, g_states=None, g_actions=None, g_costs=None, C_final=None,
                  c_final=None, want=None, dtype=None):
    """Vector-Jacobian product of a control-limited time-varying LQR solution.

    ``states[B, T+1, n]`` (``states[:, 0]`` is ``x0``) and ``actions[B, T, m]`` are the optimum of the problem of
    :class:`tfmpc.solvers.TimeVaryingLQR` (same operand shapes: ``[T|1, ...]`` or ``[B, T|1, ...]``) under
    ``low <= u_t <= high``; ``low`` / ``high`` are ``[m]``, ``[T|1, m]`` or ``[B, T|1, m]``, ±inf allowed.  ``g_states``,
    ``g_actions``, ``g_costs[B, T+1]`` are the upstream gradients (``None`` = zero).

    Returns a dict with the gradient of every name in ``want`` (default: every operand given, ``x0``, ``low``, ``high``)
    in the operand's own shape -- an operand without a batch axis gets the sum over the batch, a time axis of 1 the sum
    over time; the default final cost's gradient is part of ``C``'s and ``c``'s -- plus ``"clamped"`` (bool
    ``[B, T, m]``: the held set) and ``"status"`` (``[B]``: the adjoint solve's).  An instance whose adjoint is not
    positive definite gets NaN in its own rows and in every sum that contains it.

    ``dtype``: ``None`` or ``torch.float32`` is ``tfmpc_tvlqr_box_vjp_f32``; float64 inputs are cast to fp32.
    ``torch.float64`` keeps operands, bounds, the trajectory and the upstream gradients in double, with no pass through
    fp32, runs ``tfmpc_tvlqr_box_vjp_f64`` (n <= 32, value-function costates, the held set read off
    the actions' double bits) and returns float64 gradients; ``"status"`` is then the OR of both masked sweeps'."""
    if dtype not in (None, torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype!r}")
    dt = torch.float64 if dtype == torch.float64 else torch.float32
    size = 8 if dt == torch.float64 else 4
    lib = _hip.require_gpu()
    dev = next((t.device for t in (states, actions, F) if isinstance(t, torch.Tensor) and t.device.type != "cpu"),
               _hip.default_device())
    states, actions = _cast(states, dev, dt), _cast(actions, dev, dt)
    if states.dim() == 4:
        states = states.squeeze(-1)
    if actions.dim() == 4:
        actions = actions.squeeze(-1)
    if states.dim() != 3 or actions.dim() != 3 or states.shape[1] != actions.shape[1] + 1 or states.shape[0] != actions.shape[0]:
        raise ValueError(f"states must be [B, T+1, n] and actions [B, T, m], got {tuple(states.shape)}, {tuple(actions.shape)}")
    states, actions = states.contiguous(), actions.contiguous()
    B, T, n, m = states.shape[0], actions.shape[1], states.shape[2], actions.shape[2]
    if T < 1:
        raise ValueError("the horizon must be at least 1 step")
    d = n + m
    if m > 32:
        raise ValueError("tvlqr_box_vjp serves at most 32 controls (one held-set word per step)")
    if (C_final is None) != (c_final is None):
        raise ValueError("give both C_final and c_final, or neither")
    ops = {}
    for name, a, inner in (("F", F, (n, d)), ("f", f, (n,)), ("C", C, (d, d)), ("c", c, (d,))):
        ops[name] = _timed(_cast(a, dev, dt), inner, name, B, T)
    for name, a in (("low", low), ("high", high)):
        ops[name] = _bound(_cast(a, dev, dt), m, name, B, T)
    if C_final is not None:
        Cf, cf = _cast(C_final, dev, dt), _cast(c_final, dev, dt)
        if cf.dim() >= 2 and cf.shape[-1] == 1 and cf.shape[-2] == n:
            cf = cf.squeeze(-1)
        if Cf.dim() not in (2, 3) or tuple(Cf.shape[-2:]) != (n, n) or cf.dim() not in (1, 2) or cf.shape[-1] != n:
            raise ValueError(f"C_final must be [n, n] or [B, n, n] and c_final [n] or [B, n], got {tuple(Cf.shape)}, {tuple(cf.shape)}")
        ops["C_final"] = (Cf.contiguous(), n * n if Cf.dim() == 3 else 0, 0)
        ops["c_final"] = (cf.contiguous(), n if cf.dim() == 2 else 0, 0)
    if want is None:
        want = tuple(ops) + ("x0",)
    unknown = [k for k in want if k not in NAMES or (k != "x0" and k not in ops)]
    if unknown:
        raise ValueError(f"cannot give the gradient of {unknown}: not an operand of this call")
    alloc = torch.zeros if B == 0 else torch.empty
    grads = {k: alloc(ops[k][0].shape, dtype=dt, device=dev) for k in want if k != "x0"}
    if "x0" in want:
        grads["x0"] = alloc((B, n), dtype=dt, device=dev)

    def out3(k):
        return [_hip.ptr(grads[k]), ops[k][1], ops[k][2]] if k in grads else [None, 0, 0]

    def out2(k, sb):
        return [_hip.ptr(grads[k]), sb] if k in grads else [None, 0]

    model = []
    for k in ("F", "f", "C", "c"):
        model += [_hip.ptr(ops[k][0]), ops[k][1], ops[k][2]]
    if C_final is None:
        model += [None, 0, None, 0]
    else:
        model += [_hip.ptr(ops["C_final"][0]), ops["C_final"][1], _hip.ptr(ops["c_final"][0]), ops["c_final"][1]]
    bounds = []
    for k in ("low", "high"):
        bounds += [_hip.ptr(ops[k][0]), ops[k][1], ops[k][2]]
    ups = []
    for g, ref in ((g_states, states), (g_actions, actions), (g_costs, states[..., 0])):
        ups.append(None if g is None else _cast(g, dev, dt).reshape(ref.shape).contiguous())
    outs = out3("F") + out3("f") + out3("C") + out3("c")
    outs += out2("C_final", ops["C_final"][1] if C_final is not None else 0)
    outs += out2("c_final", ops["c_final"][1] if C_final is not None else 0) + out2("x0", n)
    outs += out3("low") + out3("high")
    mask = torch.zeros((B, T), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    query, vjp, name = ((lib.tfmpc_tvlqr_box_vjp_workspace_bytes_f64, lib.tfmpc_tvlqr_box_vjp_f64, "tfmpc_tvlqr_box_vjp_f64")
                        if dt == torch.float64 else
                        (lib.tfmpc_tvlqr_box_vjp_workspace_bytes, lib.tfmpc_tvlqr_box_vjp_f32, "tfmpc_tvlqr_box_vjp_f32"))
    ws_bytes = int(query(B, n, m, T))
    ws = torch.empty((max(ws_bytes, size) + size - 1) // size, dtype=dt, device=dev)
    rc = vjp(B, n, m, T, *model, *bounds, _hip.ptr(states), _hip.ptr(actions), *(_hip.ptr(u) for u in ups), *outs,
             _hip.ptr(mask), _hip.ptr(status), _hip.ptr(ws), ws.numel() * size, _hip.stream())
    _hip.check(rc, name)
    grads["clamped"] = (mask.unsqueeze(-1) >> torch.arange(m, device=dev, dtype=torch.int32)) & 1 != 0
    grads["status"] = status
    return grads


class BoxLQRInfo:
    """What a :func:`box_lqr_solve` call leaves behind: ``last_status`` and ``last_iterations`` of the forward (per
    instance), ``last_grad_status`` of the backward pass once it ran, ``last_clamped`` its held set."""

    def __init__(self):
        self.last_status = self.last_iterations = self.last_grad_status = self.last_clamped = None
        self.batched = None          # did the problem carry a batch axis?


class BoxLQRResult(tuple):
    """``(states, actions, costs)`` with the call's :class:`BoxLQRInfo` as ``.info``."""

    def __new__(cls, tensors, info):
        self = super().__new__(cls, tensors)
        self.info = info
        return self


def _run_forward(info, F, f, C, c, x0, low, high, T, u_init, options):
    from tfmpc.envs.lq import LQEnv
    from tfmpc.solvers.ilqr import iLQR
    lo, hi = (float(b) if b.numel() == 1 else b.detach().cpu().numpy().reshape(-1, 1) for b in (low, high))
    solver = iLQR(LQEnv(F.detach(), f.detach(), C.detach(), c.detach(), lo, hi), **options)
    out = solver.solve_device(x0.detach(), T, u_init=u_init)
    info.last_status, info.last_iterations, info.batched = out["status"], out["iterations"], out["batched"]
    return out


class BoxSolveFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, call, F, f, C, c, x0, low, high):
        out = call["run"](F, f, C, c, x0, low, high)
        states, actions = out["states"], out["actions"]
        ctx.call = call
        ctx.ops = (F, f, C, c, low, high)                 # operands (not outputs): plain references
        ctx.x0_shape = x0.shape
        ctx.save_for_backward(states, actions)
        return states, actions, out["costs"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_states, g_actions, g_costs):
        states, actions = ctx.saved_tensors
        F, f, C, c, low, high = ctx.ops
        n, m = states.shape[2], actions.shape[2]
        names = ("F", "f", "C", "c", "x0", "low", "high")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad[1:]) if need)
        t1 = lambda a, k: a.unsqueeze(-k - 1)                                          # noqa: E731  a time axis of 1
        fv, cv = (a.squeeze(-1) if a.dim() >= 2 and a.shape[-1] == 1 and a.shape[-2] == size else a
                  for a, size in ((f, n), (c, n + m)))
        got = tvlqr_box_vjp(t1(F, 2), t1(fv, 1), t1(C, 2), t1(cv, 1), low.reshape(-1).expand(m), high.reshape(-1).expand(m),
                            states, actions, g_states, g_actions, g_costs, want=want)
        ctx.call["info"].last_grad_status = got["status"]
        ctx.call["info"].last_clamped = got["clamped"]
        res = []
        for k, op in zip(names, (F, f, C, c, None, low, high)):
            if k not in want:
                res.append(None)
            elif k == "x0":
                g = got[k]
                res.append(g.reshape(ctx.x0_shape) if g.numel() == int(np.prod(ctx.x0_shape)) else g.sum(0).reshape(ctx.x0_shape))
            elif k in ("low", "high"):                      # [1, m] -> the operand's shape (a scalar bound: the sum)
                g = got[k].reshape(-1)
                res.append(g.sum().reshape(op.shape) if op.numel() == 1 and m > 1 else g.reshape(op.shape))
            else:
                res.append(got[k].reshape(op.shape))
        return (None, *res)


def box_lqr_solve(F, f, C, c, x0, low, high, T, u_init=None, **ilqr_options):
    """Solve the control-limited LQ problem ``min sum_t 1/2 z_t^T C z_t + c^T z_t + 1/2 x_T^T C[:n,:n] x_T + c[:n]^T x_T``,
    ``x_{t+1} = F z_t + f``, ``low <= u_t <= high`` from ``x0`` over ``T`` steps and return ``(states, actions, costs)``
    as tensors -- ``states[(B,)T+1,n,1]``, ``actions[(B,)T,m,1]``, ``costs[(B,)T+1,1,1]`` as
    :func:`tfmpc.solvers.tvlqr_solve` -- differentiable with respect to ``F``, ``f``, ``C``, ``c``, ``x0``, ``low`` and
    ``high``.  The result also carries ``.info`` (:class:`BoxLQRInfo`).

    Forward: the control-limited iLQR launch ``iLQR(LQEnv(F, f, C, c, low, high), **ilqr_options).solve_device`` on
    detached operands, unchanged, so the values are bit for bit that solver's.  It serves a time-invariant model
    (``F[n, d]`` or ``F[B, n, d]``, likewise ``f``, ``C``, ``c``) and finite bounds shared by the batch (a scalar, ``[m]``
    or ``[m, 1]``); anything else raises ``ValueError``.  ``u_init=None`` starts from zeros clipped into the box, so
    the call is deterministic.  Backward: :func:`tvlqr_box_vjp` on the saved states and actions.

    The gradient is that of the OPTIMUM: it is exact only where the forward converged, and its error grows with the
    distance between the returned trajectory and the optimum.  The solver's default ``atol = 5e-3`` is a stopping
    rule for control, not for learning: pass ``atol=1e-6`` or thereabouts when the gradient matters.  Controls on a
    bound are held in the backward pass whatever their multiplier (see the module docstring).  Double backward is not
    supported."""
    operands = (F, f, C, c, x0, low, high)
    dev = next((t.device for t in operands if isinstance(t, torch.Tensor) and t.device.type != "cpu"), _hip.default_device())
    Ft, ft, Ct, ct, xt, lo, hi = (as_f32_graph(a, dev) for a in operands)
    if Ft.dim() not in (2, 3):
        raise ValueError(f"box_lqr_solve serves a time-invariant model: F must be [n, d] or [B, n, d], got {tuple(Ft.shape)} "
                         "(a control-limited forward for time-varying models does not exist; tvlqr_box_vjp has the gradient)")
    n, d = Ft.shape[-2], Ft.shape[-1]
    m = d - n
    if m < 1:
        raise ValueError(f"F must end in [n, n+m] with m > 0, got {tuple(Ft.shape)}")
    if Ct.dim() != Ft.dim() or tuple(Ct.shape[-2:]) != (d, d):
        raise ValueError(f"C must be [d, d] or [B, d, d] like F, got {tuple(Ct.shape)}")
    for name, b in (("low", lo), ("high", hi)):
        if b.numel() not in (1, m) or b.dim() > 2 or (b.dim() == 2 and b.shape[-1] != 1):
            raise ValueError(f"box_lqr_solve serves bounds shared by the batch: {name} must be a scalar, [m] or [m, 1], got "
                             f"{tuple(b.shape)}")
        if not bool(torch.isfinite(b).all()):
            raise ValueError(f"box_lqr_solve serves finite bounds: {name} has an infinite or NaN entry")
    T = int(T)
    if u_init is None:
        u_init = torch.zeros((T, m), device=dev).clamp(lo.detach().reshape(-1), hi.detach().reshape(-1))
    info = BoxLQRInfo()

    def run(F_, f_, C_, c_, x0_, lo_, hi_):
        return _run_forward(info, F_, f_, C_, c_, x0_, lo_, hi_, T, u_init, ilqr_options)

    if wants_grad(*operands):
        states, actions, costs = BoxSolveFunction.apply(dict(run=run, info=info), Ft, ft, Ct, ct, xt, lo, hi)
        batched = info.batched
    else:
        out = run(Ft, ft, Ct, ct, xt, lo, hi)
        states, actions, costs, batched = out["states"], out["actions"], out["costs"], out["batched"]
    costs = costs.reshape(*costs.shape, 1, 1)
    if not batched:
        states, actions, costs = states[0], actions[0], costs[0]
    return BoxLQRResult((states, actions, costs), info)


__all__ = ["BoxLQRInfo", "BoxLQRResult", "BoxSolveFunction", "box_lqr_solve", "tvlqr_box_vjp"]

"""Control-limited time-varying LQR: ``tfmpc_tvlqr_box_solve_f32`` (include/tfmpc_hip.h), the forward
of :func:`tfmpc.solvers.tvlqr_box_vjp`, and its double-precision twin ``tfmpc_tvlqr_box_solve_f64`` (DESIGN.md §3.18,
``dtype=torch.float64``: n <= 32; gradients on request, ``differentiable=True``, through ``tfmpc_tvlqr_box_vjp_f64``, §3.20).

The problem of :class:`tfmpc.solvers.TimeVaryingLQR` under ``low <= u_t <= high``: a convex QP with an exact model,
solved per instance by control-limited Newton sweeps without regularisation.  Models may vary in time and by instance,
bounds per instance and per step, and there is no horizon cap.  The result is differentiable through
``tfmpc_tvlqr_box_vjp_f32``: a control on a bound carries the bound's bits, which is what the VJP's held-set rule reads.
"""

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from tfmpc import _hip
from tfmpc.solvers.box_lqr_grad import BoxLQRInfo, BoxLQRResult, tvlqr_box_vjp
from tfmpc.solvers.tvlqr_grad import as_graph, wants_grad

GRAD_NAMES = ("F", "f", "C", "c", "x0", "low", "high", "C_final", "c_final")


def _timed(t, inner, name):
    """``[T|1, *inner]`` or ``[B|1, T|1, *inner]`` (a trailing column axis of 1 on a vector dropped) -> the tensor with
    exactly those axes, or ``ValueError``."""
    k = len(inner)
    if k == 1 and t.dim() >= 3 and t.shape[-1] == 1 and t.shape[-2] == inner[0]:
        t = t.squeeze(-1)
    if t.dim() not in (k + 1, k + 2) or tuple(t.shape[-k:]) != tuple(inner):
        raise ValueError(f"{name} must be [T|1, {', '.join(map(str, inner))}] with an optional leading batch axis, got "
                         f"{tuple(t.shape)}")
    return t


def _bound(t, m, name):
    """A scalar, ``[m]``, ``[T|1, m]`` or ``[B|1, T|1, m]`` -> one of the last two."""
    if t.dim() == 0:
        t = t.expand(m)
    if t.dim() == 1:
        if t.shape[0] != m:
            raise ValueError(f"{name} must be a scalar, [m], [T, m] or [B, T, m] with m = {m}, got {tuple(t.shape)}")
        t = t.unsqueeze(0)
    return _timed(t, (m,), name)


def _strided(t, k, batched):
    """The operand as the launch reads it: (tensor to keep alive, batch stride, time stride) in elements.  A view whose
    per-step block is dense row-major is kept (an axis of 1 or an expanded axis: stride 0, no copy)."""
    t = t.detach()
    dense, run = True, 1
    for ax in range(t.dim() - 1, t.dim() - 1 - k, -1):
        dense &= t.shape[ax] == 1 or t.stride(ax) == run
        run *= t.shape[ax]
    if not dense:
        t = t.contiguous()
    time_ax = t.dim() - k - 1
    st = t.stride(time_ax) if t.shape[time_ax] > 1 else 0
    sb = t.stride(0) if batched and t.shape[0] > 1 else 0
    return t, sb, st


class _Call:
    """The launch of one ``tvlqr_box_solve`` call: sizes, options and the :class:`BoxLQRInfo` it fills."""

    def __init__(self, B, T, n, m, u_init, max_iter, tol, info, device, dtype=torch.float32):
        self.B, self.T, self.n, self.m = B, T, n, m
        self.u_init, self.max_iter, self.tol, self.info, self.device = u_init, max_iter, tol, info, device
        self.dtype = dtype

    def launch(self, F, f, C, c, x0, low, high, Cf, cf):
        lib = _hip.require_gpu()
        B, T, n, m, dev, dt = self.B, self.T, self.n, self.m, self.device, self.dtype
        double = dt == torch.float64
        keep, model = [], []
        for t, k in ((F, 2), (f, 1), (C, 2), (c, 1)):
            t, sb, st = _strided(t, k, t.dim() == k + 2)
            keep.append(t)
            model += [_hip.ptr(t), sb, st]
        if Cf is None:
            model += [None, 0, None, 0]
        else:
            Cf, cf = Cf.detach().contiguous(), cf.detach().contiguous()
            keep += [Cf, cf]
            model += [_hip.ptr(Cf), n * n if Cf.dim() == 3 and Cf.shape[0] > 1 else 0,
                      _hip.ptr(cf), n if cf.dim() == 2 and cf.shape[0] > 1 else 0]
        bounds = []
        for t in (low, high):
            t, sb, st = _strided(t, 1, t.dim() == 3)
            keep.append(t)
            bounds += [_hip.ptr(t), sb, st]
        x0 = x0.detach().contiguous()
        u_init = self.u_init
        su = 0 if u_init is None or u_init.dim() == 2 else T * m
        alloc = torch.zeros if B == 0 else torch.empty
        states = alloc((B, T + 1, n), dtype=dt, device=dev)
        actions = alloc((B, T, m), dtype=dt, device=dev)
        costs = alloc((B, T + 1), dtype=dt, device=dev)
        iterations, status, reason = (torch.zeros((B,), dtype=torch.int32, device=dev) for _ in range(3))
        mask = torch.zeros((B, T), dtype=torch.int32, device=dev)
        size = 8 if double else 4
        query = lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64 if double else lib.tfmpc_tvlqr_box_solve_workspace_bytes
        solve, name = ((lib.tfmpc_tvlqr_box_solve_f64, "tfmpc_tvlqr_box_solve_f64") if double else
                       (lib.tfmpc_tvlqr_box_solve_f32, "tfmpc_tvlqr_box_solve_f32"))
        ws_bytes = int(query(B, n, m, T))
        ws = torch.empty((max(ws_bytes, size) + size - 1) // size, dtype=dt, device=dev)
        rc = solve(B, n, m, T, *model, *bounds, _hip.ptr(x0), _hip.ptr(u_init), su, self.max_iter, self.tol,
                   _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs), _hip.ptr(iterations), _hip.ptr(status),
                   _hip.ptr(reason), _hip.ptr(mask), _hip.ptr(ws), ws.numel() * size, _hip.stream())
        _hip.check(rc, name)
        info = self.info
        info.last_status, info.last_iterations, info.last_reason = status, iterations, reason
        info.last_clamped = (mask.unsqueeze(-1) >> torch.arange(m, device=dev, dtype=torch.int32)) & 1 != 0
        return states, actions, costs


class TvBoxSolveFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, call, F, f, C, c, x0, low, high, Cf, cf):
        states, actions, costs = call.launch(F, f, C, c, x0, low, high, Cf, cf)
        ctx.call = call
        ctx.ops = (F, f, C, c, low, high, Cf, cf)         # operands (not outputs): plain references
        ctx.save_for_backward(states, actions)
        return states, actions, costs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_states, g_actions, g_costs):
        states, actions = ctx.saved_tensors
        F, f, C, c, low, high, Cf, cf = ctx.ops
        want = tuple(k for k, need in zip(GRAD_NAMES, ctx.needs_input_grad[1:]) if need)
        got = tvlqr_box_vjp(F, f, C, c, low, high, states, actions, g_states, g_actions, g_costs, C_final=Cf, c_final=cf,
                            want=want, dtype=ctx.call.dtype)
        info = ctx.call.info
        info.last_grad_status, info.last_clamped = got["status"], got["clamped"]
        shapes = dict(zip(GRAD_NAMES, (F, f, C, c, states[:, 0], low, high, Cf, cf)))
        return (None, *(got[k].reshape(shapes[k].shape) if k in want else None for k in GRAD_NAMES))


def tvlqr_box_solve(F, f, C, c, x0, low, high, C_final=None, c_final=None, u_init=None, max_iter=None, tol=None,
                    dtype=None, differentiable=False):
    """Solve ``min sum_t 1/2 z_t^T C_t z_t + c_t^T z_t + 1/2 x_T^T C_fin x_T + c_fin^T x_T``, ``x_{t+1} = F_t z_t + f_t``,
    ``low_t <= u_t <= high_t`` from ``x0`` and return ``(states, actions, costs)`` -- ``states[(B,)T+1,n,1]``,
    ``actions[(B,)T,m,1]``, ``costs[(B,)T+1,1,1]`` as :func:`tfmpc.solvers.box_lqr_solve` -- with ``.info``
    (:class:`~tfmpc.solvers.box_lqr_grad.BoxLQRInfo`: ``last_status`` (of the last sweep), ``last_iterations``
    (backward sweeps run), ``last_reason`` (0 converged by the step norm, 1 no step lowered the cost, 2 the pass cap, 3 flagged) and
    ``last_clamped``, the last sweep's held sets ``[B, T, m]``).

    Operands as :func:`tfmpc.solvers.tvlqr_solve`: ``F[T, n, d]`` or ``[B, T, n, d]``, likewise ``f``, ``C``, ``c`` (vectors
    with an optional trailing column axis); the time axis is required, and an axis of 1 or an expanded axis is read with
    stride 0, without a copy.  ``low`` / ``high``: a scalar, ``[m]``, ``[T, m]`` or ``[B, T, m]``, ±inf allowed.  ``C_final``
    ``[n, n]`` / ``[B, n, n]`` and ``c_final`` ``[n]`` / ``[B, n]`` default to ``C_{T-1}[:n,:n]``, ``c_{T-1}[:n]``.  ``u_init``
    (``[T, m]`` or ``[B|1, T, m]``, default zeros) is clipped into the box.  ``max_iter`` (default 100) caps the passes,
    ``tol`` (default 4e-6) is the stop rule ``max |k| <= tol max(1, max |u|)``; the sweep that meets it still has its
    step applied, so the result is not left a ``tol`` short of the optimum.  ``C_t`` symmetric positive semidefinite
    with ``C_t,uu`` positive definite is the precondition; an instance that breaks it is flagged in ``last_status`` and
    gets NaN in its own rows.

    When autograd is recording and an operand, a bound or ``x0`` requires grad, the result is in the autograd graph:
    gradients for ``F, f, C, c, x0, low, high, C_final, c_final`` in the operands' own shapes through
    :func:`tfmpc.solvers.tvlqr_box_vjp` on the returned trajectory (once differentiable; exact where the forward
    converged).  Shape or bound errors (``low > high``, NaN bounds) raise ``ValueError`` before any launch.

    ``dtype``: ``None`` or ``torch.float32`` is the fp32 kernel; float64 inputs are cast to fp32, silently.
    ``torch.float64`` keeps tensor and numpy operands, bounds, ``x0``, ``u_init`` and the final cost in double, with no
    pass through fp32, runs ``tfmpc_tvlqr_box_solve_f64`` (n <= 32, ``tol`` defaults to 1e-12) and
    returns float64 tensors; a held control carries the double bound's bits.  Double gradients are opt-in: with
    ``torch.float64`` an operand that requires grad raises ``NotImplementedError`` unless ``differentiable=True``, which
    runs the same forward on the detached operands (the same trajectory, bit for bit) and puts the result in the graph
    with ``tvlqr_box_vjp(dtype=torch.float64)`` as its backward (once differentiable).  With ``dtype``
    fp32 or ``None`` the flag changes nothing."""
    if dtype not in (None, torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype!r}")
    dt = torch.float64 if dtype == torch.float64 else torch.float32
    given = (F, f, C, c, x0, low, high, C_final, c_final)
    if dt == torch.float64 and not differentiable and wants_grad(*given):
        raise NotImplementedError("gradients of the control-limited time-varying LQR in double are opt-in: pass "
                                  "differentiable=True for the double box VJP, call with dtype=torch.float32, or detach "
                                  "the operands, bounds and x0 for a dtype=torch.float64 solve")
    dev = next((t.device for t in given if isinstance(t, torch.Tensor) and t.device.type != "cpu"), _hip.default_device())
    if (C_final is None) != (c_final is None):
        raise ValueError("give both C_final and c_final, or neither")
    Ft, ft, Ct, ct, xt, lo, hi = (as_graph(a, dev, dt) for a in given[:7])
    if Ft.dim() not in (3, 4):
        raise ValueError(f"F must be [T, n, d] or [B, T, n, d], got {tuple(Ft.shape)}")
    n, d = Ft.shape[-2], Ft.shape[-1]
    m = d - n
    if not 0 < n < d:
        raise ValueError(f"F must end in [n, n+m] with m > 0, got {tuple(Ft.shape)}")
    if m > 32:
        raise ValueError("tvlqr_box_solve serves at most 32 controls (one held-set word per step)")
    ops = dict(F=_timed(Ft, (n, d), "F"), f=_timed(ft, (n,), "f"), C=_timed(Ct, (d, d), "C"), c=_timed(ct, (d,), "c"),
               low=_bound(lo, m, "low"), high=_bound(hi, m, "high"))
    inner = dict(F=2, f=1, C=2, c=1, low=1, high=1)
    if u_init is not None:
        u_init = as_graph(u_init, dev, dt).detach()
        if u_init.dim() >= 3 and u_init.shape[-1] == 1 and u_init.shape[-2] == m:
            u_init = u_init.squeeze(-1)
        if u_init.dim() not in (2, 3) or u_init.shape[-1] != m:
            raise ValueError(f"u_init must be [T, m] or [B, T, m] with m = {m}, got {tuple(u_init.shape)}")
        u_init = u_init.contiguous()
    horizons = {t.shape[-inner[k] - 1] for k, t in ops.items()} - {1}
    if u_init is not None:
        horizons.add(u_init.shape[-2])
    if len(horizons) > 1:
        raise ValueError(f"time axes disagree: {sorted(horizons)} (each must be 1 or the horizon T)")
    T = horizons.pop() if horizons else 1
    if xt.dim() == 1 or (xt.dim() == 2 and tuple(xt.shape) == (n, 1)):
        xt = xt.reshape(1, n)
        x_batched = False
    elif xt.dim() in (2, 3) and xt.shape[1] == n and (xt.dim() == 2 or xt.shape[2] == 1):
        xt = xt.reshape(xt.shape[0], n)
        x_batched = True
    else:
        raise ValueError(f"x0 must be [n], [n, 1], [B, n] or [B, n, 1] with n = {n}, got {tuple(xt.shape)}")
    Cf = cf = None
    if C_final is not None:
        Cf, cf = as_graph(C_final, dev, dt), as_graph(c_final, dev, dt)
        if cf.dim() >= 2 and cf.shape[-1] == 1 and cf.shape[-2] == n:
            cf = cf.squeeze(-1)
        if Cf.dim() not in (2, 3) or tuple(Cf.shape[-2:]) != (n, n) or cf.dim() not in (1, 2) or cf.shape[-1] != n:
            raise ValueError(f"C_final must be [n, n] or [B, n, n] and c_final [n] or [B, n], got {tuple(Cf.shape)}, "
                             f"{tuple(cf.shape)}")
    batch_axes = [t.shape[0] for k, t in ops.items() if t.dim() == inner[k] + 2]
    batch_axes += [xt.shape[0]] if x_batched else []
    batch_axes += [t.shape[0] for t, k in ((Cf, 2), (cf, 1)) if t is not None and t.dim() == k + 1]
    batch_axes += [u_init.shape[0]] if u_init is not None and u_init.dim() == 3 else []
    sizes = set(batch_axes) - {1}
    if len(sizes) > 1:
        raise ValueError(f"batch axes disagree: {sorted(sizes)}")
    batched = bool(batch_axes)
    B = sizes.pop() if sizes else 1
    if u_init is not None and u_init.dim() == 3 and u_init.shape[0] == 1 and B > 1:
        u_init = u_init[0]                                  # a batch axis of 1 beside a larger batch: one start for all
    if u_init is not None and (u_init.shape[-2] != T or (u_init.dim() == 3 and u_init.shape[0] != B)):
        raise ValueError(f"u_init must be [T, m] or [B, T, m] with T = {T}, B = {B}, got {tuple(u_init.shape)}")
    # a batch axis of 1 beside a larger batch: the operand is shared (the VJP then sums its gradient)
    for k, t in ops.items():
        if t.dim() == inner[k] + 2 and t.shape[0] == 1 and B > 1:
            ops[k] = t.squeeze(0)
    if Cf is not None:
        Cf = Cf.squeeze(0) if Cf.dim() == 3 and Cf.shape[0] == 1 and B > 1 else Cf
        cf = cf.squeeze(0) if cf.dim() == 2 and cf.shape[0] == 1 and B > 1 else cf
    with torch.no_grad():
        l, h = ops["low"], ops["high"]
        if bool(torch.isnan(l).any()) or bool(torch.isnan(h).any()):
            raise ValueError("low and high must not hold NaN")
        if bool((l > h).any()):
            raise ValueError("low must not exceed high")
    max_iter = 0 if max_iter is None else int(max_iter)
    tol = 0.0 if tol is None else float(tol)
    if max_iter < 0 or not tol >= 0.0:
        raise ValueError(f"max_iter and tol must not be negative (0 or None: the defaults), got {max_iter}, {tol}")
    xt = xt.expand(B, n)
    info = BoxLQRInfo()
    info.last_reason = None
    info.batched = batched
    call = _Call(B, T, n, m, u_init, max_iter, tol, info, dev, dt)
    args = (ops["F"], ops["f"], ops["C"], ops["c"], xt, ops["low"], ops["high"], Cf, cf)
    if wants_grad(*given):
        states, actions, costs = TvBoxSolveFunction.apply(call, *args)
    else:
        states, actions, costs = call.launch(*args)
    states, actions, costs = states.unsqueeze(-1), actions.unsqueeze(-1), costs.reshape(*costs.shape, 1, 1)
    if not batched:
        states, actions, costs = states[0], actions[0], costs[0]
    return BoxLQRResult((states, actions, costs), info)


__all__ = ["TvBoxSolveFunction", "tvlqr_box_solve"]

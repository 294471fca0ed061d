"""Differentiable LQR solves: a ``torch.autograd.Function`` over ``tfmpc_tvlqr_solve_f32`` (or ``LQR``'s own solve) and
``tfmpc_tvlqr_vjp_f32`` (include/tfmpc_hip.h), and its double-precision twin over
``tfmpc_tvlqr_solve_f64`` and ``tfmpc_tvlqr_vjp_f64``, which also saves the forward's ``v``.  A third
Function stands over the time-parallel double solve and its segmented adjoint (``tfmpc_tvlqr_solve_time_parallel_f64``,
``tfmpc_tvlqr_vjp_time_parallel_f64``): it saves the forward's ``K, V, v`` too, and its backward
repeats no Riccati step.

The backward pass is one more time-varying LQR solve (the adjoint) plus a costate sweep; it needs the forward
trajectory only, which is what the Function saves.  Each gradient has the shape of its operand: an operand without a
batch axis (shared by the batch) gets the gradient summed over the batch, a time axis of size 1 (or an ``LQR``
operand, which has none) the gradient summed over time.

``C`` and ``C_final`` enter the kernels only as symmetric matrices, so their gradients are the symmetric ones: an fp64
autograd oracle through a general-matrix recursion matches after ``(G + G^T) / 2``.  An instance whose solve is not
positive definite gets NaN in its own gradient rows and in every gradient summed over a batch that contains it
(``last_grad_status`` on the solver holds the per-instance status of the backward pass).  Double backward is not
supported.
"""

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from tfmpc import _hip
from tfmpc.utils import trajectory


def wants_grad(*operands):
    """True when autograd is recording and some operand is a tensor that requires grad."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in operands)


def as_graph(a, device, dtype):
    """Like ``lqr._as_f32`` / ``tvlqr._as_dtype`` but without ``detach``: a dtype / device conversion stays in the autograd
    graph."""
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype)
    return torch.as_tensor(np.asarray(a, dtype=np.float64 if dtype == torch.float64 else np.float32), device=device)


def as_f32_graph(a, device):
    return as_graph(a, device, torch.float32)


class Problem:
    """What the Function needs besides tensors: ``run(x0)`` -> the forward's ``solve_device`` dict (batched outputs),
    ``model()`` -> the :class:`TimeVaryingLQR` whose ``_model_args`` the VJP reads, ``timed`` (operands carry a time
    axis) and ``owner`` (receives ``last_grad_status``); for the time-parallel solve also ``vjp_segments(B, segments)`` ->
    the backward's segment count from the forward's."""

    def __init__(self, run, model, timed, owner, vjp_segments=None):
        self.run, self.model, self.timed, self.owner, self.vjp_segments = run, model, timed, owner, vjp_segments


def grad_strides(g, ndim_batched, timed):
    """(batch stride, time stride) of a contiguous gradient buffer ``g`` (``None``: no gradient, (0, 0)); 0 = summed over
    that axis."""
    if g is None:
        return 0, 0
    batched = g.dim() == ndim_batched
    sb = g[0].numel() if batched and g.shape[0] > 0 else 0
    st = 0
    if timed and g.shape[-3] > 1:
        st = g.shape[-2] * g.shape[-1]
    return sb, st


def alloc_grads(shapes, needed, Bk, device, dtype=torch.float32):
    """One buffer (fp32 by default) per operand shape whose gradient is needed, else ``None`` (also for an absent operand,
    shape ``None``).  Zeros over an empty batch, where no kernel writes."""
    alloc = torch.zeros if Bk == 0 else torch.empty
    return [alloc(shape, device=device, dtype=dtype) if need and shape is not None else None
            for shape, need in zip(shapes, needed)]


class SolveFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, problem, x0, F, f, C, c, C_final, c_final):
        out = problem.run(x0.detach())
        states, actions = out["states"], out["actions"]
        ctx.problem = problem
        ctx.meta = [(t.shape if t is not None else None) for t in (x0, F, f, C, c, C_final, c_final)]
        ctx.save_for_backward(states, actions)
        return states, out["actions"], out["costs"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_states, g_actions, g_costs):
        states, actions = ctx.saved_tensors
        problem = ctx.problem
        tv = problem.model()
        lib = _hip.require_gpu()
        Bk, T1, n = states.shape[0], states.shape[1], states.shape[2]
        T, m = T1 - 1, actions.shape[2]
        dev = states.device
        nd_model = 4 if problem.timed else 3
        gx0, gF, gf, gC, gc, gCf, gcf = alloc_grads(ctx.meta, ctx.needs_input_grad[1:], Bk, dev)
        args = []
        for g in (gF, gf, gC, gc):
            args += [_hip.ptr(g), *grad_strides(g, nd_model, problem.timed)]
        for g in (gCf, gcf, gx0):
            args += [_hip.ptr(g), grad_strides(g, 3, False)[0]]
        ups = [None if g is None else g.to(torch.float32).contiguous() for g in (g_states, g_actions, g_costs)]
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        ws_bytes = int(lib.tfmpc_tvlqr_vjp_workspace_bytes(Bk, n, m, T))
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
        rc = lib.tfmpc_tvlqr_vjp_f32(Bk, n, m, T, *tv._model_args(), _hip.ptr(states), _hip.ptr(actions),
                                     *(_hip.ptr(u) for u in ups), *args, _hip.ptr(status), _hip.ptr(ws),
                                     ws.numel() * 4, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_vjp_f32")
        problem.owner.last_grad_status = status
        return (None, gx0, gF, gf, gC, gc, gCf, gcf)


class SolveFunctionF64(torch.autograd.Function):
    """``SolveFunction`` in double: the forward asks the solve for ``v`` as well (``problem.run`` returns it) and saves
    it, the backward keeps upstream gradients, gradients and workspace in fp64 and calls ``tfmpc_tvlqr_vjp_f64``."""

    @staticmethod
    def forward(ctx, problem, x0, F, f, C, c, C_final, c_final):
        out = problem.run(x0.detach())
        ctx.problem = problem
        ctx.meta = [(t.shape if t is not None else None) for t in (x0, F, f, C, c, C_final, c_final)]
        ctx.save_for_backward(out["states"], out["actions"], out["v"])
        return out["states"], out["actions"], out["costs"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_states, g_actions, g_costs):
        states, actions, v = ctx.saved_tensors
        problem = ctx.problem
        tv = problem.model()
        lib = _hip.require_gpu()
        Bk, T1, n = states.shape[0], states.shape[1], states.shape[2]
        T, m = T1 - 1, actions.shape[2]
        dev, f64 = states.device, torch.float64
        nd_model = 4 if problem.timed else 3
        gx0, gF, gf, gC, gc, gCf, gcf = alloc_grads(ctx.meta, ctx.needs_input_grad[1:], Bk, dev, f64)
        args = []
        for g in (gF, gf, gC, gc):
            args += [_hip.ptr(g), *grad_strides(g, nd_model, problem.timed)]
        for g in (gCf, gcf, gx0):
            args += [_hip.ptr(g), grad_strides(g, 3, False)[0]]
        ups = [None if g is None else g.to(f64).contiguous() for g in (g_states, g_actions, g_costs)]
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        ws_bytes = int(lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(Bk, n, m, T))
        ws = torch.empty((max(ws_bytes, 8) + 7) // 8, dtype=f64, device=dev)
        rc = lib.tfmpc_tvlqr_vjp_f64(Bk, n, m, T, *tv._model_args(), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(v),
                                     *(_hip.ptr(u) for u in ups), *args, _hip.ptr(status), _hip.ptr(ws),
                                     ws.numel() * 8, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_vjp_f64")
        problem.owner.last_grad_status = status
        return (None, gx0, gF, gf, gC, gc, gCf, gcf)


def vjp_time_parallel_f64(tv, states, actions, K, V, v, ups, grads, segments):
    """One ``tfmpc_tvlqr_vjp_time_parallel_f64`` call on the model of ``tv``: the forward's batched
    ``states, actions, K, V, v``, the upstream gradients ``ups`` (three fp64 tensors or ``None``), the gradient buffers
    ``grads = (gF, gf, gC, gc, gCf, gcf, gx0)`` (``None``: not computed; a missing batch or time axis sums over it).
    Returns the per-instance status.  Never synchronises."""
    lib = _hip.require_gpu()
    Bk, T1, n = states.shape[0], states.shape[1], states.shape[2]
    T, m = T1 - 1, actions.shape[2]
    args = []
    for g in grads[:4]:
        args += [_hip.ptr(g), *grad_strides(g, 4, True)]
    for g in grads[4:]:
        args += [_hip.ptr(g), grad_strides(g, 3, False)[0]]
    status = torch.zeros((Bk,), dtype=torch.int32, device=states.device)
    ws_bytes = int(lib.tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64(Bk, n, m, T, segments))
    ws = torch.empty((max(ws_bytes, 8) + 7) // 8, dtype=torch.float64, device=states.device)
    rc = lib.tfmpc_tvlqr_vjp_time_parallel_f64(Bk, n, m, T, *tv._model_args(), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(v),
                                               _hip.ptr(K), _hip.ptr(V), *(_hip.ptr(u) for u in ups), *args, _hip.ptr(status),
                                               segments, _hip.ptr(ws), ws.numel() * 8, _hip.stream())
    _hip.check(rc, "tfmpc_tvlqr_vjp_time_parallel_f64")
    return status


class SolveTimeParallelFunctionF64(torch.autograd.Function):
    """``SolveFunctionF64`` over the time-parallel solve: the forward asks it for ``K, k, V, v``
    (``problem.run`` returns them and the resolved ``segments``) and saves ``states, actions, K, V, v``; the backward calls
    ``tfmpc_tvlqr_vjp_time_parallel_f64`` with ``problem.vjp_segments(B, segments)`` segments."""

    @staticmethod
    def forward(ctx, problem, x0, F, f, C, c, C_final, c_final):
        out = problem.run(x0.detach())
        ctx.problem = problem
        ctx.segments = out["segments"]
        ctx.meta = [(t.shape if t is not None else None) for t in (x0, F, f, C, c, C_final, c_final)]
        ctx.save_for_backward(out["states"], out["actions"], out["K"], out["V"], out["v"])
        return out["states"], out["actions"], out["costs"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_states, g_actions, g_costs):
        states, actions, K, V, v = ctx.saved_tensors
        problem = ctx.problem
        f64 = torch.float64
        gx0, gF, gf, gC, gc, gCf, gcf = alloc_grads(ctx.meta, ctx.needs_input_grad[1:], states.shape[0], states.device, f64)
        ups = [None if g is None else g.to(f64).contiguous() for g in (g_states, g_actions, g_costs)]
        segments = problem.vjp_segments(states.shape[0], ctx.segments)
        problem.owner.last_grad_status = vjp_time_parallel_f64(problem.model(), states, actions, K, V, v, ups,
                                                               (gF, gf, gC, gc, gCf, gcf, gx0), segments)
        return (None, gx0, gF, gf, gC, gc, gCf, gcf)


class TensorTrajectory(trajectory.Trajectory):
    """The :class:`~tfmpc.utils.trajectory.Trajectory` a differentiable ``solve`` returns: the same shapes and
    properties, but ``states``, ``actions`` and ``costs`` stay torch tensors in the autograd graph."""

    def __init__(self, states, actions, costs):
        self.states = states.squeeze(-1) if states.shape[-1] == 1 else states
        self.actions = actions.squeeze(-1) if actions.shape[-1] == 1 else actions
        while costs.dim() > self.states.dim() - 1 and costs.shape[-1] == 1:
            costs = costs.squeeze(-1)
        self.costs = costs

    @property
    def batched(self):
        return self.states.dim() == 3

    @property
    def total_cost(self):
        return self.costs.sum(-1)

    @property
    def cumulative_cost(self):
        return self.costs.cumsum(-1)

    @property
    def cost_to_go(self):
        return self.costs.flip(-1).cumsum(-1).flip(-1)

    def instance(self, b):
        if not self.batched:
            raise IndexError("not a batched trajectory")
        return TensorTrajectory(self.states[b], self.actions[b], self.costs[b])

    def detached(self):
        """The plain numpy :class:`Trajectory` of the same values."""
        return trajectory.Trajectory(self.states.detach()[..., None], self.actions.detach()[..., None], self.costs.detach())

    def __repr__(self):
        return "Tensor" + repr(self.detached())

    def __str__(self):
        return str(self.detached())

    def save(self, filepath):
        self.detached().save(filepath)


def tvlqr_solve(F, f, C, c, x0, C_final=None, c_final=None, dtype=torch.float32):
    """Solve the time-varying LQR of :class:`tfmpc.solvers.TimeVaryingLQR` (same operand shapes) from ``x0`` and
    return ``(states, actions, costs)`` as tensors -- ``states[(B,)T+1,n,1]``, ``actions[(B,)T,m,1]``,
    ``costs[(B,)T+1,1,1]`` -- differentiable with respect to every tensor operand and ``x0`` that requires grad.
    ``dtype=torch.float64``: the double-precision solve (n <= 32, m <= 32), outputs and every gradient in fp64."""
    from tfmpc.solvers.tvlqr import TimeVaryingLQR
    device = next((t.device for t in (F, f, C, c, x0) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    tv = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=device, dtype=dtype)
    return tv.solve_tensors(x0, differentiable=True)


def tvlqr_vjp_time_parallel(F, f, C, c, states, actions, K, V, v, g_states=None, g_actions=None, g_costs=None, C_final=None,
                            c_final=None, segments=None):
    """The vector-Jacobian product of the double-precision solve alone through the segmented adjoint
    (``tfmpc_tvlqr_vjp_time_parallel_f64``), for any forward: ``states, actions, K, V, v`` as a solve of
    ``(F, f, C, c, C_final, c_final)`` gave them (batched; operands that all lack the batch axis are shared by the
    trajectories' batch), ``g_states, g_actions, g_costs`` the upstream gradients (``None`` = zero).  ``segments=None`` picks
    :meth:`TimeVaryingLQR.default_vjp_segments`; 1 is ``tfmpc_tvlqr_vjp_f64``, bit for bit.  Returns ``(dF, df, dC, dc,
    dC_final, dc_final, dx0, status)``: each gradient float64 in its operand's shape as :class:`TimeVaryingLQR` holds it
    (vectors as columns; an operand without a batch axis gets the sum over the batch, a time axis of 1 the sum over time;
    ``None`` for an absent final cost, whose gradient is then in ``dC, dc`` at the last step; ``dx0`` is ``[(B,) n, 1]``)
    and the per-instance status; a flagged instance has NaN in its own gradient rows and in every sum that contains it."""
    from tfmpc.solvers.tvlqr import TimeVaryingLQR, _as_dtype
    f64 = torch.float64
    tensors = (F, f, C, c, C_final, c_final, states)
    device = next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    tv = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=device, dtype=f64)
    dev = tv.device
    n, m, T = tv.state_size, tv.action_size, tv.horizon
    states, actions, K, V, v = (_as_dtype(t, dev, f64).reshape(-1, steps, *inner).contiguous()
                                for t, steps, inner in ((states, T + 1, (n, 1)), (actions, T, (m, 1)), (K, T, (m, n)),
                                                        (V, T, (n, n)), (v, T, (n, 1))))
    Bk = tv.batch_size if tv.batch_size is not None else states.shape[0]      # a model shared by a batch of trajectories
    if any(t.shape[0] != Bk for t in (states, actions, K, V, v)):
        raise ValueError("states, actions, K, V and v must share the operands' batch size")
    ups = [None if g is None else _as_dtype(g, dev, f64).reshape(Bk, steps, *inner).contiguous()
           for g, steps, inner in ((g_states, T + 1, (n, 1)), (g_actions, T, (m, 1)), (g_costs, T + 1, (1, 1)))]
    shapes = [(t.shape if t is not None else None) for t in (tv.F, tv.f, tv.C, tv.c, tv.C_final, tv.c_final)]
    shapes.append((Bk, n, 1) if tv.batch_size is not None or Bk > 1 else (n, 1))
    grads = alloc_grads(shapes, (True,) * 7, Bk, dev, f64)
    segments = tv.default_vjp_segments(Bk) if segments is None else int(segments)
    if segments < 1:
        raise ValueError(f"segments must be at least 1, got {segments}")
    status = vjp_time_parallel_f64(tv, states, actions, K, V, v, ups, grads, segments)
    tv.last_grad_status = status
    return (*grads, status)


def periodic_vjp_f64(tv, K, k, V, v, fwd_status, ups, shapes, needed, segments, max_iter=0, tol=0.0):
    """One tfmpc_tvlqr_periodic_vjp_f64 call on the double problem ``tv``, whose time axis is one period.
    ``K, k, V, v, fwd_status``: the periodic forward's batched outputs; ``ups``: ``gK, gk, gV, gv`` (``None`` = zero, a NULL
    pointer).  One double gradient per entry of ``shapes`` (``F, f, C, c`` as the solver shapes them) that ``needed`` asks
    for -- summed over the batch where the shape has no batch axis, over time where its time axis is 1 -- then
    ``residual[B]``, ``iterations[B]`` (the Smith steps) and the backward's ``status[B]``."""
    lib = _hip.require_gpu()
    Bk, N, m, n = K.shape
    dev, f64 = K.device, torch.float64
    grads = alloc_grads(shapes, needed, Bk, dev, f64)
    args = []
    for g in grads:
        args += [_hip.ptr(g), *grad_strides(g, 4, True)]
    ups = [None if g is None else g.to(device=dev, dtype=f64).contiguous() for g in ups]
    alloc = torch.zeros if Bk == 0 else torch.empty
    residual = alloc((Bk,), dtype=f64, device=dev)
    iterations = alloc((Bk,), dtype=torch.int32, device=dev)
    status = alloc((Bk,), dtype=torch.int32, device=dev)
    ws_bytes = int(lib.tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(Bk, n, m, N, segments))
    ws = torch.empty((max(ws_bytes // 8, 1),), dtype=f64, device=dev)
    rc = lib.tfmpc_tvlqr_periodic_vjp_f64(Bk, n, m, N, *tv._model_args()[:12], _hip.ptr(K), _hip.ptr(k), _hip.ptr(V), _hip.ptr(v),
                                          _hip.ptr(fwd_status), *(_hip.ptr(u) for u in ups), *args, _hip.ptr(residual),
                                          _hip.ptr(iterations), _hip.ptr(status), segments, max_iter, tol, _hip.ptr(ws),
                                          ws.numel() * 8, _hip.stream())
    _hip.check(rc, "tfmpc_tvlqr_periodic_vjp_f64")
    return grads, residual, iterations, status


class PeriodicSteadyStateFunctionF64(torch.autograd.Function):
    """The periodic steady state in the autograd graph: the forward is the unchanged
    ``tfmpc_tvlqr_periodic_steady_state_f64`` launch of ``tv`` (which holds the detached operands), so every output keeps
    its bits; the backward is ``tfmpc_tvlqr_periodic_vjp_f64`` with ``vjp_segments``.  ``residual``, ``iterations`` and
    ``status`` are not differentiable.  ``tv.last_grad_status`` gets the backward's status."""

    @staticmethod
    def forward(ctx, tv, launch, vjp_segments, max_iter, tol, F, f, C, c):
        K, k, V, v, residual, iterations, status = launch()
        ctx.tv, ctx.call = tv, (vjp_segments, max_iter, tol)
        ctx.shapes = [t.shape for t in (F, f, C, c)]
        ctx.save_for_backward(K, k, V, v, status)
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None: a NULL upstream pointer
        ctx.mark_non_differentiable(residual, iterations, status)
        return K, k, V, v, residual, iterations, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gK, gk, gV, gv, *_):
        K, k, V, v, fwd_status = ctx.saved_tensors
        grads, _, _, status = periodic_vjp_f64(ctx.tv, K, k, V, v, fwd_status, (gK, gk, gV, gv), ctx.shapes,
                                               ctx.needs_input_grad[5:], *ctx.call)
        ctx.tv.last_grad_status = status
        return (None,) * 5 + tuple(grads)


def tvlqr_periodic_vjp(F, f, C, c, K, k, V, v, fwd_status, gK=None, gk=None, gV=None, gv=None, segments=None, max_iter=0,
                       tol=0.0):
    """The vector-Jacobian product of the periodic steady state alone, in double (``tfmpc_tvlqr_periodic_vjp_f64``,
    DESIGN.md 3.26), for any forward: ``K, k, V, v, fwd_status`` as :func:`tvlqr_periodic_steady_state` of ``(F, f, C, c)``
    gave them (batched, or without a batch axis when no operand has one), ``gK, gk, gV, gv`` the upstream gradients
    (``None`` = zero).  ``segments=None`` picks :meth:`TimeVaryingLQR.default_periodic_vjp_segments`; ``max_iter=0`` is 40
    Smith steps, ``tol=0`` is 4 ``DBL_EPSILON``.  Returns ``(dF, df, dC, dc, residual, iterations, status)``: each gradient
    float64 in its operand's shape as :class:`TimeVaryingLQR` holds it (vectors as columns; an operand without a batch axis
    gets the sum over the batch, a time axis of 1 the sum over time -- the call then sweeps the period as one segment),
    ``residual[(B)]`` the fixed point's self-check, ``iterations[(B)]`` the Smith steps and the per-instance status -- the
    forward's where that was flagged; a flagged instance has NaN in its own gradient rows and in every sum that contains
    it.  A ``K`` of the caller's own that is not stabilising is ``TFMPC_ST_NOT_STABILISING``."""
    from tfmpc.solvers.tvlqr import TimeVaryingLQR, _as_dtype
    f64 = torch.float64
    device = next((t.device for t in (F, f, C, c, K) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    tv = TimeVaryingLQR(F, f, C, c, device=device, dtype=f64)
    dev = tv.device
    n, m, N = tv.state_size, tv.action_size, tv.horizon
    batched = tv.batch_size is not None
    Bk = tv.batch_size if batched else 1
    K, k, V, v = (_as_dtype(t, dev, f64).reshape(-1, N, *inner).contiguous()
                  for t, inner in ((K, (m, n)), (k, (m, 1)), (V, (n, n)), (v, (n, 1))))
    fwd_status = torch.as_tensor(fwd_status).detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if any(t.shape[0] != Bk for t in (K, k, V, v, fwd_status)):
        raise ValueError("K, k, V, v and fwd_status must share the operands' batch size")
    ups = [None if g is None else _as_dtype(g, dev, f64).reshape(Bk, N, *inner)
           for g, inner in ((gK, (m, n)), (gk, (m, 1)), (gV, (n, n)), (gv, (n, 1)))]
    segments = tv.default_periodic_vjp_segments(Bk) if segments is None else int(segments)
    max_iter, tol = int(max_iter), float(tol)
    if segments < 1 or max_iter < 0 or not tol >= 0.0:
        raise ValueError(f"segments must be at least 1 and max_iter, tol not negative, got {segments}, {max_iter}, {tol}")
    shapes = [t.shape for t in (tv.F, tv.f, tv.C, tv.c)]
    grads, residual, iterations, status = periodic_vjp_f64(tv, K, k, V, v, fwd_status, ups, shapes, (True,) * 4, segments,
                                                           max_iter, tol)
    tv.last_grad_status = status
    tail = (residual, iterations, status) if batched else (residual[0], iterations[0], status[0])
    return (*grads, *tail)


__all__ = ["SolveFunction", "SolveFunctionF64", "SolveTimeParallelFunctionF64", "PeriodicSteadyStateFunctionF64",
           "TensorTrajectory", "tvlqr_solve", "tvlqr_vjp_time_parallel", "tvlqr_periodic_vjp"]

"""Differentiable Riccati recursion: a ``torch.autograd.Function`` over ``tfmpc_tvlqr_backward_f32`` (or ``LQR``'s own
backward kernel) and ``tfmpc_tvlqr_backward_vjp_f32`` (include/tfmpc_hip.h), and its double-precision
twin over ``tfmpc_tvlqr_backward_f64`` and ``tfmpc_tvlqr_backward_vjp_f64``.

The forward is the unchanged backward-recursion launch (the same bits as a call without grad); the Function saves its
``K, k, V, v`` and status.  The backward pass is one sweep forward in time that carries the adjoints of ``V_t, v_t`` and
``const_t``; it reads the model and the saved outputs only.  Each gradient has the shape of its operand: an operand
without a batch axis (shared by the batch) gets the gradient summed over the batch, a time axis of size 1 (or an ``LQR``
operand, which has none) the gradient summed over time.

``C`` and ``C_final`` enter the kernels only as symmetric matrices, so their gradients are the symmetric ones.  An
instance whose recursion or adjoint sweep is flagged gets NaN in its own gradient rows and in every gradient summed over
a batch that contains it (``last_grad_status`` on the solver holds the per-instance status of the backward pass; the
double path has no solver object: :func:`tvlqr_backward_vjp` returns the status).  Double backward is not supported.
"""

import torch
from torch.autograd.function import once_differentiable

from tfmpc import _hip
from tfmpc.solvers import tvlqr_grad


class BackwardFunction(torch.autograd.Function):
    """``problem``: a :class:`tfmpc.solvers.tvlqr_grad.Problem` whose ``run()`` launches the recursion and returns the
    batched ``K, k, V, v, const, status``."""

    @staticmethod
    def forward(ctx, problem, F, f, C, c, C_final, c_final):
        K, k, V, v, const, status = problem.run()
        ctx.problem = problem
        ctx.shapes = [(t.shape if t is not None else None) for t in (F, f, C, c, C_final, c_final)]
        ctx.save_for_backward(K, k, V, v, status)
        ctx.set_materialize_grads(False)
        return K, k, V, v, const

    @staticmethod
    @once_differentiable
    def backward(ctx, gK, gk, gV, gv, gconst):
        K, k, V, v, fwd_status = ctx.saved_tensors
        problem = ctx.problem
        tv = problem.model()
        lib = _hip.require_gpu()
        Bk, T, m, n = K.shape
        dev = K.device
        nd_model = 4 if problem.timed else 3
        grads = tvlqr_grad.alloc_grads(ctx.shapes, ctx.needs_input_grad[1:], Bk, dev)
        args = []
        for g in grads[:4]:
            args += [_hip.ptr(g), *tvlqr_grad.grad_strides(g, nd_model, problem.timed)]
        for g in grads[4:]:
            args += [_hip.ptr(g), tvlqr_grad.grad_strides(g, 3, False)[0]]
        ups = [None if g is None else g.to(torch.float32).contiguous() for g in (gK, gk, gV, gv, gconst)]
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        ws_bytes = int(lib.tfmpc_tvlqr_backward_vjp_workspace_bytes(Bk, n, m, T))
        ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.float32, device=dev) if ws_bytes else None
        rc = lib.tfmpc_tvlqr_backward_vjp_f32(Bk, n, m, T, *tv._model_args(), _hip.ptr(K), _hip.ptr(k), _hip.ptr(V),
                                              _hip.ptr(v), _hip.ptr(fwd_status), *(_hip.ptr(u) for u in ups), *args,
                                              _hip.ptr(status), _hip.ptr(ws), ws_bytes, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_backward_vjp_f32")
        problem.owner.last_grad_status = status
        return (None, *grads)


def tv_graph_operands(tv):
    """``F, f, C, c, C_final, c_final`` of a :class:`TimeVaryingLQR` as graph tensors: the caller's tensor operands
    converted without ``detach`` and shaped as the solver's own (numpy operands, which cannot require grad, are the
    solver's tensors)."""
    n, d = tv.state_size, tv.n_dim
    src = tv._sources

    def op(i, own, shape=None):
        if src[i] is None:
            return own
        t = tvlqr_grad.as_graph(src[i], tv.device, tv.dtype)
        return shape(t) if shape else t
    return (op(0, tv.F), op(1, tv.f, lambda t: tv._vector(t, n, "f")), op(2, tv.C), op(3, tv.c, lambda t: tv._vector(t, d, "c")),
            op(4, tv.C_final),
            op(5, tv.c_final, lambda t: t.unsqueeze(-1) if t.dim() == 1 or (t.dim() == 2 and t.shape != (n, 1)) else t))


def _vjp_f64_launch(tv, K, k, V, v, fwd_status, ups, shapes, needed):
    """One tfmpc_tvlqr_backward_vjp_f64 launch on the double problem ``tv``.  ``K, k, V, v, fwd_status``: the recursion's
    batched outputs; ``ups``: ``gK, gk, gV, gv, gconst`` (``None`` = zero, a NULL pointer).  One double gradient per entry
    of ``shapes`` (``F, f, C, c, C_final, c_final`` as the solver shapes them) that ``needed`` asks for -- summed over the
    batch where the shape has no batch axis, over time where its time axis is 1 -- and the backward's status ``[B]``."""
    lib = _hip.require_gpu()
    Bk, T, m, n = K.shape
    dev, f64 = K.device, torch.float64
    grads = tvlqr_grad.alloc_grads(shapes, needed, Bk, dev, f64)
    args = []
    summed = False
    for g, nd, timed in zip(grads, (4, 4, 4, 4, 3, 3), (True,) * 4 + (False,) * 2):
        sb, st = tvlqr_grad.grad_strides(g, nd, timed)
        summed |= g is not None and sb == 0 and Bk > 1
        args += [_hip.ptr(g), sb, st] if timed else [_hip.ptr(g), sb]
    ups = [None if g is None else g.to(device=dev, dtype=f64).contiguous() for g in ups]
    status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
    ws, ws_bytes = None, 0
    if summed:                       # records of the batch sum; nothing is summed over a batch of one
        ws_bytes = int(lib.tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(Bk, n, m, T))
        ws = torch.empty(((ws_bytes + 7) // 8,), dtype=f64, device=dev)
    rc = lib.tfmpc_tvlqr_backward_vjp_f64(Bk, n, m, T, *tv._model_args(), _hip.ptr(K), _hip.ptr(k), _hip.ptr(V), _hip.ptr(v),
                                          _hip.ptr(fwd_status), *(_hip.ptr(u) for u in ups), *args, _hip.ptr(status),
                                          _hip.ptr(ws), ws_bytes, _hip.stream())
    _hip.check(rc, "tfmpc_tvlqr_backward_vjp_f64")
    return grads, status


class BackwardFunctionF64(torch.autograd.Function):
    """``BackwardFunction`` in double: the forward is the unchanged ``tfmpc_tvlqr_backward_f64`` launch
    of ``tv`` (a ``TimeVaryingLQR(dtype=torch.float64)``, which holds the detached operands), the backward
    ``tfmpc_tvlqr_backward_vjp_f64``; upstream gradients, gradients and the workspace are fp64."""

    @staticmethod
    def forward(ctx, tv, F, f, C, c, C_final, c_final):
        K, k, V, v, const, status = tv._backward_launch()
        ctx.tv = tv
        ctx.shapes = [(t.shape if t is not None else None) for t in (F, f, C, c, C_final, c_final)]
        ctx.save_for_backward(K, k, V, v, status)
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None: a NULL upstream pointer
        return K, k, V, v, const

    @staticmethod
    @once_differentiable
    def backward(ctx, gK, gk, gV, gv, gconst):
        K, k, V, v, fwd_status = ctx.saved_tensors
        grads, status = _vjp_f64_launch(ctx.tv, K, k, V, v, fwd_status, (gK, gk, gV, gv, gconst), ctx.shapes,
                                        ctx.needs_input_grad[1:])
        ctx.tv.last_grad_status = status
        return (None, *grads)


def _device_of(*operands):
    return next((t.device for t in operands if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)


def tvlqr_backward(F, f, C, c, C_final=None, c_final=None, dtype=None):
    """The Riccati recursion of the time-varying LQR of :class:`tfmpc.solvers.TimeVaryingLQR` (same operand shapes):
    ``(K, k, V, v, const)`` as tensors -- ``K[(B,)T,m,n]``, ``k[(B,)T,m,1]``, ``V[(B,)T,n,n]``, ``v[(B,)T,n,1]``,
    ``const[(B,)T,1,1]`` -- differentiable with respect to every tensor operand that requires grad.

    ``dtype=None`` or ``torch.float32`` is the fp32 path.  ``dtype=torch.float64`` keeps the operands in double inside the
    autograd graph, with no pass through fp32: the outputs are the bits of ``TimeVaryingLQR(..., dtype=torch.float64)
    .backward()`` (``tfmpc_tvlqr_backward_f64``, n <= 32 and m <= 32) and the gradients come from
    ``tfmpc_tvlqr_backward_vjp_f64``, each float64 in its operand's shape.  The backward's status is not
    kept on this path: :func:`tvlqr_backward_vjp` returns it."""
    from tfmpc.solvers.tvlqr import TimeVaryingLQR
    if dtype not in (None, torch.float32, torch.float64):
        raise ValueError(f"dtype must be None, torch.float32 or torch.float64, got {dtype!r}")
    device = _device_of(F, f, C, c, C_final, c_final)
    if dtype != torch.float64:
        policy, value = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=device).backward(differentiable=True)
        return policy.K, policy.k, value.V, value.v, value.const
    tv = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=device, dtype=torch.float64)
    if tvlqr_grad.wants_grad(*tv._sources):
        K, k, V, v, const = BackwardFunctionF64.apply(tv, *tv_graph_operands(tv))
    else:
        K, k, V, v, const, _ = tv._backward_launch()
    if tv.batch_size is None:
        K, k, V, v, const = K[0], k[0], V[0], v[0], const[0]
    return K, k, V, v, const


def tvlqr_backward_vjp(F, f, C, c, K, k, V, v, fwd_status, gK=None, gk=None, gV=None, gv=None, gconst=None, C_final=None,
                       c_final=None, dtype=torch.float64):
    """The vector-Jacobian product of the Riccati recursion alone, in double (``tfmpc_tvlqr_backward_vjp_f64``, DESIGN.md
    3.23), for any forward: ``K, k, V, v, fwd_status`` as the recursion of ``(F, f, C, c, C_final, c_final)`` gave them
    (batched, or without a batch axis when no operand has one), ``gK, gk, gV, gv, gconst`` the upstream gradients
    (``None`` = zero).  Returns ``(dF, df, dC, dc, dC_final, dc_final, status)``: each gradient float64 in its operand's
    shape as :class:`TimeVaryingLQR` holds it (vectors as columns; an operand without a batch axis gets the sum over the
    batch, a time axis of 1 the sum over time; ``None`` for an absent final cost, whose gradient is then in ``dC, dc`` at
    the last step) and the backward's per-instance status -- the forward's where that was flagged; a flagged instance has
    NaN in its own gradient rows and in every sum that contains it.  Only ``dtype=torch.float64`` is served."""
    from tfmpc.solvers.tvlqr import TimeVaryingLQR, _as_dtype
    if dtype != torch.float64:
        raise ValueError(f"tvlqr_backward_vjp serves dtype=torch.float64 only, got {dtype!r}")
    f64 = torch.float64
    tv = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=_device_of(F, f, C, c, C_final, c_final, K), dtype=f64)
    dev = tv.device
    n, m, T = tv.state_size, tv.action_size, tv.horizon
    Bk = tv.batch_size if tv.batch_size is not None else 1
    K, k, V, v = (_as_dtype(t, dev, f64).reshape(-1, T, *inner).contiguous()
                  for t, inner in ((K, (m, n)), (k, (m, 1)), (V, (n, n)), (v, (n, 1))))
    fwd_status = torch.as_tensor(fwd_status).detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if any(t.shape[0] != Bk for t in (K, k, V, v, fwd_status)):
        raise ValueError("K, k, V, v and fwd_status must share the operands' batch size")
    ups = [None if g is None else _as_dtype(g, dev, f64).reshape(Bk, T, *inner)
           for g, inner in ((gK, (m, n)), (gk, (m, 1)), (gV, (n, n)), (gv, (n, 1)), (gconst, (1, 1)))]
    shapes = [(t.shape if t is not None else None) for t in (tv.F, tv.f, tv.C, tv.c, tv.C_final, tv.c_final)]
    grads, status = _vjp_f64_launch(tv, K, k, V, v, fwd_status, ups, shapes, (True,) * 6)
    return (*grads, status)


__all__ = ["BackwardFunction", "BackwardFunctionF64", "tvlqr_backward", "tvlqr_backward_vjp"]

"""Differentiable infinite-horizon LQR: a ``torch.autograd.Function`` over ``tfmpc_lqr_steady_state_f32`` (forward) and
``tfmpc_lqr_steady_state_vjp_f32`` (backward), include/tfmpc_hip.h, DESIGN.md §3.10, and its double-precision twin over
``tfmpc_lqr_steady_state_f64`` and ``tfmpc_lqr_steady_state_vjp_f64``.

The forward is the unchanged steady-state launch of :meth:`tfmpc.solvers.lqr.LQR.steady_state` (the same bits as a
call without grad); the Function saves its ``K, k, P, p`` and status.  The backward recomputes ``A_cl`` and
``R + B'PB`` from them, reverses the explicit formulas of ``K, k, p`` and solves one Stein equation for P's implicit
dependence through the Riccati equation.  Each gradient has the shape of its operand: an operand without a batch axis
(shared by the batch) gets the gradient summed over the batch.

``C`` enters the kernels only as a symmetric matrix, so its gradient is the symmetric one.  An instance whose forward
or backward is flagged gets NaN in its own gradient rows and in every gradient summed over a batch that contains it
(``last_grad_status`` on the solver holds the backward's per-instance status).  ``iterations`` and ``status`` are not
differentiable.  Double backward is not supported.
"""

import torch
from torch.autograd.function import once_differentiable

from tfmpc import _hip
from tfmpc.solvers import tvlqr_grad


def graph_operands(lqr):
    """F, f, C, c of ``lqr`` as graph tensors: the caller's tensor operands converted without ``detach`` (numpy operands,
    which cannot require grad, are the solver's own tensors)."""
    from tfmpc.solvers.lqr import _as_column
    n, d = lqr.state_size, lqr.n_dim
    F, f, C, c = (own if src is None else tvlqr_grad.as_f32_graph(src, lqr.device)
                  for src, own in zip(lqr._sources, (lqr.F, lqr.f, lqr.C, lqr.c)))
    return F, _as_column(f, n), C, _as_column(c, d)


class SteadyStateFunction(torch.autograd.Function):

    @staticmethod
    def forward(ctx, lqr, max_iter, tol, F, f, C, c):
        K, k, P, p, iterations, status = lqr._steady_state_launch(max_iter, tol)
        ctx.lqr, ctx.max_iter, ctx.tol = lqr, max_iter, tol
        ctx.shapes = [t.shape for t in (F, f, C, c)]
        ctx.save_for_backward(K, k, P, p, status)
        ctx.mark_non_differentiable(iterations, status)
        return K, k, P, p, iterations, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gK, gk, gP, gp, _g_iterations, _g_status):
        K, k, P, p, fwd_status = ctx.saved_tensors
        lqr = ctx.lqr
        lib = _hip.require_gpu()
        Bk, m, n = K.shape
        dev = K.device
        grads = tvlqr_grad.alloc_grads(ctx.shapes, ctx.needs_input_grad[3:], Bk, dev)
        out_args = []
        summed = False
        for g in grads:
            stride = tvlqr_grad.grad_strides(g, 3, False)[0]      # 0 (summed over the batch) for an operand without a batch axis
            summed |= g is not None and stride == 0 and Bk > 1
            out_args += [_hip.ptr(g), stride]
        ups = [None if g is None else g.to(torch.float32).contiguous() for g in (gK, gk, gP, gp)]
        model = []
        for t in (lqr.F, lqr.f, lqr.C, lqr.c):
            model += [_hip.ptr(t), t.stride(0) if t.dim() == 3 else 0]
        ws, ws_bytes = None, 0
        if summed:
            ws_bytes = int(lib.tfmpc_lqr_steady_state_vjp_workspace_bytes(Bk, n, m))
            ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.float32, device=dev)
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        rc = lib.tfmpc_lqr_steady_state_vjp_f32(Bk, n, m, *model, _hip.ptr(K), _hip.ptr(k), _hip.ptr(P), _hip.ptr(p),
                                                _hip.ptr(fwd_status), *(_hip.ptr(u) for u in ups), ctx.max_iter, ctx.tol,
                                                *out_args, _hip.ptr(status), _hip.ptr(ws), ws_bytes, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_steady_state_vjp_f32")
        lqr.last_grad_status = status
        return (None, None, None, *grads)


def _vjp_f64_launch(model, K, k, P, p, fwd_status, ups, max_iter, tol, shapes, needed):
    """One tfmpc_lqr_steady_state_vjp_f64 launch.  ``model``: contiguous double ``F, f, C, c`` (``f, c`` columns, a batch
    axis or none each); ``K, k, P, p, fwd_status``: the forward's batched outputs; ``ups``: ``gK, gk, gP, gp`` (``None`` =
    zero).  One double gradient per entry of ``shapes`` that ``needed`` asks for (summed over the batch where the shape
    has no batch axis), and the backward's status ``[B]``."""
    lib = _hip.require_gpu()
    Bk, m, n = K.shape
    dev, f64 = K.device, torch.float64
    grads = tvlqr_grad.alloc_grads(shapes, needed, Bk, dev, f64)
    out_args = []
    summed = False
    for g in grads:
        stride = tvlqr_grad.grad_strides(g, 3, False)[0]      # 0 (summed over the batch) for an operand without a batch axis
        summed |= g is not None and stride == 0 and Bk > 1
        out_args += [_hip.ptr(g), stride]
    ups = [None if g is None else g.to(device=dev, dtype=f64).contiguous() for g in ups]
    model_args = []
    for t in model:
        model_args += [_hip.ptr(t), t.stride(0) if t.dim() == 3 else 0]
    ws, ws_bytes = None, 0
    if summed:
        ws_bytes = int(lib.tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(Bk, n, m))
        ws = torch.empty(((ws_bytes + 7) // 8,), dtype=f64, device=dev)
    status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
    rc = lib.tfmpc_lqr_steady_state_vjp_f64(Bk, n, m, *model_args, _hip.ptr(K), _hip.ptr(k), _hip.ptr(P), _hip.ptr(p),
                                            _hip.ptr(fwd_status), *(_hip.ptr(u) for u in ups), int(max_iter), float(tol),
                                            *out_args, _hip.ptr(status), _hip.ptr(ws), ws_bytes, _hip.stream())
    _hip.check(rc, "tfmpc_lqr_steady_state_vjp_f64")
    return grads, status


class SteadyStateFunctionF64(torch.autograd.Function):
    """``SteadyStateFunction`` in double: the forward is the unchanged ``tfmpc_lqr_steady_state_f64``
    launch on the detached operands, the backward ``tfmpc_lqr_steady_state_vjp_f64``; upstream gradients, gradients and
    the workspace are fp64."""

    @staticmethod
    def forward(ctx, batch_size, max_iter, tol, F, f, C, c):
        from tfmpc.solvers.lqr import _steady_state_launch_f64
        model = [t.detach().contiguous() for t in (F, f, C, c)]
        K, k, P, p, iterations, status = _steady_state_launch_f64(*model, batch_size, max_iter, tol)
        ctx.max_iter, ctx.tol = max_iter, tol
        ctx.shapes = [t.shape for t in (F, f, C, c)]
        ctx.save_for_backward(*model, K, k, P, p, status)
        ctx.mark_non_differentiable(iterations, status)
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None: a NULL upstream pointer
        return K, k, P, p, iterations, status

    @staticmethod
    @once_differentiable
    def backward(ctx, gK, gk, gP, gp, _g_iterations, _g_status):
        *model, K, k, P, p, fwd_status = ctx.saved_tensors
        grads, _ = _vjp_f64_launch(model, K, k, P, p, fwd_status, (gK, gk, gP, gp), ctx.max_iter, ctx.tol, ctx.shapes,
                                   ctx.needs_input_grad[3:])
        return (None, None, None, *grads)


def _f64_operands(F, f, C, c, device, convert):
    """The operands in double on ``device`` (``convert(a, device)``), shapes checked, ``f, c`` as columns, ``C`` symmetric
    to 1e-12 of its largest entry: ``(F, f, C, c, batch_size)``."""
    from tfmpc.solvers.lqr import _model_shapes
    F, f, C, c = (convert(a, device) for a in (F, f, C, c))
    f, c, batch_size = _model_shapes(F, f, C, c)
    Cd = C.detach()
    if Cd.numel() and not bool((Cd - Cd.transpose(-1, -2)).abs().amax() <= 1e-12 * Cd.abs().amax()):
        raise NotImplementedError("the steady state is served for a symmetric C only")
    return F, f, C, c, batch_size


def _steady_state_f64_differentiable(F, f, C, c, max_iter, tol, device):
    from tfmpc.solvers.lqr import SteadyState, _steady_state_limits
    device = torch.device(device) if device is not None else _hip.default_device()
    F, f, C, c, batch_size = _f64_operands(F, f, C, c, device, lambda a, dev: tvlqr_grad.as_graph(a, dev, torch.float64))
    max_iter, tol = _steady_state_limits(max_iter, tol, F.shape[-2], F.shape[-1] - F.shape[-2])
    outs = SteadyStateFunctionF64.apply(batch_size, max_iter, tol, F, f, C, c)
    if batch_size is None:
        outs = tuple(t[0] for t in outs)
    return SteadyState(*outs)


def lqr_steady_state(F, f, C, c, max_iter=None, tol=None, dtype=None, differentiable=False):
    """The stationary solution of the LQR ``(F, f, C, c)`` (operand shapes as :class:`tfmpc.solvers.lqr.LQR`) as a
    :class:`~tfmpc.solvers.lqr.SteadyState` whose ``K, k, P, p`` are differentiable with respect to every tensor operand
    that requires grad.  ``max_iter`` and ``tol`` as :meth:`LQR.steady_state`; they also bound the backward's Stein
    solve.

    ``dtype=torch.float64`` keeps the caller's operands (tensors, or numpy arrays through ``np.float64``) in double, with
    no pass through fp32, and returns float64 tensors from ``tfmpc_lqr_steady_state_f64``; ``C`` must
    then be symmetric to 1e-12 relative.  Gradients in double are an opt-in: with ``differentiable=True`` the operands
    stay in the autograd graph in double and the backward is ``tfmpc_lqr_steady_state_vjp_f64``, every
    gradient float64; without it an operand that requires grad raises ``NotImplementedError``.  The backward's status
    is not kept anywhere on this path: :func:`lqr_steady_state_vjp` returns it.  ``None`` or ``torch.float32`` is the
    fp32 path, which is differentiable as it is (the flag changes nothing there)."""
    from tfmpc.solvers.lqr import LQR, _steady_state_dtype, steady_state_f64
    device = next((t.device for t in (F, f, C, c) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    if _steady_state_dtype(dtype) == torch.float64:
        if differentiable and tvlqr_grad.wants_grad(F, f, C, c):
            return _steady_state_f64_differentiable(F, f, C, c, max_iter, tol, device)
        return steady_state_f64(F, f, C, c, max_iter, tol, device=device)
    return LQR(F, f, C, c, device=device).steady_state(max_iter, tol, differentiable=True)


def lqr_steady_state_vjp(F, f, C, c, K, k, P, p, fwd_status, gK=None, gk=None, gP=None, gp=None, max_iter=None, tol=None,
                         dtype=torch.float64):
    """The vector-Jacobian product of the steady state alone, in double (``tfmpc_lqr_steady_state_vjp_f64``, DESIGN.md
    3.22), for any forward: ``K, k, P, p, fwd_status`` as :func:`lqr_steady_state` returned them for ``(F, f, C, c)``
    (batched, or without a batch axis when no operand has one), ``gK, gk, gP, gp`` the upstream gradients (``None`` =
    zero).  Returns ``(dF, df, dC, dc, status)``: each gradient float64 in its operand's shape (``f, c`` as columns; an
    operand without a batch axis gets the sum over the batch) and the backward's per-instance status -- the forward's
    where that was flagged; a flagged instance has NaN in its own gradient rows and in every sum that contains it.
    ``max_iter`` and ``tol`` bound the Smith loop.  Only ``dtype=torch.float64`` is served."""
    from tfmpc.solvers.lqr import _as_f64, _steady_state_limits
    if dtype != torch.float64:
        raise ValueError(f"lqr_steady_state_vjp serves dtype=torch.float64 only, got {dtype!r}")
    device = next((t.device for t in (F, f, C, c, K) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    device = torch.device(device) if device is not None else _hip.default_device()
    F, f, C, c, batch_size = _f64_operands(F, f, C, c, device, _as_f64)
    n, m = F.shape[-2], F.shape[-1] - F.shape[-2]
    max_iter, tol = _steady_state_limits(max_iter, tol, n, m)
    K, k, P, p = (_as_f64(t, device).reshape(-1, *inner).contiguous()
                  for t, inner in ((K, (m, n)), (k, (m, 1)), (P, (n, n)), (p, (n, 1))))
    Bk = K.shape[0]
    fwd_status = torch.as_tensor(fwd_status).detach().to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    if Bk != (batch_size if batch_size is not None else Bk) or any(t.shape[0] != Bk for t in (k, P, p, fwd_status)):
        raise ValueError("K, k, P, p and fwd_status must share the operands' batch size")
    ups = [None if g is None else _as_f64(g, device).reshape(Bk, *inner)
           for g, inner in ((gK, (m, n)), (gk, (m, 1)), (gP, (n, n)), (gp, (n, 1)))]
    model = [t.contiguous() for t in (F, f, C, c)]
    grads, status = _vjp_f64_launch(model, K, k, P, p, fwd_status, ups, max_iter, tol, [t.shape for t in model], (True,) * 4)
    return (*grads, status)


__all__ = ["SteadyStateFunction", "SteadyStateFunctionF64", "lqr_steady_state", "lqr_steady_state_vjp"]

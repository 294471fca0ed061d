"""Differentiable infinite-horizon LQR: a ``torch.autograd.Function`` over ``tfmpc_lqr_steady_state_f32`` (forward) and
``tfmpc_lqr_steady_state_vjp_f32`` (backward), include/tfmpc_hip.h, DESIGN.md §3.10.

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


def lqr_steady_state(F, f, C, c, max_iter=None, tol=None, dtype=None):
    """The stationary solution of the LQR ``(F, f, C, c)`` (operand shapes as :class:`tfmpc.solvers.lqr.LQR`) as a
    :class:`~tfmpc.solvers.lqr.SteadyState` whose ``K, k, P, p`` are differentiable with respect to every tensor operand
    that requires grad.  ``max_iter`` and ``tol`` as :meth:`LQR.steady_state`; they also bound the backward's Stein
    solve.

    ``dtype=torch.float64`` keeps the caller's operands (tensors, or numpy arrays through ``np.float64``) in double, with
    no pass through fp32, and returns float64 tensors from ``tfmpc_lqr_steady_state_f64``; ``C`` must
    then be symmetric to 1e-12 relative, and an operand that requires grad raises ``NotImplementedError`` (gradients
    are fp32 only).  ``None`` or ``torch.float32`` is the fp32 path."""
    from tfmpc.solvers.lqr import LQR, _steady_state_dtype, steady_state_f64
    device = next((t.device for t in (F, f, C, c) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    if _steady_state_dtype(dtype) == torch.float64:
        return steady_state_f64(F, f, C, c, max_iter, tol, device=device)
    return LQR(F, f, C, c, device=device).steady_state(max_iter, tol, differentiable=True)


__all__ = ["SteadyStateFunction", "lqr_steady_state"]

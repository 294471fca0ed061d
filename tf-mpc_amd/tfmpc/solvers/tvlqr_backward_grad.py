"""Differentiable Riccati recursion: a ``torch.autograd.Function`` over ``tfmpc_tvlqr_backward_f32`` (or ``LQR``'s own
backward kernel) and ``tfmpc_tvlqr_backward_vjp_f32`` (include/tfmpc_hip.h).

The forward is the unchanged backward-recursion launch (the same bits as a call without grad); the Function saves its
``K, k, V, v`` and status.  The backward pass is one sweep forward in time that carries the adjoints of ``V_t, v_t`` and
``const_t``; it reads the model and the saved outputs only.  Each gradient has the shape of its operand: an operand
without a batch axis (shared by the batch) gets the gradient summed over the batch, a time axis of size 1 (or an ``LQR``
operand, which has none) the gradient summed over time.

``C`` and ``C_final`` enter the kernels only as symmetric matrices, so their gradients are the symmetric ones.  An
instance whose recursion or adjoint sweep is flagged gets NaN in its own gradient rows and in every gradient summed over
a batch that contains it (``last_grad_status`` on the solver holds the per-instance status of the backward pass).  Double
backward is not supported.
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
        t = tvlqr_grad.as_f32_graph(src[i], tv.device)
        return shape(t) if shape else t
    return (op(0, tv.F), op(1, tv.f, lambda t: tv._vector(t, n, "f")), op(2, tv.C), op(3, tv.c, lambda t: tv._vector(t, d, "c")),
            op(4, tv.C_final),
            op(5, tv.c_final, lambda t: t.unsqueeze(-1) if t.dim() == 1 or (t.dim() == 2 and t.shape != (n, 1)) else t))


def tvlqr_backward(F, f, C, c, C_final=None, c_final=None):
    """The Riccati recursion of the time-varying LQR of :class:`tfmpc.solvers.TimeVaryingLQR` (same operand shapes):
    ``(K, k, V, v, const)`` as tensors -- ``K[(B,)T,m,n]``, ``k[(B,)T,m,1]``, ``V[(B,)T,n,n]``, ``v[(B,)T,n,1]``,
    ``const[(B,)T,1,1]`` -- differentiable with respect to every tensor operand that requires grad."""
    from tfmpc.solvers.tvlqr import TimeVaryingLQR
    device = next((t.device for t in (F, f, C, c, C_final, c_final) if isinstance(t, torch.Tensor) and t.device.type != "cpu"),
                  None)
    policy, value = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=device).backward(differentiable=True)
    return policy.K, policy.k, value.V, value.v, value.const


__all__ = ["BackwardFunction", "tvlqr_backward"]

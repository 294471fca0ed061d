"""Finite-horizon LQR on MI355X -- drop-in for the reference's
``tfmpc/solvers/lqr.py`` (``LQR``: ``__init__`` :18-22, ``transition`` :36-39,
``cost`` :41-47, ``final_cost`` :49-57, ``backward`` :59-129, ``forward``
:131-161, ``solve`` :163-166, ``dump``/``load`` :168-181).

Differences from the reference, all additive:

* tensors are torch (fp32, on the ROCm device) / numpy instead of ``tf.Tensor``;
* ``F, f, C, c`` and ``x0`` may each carry one leading batch axis ``B``: the call
  then solves ``B`` independent problems in ONE kernel launch (an operand without
  the axis is shared by all instances);
* ``backward`` / ``forward`` / ``solve`` execute as hand-written gfx950 kernels
  through the C ABI (``include/tfmpc_hip.h``).  No CPU fallback.
* ``C`` is expected to be symmetric (every problem the reference builds is:
  ``make_lqr`` draws ``make_spd_matrix``, ``tfmpc/envs/__init__.py:9-18``) with ``C_uu``
  positive definite; the fast kernels use that.  A ``C`` that is NOT symmetric is detected
  once at construction and solved by the ``*_general_f32`` entry points, which restate the
  reference's recursion term by term (``lqr.py:74-105``: ``Q_ux`` and ``Q_xu`` separately,
  general inverse, no symmetrisation) -- slower, same results as the reference.
"""

import json

import numpy as np
import torch

from tfmpc import _hip
from tfmpc.solvers import tvlqr_grad
from tfmpc.utils import trajectory


class Policy(list):
    """``policy[t] == (K_t, k_t)`` like the reference's list, plus the stacked
    device tensors ``K[(B,)T,m,n]``, ``k[(B,)T,m,1]`` the kernels read."""

    def __init__(self, K, k):
        tdim = K.dim() - 3
        super().__init__((K.select(tdim, t), k.select(tdim, t)) for t in range(K.shape[tdim]))
        self.K, self.k = K, k


class ValueFn(list):
    """``value_fn[t] == (V_t, v_t, const_t)`` plus the stacked tensors."""

    def __init__(self, V, v, const):
        tdim = V.dim() - 3
        super().__init__((V.select(tdim, t), v.select(tdim, t), const.select(tdim, t))
                         for t in range(V.shape[tdim]))
        self.V, self.v, self.const = V, v, const


class SteadyState:
    """The infinite-horizon solution of an :class:`LQR` (``LQR.steady_state``): the stationary feedback ``u = K x + k``
    and value function ``V(x) = 1/2 x^T P x + p^T x`` as device tensors ``K[(B,)m,n]``, ``k[(B,)m,1]``, ``P[(B,)n,n]``,
    ``p[(B,)n,1]``, with ``iterations[(B)]`` (doubling steps) and ``status[(B)]`` (``_hip.ST_*`` bits; a flagged instance
    has NaN outputs)."""

    def __init__(self, K, k, P, p, iterations, status):
        self.K, self.k, self.P, self.p = K, k, P, p
        self.iterations, self.status = iterations, status

    def policy(self, T):
        """The stationary controller as a :class:`Policy` of ``T`` steps: views of ``K``, ``k`` expanded along a time axis."""
        T = int(T)
        tdim = self.K.dim() - 2
        expand = lambda t: t.unsqueeze(tdim).expand(*t.shape[:tdim], T, *t.shape[tdim:])    # noqa: E731
        return Policy(expand(self.K), expand(self.k))


def _as_f32(a, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=torch.float32)
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)


def _as_f64(a, device):
    """The caller's operand in double, with no pass through fp32."""
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=torch.float64)
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)


def _as_column(t, size):
    """``[..., size]`` -> ``[..., size, 1]``; column vectors pass through."""
    if t.dim() >= 2 and t.shape[-1] == 1 and t.shape[-2] == size:
        return t
    return t.unsqueeze(-1)


def _model_shapes(F, f, C, c):
    """Checks the shapes of converted operands; returns ``f, c`` as columns and the batch size (None: un-batched)."""
    n, d = F.shape[-2], F.shape[-1]
    f, c = _as_column(f, n), _as_column(c, d)
    if not (0 < n < d):
        raise ValueError(f"F must be [n, n+m] with m > 0, got {tuple(F.shape)}")
    for name, t, shape in (("f", f, (n, 1)), ("C", C, (d, d)), ("c", c, (d, 1))):
        if tuple(t.shape[-2:]) != shape:
            raise ValueError(f"{name} must end in shape {shape}, got {tuple(t.shape)}")
    batches = {t.shape[0] for t, nd in ((F, 3), (f, 3), (C, 3), (c, 3)) if t.dim() == nd}
    if any(t.dim() not in (2, 3) for t in (F, f, C, c)) or len(batches) > 1:
        raise ValueError("F, f, C, c take at most one leading batch axis of a common size")
    return f, c, (batches.pop() if batches else None)


def _steady_state_limits(max_iter, tol, n, m):
    """``max_iter``, ``tol`` as the C ABI takes them (0 / 0.0: the kernel's defaults), after the front end's checks."""
    if max_iter is None:
        max_iter = 0
    elif int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
    if tol is None:
        tol = 0.0
    elif not (np.isfinite(tol) and tol > 0):
        raise ValueError(f"tol must be a positive finite number, got {tol!r}")
    if n > 32 or m > 32:
        raise ValueError(f"the steady-state kernels serve n <= 32 and m <= 32, got n={n}, m={m}")
    return int(max_iter), float(tol)


def _steady_state_dtype(dtype):
    if dtype not in (None, torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype!r}")
    return torch.float64 if dtype == torch.float64 else torch.float32


_NO_F64_GRAD = ("gradients of the double steady state are an opt-in of the functional form: call "
                "tfmpc.solvers.lqr_steady_state(..., dtype=torch.float64, differentiable=True); otherwise detach the operands "
                "(or call under torch.no_grad()) for dtype=torch.float64, or use the fp32 steady_state(differentiable=True)")


def _steady_state_launch_f64(F, f, C, c, batch_size, max_iter, tol):
    """One tfmpc_lqr_steady_state_f64 launch on contiguous double operands of checked shapes: batched
    ``K, k, P, p, iterations, status``."""
    n, m = F.shape[-2], F.shape[-1] - F.shape[-2]
    lib = _hip.require_gpu()
    Bk = batch_size if batch_size is not None else 1
    dev, dt = F.device, torch.float64
    K = torch.empty((Bk, m, n), device=dev, dtype=dt)
    k = torch.empty((Bk, m, 1), device=dev, dtype=dt)
    P = torch.empty((Bk, n, n), device=dev, dtype=dt)
    p = torch.empty((Bk, n, 1), device=dev, dtype=dt)
    iterations = torch.zeros((Bk,), dtype=torch.int32, device=dev)
    status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
    args = []
    for t in (F, f, C, c):
        args += [_hip.ptr(t), t.stride(0) if t.dim() == 3 else 0]
    rc = lib.tfmpc_lqr_steady_state_f64(Bk, n, m, *args, int(max_iter), float(tol),
                                        _hip.ptr(K), _hip.ptr(k), _hip.ptr(P), _hip.ptr(p),
                                        _hip.ptr(iterations), _hip.ptr(status), _hip.stream())
    _hip.check(rc, "tfmpc_lqr_steady_state_f64")
    return K, k, P, p, iterations, status


def steady_state_f64(F, f, C, c, max_iter=None, tol=None, device=None):
    """The double-precision steady state of the caller's operands (``tfmpc_lqr_steady_state_f64``):
    tensors or numpy arrays of any dtype are taken to float64 directly, never through fp32.  Returns a
    :class:`SteadyState` of float64 tensors (``iterations``, ``status`` int32).  ``C`` must be symmetric to 1e-12 of its
    largest entry.  This is the call without gradients: an operand that requires grad while autograd is recording
    raises ``NotImplementedError`` (``tfmpc.solvers.lqr_steady_state(..., dtype=torch.float64, differentiable=True)``
    serves them)."""
    if tvlqr_grad.wants_grad(*(a for a in (F, f, C, c) if isinstance(a, torch.Tensor))):
        raise NotImplementedError(_NO_F64_GRAD)
    device = torch.device(device) if device is not None else _hip.default_device()
    F, f, C, c = (_as_f64(a, device) for a in (F, f, C, c))
    f, c, batch_size = _model_shapes(F, f, C, c)
    if C.numel() and not bool((C - C.transpose(-1, -2)).abs().amax() <= 1e-12 * C.abs().amax()):
        raise NotImplementedError("the steady state is served for a symmetric C only")
    n, m = F.shape[-2], F.shape[-1] - F.shape[-2]
    max_iter, tol = _steady_state_limits(max_iter, tol, n, m)
    outs = _steady_state_launch_f64(*(t.contiguous() for t in (F, f, C, c)), batch_size, max_iter, tol)
    if batch_size is None:
        outs = tuple(t[0] for t in outs)
    return SteadyState(*outs)


class LQR:

    def __init__(self, F, f, C, c, device=None, symmetric=None):
        """``symmetric``: ``None`` (default) checks once whether ``C`` is symmetric -- the fast kernels' precondition,
        include/tfmpc_hip.h -- which costs two temporaries and a host read-back; ``True`` / ``False`` states it and
        skips the check (construction is then free of synchronisation, e.g. inside a stream capture)."""
        self.device = torch.device(device) if device is not None else _hip.default_device()
        # the caller's TENSOR operands (a reference that keeps them alive with the solver), where the differentiable
        # solve starts; numpy operands cannot require grad (None)
        self._sources = tuple(a if isinstance(a, torch.Tensor) else None for a in (F, f, C, c))
        self.last_grad_status = None
        F, f, C, c = (_as_f32(a, self.device) for a in (F, f, C, c))
        f, c, self.batch_size = _model_shapes(F, f, C, c)
        self.F, self.f, self.C, self.c = (t.contiguous() for t in (F, f, C, c))
        self.last_status = None
        # asymmetry beyond fp32 rounding of a symmetric matrix -> the reference's term-by-term recursion
        if symmetric is not None:
            self.symmetric_cost = bool(symmetric)
        elif self.C.numel() == 0:                      # an empty shard (parallel.shard of a small batch)
            self.symmetric_cost = True
        else:
            asym = (self.C - self.C.transpose(-1, -2)).abs().amax()
            self.symmetric_cost = bool(asym <= 1e-6 * self.C.abs().amax())
        self._suffix = "_f32" if self.symmetric_cost else "_general_f32"

    # -- reference properties (lqr.py:24-34) -----------------------------------
    @property
    def n_dim(self):
        return self.F.shape[-1]

    @property
    def state_size(self):
        return self.F.shape[-2]

    @property
    def action_size(self):
        return self.n_dim - self.state_size

    # -- single-step model (lqr.py:36-57); plain tensor ops, not the hot path ---
    def transition(self, x, u):
        z = torch.cat([_as_f32(x, self.device), _as_f32(u, self.device)], dim=-2)
        return self.F @ z + self.f

    def cost(self, x, u):
        z = torch.cat([_as_f32(x, self.device), _as_f32(u, self.device)], dim=-2)
        zt = z.transpose(-1, -2)
        return 0.5 * (zt @ self.C) @ z + zt @ self.c

    def final_cost(self, x):
        x = _as_f32(x, self.device)
        n = self.state_size
        xt = x.transpose(-1, -2)
        return 0.5 * (xt @ self.C[..., :n, :n]) @ x + xt @ self.c[..., :n, :]

    # -- helpers -----------------------------------------------------------------
    def _operands(self):
        """(tensor, batch stride in elements) for F, f, C, c."""
        out = []
        for t in (self.F, self.f, self.C, self.c):
            out.append((t, t[0].numel() if t.dim() == 3 else 0))
        return out

    def _ptr_args(self):
        args = []
        for t, stride in self._operands():
            args += [_hip.ptr(t), stride]
        return args

    def _resolve_batch(self, x0=None):
        B = self.batch_size
        if x0 is not None and x0.dim() == 3:
            if B is not None and x0.shape[0] != B:
                raise ValueError(f"x0 batch {x0.shape[0]} != problem batch {B}")
            B = x0.shape[0]
        return B

    def _prep_x0(self, x0):
        x0 = _as_f32(x0, self.device)
        n = self.state_size
        x0 = _as_column(x0, n)
        if tuple(x0.shape[-2:]) != (n, 1) or x0.dim() not in (2, 3):
            raise ValueError(f"x0 must be [n,1] or [B,n,1] with n={n}, got {tuple(x0.shape)}")
        return x0.contiguous()

    # -- lqr.py:59-129 -------------------------------------------------------------
    def backward(self, T, differentiable=False):
        """``differentiable=True``: when autograd is recording and a tensor operand requires grad, the returned
        ``Policy`` / ``ValueFn`` hold tensors in the autograd graph (the same bits: this class's own kernel runs the
        recursion), with gradients summed over the horizon from ``tfmpc_tvlqr_backward_vjp_f32`` at time stride 0
        (tfmpc/solvers/tvlqr_backward_grad.py)."""
        T = int(T)
        if differentiable and tvlqr_grad.wants_grad(*self._sources):
            if not self.symmetric_cost:
                raise NotImplementedError("gradients of the Riccati recursion are served for a symmetric C only")
            from tfmpc.solvers import steady_state_grad, tvlqr_backward_grad
            from tfmpc.solvers.tvlqr import TimeVaryingLQR
            problem = tvlqr_grad.Problem(lambda: self._backward_launch(T), lambda: TimeVaryingLQR.from_lqr(self, T), False, self)
            K, k, V, v, const = tvlqr_backward_grad.BackwardFunction.apply(problem, *steady_state_grad.graph_operands(self),
                                                                           None, None)
        else:
            K, k, V, v, const, _ = self._backward_launch(T)
        if self.batch_size is None:
            K, k, V, v, const = K[0], k[0], V[0], v[0], const[0]
        return Policy(K, k), ValueFn(V, v, const)

    def _backward_launch(self, T):
        """One tfmpc_lqr_backward launch: batched ``K, k, V, v, const, status``; sets ``last_status``."""
        lib = _hip.require_gpu()
        n, m = self.state_size, self.action_size
        B = self.batch_size
        Bk = B or 1
        dev = self.device
        K = torch.empty((Bk, T, m, n), device=dev)
        k = torch.empty((Bk, T, m, 1), device=dev)
        V = torch.empty((Bk, T, n, n), device=dev)
        v = torch.empty((Bk, T, n, 1), device=dev)
        const = torch.empty((Bk, T, 1, 1), device=dev)
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        rc = getattr(lib, "tfmpc_lqr_backward" + self._suffix)(Bk, n, m, T, *self._ptr_args(),
                                        _hip.ptr(K), _hip.ptr(k), _hip.ptr(V), _hip.ptr(v), _hip.ptr(const),
                                        _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_backward_f32")
        self.last_status = status
        return K, k, V, v, const, status

    # -- lqr.py:131-161 ------------------------------------------------------------
    def forward(self, policy, x0, T):
        lib = _hip.require_gpu()
        T = int(T)
        n, m = self.state_size, self.action_size
        x0 = self._prep_x0(x0)
        if isinstance(policy, Policy):
            K, k = policy.K, policy.k
        else:       # a plain list of (K_t, k_t) as the reference returns
            tdim = _as_f32(policy[0][0], self.device).dim() - 2
            K = torch.stack([_as_f32(p[0], self.device) for p in policy], dim=tdim)
            k = torch.stack([_as_f32(p[1], self.device) for p in policy], dim=tdim)
        K, k = K.contiguous(), k.contiguous()
        if K.shape[-3] < T:
            raise ValueError(f"policy has {K.shape[-3]} steps, horizon is {T}")
        pol_batched = K.dim() == 4
        B = self._resolve_batch(x0)
        if pol_batched:
            if B is not None and K.shape[0] != B:
                raise ValueError("policy batch does not match")
            B = K.shape[0]
        Bk = B or 1
        if x0.dim() == 2:
            x0 = x0.unsqueeze(0).expand(Bk, n, 1).contiguous()
        dev = self.device
        states = torch.empty((Bk, T + 1, n, 1), device=dev)
        actions = torch.empty((Bk, T, m, 1), device=dev)
        costs = torch.empty((Bk, T + 1, 1, 1), device=dev)
        sK = K[0].numel() if pol_batched else 0
        sk = k[0].numel() if pol_batched else 0
        rc = getattr(lib, "tfmpc_lqr_forward" + self._suffix)(Bk, n, m, T, *self._ptr_args(),
                                       _hip.ptr(K), sK, _hip.ptr(k), sk, _hip.ptr(x0),
                                       _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_forward_f32")
        if B is None:
            states, actions, costs = states[0], actions[0], costs[0]
        return states, actions, costs

    # -- fused backward + forward, device tensors in/out ----------------------------
    def solve_device(self, x0, T, want_policy=False, want_value=False, workspace=None, storage_bf16=False):
        """One kernel launch for ``B`` solves; returns a dict of device tensors
        (``states[B,T+1,n,1]``, ``actions[B,T,m,1]``, ``costs[B,T+1,1,1]``,
        ``status[B]`` and, on request, ``K, k, V, v, const``).  Never synchronises.

        ``storage_bf16=True``: the requested policy / value-function tensors come back as ``torch.bfloat16`` (half the
        bytes of the path's largest outputs, lqr.py:107-129; each value = the fp32 result rounded to nearest even,
        ``tfmpc_lqr_solve_bf16out_f32``); the trajectory stays fp32 and is the one the fp32 gains give."""
        lib = _hip.require_gpu()
        T = int(T)
        n, m = self.state_size, self.action_size
        x0 = self._prep_x0(x0)
        B = self._resolve_batch(x0)
        Bk = B or 1
        if x0.dim() == 2:
            x0 = x0.unsqueeze(0).expand(Bk, n, 1).contiguous()
        dev = self.device
        out = dict(states=torch.empty((Bk, T + 1, n, 1), device=dev),
                   actions=torch.empty((Bk, T, m, 1), device=dev),
                   costs=torch.empty((Bk, T + 1, 1, 1), device=dev),
                   # every LQR kernel writes status[b] of every instance it is launched on: no memset kernel per call
                   status=(torch.zeros if B == 0 else torch.empty)((Bk,), dtype=torch.int32, device=dev))
        odt = torch.bfloat16 if storage_bf16 else torch.float32
        if storage_bf16 and self._suffix != "_f32":
            raise NotImplementedError("16-bit outputs are served for symmetric C (the fast kernels and the wave kernel)")
        if want_policy:
            out.update(K=torch.empty((Bk, T, m, n), device=dev, dtype=odt), k=torch.empty((Bk, T, m, 1), device=dev, dtype=odt))
        if want_value:
            out.update(V=torch.empty((Bk, T, n, n), device=dev, dtype=odt), v=torch.empty((Bk, T, n, 1), device=dev, dtype=odt),
                       const=torch.empty((Bk, T, 1, 1), device=dev, dtype=odt))
        ws_bytes = 0
        if not want_policy or storage_bf16:
            ws_bytes = int(lib.tfmpc_lqr_workspace_bytes(Bk, n, m, T))
            if workspace is None or workspace.numel() * workspace.element_size() < ws_bytes:
                workspace = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
            ws_bytes = workspace.numel() * workspace.element_size()
        entry = "tfmpc_lqr_solve_bf16out_f32" if storage_bf16 else "tfmpc_lqr_solve" + self._suffix
        rc = getattr(lib, entry)(Bk, n, m, T, *self._ptr_args(), _hip.ptr(x0),
                                     _hip.ptr(out["states"]), _hip.ptr(out["actions"]), _hip.ptr(out["costs"]),
                                     _hip.ptr(out.get("K")), _hip.ptr(out.get("k")), _hip.ptr(out.get("V")),
                                     _hip.ptr(out.get("v")), _hip.ptr(out.get("const")), _hip.ptr(out["status"]),
                                     _hip.ptr(workspace), ws_bytes, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_solve_f32")
        self.last_status = out["status"]
        out["batched"] = B is not None
        out["workspace"] = workspace
        return out

    # -- lqr.py:163-166 ------------------------------------------------------------
    def solve(self, x0, T):
        if tvlqr_grad.wants_grad(*self._sources, x0):
            return tvlqr_grad.TensorTrajectory(*self._solve_differentiable(x0, T))
        out = self.solve_device(x0, T)
        states, actions, costs = out["states"], out["actions"], out["costs"]
        if not out["batched"]:
            states, actions, costs = states[0], actions[0], costs[0]
        return trajectory.Trajectory(states, actions, costs)

    def _solve_differentiable(self, x0, T):
        """This class's own solve kernel forward (the same bits as without grad); backward through
        ``tfmpc_tvlqr_vjp_f32`` with time stride 0, i.e. gradients summed over the horizon (tfmpc/solvers/tvlqr_grad.py)."""
        if not self.symmetric_cost:
            raise NotImplementedError("gradients of an LQR solve are served for a symmetric C only")
        from tfmpc.solvers.tvlqr import TimeVaryingLQR
        T = int(T)
        n, d = self.state_size, self.n_dim
        F, f, C, c = (own if a is None else tvlqr_grad.as_f32_graph(a, self.device)
                      for a, own in zip(self._sources, (self.F, self.f, self.C, self.c)))
        f, c = _as_column(f, n), _as_column(c, d)
        x0g = _as_column(tvlqr_grad.as_f32_graph(x0, self.device), n)
        problem = tvlqr_grad.Problem(lambda x: self.solve_device(x, T), lambda: TimeVaryingLQR.from_lqr(self, T), False, self)
        states, actions, costs = tvlqr_grad.SolveFunction.apply(problem, x0g, F, f, C, c, None, None)
        if self._resolve_batch(x0g) is None:
            states, actions, costs = states[0], actions[0], costs[0]
        return states, actions, costs

    # -- infinite horizon (tfmpc_lqr_steady_state_f32 / _f64) ---
    def steady_state(self, max_iter=None, tol=None, differentiable=False, dtype=None):
        """The stationary solution of this problem: the limits of ``backward(T)``'s ``K_0, k_0, V_0, v_0`` as T grows,
        found by the structure-preserving doubling algorithm in one kernel launch.  ``max_iter`` caps the doubling steps
        (default 40), ``tol`` is the relative change of P at which it stops (default 4 fp32 ulps).  Returns a
        :class:`SteadyState`; never synchronises; sets ``last_status``.  An instance without a stabilising solution has
        ``_hip.ST_NOT_STABILISING`` in its status and NaN outputs.

        ``differentiable=True``: when autograd is recording and a tensor operand requires grad, ``K, k, P, p`` are in the
        autograd graph, with gradients from ``tfmpc_lqr_steady_state_vjp_f32`` (tfmpc/solvers/steady_state_grad.py,
        DESIGN.md 3.10); the backward pass's per-instance status goes to ``last_grad_status``.  The outputs are the same
        bits as without grad.

        ``dtype``: ``None`` or ``torch.float32`` is the fp32 kernel.  ``torch.float64`` upcasts the operands this solver
        STORES, which are fp32, and returns the double solution of that fp32-rounded problem as float64 tensors
        (``tfmpc_lqr_steady_state_f64``; ``tol`` then defaults to 4 double ulps): the terminal cost for
        ``TimeVaryingLQR.from_lqr(lqr, T, ss.P, ss.p, dtype=torch.float64)``.  For operands that are double to begin
        with, use ``tfmpc.solvers.lqr_steady_state(..., dtype=torch.float64)``.  This method's gradients are fp32 only
        (double gradients with respect to fp32-rounded stored operands would be a different contract): with
        ``torch.float64``, ``differentiable=True`` or an operand that requires grad raises ``NotImplementedError``;
        ``tfmpc.solvers.lqr_steady_state(..., dtype=torch.float64, differentiable=True)`` serves them."""
        double = _steady_state_dtype(dtype) == torch.float64
        if not self.symmetric_cost:
            raise NotImplementedError("the steady state is served for a symmetric C only")
        grad = tvlqr_grad.wants_grad(*self._sources)
        if double and (grad or differentiable):
            raise NotImplementedError(_NO_F64_GRAD)
        if grad and not differentiable:
            raise NotImplementedError("gradients through the steady state are served with steady_state(differentiable=True) "
                                      "or tfmpc.solvers.lqr_steady_state: otherwise call it under torch.no_grad() or with "
                                      "operands that do not require grad")
        max_iter, tol = _steady_state_limits(max_iter, tol, self.state_size, self.action_size)
        if double:
            outs = _steady_state_launch_f64(*(t.to(torch.float64) for t in (self.F, self.f, self.C, self.c)),
                                            self.batch_size, max_iter, tol)
            self.last_status = outs[-1]
        elif grad:
            from tfmpc.solvers import steady_state_grad
            outs = steady_state_grad.SteadyStateFunction.apply(self, int(max_iter), float(tol),
                                                               *steady_state_grad.graph_operands(self))
        else:
            outs = self._steady_state_launch(int(max_iter), float(tol))
        if self.batch_size is None:
            outs = tuple(t[0] for t in outs)
        return SteadyState(*outs)

    def _steady_state_launch(self, max_iter, tol):
        """One tfmpc_lqr_steady_state_f32 launch on this solver's operands (0 / 0.0 select the kernel's defaults):
        batched ``K, k, P, p, iterations, status``; sets ``last_status``."""
        n, m = self.state_size, self.action_size
        lib = _hip.require_gpu()
        B = self.batch_size
        Bk = B if B is not None else 1
        dev = self.device
        K = torch.empty((Bk, m, n), device=dev)
        k = torch.empty((Bk, m, 1), device=dev)
        P = torch.empty((Bk, n, n), device=dev)
        p = torch.empty((Bk, n, 1), device=dev)
        iterations = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        args = []
        for t in (self.F, self.f, self.C, self.c):        # (batch strides from the layout: an empty batch has no t[0])
            args += [_hip.ptr(t), t.stride(0) if t.dim() == 3 else 0]
        rc = lib.tfmpc_lqr_steady_state_f32(Bk, n, m, *args, int(max_iter), float(tol),
                                            _hip.ptr(K), _hip.ptr(k), _hip.ptr(P), _hip.ptr(p),
                                            _hip.ptr(iterations), _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_steady_state_f32")
        self.last_status = status
        return K, k, P, p, iterations, status

    # -- lqr.py:168-181 ------------------------------------------------------------
    def dump(self, file):
        config = {name: getattr(self, name).cpu().numpy().tolist() for name in ("F", "f", "C", "c")}
        json.dump(config, file)

    @classmethod
    def load(cls, file, device=None):
        config = json.load(file)
        return cls(**{key: np.array(val).astype("f") for key, val in config.items()}, device=device)

"""Time-varying batched LQR on MI355X (``tfmpc_tvlqr_*_f32``, include/tfmpc_hip.h).

The problem of :class:`tfmpc.solvers.lqr.LQR` with a model per step: ``x_{t+1} = F_t z_t + f_t``, stage cost
``1/2 z_t^T C_t z_t + c_t^T z_t`` with ``z_t = [x_t; u_t]``, final cost ``1/2 x_T^T C_fin x_T + c_fin^T x_T``
(default ``C_fin = C_{T-1}[:n,:n]``, ``c_fin = c_{T-1}[:n]``: with every step equal this is exactly ``LQR``'s problem).

Operand shapes: ``F`` is ``[T, n, d]`` (shared by the batch) or ``[B, T, n, d]``; ``f``, ``C``, ``c`` likewise
(vectors as ``[..., size]`` or columns ``[..., size, 1]``).  A time axis of size 1 is broadcast over the horizon with
time stride 0 (no copy).  ``C_final`` is ``[n, n]`` or ``[B, n, n]``, ``c_final`` ``[n]`` / ``[n, 1]`` / ``[B, n(, 1)]``.
``C_t`` and ``C_final`` must be symmetric (the kernels' precondition; there is no general-C path).

Precision: the default ``dtype=torch.float32`` casts every operand to fp32, float64 inputs included, silently.  Pass
``dtype=torch.float64`` for the double-precision kernels (``tfmpc_tvlqr_*_f64``, DESIGN.md 3.14, n <= 32 and m <= 32):
operands, ``x0`` and every output then stay in double.  Gradients of the double solve are opt-in:
``solve(x0, differentiable=True)`` / ``solve_tensors(x0, differentiable=True)`` (``tfmpc_tvlqr_vjp_f64``);
the Riccati recursion's gradients (``backward(differentiable=True)``) are served in fp32 only by the method; in double they
are :func:`tfmpc.solvers.tvlqr_backward` with ``dtype=torch.float64`` (``tfmpc_tvlqr_backward_vjp_f64``).

A few long horizons (B <= 64 or so, T in the hundreds or thousands): ``solve_time_parallel`` /
:func:`tvlqr_solve_time_parallel` cut the horizon into segments that are worked on concurrently
(``tfmpc_tvlqr_solve_time_parallel_f64``; double only).  Their gradients are opt-in as the double
solve's: ``differentiable=True`` saves the forward's gains and value function and differentiates through the segmented
adjoint (``tfmpc_tvlqr_vjp_time_parallel_f64``), which repeats no Riccati step.

A model that REPEATS with period N, over an infinite horizon: ``periodic_steady_state`` /
:func:`tvlqr_periodic_steady_state` take the time axis as one period and return the stationary cycle of gains and value
functions with a per-instance status (``tfmpc_tvlqr_periodic_steady_state_f64``; double only).  Their
gradients are opt-in, as the others': ``differentiable=True`` differentiates through the wrap-around adjoint
(``tfmpc_tvlqr_periodic_vjp_f64``); :func:`tfmpc.solvers.tvlqr_periodic_vjp` is that VJP alone.
"""

import collections

import numpy as np
import torch

from tfmpc import _hip
from tfmpc.solvers import tvlqr_grad
from tfmpc.solvers.lqr import LQR, Policy, ValueFn, _as_column, _as_f32
from tfmpc.utils import trajectory


_DTYPES = (torch.float32, torch.float64)

# The periodic stationary solution: K[(B,)N,m,n], k[(B,)N,m,1], V[(B,)N,n,n], v[(B,)N,n,1] -- V[t], v[t] the
# value function AT step t of the period, so V[0] = P_0 and V_N = V_0 -- residual[(B)], iterations[(B)], status[(B)]
PeriodicSteadyState = collections.namedtuple("PeriodicSteadyState", "K k V v residual iterations status")


def _check_dtype(dtype):
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype!r}")
    return dtype


def _as_dtype(a, device, dtype):
    """``lqr._as_f32`` for either precision: a detached copy on ``device`` in ``dtype``."""
    if dtype == torch.float32:
        return _as_f32(a, device)
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=dtype)
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)


def _is_symmetric(t):
    if t.numel() == 0:
        return True
    tol = 1e-12 if t.dtype == torch.float64 else 1e-6
    return bool((t - t.transpose(-1, -2)).abs().amax() <= tol * t.abs().amax())


class TimeVaryingLQR:

    def __init__(self, F, f, C, c, C_final=None, c_final=None, device=None, symmetric=None, dtype=torch.float32):
        """``symmetric``: ``None`` checks ``C`` (and ``C_final``) once on the device; ``True`` states it and skips the
        check (no synchronisation); ``False`` raises -- only symmetric costs are served.

        ``dtype``: ``torch.float32`` (default) stores fp32 copies of the operands -- float64 inputs are cast down
        silently, as they always were -- and runs the fp32 kernels.  ``torch.float64`` keeps operands, ``x0`` and every
        output in double and runs ``tfmpc_tvlqr_*_f64``; the symmetry check then uses 1e-12 relative in place of 1e-6,
        and an operand or ``x0`` that requires grad is refused unless the solve is called with ``differentiable=True``
        (or the problem is built with ``dtype=torch.float32``)."""
        self.dtype = _check_dtype(dtype)
        self._sfx = "f64" if dtype == torch.float64 else "f32"
        self.device = torch.device(device) if device is not None else _hip.default_device()
        # The caller's TENSOR operands, where the differentiable path starts (numpy operands cannot require grad: None).
        # A reference, not a copy -- but it keeps them alive as long as the solver, e.g. an fp64 / CPU original of a
        # large per-instance model next to its fp32 device copy; drop the solver (or the originals) to free them.
        self._sources = tuple(a if isinstance(a, torch.Tensor) else None for a in (F, f, C, c, C_final, c_final))
        self.last_grad_status = None
        F, f, C, c = (self._cast(a) for a in (F, f, C, c))
        if F.dim() not in (3, 4):
            raise ValueError(f"F must be [T, n, d] or [B, T, n, d], got {tuple(F.shape)}")
        n, d = F.shape[-2], F.shape[-1]
        if not (0 < n < d):
            raise ValueError(f"F must end in [n, n+m] with m > 0, got {tuple(F.shape)}")
        f, c = self._vector(f, n, "f"), self._vector(c, d, "c")
        if C.dim() not in (3, 4) or tuple(C.shape[-2:]) != (d, d):
            raise ValueError(f"C must be [T, d, d] or [B, T, d, d] with d={d}, got {tuple(C.shape)}")
        ops = [F, f, C, c]
        horizons = {t.shape[-3] for t in ops if t.shape[-3] != 1}
        if len(horizons) > 1:
            raise ValueError(f"time axes disagree: {sorted(horizons)} (each must be 1 or the horizon T)")
        self.horizon = horizons.pop() if horizons else 1
        if self.horizon < 1:
            raise ValueError("the horizon must be at least 1 step")
        batches = {t.shape[0] for t in ops if t.dim() == 4}
        if (C_final is None) != (c_final is None):
            raise ValueError("give both C_final and c_final, or neither")
        if C_final is not None:
            C_final, c_final = self._cast(C_final), self._cast(c_final)
            if C_final.dim() not in (2, 3) or tuple(C_final.shape[-2:]) != (n, n):
                raise ValueError(f"C_final must be [n, n] or [B, n, n] with n={n}, got {tuple(C_final.shape)}")
            if c_final.dim() == 1 or (c_final.dim() == 2 and c_final.shape != (n, 1)):
                c_final = c_final.unsqueeze(-1)
            if tuple(c_final.shape[-2:]) != (n, 1) or c_final.dim() not in (2, 3):
                raise ValueError(f"c_final must be [n], [n, 1], [B, n] or [B, n, 1] with n={n}, got {tuple(c_final.shape)}")
            batches |= {t.shape[0] for t in (C_final, c_final) if t.dim() == 3}
            C_final, c_final = C_final.contiguous(), c_final.contiguous()
        if len(batches) > 1:
            raise ValueError(f"batch axes disagree: {sorted(batches)}")
        self.batch_size = batches.pop() if batches else None
        self.F, self.f, self.C, self.c = (self._inner_contiguous(t) for t in ops)
        self.C_final, self.c_final = C_final, c_final
        self.last_status = None
        if symmetric is None:
            symmetric = _is_symmetric(self.C) and (C_final is None or _is_symmetric(C_final))
        if not symmetric:
            raise ValueError("C (and C_final) must be symmetric: the time-varying kernels serve symmetric costs only")

    def _cast(self, a):
        return _as_dtype(a, self.device, self.dtype)

    def _refuse_grad(self, *more, solve=False):
        """Double-precision gradients are opt-in (the Riccati recursion's through ``tvlqr_backward(..., dtype=torch.float64)``
        only): say so before any launch, never downcast."""
        if self.dtype == torch.float64 and tvlqr_grad.wants_grad(*self._sources, *more):
            how = ("pass differentiable=True to solve / solve_tensors for the double-precision gradients, build the problem "
                   "with dtype=torch.float32" if solve else
                   "build the problem with dtype=torch.float32, call tfmpc.solvers.tvlqr_backward(..., dtype=torch.float64) for the "
                   "Riccati recursion's gradients in double")
            raise NotImplementedError(f"gradients of the time-varying LQR in double are not served by this call: {how}, or "
                                      "detach the operands and x0 for a dtype=torch.float64 solve")

    @staticmethod
    def _vector(t, size, name):
        """``[(B,)T, size]`` or ``[(B,)T, size, 1]`` -> ``[(B,)T, size, 1]``."""
        if t.dim() >= 3 and t.shape[-1] == 1 and t.shape[-2] == size:
            out = t
        else:
            out = t.unsqueeze(-1)
        if out.dim() not in (3, 4) or out.shape[-2] != size:
            raise ValueError(f"{name} must be [T, {size}] / [T, {size}, 1] (or with a leading batch axis), got {tuple(t.shape)}")
        return out

    @staticmethod
    def _inner_contiguous(t):
        """Keep views whose per-step matrix is dense row-major (e.g. a time axis expanded with stride 0)."""
        r, cols = t.shape[-2], t.shape[-1]
        if (t.stride(-1) == 1 or cols == 1) and (t.stride(-2) == cols or r == 1):
            return t
        return t.contiguous()

    @classmethod
    def time_invariant(cls, F, f, C, c, T, C_final=None, c_final=None, device=None, symmetric=None, dtype=torch.float32):
        """The time-invariant problem ``F, f, C, c`` over ``T`` steps, from :class:`~tfmpc.solvers.lqr.LQR`'s operand
        shapes (``[n, d]`` or ``[B, n, d]``; vectors ``[size]``, ``[size, 1]`` or with a leading batch axis): each operand
        is converted once and expanded along a time axis of stride 0, no copy per step.  With ``dtype=torch.float64`` this
        is the double-precision solve of an ``LQR`` problem; ``LQR`` itself stores fp32 copies."""
        T = int(T)
        if T < 1:
            raise ValueError("the horizon must be at least 1 step")
        dtype = _check_dtype(dtype)
        dev = torch.device(device) if device is not None else _hip.default_device()

        def convert(a):             # tensors stay in the caller's autograd graph (the fp32 gradients start there)
            if isinstance(a, torch.Tensor):
                return a.to(device=dev, dtype=dtype)
            return _as_dtype(a, dev, dtype)
        F, f, C, c = (convert(a) for a in (F, f, C, c))
        if F.dim() not in (2, 3):
            raise ValueError(f"F must be [n, d] or [B, n, d], got {tuple(F.shape)}")
        n, d = F.shape[-2], F.shape[-1]
        f, c = _as_column(f, n), _as_column(c, d)
        views = [t.unsqueeze(-3).expand(*t.shape[:-2], T, *t.shape[-2:]) for t in (F, f, C, c)]
        return cls(*views, C_final, c_final, device=dev, symmetric=symmetric, dtype=dtype)

    @classmethod
    def from_lqr(cls, lqr, T, C_final=None, c_final=None, dtype=None):
        """The time-invariant problem of ``lqr`` over ``T`` steps as a TV problem: views with time stride 0.  ``C_final``,
        ``c_final`` replace the default final cost, e.g. ``from_lqr(lqr, T, ss.P, ss.p)`` with ``ss = lqr.steady_state()``:
        the stationary value function as terminal cost of a short horizon.  ``C_final`` must be symmetric.

        ``dtype=None`` is the ``lqr``'s own fp32.  ``torch.float64`` upcasts the operands ``lqr`` STORES, which are fp32:
        their rounding to fp32 has already happened (for a problem posed in double, use :meth:`time_invariant`)."""
        T = int(T)
        dtype = torch.float32 if dtype is None else _check_dtype(dtype)
        views = [t.unsqueeze(-3).expand(*t.shape[:-2], T, *t.shape[-2:])
                 for t in (op.to(dtype) for op in (lqr.F, lqr.f, lqr.C, lqr.c))]
        if not lqr.symmetric_cost:
            raise ValueError("only a symmetric C has a time-varying counterpart")
        if C_final is None and c_final is None:
            return cls(*views, device=lqr.device, symmetric=True, dtype=dtype)
        if C_final is None or c_final is None:
            raise ValueError("give both C_final and c_final, or neither")
        # C is known symmetric; C_final is checked here, NaN entries (a flagged steady-state instance) left out of the test
        symmetric = _is_symmetric(torch.nan_to_num(_as_dtype(C_final, lqr.device, dtype), nan=0.0))
        return cls(*views, C_final, c_final, device=lqr.device, symmetric=symmetric, dtype=dtype)

    # -- properties ----------------------------------------------------------------
    @property
    def n_dim(self):
        return self.F.shape[-1]

    @property
    def state_size(self):
        return self.F.shape[-2]

    @property
    def action_size(self):
        return self.n_dim - self.state_size

    # -- per-step model (plain tensor ops, not the hot path) -------------------------
    def _step(self, t_op, t):
        return t_op.select(-3, t if t_op.shape[-3] > 1 else 0)

    def transition(self, x, u, t):
        z = torch.cat([self._cast(x), self._cast(u)], dim=-2)
        return self._step(self.F, t) @ z + self._step(self.f, t)

    def cost(self, x, u, t):
        z = torch.cat([self._cast(x), self._cast(u)], dim=-2)
        zt = z.transpose(-1, -2)
        return 0.5 * (zt @ self._step(self.C, t)) @ z + zt @ self._step(self.c, t)

    def final_cost(self, x):
        x = self._cast(x)
        n = self.state_size
        if self.C_final is not None:
            Cf, cf = self.C_final, self.c_final
        else:
            T = self.horizon
            Cf, cf = self._step(self.C, T - 1)[..., :n, :n], self._step(self.c, T - 1)[..., :n, :]
        xt = x.transpose(-1, -2)
        return 0.5 * (xt @ Cf) @ x + xt @ cf

    # -- helpers -----------------------------------------------------------------------
    def _model_args(self):
        args = []
        for t in (self.F, self.f, self.C, self.c):
            sb = t.stride(0) if t.dim() == 4 else 0
            st = t.stride(-3) if t.shape[-3] > 1 else 0
            args += [_hip.ptr(t), sb, st]
        if self.C_final is None:
            args += [None, 0, None, 0]
        else:
            args += [_hip.ptr(self.C_final), self.C_final.stride(0) if self.C_final.dim() == 3 else 0,
                     _hip.ptr(self.c_final), self.c_final.stride(0) if self.c_final.dim() == 3 else 0]
        return args

    def _prep_x0(self, x0):
        if self.dtype == torch.float32:
            return LQR._prep_x0(self, x0)
        n = self.state_size
        x0 = _as_column(self._cast(x0), n)
        if tuple(x0.shape[-2:]) != (n, 1) or x0.dim() not in (2, 3):
            raise ValueError(f"x0 must be [n,1] or [B,n,1] with n={n}, got {tuple(x0.shape)}")
        return x0.contiguous()

    def _entry(self, lib, name):
        """``tfmpc_tvlqr_<name>_f32`` or its ``_f64`` twin, and the name for error messages."""
        full = f"tfmpc_tvlqr_{name}_{self._sfx}"
        return getattr(lib, full), full

    def _resolve_batch(self, x0=None):
        return LQR._resolve_batch(self, x0)

    # -- backward / forward / solve ------------------------------------------------------
    def backward(self, differentiable=False):
        """The Riccati recursion: ``(Policy, ValueFn)``.  ``differentiable=True``: when autograd is recording and a tensor
        operand requires grad, their tensors are in the autograd graph, with gradients from
        ``tfmpc_tvlqr_backward_vjp_f32`` (tfmpc/solvers/tvlqr_backward_grad.py); the backward pass's
        per-instance status goes to ``last_grad_status``.  The outputs are the same bits as without grad.
        With ``dtype=torch.float64`` that request raises ``NotImplementedError`` (this method's gradients are fp32 only):
        the double gradients are ``tfmpc.solvers.tvlqr_backward(..., dtype=torch.float64)``."""
        if differentiable:
            self._refuse_grad()
        if differentiable and tvlqr_grad.wants_grad(*self._sources):
            from tfmpc.solvers import tvlqr_backward_grad as bgrad
            problem = tvlqr_grad.Problem(self._backward_launch, lambda: self, True, self)
            K, k, V, v, const = bgrad.BackwardFunction.apply(problem, *bgrad.tv_graph_operands(self))
        else:
            K, k, V, v, const, _ = self._backward_launch()
        if self.batch_size is None:
            K, k, V, v, const = K[0], k[0], V[0], v[0], const[0]
        return Policy(K, k), ValueFn(V, v, const)

    def _backward_launch(self):
        """One tfmpc_tvlqr_backward_f32 / _f64 launch: batched ``K, k, V, v, const, status``; sets ``last_status``."""
        lib = _hip.require_gpu()
        n, m, T = self.state_size, self.action_size, self.horizon
        B = self.batch_size
        Bk = B if B is not None else 1
        dev, dt = self.device, self.dtype
        K = torch.empty((Bk, T, m, n), device=dev, dtype=dt)
        k = torch.empty((Bk, T, m, 1), device=dev, dtype=dt)
        V = torch.empty((Bk, T, n, n), device=dev, dtype=dt)
        v = torch.empty((Bk, T, n, 1), device=dev, dtype=dt)
        const = torch.empty((Bk, T, 1, 1), device=dev, dtype=dt)
        status = torch.zeros((Bk,), dtype=torch.int32, device=dev)
        fn, name = self._entry(lib, "backward")
        rc = fn(Bk, n, m, T, *self._model_args(), _hip.ptr(K), _hip.ptr(k), _hip.ptr(V),
                _hip.ptr(v), _hip.ptr(const), _hip.ptr(status), _hip.stream())
        _hip.check(rc, name)
        self.last_status = status
        return K, k, V, v, const, status

    def forward(self, policy, x0):
        lib = _hip.require_gpu()
        n, m, T = self.state_size, self.action_size, self.horizon
        x0 = self._prep_x0(x0)
        if isinstance(policy, Policy):
            K, k = policy.K, policy.k
        elif isinstance(policy, tuple) and len(policy) == 2 and all(isinstance(t, torch.Tensor) and t.dim() >= 3 for t in policy):
            K, k = policy                   # (K[(B,)T,m,n], k[(B,)T,m,1]) as stacked tensors
        else:
            tdim = self._cast(policy[0][0]).dim() - 2
            K = torch.stack([self._cast(p[0]) for p in policy], dim=tdim)
            k = torch.stack([self._cast(p[1]) for p in policy], dim=tdim)
        if self.dtype == torch.float64:      # (a policy computed elsewhere, e.g. in fp32, is taken in double)
            K, k = self._cast(K), self._cast(k)
        K, k = K.contiguous(), k.contiguous()
        if K.shape[-3] < T:
            raise ValueError(f"policy has {K.shape[-3]} steps, horizon is {T}")
        if K.shape[-3] != T:            # the kernels read K[b][t] at b * T * m * n + t * m * n
            K, k = K.narrow(-3, 0, T).contiguous(), k.narrow(-3, 0, T).contiguous()
        pol_batched = K.dim() == 4
        B = self._resolve_batch(x0)
        if pol_batched:
            if B is not None and K.shape[0] != B:
                raise ValueError("policy batch does not match")
            B = K.shape[0]
        Bk = B if B is not None else 1
        if x0.dim() == 2:
            x0 = x0.unsqueeze(0).expand(Bk, n, 1).contiguous()
        dev, dt = self.device, self.dtype
        states = torch.empty((Bk, T + 1, n, 1), device=dev, dtype=dt)
        actions = torch.empty((Bk, T, m, 1), device=dev, dtype=dt)
        costs = torch.empty((Bk, T + 1, 1, 1), device=dev, dtype=dt)
        sK = K[0].numel() if pol_batched else 0
        sk = k[0].numel() if pol_batched else 0
        fn, name = self._entry(lib, "forward")
        rc = fn(Bk, n, m, T, *self._model_args(), _hip.ptr(K), sK, _hip.ptr(k), sk,
                _hip.ptr(x0), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs), _hip.stream())
        _hip.check(rc, name)
        if B is None:
            states, actions, costs = states[0], actions[0], costs[0]
        return states, actions, costs

    def solve_device(self, x0, want_policy=False, want_value=False, workspace=None, want_v=False):
        """One kernel launch for ``B`` solves; a dict of device tensors shaped like ``LQR.solve_device``'s
        (``states[B,T+1,n,1]``, ``actions[B,T,m,1]``, ``costs[B,T+1,1,1]``, ``status[B]``, on request
        ``K, k, V, v, const``; ``want_v``: ``v`` alone, what the double-precision gradients keep).  Never synchronises."""
        lib = _hip.require_gpu()
        n, m, T = self.state_size, self.action_size, self.horizon
        x0 = self._prep_x0(x0)
        B = self._resolve_batch(x0)
        Bk = B if B is not None else 1
        if x0.dim() == 2:
            x0 = x0.unsqueeze(0).expand(Bk, n, 1).contiguous()
        dev, dt = self.device, self.dtype
        out = dict(states=torch.empty((Bk, T + 1, n, 1), device=dev, dtype=dt),
                   actions=torch.empty((Bk, T, m, 1), device=dev, dtype=dt),
                   costs=torch.empty((Bk, T + 1, 1, 1), device=dev, dtype=dt),
                   status=(torch.zeros if Bk == 0 else torch.empty)((Bk,), dtype=torch.int32, device=dev))
        if want_policy:
            out.update(K=torch.empty((Bk, T, m, n), device=dev, dtype=dt), k=torch.empty((Bk, T, m, 1), device=dev, dtype=dt))
        if want_value:
            out.update(V=torch.empty((Bk, T, n, n), device=dev, dtype=dt), v=torch.empty((Bk, T, n, 1), device=dev, dtype=dt),
                       const=torch.empty((Bk, T, 1, 1), device=dev, dtype=dt))
        elif want_v:
            out.update(v=torch.empty((Bk, T, n, 1), device=dev, dtype=dt))
        ws_bytes = 0
        if not want_policy:
            size = dt.itemsize
            query = lib.tfmpc_tvlqr_workspace_bytes_f64 if dt == torch.float64 else lib.tfmpc_tvlqr_workspace_bytes
            ws_bytes = int(query(Bk, n, m, T))
            if workspace is None or workspace.numel() * workspace.element_size() < ws_bytes or workspace.data_ptr() % size:
                workspace = torch.empty((max(ws_bytes, size) + size - 1) // size, dtype=dt, device=dev)
            ws_bytes = workspace.numel() * workspace.element_size()
        fn, name = self._entry(lib, "solve")
        rc = fn(Bk, n, m, T, *self._model_args(), _hip.ptr(x0),
                _hip.ptr(out["states"]), _hip.ptr(out["actions"]), _hip.ptr(out["costs"]),
                _hip.ptr(out.get("K")), _hip.ptr(out.get("k")), _hip.ptr(out.get("V")),
                _hip.ptr(out.get("v")), _hip.ptr(out.get("const")), _hip.ptr(out["status"]),
                _hip.ptr(workspace), ws_bytes, _hip.stream())
        _hip.check(rc, name)
        self.last_status = out["status"]
        out["batched"] = B is not None
        out["workspace"] = workspace
        return out

    # -- one long horizon on many waves (tfmpc_tvlqr_solve_time_parallel_f64) ---------------
    def default_segments(self, batch_size=None):
        """The ``segments`` that :meth:`solve_time_parallel` picks for ``segments=None``, fitted to
        profiles/tvlqr_time_parallel_rate.json.  In units of one sequential step a step of a segment costs
        2.7 (condense + expand) and a segment 2.3 (its two solves in the serial stitch), so the time is
        ``2.7 ceil(T / P) + 2.3 P``, least at ``P = sqrt(1.2 T)``; ``P`` is capped by the condense waves the device keeps
        resident (five per compute unit) shared among the batch, and is 1 -- the sequential kernel -- where that time is
        not below ``T``."""
        B = max(batch_size if batch_size is not None else (self.batch_size or 1), 1)
        T = self.horizon
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count if self.device.type == "cuda" else 256
        segments = min(int(round((1.2 * T) ** 0.5)), (5 * cus) // B, T)
        if segments < 2 or 2.7 * -(-T // segments) + 2.3 * segments >= T:
            return 1
        return segments

    def default_vjp_segments(self, batch_size=None):
        """The ``segments`` of the segmented adjoint (``tfmpc_tvlqr_vjp_time_parallel_f64``) where the forward's were not
        given, fitted to profiles/tvlqr_time_parallel_grad_rate.json as :meth:`default_segments` was.  In
        units of one step of the sequential VJP (25.5 us) a step of a segment costs 0.45 (condense and both expands), a
        segment 0.22 (its two matrix-vector products in the serial stitches) and the call 4 (its launches), so the time is
        ``0.45 ceil(T / P) + 0.22 P + 4``, least at ``P = sqrt(2.1 T)``: more, shorter segments than the forward's, whose
        boundaries cost ten times as much.  The optimum did not move with the batch and the sequential VJP did not win
        again at any measured batch (B <= 4096 at T = 512: it repeats the factorisation, this call does not), so there is
        no cap in ``batch_size``; the answer is 1 -- ``tfmpc_tvlqr_vjp_f64`` -- where the model's time is not below ``T``."""
        T = self.horizon
        segments = min(int(round((2.1 * T) ** 0.5)), T)
        if segments < 2 or 0.45 * -(-T // segments) + 0.22 * segments + 4 >= T:
            return 1
        return segments

    def solve_time_parallel(self, x0, segments=None, want_policy=False, want_value=False, differentiable=False):
        """The solve with the horizon cut into ``segments`` pieces that are condensed, stitched and expanded concurrently
        (DESIGN.md 3.19): for a few long horizons, where one wavefront per instance leaves the device idle.  A
        :class:`Trajectory`; with ``want_policy`` / ``want_value`` a tuple ``(trajectory, K, k)``, ``(trajectory, V, v)`` or
        ``(trajectory, K, k, V, v)`` of device tensors (no ``const``: the value function's constant term is not carried
        across segments).  ``segments=None`` picks :meth:`default_segments`; a value above the horizon is clamped, 1 is the
        sequential solve, bit for bit.  ``last_status`` is set as in :meth:`solve_device`.  Double precision only.

        Gradients are opt-in: with ``differentiable=True``, autograd recording and an operand or ``x0`` requiring grad, the
        result is a :class:`~tfmpc.solvers.tvlqr_grad.TensorTrajectory` in the autograd graph (``K, k, V, v`` stay plain
        tensors) whose backward is the segmented adjoint (``tfmpc_tvlqr_vjp_time_parallel_f64``) with the
        forward's ``segments`` (:meth:`default_vjp_segments` where none were given); every gradient is fp64 and has its
        operand's shape, and ``last_grad_status`` gets the backward's status.  Without the flag that request raises
        ``NotImplementedError``; ``solve(x0, differentiable=True)`` is the sequential alternative."""
        if differentiable and self.dtype == torch.float64 and tvlqr_grad.wants_grad(*self._sources, x0):
            states, actions, costs, out = self._time_parallel_tensors(x0, segments)
            fields = (("K", "k") if want_policy else ()) + (("V", "v") if want_value else ())
            more = [out[name] if out["batched"] else out[name][0] for name in fields]
            traj = tvlqr_grad.TensorTrajectory(states, actions, costs)
            return (traj, *more) if more else traj
        out = self._time_parallel_device(x0, segments, want_policy, want_value)
        fields = ("states", "actions", "costs") + (("K", "k") if want_policy else ()) + (("V", "v") if want_value else ())
        tensors = [out[name] if out["batched"] else out[name][0] for name in fields]
        traj = trajectory.Trajectory(*tensors[:3])
        return (traj, *tensors[3:]) if tensors[3:] else traj

    def _time_parallel_tensors(self, x0, segments=None):
        """``(states, actions, costs, out)``: the time-parallel solve in the autograd graph of the caller's operands and
        ``x0`` (``SolveTimeParallelFunctionF64``; without the batch axis for an un-batched problem), and the forward's device
        dict (``K, k, V, v, batched, segments``: plain batched tensors)."""
        if segments is not None and int(segments) < 1:
            raise ValueError(f"segments must be at least 1, got {segments}")
        out = {}

        def run(x):
            out.update(self._time_parallel_device(x, segments, True, True))
            return out
        given = segments is not None
        problem = tvlqr_grad.Problem(run, lambda: self, True, self,
                                     lambda B, used: used if given else self.default_vjp_segments(B))
        states, actions, costs = tvlqr_grad.SolveTimeParallelFunctionF64.apply(problem, *self._graph_operands(x0))
        if not out["batched"]:
            states, actions, costs = states[0], actions[0], costs[0]
        return states, actions, costs, out

    def _time_parallel_device(self, x0, segments=None, want_policy=False, want_value=False):
        """One tfmpc_tvlqr_solve_time_parallel_f64 call; a dict of batched device tensors as :meth:`solve_device`'s (no
        ``const``).  Never synchronises."""
        if self.dtype != torch.float64:
            raise NotImplementedError("the time-parallel solve is served in double only: build the problem with "
                                      "dtype=torch.float64")
        if tvlqr_grad.wants_grad(*self._sources, x0):
            raise NotImplementedError("gradients of the time-parallel solve are opt-in: pass differentiable=True to "
                                      "solve_time_parallel / tvlqr_solve_time_parallel for the segmented adjoint, use "
                                      "solve(x0, differentiable=True) for the sequential one, or detach the operands and x0")
        if segments is not None and int(segments) < 1:
            raise ValueError(f"segments must be at least 1, got {segments}")
        lib = _hip.require_gpu()
        n, m, T = self.state_size, self.action_size, self.horizon
        x0 = self._prep_x0(x0)
        B = self._resolve_batch(x0)
        Bk = B if B is not None else 1
        if x0.dim() == 2:
            x0 = x0.unsqueeze(0).expand(Bk, n, 1).contiguous()
        segments = self.default_segments(Bk) if segments is None else int(segments)
        dev, dt = self.device, self.dtype
        states = torch.empty((Bk, T + 1, n, 1), device=dev, dtype=dt)
        actions = torch.empty((Bk, T, m, 1), device=dev, dtype=dt)
        costs = torch.empty((Bk, T + 1, 1, 1), device=dev, dtype=dt)
        status = (torch.zeros if Bk == 0 else torch.empty)((Bk,), dtype=torch.int32, device=dev)
        K = k = V = v = None
        if want_policy:
            K, k = torch.empty((Bk, T, m, n), device=dev, dtype=dt), torch.empty((Bk, T, m, 1), device=dev, dtype=dt)
        if want_value:
            V, v = torch.empty((Bk, T, n, n), device=dev, dtype=dt), torch.empty((Bk, T, n, 1), device=dev, dtype=dt)
        ws_bytes = int(lib.tfmpc_tvlqr_time_parallel_workspace_bytes_f64(Bk, n, m, T, segments))
        workspace = torch.empty(max(ws_bytes // 8, 1), dtype=dt, device=dev)
        rc = lib.tfmpc_tvlqr_solve_time_parallel_f64(
            Bk, n, m, T, *self._model_args(), _hip.ptr(x0), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs),
            _hip.ptr(K), _hip.ptr(k), _hip.ptr(V), _hip.ptr(v), None, _hip.ptr(status), segments,
            _hip.ptr(workspace), workspace.numel() * 8, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_solve_time_parallel_f64")
        self.last_status = status
        out = dict(states=states, actions=actions, costs=costs, status=status, K=K, k=k, V=V, v=v)
        out = {name: t for name, t in out.items() if t is not None}
        out.update(batched=B is not None, segments=segments, workspace=workspace)
        return out

    # -- the model as one period of an infinite horizon (tfmpc_tvlqr_periodic_steady_state_f64) -----
    def default_periodic_vjp_segments(self, batch_size=None):
        """The ``segments`` of the periodic steady state's backward (``tfmpc_tvlqr_periodic_vjp_f64``) where
        none were given, fitted to profiles/tvlqr_periodic_grad_rate.json as :meth:`default_vjp_segments` was (measured, not
        inherited from it).  A step of a segment costs 67 us (its three sweeps), a segment 7.6 us (its products in the two
        serial stitches) and the call about 50 us (its launches), so the time is ``67 ceil(N / P) + 7.6 P + 50`` us, least at
        ``P = sqrt(8.8 N)`` (67 at N = 512, where 64 measured best; 190 at N = 4096, where 128 and 256 tie within 2 %).
        ``P`` is capped by the sweep waves that the batch leaves each compute unit (four: 16 at B = 64 and one segment at
        B = 4096 measured best), and by N."""
        B = max(batch_size if batch_size is not None else (self.batch_size or 1), 1)
        N = self.horizon
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count if self.device.type == "cuda" else 256
        return max(min(int(round((8.8 * N) ** 0.5)), (4 * cus) // B, N), 1)

    def periodic_steady_state(self, segments=None, max_iter=0, tol=0.0, differentiable=False):
        """The model's time axis taken as ONE PERIOD of an infinite-horizon problem whose model repeats: the stationary
        cycle of gains and value functions, a :class:`PeriodicSteadyState` of float64 device tensors ``K[(B,)N,m,n]``,
        ``k[(B,)N,m,1]``, ``V[(B,)N,n,n]``, ``v[(B,)N,n,1]`` (``V[t], v[t]`` AT step t: ``V[0]`` is the value function at
        phase 0, and ``V_N = V_0``), ``residual[(B)]`` (one more turn around the period from ``V[0], v[0]``, relative: a
        self-check), ``iterations[(B)]`` (doubling steps) and ``status[(B)]`` (0, or ``TFMPC_ST_NOT_PD`` / ``_SINGULAR`` /
        ``_NOT_STABILISING`` / ``_NAN``; a flagged instance has NaN in its outputs).  ``last_status`` is set.  One period is
        condensed into a segment element on ``segments`` concurrent waves (``None``: :meth:`default_segments`), the
        element is doubled until it is stationary, and every segment is expanded.  ``max_iter=0`` is 40
        doubling steps, ``tol=0`` is 4 ``DBL_EPSILON``.  Never synchronises.

        The result composes with the finite solvers: ``forward((K, k), x0)`` rolls one period out, and
        ``TimeVaryingLQR(F[:, :L], ..., C_final=V[:, L % N], c_final=v[:, L % N], dtype=torch.float64)`` is the finite
        solve that ends at phase ``L`` of the cycle.

        Double precision only (``NotImplementedError`` for an fp32 problem: build it with ``dtype=torch.float64``); the
        periodic problem has no final cost (``ValueError`` if the problem carries ``C_final`` / ``c_final``).

        Gradients are opt-in: with ``differentiable=True``, autograd recording and a tensor operand requiring grad, ``K, k,
        V, v`` are in the autograd graph of the caller's operands (taken to double inside the graph) and keep the bits of
        the call without the flag -- the forward launch is unchanged, on the detached operands.  The backward is the
        wrap-around adjoint (``tfmpc_tvlqr_periodic_vjp_f64``) with the forward's ``segments`` where they
        were given, else :meth:`default_periodic_vjp_segments`, and this call's ``max_iter`` and ``tol`` for its Smith
        doubling; an output the loss does not use is a NULL upstream pointer, every gradient is float64 in its operand's
        shape (an operand without a batch axis: summed over the batch; a time axis of 1: summed over time), and
        ``last_grad_status`` gets the backward's status.  Without the flag an operand that requires grad raises
        ``NotImplementedError``."""
        if self.dtype != torch.float64:
            raise NotImplementedError("the periodic steady state is served in double only: build the problem with "
                                      "dtype=torch.float64")
        if self.C_final is not None:
            raise ValueError("the periodic infinite-horizon problem has no final cost: build the problem without "
                             "C_final / c_final")
        wants = tvlqr_grad.wants_grad(*self._sources)
        if wants and not differentiable:
            raise NotImplementedError("gradients of the periodic steady state are opt-in: pass differentiable=True to "
                                      "periodic_steady_state / tvlqr_periodic_steady_state for the wrap-around adjoint "
                                      "(DESIGN.md 3.26), or detach the operands")
        if segments is not None and int(segments) < 1:
            raise ValueError(f"segments must be at least 1, got {segments}")
        max_iter, tol = int(max_iter), float(tol)
        if max_iter < 0 or not tol >= 0.0:
            raise ValueError(f"max_iter and tol must not be negative, got {max_iter}, {tol}")
        B = self.batch_size
        Bk = B if B is not None else 1
        given = segments is not None
        segments = int(segments) if given else self.default_segments(Bk)
        if wants:
            from tfmpc.solvers.tvlqr_backward_grad import tv_graph_operands
            out = tvlqr_grad.PeriodicSteadyStateFunctionF64.apply(
                self, lambda: self._periodic_launch(segments, max_iter, tol),
                segments if given else self.default_periodic_vjp_segments(Bk), max_iter, tol, *tv_graph_operands(self)[:4])
        else:
            out = self._periodic_launch(segments, max_iter, tol)
        return PeriodicSteadyState(*(out if B is not None else (t[0] for t in out)))

    def _periodic_launch(self, segments, max_iter, tol):
        """One tfmpc_tvlqr_periodic_steady_state_f64 call: batched ``K, k, V, v, residual, iterations, status``; sets
        ``last_status``."""
        lib = _hip.require_gpu()
        n, m, N = self.state_size, self.action_size, self.horizon
        Bk = self.batch_size if self.batch_size is not None else 1
        dev, dt = self.device, self.dtype
        K = torch.empty((Bk, N, m, n), device=dev, dtype=dt)
        k = torch.empty((Bk, N, m, 1), device=dev, dtype=dt)
        V = torch.empty((Bk, N, n, n), device=dev, dtype=dt)
        v = torch.empty((Bk, N, n, 1), device=dev, dtype=dt)
        residual = torch.empty((Bk,), device=dev, dtype=dt)
        iterations = torch.empty((Bk,), dtype=torch.int32, device=dev)
        status = (torch.zeros if Bk == 0 else torch.empty)((Bk,), dtype=torch.int32, device=dev)
        ws_bytes = int(lib.tfmpc_tvlqr_periodic_workspace_bytes_f64(Bk, n, m, N, segments))
        workspace = torch.empty(max(ws_bytes // 8, 1), dtype=dt, device=dev)
        rc = lib.tfmpc_tvlqr_periodic_steady_state_f64(
            Bk, n, m, N, *self._model_args()[:12], segments, max_iter, tol, _hip.ptr(K), _hip.ptr(k), _hip.ptr(V),
            _hip.ptr(v), _hip.ptr(residual), _hip.ptr(iterations), _hip.ptr(status), _hip.ptr(workspace),
            workspace.numel() * 8, _hip.stream())
        _hip.check(rc, "tfmpc_tvlqr_periodic_steady_state_f64")
        self.last_status = status
        return K, k, V, v, residual, iterations, status

    def solve(self, x0, differentiable=False):
        """A :class:`Trajectory`; with autograd recording and an operand or ``x0`` requiring grad, a
        :class:`~tfmpc.solvers.tvlqr_grad.TensorTrajectory` differentiable through ``tfmpc_tvlqr_vjp_f32``.  With
        ``dtype=torch.float64`` that needs ``differentiable=True`` (gradients in double through ``tfmpc_tvlqr_vjp_f64``) and
        is a ``NotImplementedError`` without it; the flag changes nothing for an fp32 problem."""
        if not differentiable:
            self._refuse_grad(x0, solve=True)
        if tvlqr_grad.wants_grad(*self._sources, x0):
            states, actions, costs = self.solve_tensors(x0, differentiable)
            return tvlqr_grad.TensorTrajectory(states, actions, costs)
        out = self.solve_device(x0)
        states, actions, costs = out["states"], out["actions"], out["costs"]
        if not out["batched"]:
            states, actions, costs = states[0], actions[0], costs[0]
        return trajectory.Trajectory(states, actions, costs)

    def _graph_operands(self, x0):
        """``(x0, F, f, C, c, C_final, c_final)`` as the differentiable Functions take them: the caller's tensors converted
        inside the autograd graph and shaped as the solver holds them."""
        n, d = self.state_size, self.n_dim
        dev = self.device
        src = self._sources

        def op(i, own, shape=None):       # a non-tensor operand needs no grad: the solver's own copy, already shaped
            if src[i] is None:
                return own
            t = tvlqr_grad.as_graph(src[i], dev, self.dtype)
            return shape(t) if shape else t
        F, C = op(0, self.F), op(2, self.C)
        f = op(1, self.f, lambda t: self._vector(t, n, "f"))
        c = op(3, self.c, lambda t: self._vector(t, d, "c"))
        Cf = op(4, self.C_final)
        cf = op(5, self.c_final, lambda t: t.unsqueeze(-1) if t.dim() == 1 or (t.dim() == 2 and t.shape != (n, 1)) else t)
        x0g = _as_column(tvlqr_grad.as_graph(x0, dev, self.dtype), n)
        return x0g, F, f, C, c, Cf, cf

    def solve_tensors(self, x0, differentiable=False):
        """``(states[(B,)T+1,n,1], actions[(B,)T,m,1], costs[(B,)T+1,1,1])`` as tensors; in the autograd graph of the
        caller's operands and ``x0`` when autograd is recording (gradients: tfmpc/solvers/tvlqr_grad.py).  With
        ``dtype=torch.float64`` the graph is built only with ``differentiable=True`` (every gradient then fp64, the
        trajectory the same bits as without grad); without the flag that request raises ``NotImplementedError``."""
        if not differentiable:
            self._refuse_grad(x0, solve=True)
        double = self.dtype == torch.float64
        if not tvlqr_grad.wants_grad(*self._sources, x0):
            out = self.solve_device(x0)
            states, actions, costs = out["states"], out["actions"], out["costs"]
        else:
            problem = tvlqr_grad.Problem(lambda x: self.solve_device(x, want_v=double), lambda: self, True, self)
            function = tvlqr_grad.SolveFunctionF64 if double else tvlqr_grad.SolveFunction
            states, actions, costs = function.apply(problem, *self._graph_operands(x0))
        if self._resolve_batch(self._prep_x0(x0.detach() if isinstance(x0, torch.Tensor) else x0)) is None:
            states, actions, costs = states[0], actions[0], costs[0]
        return states, actions, costs


def tvlqr_solve_time_parallel(F, f, C, c, x0, segments=None, C_final=None, c_final=None, differentiable=False):
    """The time-parallel double-precision solve of :meth:`TimeVaryingLQR.solve_time_parallel` on operands in
    :class:`TimeVaryingLQR`'s shapes: ``(states, actions, costs)`` as float64 device tensors -- ``states[(B,)T+1,n,1]``,
    ``actions[(B,)T,m,1]``, ``costs[(B,)T+1,1,1]``.  ``F`` must be float64 (tensor or numpy): an fp32 problem raises
    ``NotImplementedError``, as does an operand or ``x0`` that requires grad -- unless ``differentiable=True``: the three
    tensors are then in the autograd graph of every tensor operand and ``x0`` that requires grad, with fp64 gradients from
    the segmented adjoint (``tfmpc_tvlqr_vjp_time_parallel_f64``)."""
    kind = F.dtype if isinstance(F, torch.Tensor) else np.asarray(F).dtype
    if kind not in (torch.float64, np.float64):
        raise NotImplementedError(f"the time-parallel solve is served in double only (dtype=torch.float64), F is {kind}")
    device = next((t.device for t in (F, f, C, c, x0) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    tv = TimeVaryingLQR(F, f, C, c, C_final, c_final, device=device, dtype=torch.float64)
    if differentiable and tvlqr_grad.wants_grad(*tv._sources, x0):
        return tv._time_parallel_tensors(x0, segments)[:3]
    out = tv._time_parallel_device(x0, segments)
    states, actions, costs = out["states"], out["actions"], out["costs"]
    return (states, actions, costs) if out["batched"] else (states[0], actions[0], costs[0])


def tvlqr_periodic_steady_state(F, f, C, c, segments=None, max_iter=0, tol=0.0, differentiable=False):
    """:meth:`TimeVaryingLQR.periodic_steady_state` on operands in :class:`TimeVaryingLQR`'s shapes, their time axis one
    period: a :class:`PeriodicSteadyState`.  ``F`` must be float64 (tensor or numpy): an fp32 problem raises
    ``NotImplementedError``, as does an operand that requires grad -- unless ``differentiable=True``: ``K, k, V, v`` are
    then in the autograd graph of every tensor operand that requires grad, with fp64 gradients from the wrap-around
    adjoint (``tfmpc_tvlqr_periodic_vjp_f64``)."""
    kind = F.dtype if isinstance(F, torch.Tensor) else np.asarray(F).dtype
    if kind not in (torch.float64, np.float64):
        raise NotImplementedError(f"the periodic steady state is served in double only (dtype=torch.float64), F is {kind}")
    device = next((t.device for t in (F, f, C, c) if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None)
    tv = TimeVaryingLQR(F, f, C, c, device=device, dtype=torch.float64)
    return tv.periodic_steady_state(segments, max_iter, tol, differentiable)


__all__ = ["TimeVaryingLQR", "PeriodicSteadyState", "tvlqr_solve_time_parallel", "tvlqr_periodic_steady_state"]

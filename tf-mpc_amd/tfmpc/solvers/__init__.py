"""Solvers of the hot path: :mod:`tfmpc.solvers.lqr` (Riccati sweep + rollout) and :mod:`tfmpc.solvers.ilqr`
(control-limited iLQR), both thin ctypes front ends of ``tfmpc/_lib/libtfmpc_hip.so``."""

from tfmpc.solvers.tvlqr import TimeVaryingLQR  # noqa: E402,F401  (time-varying LQR, tfmpc_tvlqr_*_f32)
from tfmpc.solvers.tvlqr import tvlqr_solve_time_parallel  # noqa: E402,F401  (one long horizon on many waves, tfmpc_tvlqr_solve_time_parallel_f64)
from tfmpc.solvers.tvlqr import PeriodicSteadyState, tvlqr_periodic_steady_state  # noqa: E402,F401  (periodic infinite-horizon LQR, tfmpc_tvlqr_periodic_steady_state_f64)
from tfmpc.solvers.tvlqr_grad import tvlqr_solve  # noqa: E402,F401  (differentiable TV-LQR solve, tfmpc_tvlqr_vjp_f32 / _f64)
from tfmpc.solvers.tvlqr_grad import tvlqr_vjp_time_parallel  # noqa: E402,F401  (segmented adjoint of the double solve, tfmpc_tvlqr_vjp_time_parallel_f64)
from tfmpc.solvers.steady_state_grad import lqr_steady_state, lqr_steady_state_vjp  # noqa: E402,F401  (differentiable steady state, tfmpc_lqr_steady_state_vjp_f32 / _f64)
from tfmpc.solvers.box_lqr_grad import box_lqr_solve, tvlqr_box_vjp  # noqa: E402,F401  (differentiable control-limited LQR, tfmpc_tvlqr_box_vjp_f32)
from tfmpc.solvers.tvlqr_box import tvlqr_box_solve  # noqa: E402,F401  (control-limited TV-LQR forward, tfmpc_tvlqr_box_solve_f32)
from tfmpc.solvers.tvlqr_backward_grad import tvlqr_backward, tvlqr_backward_vjp  # noqa: E402,F401  (differentiable Riccati recursion, tfmpc_tvlqr_backward_vjp_f32 / _f64)
from tfmpc.solvers.tvlqr_grad import tvlqr_periodic_vjp  # noqa: E402,F401  (gradients of the periodic steady state, tfmpc_tvlqr_periodic_vjp_f64)

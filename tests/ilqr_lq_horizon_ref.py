"""TEST INFRASTRUCTURE ONLY -- workload, references and defect model of the horizon tests of the three matrix-core iLQR
kernels for the LQ env (tests/test_ilqr_lq_horizon_cpu.py, tests/test_ilqr_lq_horizon_gpu.py):

* ``lq_mfma``      tf-mpc_amd/csrc/ilqr_lq_mfma.hip      n <= 16, m <= 8, unbounded; the trajectories live in LDS for all T under a
                                                         40 KB cap; gain rings 4 deep (exact 16 x 8) and 2 deep (shape-generic form)
* ``lq_box_mfma``  tf-mpc_amd/csrc/ilqr_lq_box_mfma.hip  the same shapes, bounded actions; 48 KB cap; gain ring 4 deep
* ``lq_mfma32``    tf-mpc_amd/csrc/ilqr_lq_mfma32.hip    up to 32 x 16, any T; rollouts in LDS chunks of 48 steps, ring 4 deep (1 deep
                                                         with TFMPC_ILQR_LQ_REUSE=0)

What goes wrong at a horizon edge goes wrong by ONE step: the clamped prefetch of a ring (``t + ring < T ? t + ring : T - 1``), the
ring's phase when T is no multiple of its depth, a horizon shorter than the ring, the carry of x into row 0 of the next chunk.  A
time-invariant LQ problem has near-stationary gains in mid-horizon, so such a fault shows only where the gains still change from step to
step -- in the last steps of the horizon -- or while the trajectory still moves.  ``boundary_steps`` lists the steps a horizon puts
inside that logic, ``defect_ratio`` what a fault there does to the solution in units of the GPU tests' budget; the CPU file decides
from it which (kernel, T, step) are tests and which are hidden.

Workload: ``problems.make_lqr_batch_fast`` with every instance's F rescaled so that the spectral radius of its state block ``F[:, :n]``
is 0.9 (the unscaled draws of the other iLQR files reach 1.44 open loop and the start rollout overflows long before T = 148), start
actions 0.1 N(0, 1), clipped to the box in the bounded case.

Budget rule, restated from tests/test_tvlqr_gpu.py::_check: per field, per instance, ratio = max error against the fp64 restatement
/ max(the fp32 restatement's max error, 1e-6 * scale) with scale = max(1, max |fp64|); median over instances <= 2.5 and every instance
<= 10.  Pure numpy, no GPU.
"""

import functools

import numpy as np

import problems
from oracle import envs_ref, ilqr_ref

FIELDS = ("states", "actions", "costs")
MEDIAN_BAR, MAX_BAR = 2.5, 10.0
RADIUS = 0.9

# ---- the kernels' constants (tests/test_ilqr_lq_horizon_cpu.py holds them to the sources) -----------------------------------------
LQ_MFMA = dict(kDyn=512 + 16 * 20, kZld=24, slabs=2, cap=40 * 1024, ring_exact=4, ring_generic=2)
LQ_BOX = dict(kDyn=768 + 16 * 20, kZld=24, slabs=3, cap=48 * 1024, ring=4)
LQ_MFMA32 = dict(chunk=48, ring=4, ring_no_reuse=1)


def lds_bytes(kernel, T):
    """``ilqr_lq_mfma_lds_bytes`` / ``box_lds_bytes``: kDyn floats of operands, ``slabs`` trajectories of T + 1 rows of kZld floats,
    as many cost rows of T + 1 floats rounded up to 4, 8 floats of scalars."""
    Tp = T + 1
    return (kernel["kDyn"] + kernel["slabs"] * Tp * kernel["kZld"] + kernel["slabs"] * ((Tp + 3) & ~3) + 8) * 4


def t_max(kernel):
    T = 1
    while lds_bytes(kernel, T + 1) <= kernel["cap"]:
        T += 1
    return T


# ---- the horizons of the GPU file ---------------------------------------------------------------------------------------------------
# kernel family -> {(n, m, form): horizons}.  form: "exact" | "generic" (TFMPC_ILQR_KERNEL=lq_generic at (16, 8); any other shape is
# generic anyway).
T_LQ_EXACT = (1, 2, 3, 4, 5, 9, 13, 51, 53, 104, 186, 187)
T_LQ_GENERIC = (1, 2, 3, 5, 187)
T_BOX = (1, 2, 3, 5, 51, 147, 148)
T_MFMA32 = (1, 2, 3, 5, 47, 48, 49, 50, 51, 52, 97, 99, 145, 257)
T_LONG = 1000
SHAPES_LQ_GENERIC = ((12, 6), (16, 8))
SHAPES_BOX = ((16, 8), (12, 6))
SHAPES_MFMA32 = ((32, 16), (17, 9), (20, 16))
T_SWITCH_LQ, T_SWITCH_BOX = 187, 148          # the last horizons the LDS caps admit; one more runs on the wave kernel


BOUND = 0.8                                   # bounded cases: a third to a half of the final actions sit on it (the CPU file checks)
ATOL_CONFIG = (("atol", 1e-12), ("max_iterations", 4))      # every instance runs all four passes: three gain-reusing ones in a row


def batch_of(T, bounded=False):
    """Instances per case: 16, fewer where the oracle solves (python, per instance; the box-QP ones are the slow ones) would take a
    case past a few seconds.  With 5 the bounded cases can still tell an 80 % share (4 of 5) from less."""
    if bounded:
        return 16 if T <= 5 else 8 if T <= 51 else 5
    return 16 if T <= 104 else 8 if T <= 257 else 4


def ring_of(kernel, n, m, form="exact"):
    if kernel == "lq_mfma":
        return LQ_MFMA["ring_exact"] if (n, m) == (16, 8) and form == "exact" else LQ_MFMA["ring_generic"]
    if kernel == "lq_box_mfma":
        return LQ_BOX["ring"]
    return LQ_MFMA32["ring"]


def boundary_steps(T, ring, chunk=None):
    """Steps t* of a T-step rollout that sit inside the ring or chunk logic, as {t*: kind}:

    ``last-prefetch``  the step filled by the LAST in-range prefetch (issued at T - 1 - ring: ``t + ring < T`` holds for the last time);
    ``first-clamped``  does not exist as a consumed step (a clamped prefetch is never used), so the fault it guards against is a clamp
                       that is off by one: the last step T - 1 taking what a clamp to T - 2 (or to 0) would have loaded;
    ``prologue``       the steps the ring's prologue fills (``d < T ? d : T - 1``), present when T < ring as a clamped prologue;
    ``chunk-start``    row 0 of an LDS chunk after the first (carry of x, ring phase at the chunk's first step)."""
    out = {}
    for t in range(min(ring, T)):
        out[t] = "prologue"
    if T - 1 >= ring:
        out[T - 1] = "last-prefetch"
    if chunk:
        for t in range(chunk, T, chunk):
            out[t] = "chunk-start"
    return out


# ---- workload -----------------------------------------------------------------------------------------------------------------------
def workload(B, n, m, seed, T, bound=None):
    """float64 ``F[B,n,d] f[B,n] C[B,d,d] c[B,d]``, ``x0[B,n]`` and ``u0[B,T,m]`` (both exactly representable in fp32)."""
    F, f, C, c, x0 = problems.make_lqr_batch_fast(B, n, m, seed=seed)
    rho = np.abs(np.linalg.eigvals(F[:, :, :n])).max(axis=1)
    F = F * (RADIUS / rho)[:, None, None]
    u0 = 0.1 * np.random.default_rng(seed + 1).normal(size=(B, T, m))
    if bound is not None:
        u0 = np.clip(u0, -bound, bound)
    return F, f, C, c, x0.astype(np.float32).astype(np.float64), u0.astype(np.float32).astype(np.float64)


def seed_of(n, m):
    return 100 * n + m


def _env(F, f, C, c, bound, dtype):
    kw = {} if bound is None else dict(low=-bound, high=bound)
    return envs_ref.LQEnv(F, f, C, c, dtype=dtype, **kw)


def _solver(F, f, C, c, bound, dtype, kwargs):
    return ilqr_ref.ILQRRef(_env(F, f, C, c, bound, dtype), dtype=dtype, **dict(kwargs))


@functools.lru_cache(maxsize=None)
def oracle(n, m, T, seed, B, bound=None, kwargs=()):
    """The fp64 and the fp32 ``ILQRRef`` solutions of every instance: two lists of dicts ``states[T+1,n] actions[T,m] costs[T+1]
    iterations``.  Cached per case; callers must not write into the arrays.  ``kwargs``: sorted tuple of solver options."""
    F, f, C, c, x0, u0 = workload(B, n, m, seed, T, bound)
    out = []
    for dtype in (np.float64, np.float32):
        sols = []
        for b in range(B):
            x, u, cs, it = _solver(F[b], f[b], C[b], c[b], bound, dtype, kwargs).solve(x0[b], T, u_init=u0[b][..., None])
            sols.append(dict(states=x, actions=u, costs=cs, iterations=it))
        out.append(sols)
    return out[0], out[1]


def budget(r64, r32, name):
    ref = r64[name]
    scale = max(1.0, float(np.abs(ref).max()))
    return max(float(np.abs(r32[name].astype(np.float64) - ref).max()), 1e-6 * scale)


def ratios(got, r64, r32, name, idx=None):
    """Per instance: max error of ``got[b][name]`` against fp64 over the budget."""
    idx = range(len(r64)) if idx is None else idx
    return np.array([float(np.abs(np.asarray(got[b][name], dtype=np.float64) - r64[b][name]).max()) / budget(r64[b], r32[b], name)
                     for b in idx])


def check_budget(got, r64, r32, what="", fields=FIELDS, idx=None, report=None):
    """The budget rule.  ``report``: a dict that receives the worst ratio per field (for printing)."""
    for name in fields:
        r = ratios(got, r64, r32, name, idx)
        if report is not None:
            report[name] = (float(np.median(r)), float(r.max()))
        assert np.isfinite(r).all(), (what, name)
        assert np.median(r) <= MEDIAN_BAR and r.max() <= MAX_BAR, (what, name, float(np.median(r)), float(r.max()))


# ---- defect model ---------------------------------------------------------------------------------------------------------------------
def first_pass(F, f, C, c, x0, u0, bound=None):
    """The fp64 start rollout and the gains of the first backward pass (mu = 0, as ``solve`` starts): ``(solver, x_hat, u_hat, K, k)``."""
    o = _solver(F, f, C, c, bound, np.float64, ())
    T = u0.shape[0]
    x_hat, u_hat, _ = o.start(x0, T, u_init=u0[..., None])
    K, k, _, _, _ = o.backward(T, u_hat, *o.derivatives(x_hat, u_hat), mu=0.0)
    return o, x_hat, u_hat, K, k


def rollout(o, x_hat, u_hat, K, k, alpha=1.0, gain_of=None, early_row_at=None):
    """``ILQRRef.forward`` (ilqr.py:174-212) with ONE step wrong: ``gain_of = {t*: s}`` uses the gains of step s at t*;
    ``early_row_at = t*`` takes x_{t*-1} for the state of step t* (what row 0 of a chunk holds when the carry copies one row early).
    Without either it IS ``ILQRRef.forward`` (the CPU file pins that).  -> dict ``states actions costs``."""
    env, T = o.env, u_hat.shape[0]
    F, f, C, c, n = env.F, env.f, env.C, env.c, env.state_size              # the LQ env written out (F z + f, 1/2 z'Cz + c'z): no torch call per step
    stage = lambda z, C_, c_: (0.5 * (z.T @ C_ @ z) + c_.T @ z).item()
    gain_of = gain_of or {}
    state = x_hat[0]
    states, actions, costs = [state], [], []
    for t in range(T):
        if early_row_at is not None and t == early_row_at:
            state = states[t - 1]
        g = gain_of.get(t, t)
        delta_u = alpha * k[g] + K[g] @ (state - x_hat[t])
        action = np.clip(u_hat[t] + delta_u, o.low, o.high)
        z = np.concatenate([state, action])
        costs.append(stage(z, C, c))
        state = F @ z + f
        actions.append(action)
        states.append(state)
    costs.append(stage(state, C[:n, :n], c[:n]))
    return dict(states=np.stack(states)[..., 0], actions=np.stack(actions)[..., 0], costs=np.asarray(costs))


def defects(t, kind, T):
    """The faults tried at boundary step t*: name -> kwargs of ``rollout``.  (a) the neighbours' gains, (b) the gains a wrong clamp
    would hold (step 0, step T - 1), (c) at a chunk start the state one row early.  Faults that are no fault (same index) are left out."""
    out = {}
    for name, s in (("gain t*-1", t - 1), ("gain t*+1", t + 1), ("gain clamped to 0", 0), ("gain clamped to T-1", T - 1)):
        if 0 <= s < T and s != t:
            out.setdefault(f"{name}", dict(gain_of={t: s}))
    if kind == "chunk-start":
        out["row one early"] = dict(early_row_at=t)
    return out


def defect_ratio(healthy, faulty, r64, r32):
    """How far a fault moves the first search rollout, in units of the GPU assertion's per-instance budget: max over the fields."""
    return max(float(np.abs(faulty[name] - healthy[name]).max()) / budget(r64, r32, name) for name in FIELDS)

"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the LQR rollout (``tfmpc_lqr_forward_f32``, ``LQR.forward``; the
reference's ``lqr.py:131-161``) under ANY policy, and the workload of the long-horizon tests of the matrix-core kernels
(tests/test_lqr_long_horizon_cpu.py, tests/test_lqr_long_horizon_gpu.py).

Why a policy of its own: the solver's gains ``K_t`` are stationary except in the last 9 - 17 steps of a long horizon and
the closed-loop state sits at its fixed point after as many, so a rollout under them cannot tell step ``t`` from step
``t + 1`` in the middle of the horizon -- which is where the kernels change LDS chunks.  ``per_step_gains`` gives every
step a gain of its own around the stationary one, and keeps the state moving.

``dtype=np.float64`` is the truth, ``dtype=np.float32`` the error budget (the same recursion in the kernel's precision).
Pure numpy, no GPU.
"""

import functools

import numpy as np

import problems
from oracle import c_oracle

# Rollout chunk lengths of the two kernels (timesteps staged in LDS between bulk stores) and the depth of the 16 x 8
# kernel's gain ring; tests/test_lqr_long_horizon_cpu.py holds them to the kernel sources.  The 32 x 16 kernel prefetches
# one step ahead (no ring): its horizons use the same offset, there just one more horizon off the boundary.
CHUNK = {"mfma_16x8": 52, "mfma_32x16": 48}
RING = 4

# (n, m) -> the name tfmpc_lqr_kernel_name reports.  Exact and zero-padded shapes of both kernels.  No shape with one
# action: this workload is not stabilised by one input (the fp64 rollout of (16, 1) passes 1e28 by T = 97), which would
# break the reference instead of testing the kernel.
SHAPES = {(16, 8): "mfma_16x8", (12, 5): "mfma_16x8 (zero-padded)", (5, 3): "mfma_16x8 (zero-padded)",
          (32, 16): "mfma_32x16", (24, 12): "mfma_32x16 (zero-padded)", (17, 9): "mfma_32x16 (zero-padded)"}

FIELDS = ("states", "actions", "costs")


def chunk(n, m):
    return CHUNK[SHAPES[(n, m)].split(" ")[0]]


def rollout_horizons(c, r=RING):
    """One short of a chunk, exactly one, one more, one ring turn more; the same around two chunks; into a fourth; long."""
    return [c - 1, c, c + 1, c + r, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c + 1, 257, 1000]


def split_points(c, r=RING):
    """(T1, T): a rollout over T steps cut after T1; the second part crosses a chunk boundary of its own."""
    return [(T1, T1 + c + 3) for T1 in (1, c - 1, c, c + 1, c + r - 1, 2 * c)]


def solve_horizons(c, r=RING):
    """Horizons of a full solve: the chunk boundary 1 - 9 steps before the end, where the solver's own gains still change
    from step to step, then boundaries in mid-horizon (seen by the bitwise comparisons between entry points)."""
    return [c + 1, c + 2, c + r, c + 9, 2 * c + 1, 257, 1000]


def boundaries(c, T):
    """Steps t* < T whose state is row 0 of a chunk after the first."""
    return list(range(c, T, c))


def workload(B, n, m, seed):
    """``make_lqr_batch_fast`` with the spectral radius of F brought to ~1.5: open loop unstable, Riccati sweep well inside
    fp32 (the workload of tests/test_lqr_mfma32_gpu.py).  float64 ``F[B,n,d] f[B,n] C[B,d,d] c[B,d] x0[B,n]``."""
    F, f, C, c, x0 = problems.make_lqr_batch_fast(B, n, m, seed=seed)
    F *= 1.5 / np.sqrt(n)
    return F, f, C, c, x0


def stationary_gain(F, f, C, c, T=200):
    """``K_0[B,m,n]`` of a T-step solve by the fp64 C oracle: the stationary feedback, to far below fp32 rounding."""
    B, n = F.shape[0], F.shape[1]
    ref = c_oracle.lqr_solve(F, f, C, c, np.zeros((B, n)), T, dtype=np.float64, want_policy=True)
    assert ref["status"] == 0
    return ref["K"][:, 0]


def per_step_gains(K0, T, rng):
    """``K_t = K0 + 0.05 max|K0| N(0,1)`` entrywise and ``k_t ~ N(0,1)`` for one instance: ``K[T,m,n]``, ``k[T,m]``."""
    m, n = K0.shape
    K = K0[None] + 0.05 * np.abs(K0).max() * rng.normal(size=(T, m, n))
    k = rng.normal(size=(T, m))
    return K, k


def batch_gains(F, f, C, c, T, seed):
    """``per_step_gains`` for every instance of a batch: ``K[B,T,m,n]``, ``k[B,T,m]``."""
    rng = np.random.default_rng(seed)
    Ks, ks = zip(*[per_step_gains(K0, T, rng) for K0 in stationary_gain(F, f, C, c)])
    return np.stack(Ks), np.stack(ks)


EXTRA_STEPS = 7         # a policy may be longer than the horizon: steps the rollout must not read


@functools.lru_cache(maxsize=None)
def case(n, m, B):
    """THE case of a shape, shared by the CPU checks of the workload and the GPU tests: ``problem = (F, f, C, c, x0)`` and
    per-step gains ``K[B,Tmax+EXTRA_STEPS,m,n]``, ``k[B,...,m]`` drawn once for the longest horizon.  A shorter horizon
    rolls out a prefix of them, so what the CPU checks establish at the longest horizon holds at every other.

    The seed was CHOSEN (among 3n+m, 5n+m, ... 97n+m) for the third of those checks: that under the solver's own gains
    an off-by-one at the first chunk boundary is hidden.  That depends on how fast an instance's closed loop forgets x0
    (spectral radius 0.56 - 0.72 on this workload; 0.72^52 is not yet below fp32 rounding), so some seeds hold an instance
    that still moves at step 52.  The thresholds of the checks were not touched."""
    problem = workload(B, n, m, seed=13 * n + m)
    T = max(rollout_horizons(chunk(n, m))) + EXTRA_STEPS
    K, k = batch_gains(*problem[:4], T, seed=31 * n + m)
    return dict(problem=problem, K=K, k=k)


@functools.lru_cache(maxsize=None)
def solve_case(n, m, B):
    """The problem of the full-solve tests (seeded as tests/test_lqr_mfma32_gpu.py seeds its own)."""
    return workload(B, n, m, seed=97 * n + m)


def stage_cost(C, c, z):
    return 0.5 * (z @ C @ z) + c @ z


def rollout(F, f, C, c, K, k, x0, T, dtype=np.float64):
    """One instance: ``u_t = K_t x_t + k_t``, ``x_{t+1} = F [x_t; u_t] + f``, stage cost ``1/2 z'Cz + c'z`` with
    ``z = [x; u]``, final cost the stage cost with ``u = 0``.  ``F[n,d] f[n] C[d,d] c[d] K[>=T,m,n] k[>=T,m] x0[n]``, all
    cast to ``dtype`` first (as the kernel's caller casts to fp32).  -> dict ``states[T+1,n] actions[T,m] costs[T+1]``."""
    F, f, C, c, K, k, x = (np.asarray(a, dtype=dtype) for a in (F, f, C, c, K, k, x0))
    n, d = F.shape
    states, actions, costs = np.empty((T + 1, n), dtype), np.empty((T, d - n), dtype), np.empty(T + 1, dtype)
    states[0] = x
    for t in range(T):
        u = K[t] @ x + k[t]
        z = np.concatenate([x, u])
        costs[t] = stage_cost(C, c, z)
        x = F @ z + f
        states[t + 1], actions[t] = x, u
    costs[T] = stage_cost(C[:n, :n], c[:n], x)
    return dict(states=states, actions=actions, costs=costs)


def rollout_batch(F, f, C, c, K, k, x0, T, dtype=np.float64):
    """``rollout`` per instance -> list of dicts."""
    return [rollout(F[b], f[b], C[b], c[b], K[b], k[b], x0[b], T, dtype) for b in range(x0.shape[0])]


def ratios(got, r64, r32, name):
    """Per instance: max error of ``got[b][name]`` against fp64, over the fp32 restatement's own max error floored at
    1e-6 of the output's scale."""
    out = []
    for b in range(len(r64)):
        ref = r64[b][name]
        budget = max(float(np.abs(r32[b][name].astype(np.float64) - ref).max()), 1e-6 * float(np.abs(ref).max()))
        out.append(float(np.abs(np.asarray(got[b][name], dtype=np.float64) - ref).max()) / budget)
    return np.array(out)

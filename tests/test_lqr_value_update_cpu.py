"""CPU companion of ``test_lqr_value_update_gpu.py``: the workload SEES a wrong value update.

The GPU test checks the chain v' = q_x + Q_xu k of the matrix-core sweep through the outputs of the solve, against budgets whose floor is
1e-6 of a tensor's scale and which let at most 10 BUDGET = 50 floors through.  Here the fp64 recursion is restated in numpy (checked
against the C oracle) with the two faults such a chain can have -- the whole sum dropped (v' = q_x), and its last term dropped (action
m - 1 left out) -- and either must move the gains k of every instance by at least 1000 floors, at every shape of the GPU test and at
every horizon that uses a value update (T = 2, 3, 5, 53; T = 1 uses none)."""

import functools

import numpy as np
import pytest

import problems
from oracle import c_oracle

NINST = 5
SHAPES = [(16, 8), (5, 3), (7, 8), (16, 3)]
HORIZONS = (2, 3, 5, 53)
FLOOR = 1e-6          # the GPU test's budget floor, as a fraction of the tensor's scale
FACTOR = 1000.0


def _backward_k(F, f, C, c, T, fault=None):
    """k[T, m] of one instance by the recursion of the sweep in fp64 (Schur-complement form, V symmetrised).  ``fault``: None,
    "no_sum" (v' = q_x) or "last_action" (action m - 1 left out of the sum)."""
    n = F.shape[0]
    m = F.shape[1] - n
    V, v = C[:n, :n].copy(), c[:n].copy()
    ks = np.empty((T, m))
    for t in range(T - 1, -1, -1):
        Q = C + F.T @ V @ F
        q = c + F.T @ (V @ f + v)
        Qxx, Qux, Quu = Q[:n, :n], Q[n:, :n], Q[n:, n:]
        K = -np.linalg.solve(Quu, Qux)
        k = -np.linalg.solve(Quu, q[n:])
        ks[t] = k
        Vn = Qxx + Qux.T @ K
        V = 0.5 * (Vn + Vn.T)
        if fault == "no_sum":
            v = q[:n].copy()
        elif fault == "last_action":
            v = q[:n] + Qux[:m - 1].T @ k[:m - 1]
        else:
            v = q[:n] + Qux.T @ k
    return ks


@functools.lru_cache(maxsize=None)
def _instances(n, m):
    return problems.make_lqr_batch_spd(NINST, n, m, seed=17 * n + m)


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_a_wrong_value_update_moves_the_gains(n, m, T):
    F, f, C, c, x0 = _instances(n, m)
    ref = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    for b in range(NINST):
        want = ref["k"][b]
        scale = np.abs(want).max()
        good = _backward_k(F[b], f[b], C[b], c[b], T)
        # the restatement is the oracle's recursion (far below the floor: what is measured next is the fault, not the restatement)
        assert np.abs(good - want).max() <= 1e-3 * FLOOR * scale, (n, m, T, b, np.abs(good - want).max() / scale)
        for fault in ("no_sum", "last_action"):
            moved = np.abs(_backward_k(F[b], f[b], C[b], c[b], T, fault) - want).max() / (FLOOR * scale)
            print(f"({n}, {m}) T={T} instance {b} {fault}: k moves by {moved:.3g} floors")
            assert moved >= FACTOR, (n, m, T, b, fault, moved)

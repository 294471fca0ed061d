"""CPU companion of ``test_lqr_forward_value_chain_gpu.py``: the two forms of v' in the fp64 recursion, restated in numpy.

The sweep of lqr_mfma16x8.hip finishes v' inside the forward elimination of [Q_uu | Q_ux | q_u] (LDL^T without pivoting on the upper
triangle): with m^_a the reduced row a and x^_a = -m^_a / d_a,

    v' = q_x + (sum_a x^_a[q_u] m^_a)        (= q_x + Q_xu k, written with the factors of Q_uu instead of the solved k)

while V' = Q_xx + Q_xu K and the gains K, k go through the back substitution as before.  K does not depend on v; k does.  Here:

* both forms give the same k to 1e-6 relative (per instance, max over the horizon; measured <= 1.7e-12 over these cases);
* the workload SEES the two faults the new form can have -- the rows of Q_ux taken unreduced as m^ (the operand of the old form left in
  place), and action m - 1 left out of the sum.  The GPU test lets at most 10 BUDGET = 50 floors (1e-6 of a tensor's scale) through on
  k; either fault must move k of every instance by at least 1000 floors, at every shape of the GPU test and at every horizon that uses
  a value update (T = 2, 3, 5, 53; T = 1 uses none).  Measured over these cases: the smallest move is 1.88e3 floors
  ((16, 3), T = 2, last action dropped: 37 times what the GPU test lets through); unreduced rows move k by 1.8e4 floors or more
  ((5, 3), T = 2)."""

import functools

import numpy as np
import pytest

import problems
from oracle import c_oracle

NINST = 5
SHAPES = [(16, 8), (5, 3), (7, 8), (16, 3)]
HORIZONS = (2, 3, 5, 53)
FLOOR = 1e-6          # the GPU test's budget floor, as a fraction of the tensor's scale
FACTOR = 1000.0       # twenty times the 50 floors the GPU test lets through
AGREE = 1e-6


def _eliminate(Quu, Y):
    """Forward elimination without pivoting, upper triangle of Q_uu only.  Y = [Q_ux | q_u].  Returns m^ (rows as they stood when they
    became the pivot row), x^ = -m^ / d for the payload, and the multipliers -L[s][p] as L[p, s] (s > p)."""
    m = Quu.shape[0]
    R = np.concatenate([Quu, Y], axis=1)
    X = np.zeros_like(R)
    for p in range(m):
        X[p] = -R[p] / R[p, p]
        for s in range(p + 1, m):
            R[s] += X[p, s] * R[p]
    return R[:, m:], X[:, m:], X[:, :m]


def _backward_k(F, f, C, c, T, form, fault=None):
    """k[T, m] of one instance in fp64.  ``form``: "gain" (v' = q_x + Q_xu k) or "forward" (v' from m^, x^); V' = Q_xx + Q_xu K in both.
    ``fault`` ("forward" only): "unreduced" (the rows of Q_ux as they came in for m^) or "last_action" (action m - 1 left out)."""
    n = F.shape[0]
    m = F.shape[1] - n
    V, v = C[:n, :n].copy(), c[:n].copy()
    ks = np.empty((T, m))
    for t in range(T - 1, -1, -1):
        Q = C + F.T @ V @ F
        q = c + F.T @ (V @ f + v)
        Qxx, Qux, Quu = Q[:n, :n], Q[n:, :n], Q[n:, n:]
        Y = np.concatenate([Qux, q[n:, None]], axis=1)
        Mh, Xh, L = _eliminate(Quu, Y)
        Kk = Xh.copy()                          # back substitution: X_p = x^_p + sum_{s > p} (-L[s][p]) X_s
        for p in range(m - 2, -1, -1):
            for s in range(m - 1, p, -1):
                Kk[p] += L[p, s] * Kk[s]
        K, k = Kk[:, :n], Kk[:, n]
        ks[t] = k
        Vn = Qxx + Qux.T @ K
        V = 0.5 * (Vn + Vn.T)
        if form == "gain":
            v = q[:n] + Qux.T @ k
        else:
            if fault == "unreduced":
                Mh = Y
            last = m - 1 if fault == "last_action" else m
            v = q[:n] + Mh[:last, :n].T @ Xh[:last, n]
    return ks


@functools.lru_cache(maxsize=None)
def _instances(n, m):
    return problems.make_lqr_batch_spd(NINST, n, m, seed=17 * n + m)


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_both_forms_give_the_same_gains(n, m, T):
    F, f, C, c, x0 = _instances(n, m)
    ref = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    for b in range(NINST):
        want = ref["k"][b].reshape(T, m)
        scale = np.abs(want).max()
        gain = _backward_k(F[b], f[b], C[b], c[b], T, "gain")
        forward = _backward_k(F[b], f[b], C[b], c[b], T, "forward")
        # the restatement is the oracle's recursion
        assert np.abs(gain - want).max() <= AGREE * scale, (n, m, T, b, np.abs(gain - want).max() / scale)
        diff = np.abs(forward - gain).max() / scale
        print(f"({n}, {m}) T={T} instance {b}: the two forms differ by {diff:.3g} of k's scale")
        assert diff <= AGREE, (n, m, T, b, diff)


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_a_wrong_forward_chain_moves_the_gains(n, m, T):
    F, f, C, c, x0 = _instances(n, m)
    for b in range(NINST):
        want = _backward_k(F[b], f[b], C[b], c[b], T, "forward")
        scale = np.abs(want).max()
        for fault in ("unreduced", "last_action"):
            moved = np.abs(_backward_k(F[b], f[b], C[b], c[b], T, "forward", fault) - want).max() / (FLOOR * scale)
            print(f"({n}, {m}) T={T} instance {b} {fault}: k moves by {moved:.3g} floors")
            assert moved >= FACTOR, (n, m, T, b, fault, moved)

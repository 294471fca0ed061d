"""The trimmed sweep of the matrix-core LQR kernel (lqr_mfma16x8.hip) where the trimming can show (``-m gpu``):

* the last sweep step (t = 0) of a launch without value outputs is peeled and stops at its gains -- at T = 1 that step is the
  whole sweep, at T = 2, 3 the loop in front of it runs once or twice;
* ``v`` enters ``W_1`` as the accumulator of its product, which touches the offset column (``f``, ``c`` non-zero) and the
  constant of the value function.

Rule of ``test_lqr_gpu.py::test_mfma_kernel_on_padded_shapes``: per instance the ratio of |gpu - fp64 oracle| to
|fp32 oracle - fp64 oracle| (floored at 1e-6 of the tensor's scale) has median <= 2.5, 0.9 quantile <= 2 BUDGET, max <= 10 BUDGET.
The instantiations with and without value outputs and the one sized for four resident waves must agree bit for bit."""

import functools

import numpy as np
import pytest
import torch

import problems
from oracle import c_oracle
from tfmpc import _hip
from tfmpc.solvers.lqr import LQR

pytestmark = pytest.mark.gpu
BUDGET = 5.0
B = 64
TRAJ = ("states", "actions", "costs", "K", "k")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(kind, n, m, T):
    """Problem and its two oracle solves, made once per case."""
    if kind == "fast":
        F, f, C, c, x0 = problems.make_lqr_batch_fast(B, n, m, seed=41 * n + 7 * m + T)
        F *= 0.4
    else:
        F, f, C, c, x0 = problems.make_lqr_batch_spd(B, n, m, seed=91)
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True, want_value=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True, want_value=True)
    return (F, f, C, c, x0), ref64, ref32


def _check_ratios(out, ref64, ref32, keys, what):
    for key in keys:
        got = _np(out[key]).reshape(ref64[key].shape)
        assert np.isfinite(got).all(), (what, key)
        ratios = []
        for b in range(B):
            scale = np.abs(ref64[key][b]).max()
            e32 = max(np.abs(ref32[key][b].astype(np.float64) - ref64[key][b]).max(), 1e-6 * scale)
            ratios.append(np.abs(got[b] - ref64[key][b]).max() / e32)
        med, q9, top = np.median(ratios), np.quantile(ratios, 0.9), max(ratios)
        print(f"{what} {key}: median {med:.2f} q0.9 {q9:.2f} max {top:.2f}")
        assert med <= 2.5 and q9 <= 2 * BUDGET and top <= 10 * BUDGET, (what, key, med, q9, top)


def _three_solves(n, m, T):
    (F, f, C, c, x0), ref64, ref32 = _case("fast", n, m, T)
    assert _hip.require_gpu().tfmpc_lqr_kernel_name(n, m, T).startswith(b"mfma_16x8")
    lqr = LQR(F, f, C, c)
    full = lqr.solve_device(x0, T, want_policy=True, want_value=True)
    lean = lqr.solve_device(x0, T, want_policy=True)
    with _hip.option("TFMPC_LQR_WAVES", "4"):
        lean4 = lqr.solve_device(x0, T, want_policy=True)
    torch.cuda.synchronize()
    for out in (full, lean, lean4):
        assert int(out["status"].abs().sum()) == 0
    what = f"({n}, {m}) T={T}"
    _check_ratios(full, ref64, ref32, TRAJ, what)
    for key in TRAJ:
        assert torch.equal(lean[key], full[key]), (what, "no value outputs", key)
        assert torch.equal(lean4[key], full[key]), (what, "four waves", key)


@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_horizons(T):
    """(a) T = 1 is the only horizon where the peeled step is the whole sweep."""
    _three_solves(16, 8, T)


def test_padded_shape_short_horizon():
    """(b) the zero-padded instantiations peel the same step."""
    _three_solves(12, 5, 2)


def test_offset_column_and_value_constant():
    """(c) non-zero f and c: v and const, the column and the sum that take v through the accumulator."""
    n, m, T = 16, 8, 5
    (F, f, C, c, x0), ref64, ref32 = _case("spd", n, m, T)
    assert np.abs(f).min() > 0 and np.abs(c).min() > 0
    out = LQR(F, f, C, c).solve_device(x0, T, want_policy=True, want_value=True)
    torch.cuda.synchronize()
    assert int(out["status"].abs().sum()) == 0
    _check_ratios(out, ref64, ref32, ("v", "const"), f"({n}, {m}) T={T} spd")

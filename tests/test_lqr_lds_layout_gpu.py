"""The LDS layout of the matrix-core LQR sweep (lqr_mfma16x8.hip; ``-m gpu``): column stride TFMPC_LQR_COLS of the elimination input
and of K~, q_x / v' and the parking floats in the tail of the input, gains to HBM from the registers of the value update.

Nothing arithmetic depends on the layout, so the checks are those of ``test_lqr_forward_value_chain_gpu.py`` (its launch helper, its
budget rule: per instance the ratio of |gpu - fp64 oracle| to |fp32 oracle - fp64 oracle|, floored at 1e-6 of the tensor's scale, has
median <= 2.5, 0.9 quantile <= 2 BUDGET, max <= 10 BUDGET) on batches that exercise what a layout can break:

* B = 3: one pair and an odd last block whose second wave is idle, at (16, 8), (5, 3), (7, 8), (16, 3) and T = 1 (the peeled step
  alone: gains through K~), 2, 3, 5 (gains from the registers of the value update where the shape is exact; either wave as the
  solver) and 53.  Accuracy of the paired launch AND of the launch with value outputs (one-wave blocks); both give the same bits.
* An instance keeps its bits beside two different neighbours, in either wave position.
* Stale LDS: 12 289 instances at T = 2 fill every CU with blocks twice over; a launch of problems scaled by 1e3 leaves its values in
  every slice, and the launch behind it, in the same process, must return what a fresh process returns for the same problems, byte
  for byte -- a pad that is read before it is written would show.  (The fresh process is this file run as a script.)

Every launch writes into NaN-filled buffers with a guard row behind the last instance."""

import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in ("", "tf-mpc_amd", "tests"):
        sys.path.insert(0, os.path.join(ROOT, _p))

import pytest
import torch

import problems
from oracle import c_oracle
from test_lqr_forward_value_chain_gpu import BUDGET, HORIZONS, SHAPES, TRAJ, VALUE, _launch, _same_bits

pytestmark = pytest.mark.gpu
B = 3
cases = pytest.mark.parametrize("n,m,T", [(n, m, T) for (n, m) in SHAPES for T in HORIZONS])
STALE_B, STALE_T, STALE_SHAPES = 12289, 2, ((16, 8), (7, 8))


@functools.lru_cache(maxsize=None)
def _case(n, m, T):
    """Three instances and their two oracle solves, made once per shape and horizon and left unchanged."""
    F, f, C, c, x0 = problems.make_lqr_batch_spd(B, n, m, seed=29 * n + m)
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True)
    for r in (ref64, ref32):
        for key in TRAJ:
            r[key].setflags(write=False)
    return (F, f, C, c, x0), ref64, ref32


def _check_ratios(out, ref64, ref32, what):
    for key in TRAJ:
        got = out[key].detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (what, key)
        ratios = []
        for b in range(B):
            want = ref64[key][b].reshape(got[b].shape)
            scale = np.abs(want).max()
            e32 = max(np.abs(ref32[key][b].astype(np.float64).reshape(want.shape) - want).max(), 1e-6 * scale)
            ratios.append(np.abs(got[b] - want).max() / e32)
        med, q9, top = np.median(ratios), np.quantile(ratios, 0.9), max(ratios)
        print(f"{what} {key}: median {med:.2f} q0.9 {q9:.2f} max {top:.2f}")
        assert med <= 2.5 and q9 <= 2 * BUDGET and top <= 10 * BUDGET, (what, key, med, q9, top)


@cases
def test_accuracy_paired_and_one_wave(n, m, T):
    """A pair and an odd last block against the oracles, without and with value outputs; the two kinds of block give the same bits."""
    problem, ref64, ref32 = _case(n, m, T)
    what = f"({n}, {m}) T={T}"
    lean = _launch(problem, range(B), T)
    full = _launch(problem, range(B), T, value=True)
    for got in (lean, full):
        assert int(got[1].abs().sum()) == 0, what
    _check_ratios(lean[0], ref64, ref32, what + " paired")
    _check_ratios(full[0], ref64, ref32, what + " value outputs")
    for key in VALUE:
        assert torch.isfinite(full[0][key]).all(), (what, key)
    for pos in range(B):
        _same_bits(full, pos, lean, pos, (what, "one-wave against paired", pos))


@cases
def test_two_neighbours(n, m, T):
    """Instance 0 beside instance 1 and beside instance 2, as the first and as the second wave of the pair: the same bits."""
    problem = _case(n, m, T)[0]
    what = f"({n}, {m}) T={T}"
    a1, a2, b1, b2 = (_launch(problem, idx, T) for idx in ((0, 1), (0, 2), (1, 0), (2, 0)))
    for got in (a1, a2, b1, b2):
        assert int(got[1].abs().sum()) == 0, what
    _same_bits(a2, 0, a1, 0, (what, "first wave, neighbour 2 against neighbour 1"))
    _same_bits(b1, 1, a1, 0, (what, "second wave beside 1"))
    _same_bits(b2, 1, a1, 0, (what, "second wave beside 2"))
    _same_bits(b1, 0, a1, 1, (what, "the neighbour itself, either wave"))


def _stale_problem(n, m):
    return problems.make_lqr_batch_spd(STALE_B, n, m, seed=31 * n + m)


def _stale_outputs(dirty):
    """{"n_m_kind_key": array} of the launches without and with value outputs at every stale-test shape; ``dirty``: each is preceded,
    in this process, by the same launch of the problems with costs, offsets and start states scaled by 1e3."""
    got = {}
    for n, m in STALE_SHAPES:
        F, f, C, c, x0 = _stale_problem(n, m)
        big = (F, 1e3 * f, 1e3 * C, 1e3 * c, 1e3 * x0)
        for value in (False, True):
            if dirty:
                _launch(big, range(STALE_B), STALE_T, value=value)
            out, status = _launch((F, f, C, c, x0), range(STALE_B), STALE_T, value=value)
            for key in TRAJ + (VALUE if value else ()):
                got[f"{n}_{m}_{'value' if value else 'lean'}_{key}"] = out[key].cpu().numpy()
            got[f"{n}_{m}_{'value' if value else 'lean'}_status"] = status.cpu().numpy()
    return got


def test_stale_lds(tmp_path):
    """Blocks that start on slices a launch of much larger values left behind return the bits of a fresh process."""
    path = str(tmp_path / "fresh.npz")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    fresh = np.load(path)
    got = _stale_outputs(dirty=True)
    assert sorted(fresh.files) == sorted(got)
    for key, arr in got.items():
        assert np.isfinite(arr).all(), key
        assert arr.tobytes() == fresh[key].tobytes(), (key, int((arr != fresh[key]).any(axis=tuple(range(1, arr.ndim))).sum()), "instances differ")
    for n, m in STALE_SHAPES:
        assert int(np.abs(got[f"{n}_{m}_lean_status"]).sum()) == 0


if __name__ == "__main__":
    np.savez(sys.argv[1], **_stale_outputs(dirty=False))

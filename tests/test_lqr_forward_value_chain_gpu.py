"""The value chain of the matrix-core LQR sweep taken from the forward elimination (lqr_mfma16x8.hip, wave_ldlt8_pair.h; ``-m gpu``).

The 8 x 8 solve of a sweep step leaves, behind its forward elimination, the reduced rows m^_a and x^_a = -m^_a / d_a, and the sweep
finishes v'[j] = q_x[j] + (sum_a x^_a[q_u column] m^_a[j]) from those -- the products summed from 0, a = 0..7, then one addition -- with
the terms woven into the elimination: no second copy of the column, no LDS traffic of its own.  In a paired block (launches without value outputs) the solver wave runs the chain for both
instances inside the one statement of the solve; a one-wave block (launches with value outputs) runs the same chain between the two
halves of its solve (``v_readlane(., 24)`` of the rows as they stand before the back substitution).  K, k go through the chains they
went through before.

* Horizons: T = 1 (the peeled step alone, no v' used), T = 2 (one value update), T = 3 and 5 (either wave of a pair as the solver),
  T = 53 (past the rollout chunk of 52).  Five instances: two pairs and an odd last block whose second wave is idle.
* Accuracy against the fp64 C oracle, K, k, states, actions, costs, by the rule of ``test_lqr_sweep_trim_gpu.py``: per instance the ratio
  of |gpu - fp64 oracle| to |fp32 oracle - fp64 oracle| (floored at 1e-6 of the tensor's scale) has median <= 2.5, 0.9 quantile <=
  2 BUDGET, max <= 10 BUDGET.  K and k cover every time index in NaN-filled buffers.
* Same bits: paired against one-wave; backward + forward entry points against fused; TFMPC_LQR_WAVES = 4, 5, 6 among each other under
  either product kind (bf16x3 and TFMPC_LQR_MFMA=f32); an instance beside different partners and in either wave position.
* Status isolation: an instance with a non-positive C_uu flags only itself; its partner has the outputs and status of a clean launch.

Instances: ``problems.make_lqr_batch_spd``, seed 17 n + m.  Every launch writes into NaN-filled buffers with a guard row behind the
last instance."""

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
TRAJ = ("states", "actions", "costs", "K", "k")
VALUE = ("V", "v", "const")
B = 5
SHAPES = [(16, 8), (5, 3), (7, 8), (16, 3)]
HORIZONS = (1, 2, 3, 5, 53)
cases = pytest.mark.parametrize("n,m,T", [(n, m, T) for (n, m) in SHAPES for T in HORIZONS])


@functools.lru_cache(maxsize=None)
def _case(n, m, T):
    """Five instances and their two oracle solves, made once per shape and horizon and left unchanged."""
    F, f, C, c, x0 = problems.make_lqr_batch_spd(B, n, m, seed=17 * n + m)
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True)
    for r in (ref64, ref32):
        for key in TRAJ:
            r[key].setflags(write=False)
    return (F, f, C, c, x0), ref64, ref32


def _launch(problem, idx, T, split=False, value=False):
    """Instances ``idx`` of ``problem`` (in that order) in one fused launch, without or with value outputs -- or, ``split``, one
    backward launch without value outputs and one forward launch.  Returns {key: [B, rows, width]} and status [B]; checks the guards."""
    lib = _hip.require_gpu()
    idx = list(idx)
    nb = len(idx)
    F, f, C, c, x0 = (a[idx] for a in problem)
    n, m = F.shape[1], F.shape[2] - F.shape[1]
    assert lib.tfmpc_lqr_kernel_name(n, m, T).startswith(b"mfma_16x8")
    lqr = LQR(F, f, C, c)
    x0d = lqr._prep_x0(x0)
    dev = x0d.device
    rows = dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m))
    if value:
        rows.update(V=(T, n * n), v=(T, n), const=(T, 1))
    flat = {key: torch.full((nb * r + 1, w), float("nan"), device=dev) for key, (r, w) in rows.items()}
    status = torch.full((nb + 1,), -1, dtype=torch.int32, device=dev)
    if split:
        assert not value
        rc = lib.tfmpc_lqr_backward_f32(nb, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), _hip.ptr(flat["k"]), None, None, None,
                                        _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_backward_f32")
        rc = lib.tfmpc_lqr_forward_f32(nb, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), T * m * n, _hip.ptr(flat["k"]), T * m,
                                       _hip.ptr(x0d), _hip.ptr(flat["states"]), _hip.ptr(flat["actions"]), _hip.ptr(flat["costs"]),
                                       _hip.stream())
        _hip.check(rc, "tfmpc_lqr_forward_f32")
    else:
        vals = [_hip.ptr(flat[key]) for key in VALUE] if value else [None, None, None]
        rc = lib.tfmpc_lqr_solve_f32(nb, n, m, T, *lqr._ptr_args(), _hip.ptr(x0d), *(_hip.ptr(flat[key]) for key in TRAJ),
                                     *vals, _hip.ptr(status), None, 0, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_solve_f32")
    torch.cuda.synchronize()
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][nb * r:]).all(), (idx, T, key, "guard row behind the batch")
        out[key] = flat[key][:nb * r].reshape(nb, r, w)
    assert int(status[nb]) == -1, (idx, T, "guard behind the status")
    return out, status[:nb]


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


def _same_bits(got, pos, want, wpos, what):
    (out, status), (wout, wstatus) = got, want
    for key in TRAJ:
        assert torch.equal(out[key][pos], wout[key][wpos]), (what, key)
    assert int(status[pos]) == int(wstatus[wpos]), (what, "status")


@cases
def test_accuracy_paired_and_one_wave(n, m, T):
    """Paired blocks (no value outputs) against the oracles; one-wave blocks (value outputs) give the same bits."""
    problem, ref64, ref32 = _case(n, m, T)
    what = f"({n}, {m}) T={T}"
    lean = _launch(problem, range(B), T)
    full = _launch(problem, range(B), T, value=True)
    for got in (lean, full):
        assert int(got[1].abs().sum()) == 0, what
    _check_ratios(lean[0], ref64, ref32, what)
    for pos in range(B):
        _same_bits(full, pos, lean, pos, (what, "one-wave against paired", pos))


@cases
def test_split_entry_points(n, m, T):
    """Backward without value outputs, then forward: the bits of the fused launch."""
    problem = _case(n, m, T)[0]
    fused = _launch(problem, range(B), T)
    split = _launch(problem, range(B), T, split=True)
    assert int(split[1].abs().sum()) == 0
    for pos in range(B):
        _same_bits(split, pos, fused, pos, (n, m, T, "backward + forward against fused", pos))


@pytest.mark.parametrize("products", ["bf16x3", "f32"])
@cases
def test_register_budgets_within_a_product_kind(n, m, T, products):
    """Four, five and six resident waves run one instruction stream up to register allocation: same bits, under either product kind."""
    problem, ref64, ref32 = _case(n, m, T)
    got = {}
    with _hip.option("TFMPC_LQR_MFMA", "f32" if products == "f32" else None):
        for waves in ("4", "5", "6"):
            with _hip.option("TFMPC_LQR_WAVES", waves):
                got[waves] = _launch(problem, range(B), T)
    assert int(got["5"][1].abs().sum()) == 0
    _check_ratios(got["5"][0], ref64, ref32, f"({n}, {m}) T={T} {products}")
    for waves in ("4", "6"):
        for pos in range(B):
            _same_bits(got[waves], pos, got["5"], pos, (n, m, T, products, waves + " waves against five", pos))


@cases
def test_partner_and_wave_position(n, m, T):
    """Instances a = 0 and b = 1 as [a, b], [b, a], [a] and [a, b, a]: an instance keeps its bits in either wave -- as the solver of the
    even or of the odd steps --, with any partner, and alone in the odd last block."""
    problem = _case(n, m, T)[0]
    what = f"({n}, {m}) T={T}"
    ab, ba, a, aba = (_launch(problem, idx, T) for idx in ((0, 1), (1, 0), (0,), (0, 1, 0)))
    for got in (ab, ba, a, aba):
        assert int(got[1].abs().sum()) == 0, what
    _same_bits(ab, 0, a, 0, (what, "a: first wave of a pair against alone in the odd last block"))
    _same_bits(ba, 1, a, 0, (what, "a: second wave of a pair"))
    _same_bits(aba, 0, a, 0, (what, "a: first of three"))
    _same_bits(aba, 2, a, 0, (what, "a: alone in the odd last block behind a pair"))
    _same_bits(ba, 0, ab, 1, (what, "b: first wave against second"))
    _same_bits(aba, 1, ab, 1, (what, "b: second of three"))


@pytest.mark.parametrize("order", ["good_bad", "bad_good"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_status_isolation(n, m, order):
    """A partner whose C_uu is not positive (negated) reports it, and only it: the good instance next to it -- eliminated, and its v'
    formed, by the same instructions -- keeps the bits and the status 0 of a clean launch."""
    T = 5
    (F, f, C, c, x0), _, _ = _case(n, m, T)
    C2 = C[:2].copy()
    C2[1] = C[0]
    C2[1, n:, n:] = -C2[1, n:, n:]
    problem = (np.stack([F[0], F[0]]), np.stack([f[0], f[0]]), C2, np.stack([c[0], c[0]]), np.stack([x0[0], x0[0]]))
    alone = _launch(problem, (0,), T)
    assert int(alone[1][0]) == 0
    idx = (0, 1) if order == "good_bad" else (1, 0)
    got = _launch(problem, idx, T)
    good, bad = idx.index(0), idx.index(1)
    assert int(got[1][bad]) & _hip.ST_NOT_PD, (order, int(got[1][bad]))
    _same_bits(got, good, alone, 0, (order, "the good instance"))
    assert int(got[1][good]) == 0

"""The value update of the matrix-core LQR sweep (lqr_mfma16x8.hip step 4, wave_ldlt8_pair.h; ``-m gpu``): v' = q_x + Q_xu k is one
chain of eight fused multiply-adds per state, ``acc = q_x[j]; acc = fma(k[a], Q_ux[a][j], acc)`` for a = 0..7, run in the lanes of the
8 x 8 elimination that hold column j -- by the solver wave of a paired block for both instances (launches without value outputs), by
the instance's own wave in a one-wave block (launches with value outputs) -- and stored over q_x in the instance's LDS slice.

* Accuracy against the fp64 C oracle: K, k, states, actions, costs of a launch without value outputs, V, v, const of one with them.
  ``v`` at every step is the direct check of the chain; k_{t-1} depends on v_t, so the policy and the trajectory see it one step later
  (``test_lqr_value_update_cpu.py`` shows by how much).  Horizons: T = 1 (the peeled step alone, no v' used), T = 2 (one value update),
  T = 3 and 5 (both solver parities), T = 53 (past the rollout chunk).
* Same bits, paired against one-wave: both paths run the same chain, so K, k, states, actions and costs agree bit for bit.
* Same bits, partner and wave: instances a, b launched as [a, b], [b, a], [a] and [a, b, a] -- an instance keeps its bits in either
  wave, with any partner, and alone in the odd last block: the solver's lanes write v' into the right slice.  Repeated under
  TFMPC_LQR_MFMA=f32, TFMPC_LQR_WAVES=4 and 6, and for the split backward + forward entry points.
* Status isolation: next to an instance whose Q_uu is not positive definite, a good one keeps its bits and status 0.

Instances: five of ``problems.make_lqr_batch_spd``, seed 17 n + m (as in ``test_lqr_pair_solve_gpu.py``).  Accuracy rule of
``test_lqr_rollout_trim_gpu.py``: per instance the ratio of |gpu - fp64 oracle| to |fp32 oracle - fp64 oracle| (floored at 1e-6 of the
tensor's scale) has median <= 2.5, 0.9 quantile <= 2 BUDGET, max <= 10 BUDGET.  Every launch writes into NaN-filled buffers with a
guard row behind the last instance."""

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
NINST = 5
SHAPES = [(16, 8), (5, 3), (7, 8), (16, 3)]
HORIZONS = (1, 2, 3, 5, 53)


@functools.lru_cache(maxsize=None)
def _case(n, m, T):
    """Five instances and their two oracle solves, made once per shape and horizon and left unchanged."""
    F, f, C, c, x0 = problems.make_lqr_batch_spd(NINST, n, m, seed=17 * n + m)
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True, want_value=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True, want_value=True)
    for r in (ref64, ref32):
        for key in TRAJ + VALUE:
            r[key].setflags(write=False)
    return (F, f, C, c, x0), ref64, ref32


def _launch(problem, idx, T, split=False, value=False):
    """Instances ``idx`` of ``problem`` (in that order) in one fused launch, without or with value outputs -- or, ``split``, one
    backward launch without value outputs and one forward launch.  Returns {key: [B, rows, width]} and status [B]; checks the guards."""
    lib = _hip.require_gpu()
    idx = list(idx)
    B = len(idx)
    F, f, C, c, x0 = (a[idx] for a in problem)
    n, m = F.shape[1], F.shape[2] - F.shape[1]
    assert lib.tfmpc_lqr_kernel_name(n, m, T).startswith(b"mfma_16x8")
    lqr = LQR(F, f, C, c)
    x0d = lqr._prep_x0(x0)
    dev = x0d.device
    rows = dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m))
    if value:
        rows.update(V=(T, n * n), v=(T, n), const=(T, 1))
    flat = {key: torch.full((B * r + 1, w), float("nan"), device=dev) for key, (r, w) in rows.items()}
    status = torch.full((B + 1,), -1, dtype=torch.int32, device=dev)
    if split:
        assert not value
        rc = lib.tfmpc_lqr_backward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), _hip.ptr(flat["k"]), None, None, None,
                                        _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_backward_f32")
        rc = lib.tfmpc_lqr_forward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), T * m * n, _hip.ptr(flat["k"]), T * m,
                                       _hip.ptr(x0d), _hip.ptr(flat["states"]), _hip.ptr(flat["actions"]), _hip.ptr(flat["costs"]),
                                       _hip.stream())
        _hip.check(rc, "tfmpc_lqr_forward_f32")
    else:
        vals = [_hip.ptr(flat[key]) for key in VALUE] if value else [None, None, None]
        rc = lib.tfmpc_lqr_solve_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(x0d), *(_hip.ptr(flat[key]) for key in TRAJ),
                                     *vals, _hip.ptr(status), None, 0, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_solve_f32")
    torch.cuda.synchronize()
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][B * r:]).all(), (idx, T, key, "guard row behind the batch")
        out[key] = flat[key][:B * r].reshape(B, r, w)
    assert int(status[B]) == -1, (idx, T, "guard behind the status")
    return out, status[:B]


def _check_ratios(out, idx, ref64, ref32, keys, what):
    for key in keys:
        got = out[key].detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (what, key)
        ratios = []
        for pos, b in enumerate(idx):
            want = ref64[key][b].reshape(got[pos].shape)
            scale = np.abs(want).max()
            e32 = max(np.abs(ref32[key][b].astype(np.float64).reshape(want.shape) - want).max(), 1e-6 * scale)
            ratios.append(np.abs(got[pos] - want).max() / e32)
        med, q9, top = np.median(ratios), np.quantile(ratios, 0.9), max(ratios)
        print(f"{what} {key}: median {med:.2f} q0.9 {q9:.2f} max {top:.2f}")
        assert med <= 2.5 and q9 <= 2 * BUDGET and top <= 10 * BUDGET, (what, key, med, q9, top)


def _same_bits(got, pos, want, wpos, what):
    (out, status), (wout, wstatus) = got, want
    for key in TRAJ:
        assert torch.equal(out[key][pos], wout[key][wpos]), (what, key)
    assert int(status[pos]) == int(wstatus[wpos]), (what, "status")


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_accuracy_and_paired_against_one_wave(n, m, T):
    """Without value outputs (paired blocks) and with them (one-wave blocks): each against the oracle, and the same bits."""
    problem, ref64, ref32 = _case(n, m, T)
    what = f"({n}, {m}) T={T}"
    idx = range(NINST)
    lean = _launch(problem, idx, T)
    full = _launch(problem, idx, T, value=True)
    for got in (lean, full):
        assert int(got[1].abs().sum()) == 0, what
    _check_ratios(lean[0], idx, ref64, ref32, TRAJ, what + " without value outputs")
    _check_ratios(full[0], idx, ref64, ref32, VALUE, what + " with value outputs")
    for pos in idx:
        _same_bits(lean, pos, full, pos, (what, "paired against one-wave", pos))


def _partner_changes_nothing(n, m, T, split=False):
    """Instances a = 0 and b = 1 as [a, b], [b, a], [a] and [a, b, a]."""
    problem, ref64, ref32 = _case(n, m, T)
    what = f"({n}, {m}) T={T}"
    ab, ba, a, aba = (_launch(problem, idx, T, split) for idx in ((0, 1), (1, 0), (0,), (0, 1, 0)))
    for got in (ab, ba, a, aba):
        assert int(got[1].abs().sum()) == 0, what
    _check_ratios(ab[0], (0, 1), ref64, ref32, TRAJ, what)
    _same_bits(ab, 0, a, 0, (what, "a: first wave of a pair against alone in the odd last block"))
    _same_bits(ba, 1, a, 0, (what, "a: second wave of a pair"))
    _same_bits(aba, 0, a, 0, (what, "a: first of three"))
    _same_bits(aba, 2, a, 0, (what, "a: alone in the odd last block behind a pair"))
    _same_bits(ba, 0, ab, 1, (what, "b: first wave against second"))
    _same_bits(aba, 1, ab, 1, (what, "b: second of three"))
    return ab


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_a_partner_changes_nothing(n, m, T):
    _partner_changes_nothing(n, m, T)


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_variant_f32_products(n, m, T):
    with _hip.option("TFMPC_LQR_MFMA", "f32"):
        _partner_changes_nothing(n, m, T)


@pytest.mark.parametrize("waves", ["4", "6"])
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_variant_register_budgets(n, m, T, waves):
    """... and the four- and six-wave instantiations give the bits of the five-wave one."""
    with _hip.option("TFMPC_LQR_WAVES", waves):
        forced = _partner_changes_nothing(n, m, T)
    five = _launch(_case(n, m, T)[0], (0, 1), T)
    for pos in (0, 1):
        _same_bits(forced, pos, five, pos, (T, waves + " waves against five", pos))


@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_variant_split_entry_points(n, m, T):
    """Backward without value outputs, then forward: the bits of the fused launch."""
    split = _partner_changes_nothing(n, m, T, split=True)
    fused = _launch(_case(n, m, T)[0], (0, 1), T)
    for pos in (0, 1):
        _same_bits(split, pos, fused, pos, (T, "backward + forward against fused", pos))


@pytest.mark.parametrize("order", ["good_bad", "bad_good"])
@pytest.mark.parametrize("n,m", SHAPES)
def test_status_isolation(n, m, order):
    """A partner whose Q_uu is not positive definite (C_uu negated) reports it; the good instance next to it, whose system is
    eliminated -- and whose v' is formed -- by the same instructions, keeps the bits it has when solved alone and status 0."""
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

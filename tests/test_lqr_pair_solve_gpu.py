"""The paired elimination of the matrix-core LQR kernel (lqr_mfma16x8.hip, wave_ldlt8_pair.h; ``-m gpu``): launches without
value outputs run blocks of two waves, instance = 2 block + wave, and per sweep step ONE of the two waves eliminates the
8 x 8 systems of both instances (lanes 0..31 / 32..63, multipliers broadcast per row of 16 lanes).

* A partner changes nothing: an instance's states, actions, costs, status, K and k are the same bits whichever wave it sits
  in, whoever shares its block, and alone in the odd last block -- at T = 1 (the peeled step alone), T = 2 and 5 (both
  solver parities), T = 53 (past the rollout chunk of 52).
* Odd batches: the second wave of the last block has no instance and runs on the clamped index B - 1; nothing is written behind
  the batch (guard rows stay NaN, which shows the clamp; a store of the idle wave that slipped through would rewrite instance
  B - 1 with its own values and is NOT seen here), and instance B - 1 keeps the bits it has with a partner.
* Status isolation: next to an instance whose Q_uu is not positive definite, a good one keeps its bits and status 0.
* The same under TFMPC_LQR_MFMA=f32, TFMPC_LQR_WAVES=4, the split backward + forward entry points, and the zero-padded
  shapes (5, 3) and (7, 8) (which must pass whether they run paired or one wave per block).

Instances: ``problems.make_lqr_batch_spd``.  Accuracy rule of ``test_lqr_rollout_trim_gpu.py``: per instance the ratio of
|gpu - fp64 oracle| to |fp32 oracle - fp64 oracle| (floored at 1e-6 of the tensor's scale) has median <= 2.5, 0.9 quantile
<= 2 BUDGET, max <= 10 BUDGET.  Every launch writes into NaN-filled buffers with a guard row behind the last instance."""

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
NINST = 5
HORIZONS = (1, 2, 5, 53)


@functools.lru_cache(maxsize=None)
def _case(n, m, T):
    """Five instances and their two oracle solves, made once per shape and horizon."""
    F, f, C, c, x0 = problems.make_lqr_batch_spd(NINST, n, m, seed=17 * n + m)
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True)
    for r in (ref64, ref32):
        for key in TRAJ:
            r[key].setflags(write=False)
    return (F, f, C, c, x0), ref64, ref32


def _launch(problem, idx, T, split=False):
    """Instances ``idx`` of ``problem`` (in that order) in one launch without value outputs -- or, ``split``, one backward launch
    without value outputs and one forward launch.  Returns {key: [B, rows, width]} and status [B]; checks the guard rows."""
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
    flat = {key: torch.full((B * r + 1, w), float("nan"), device=dev) for key, (r, w) in rows.items()}
    status = torch.full((B + 1,), -1, dtype=torch.int32, device=dev)
    if split:
        rc = lib.tfmpc_lqr_backward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), _hip.ptr(flat["k"]), None, None, None,
                                        _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_backward_f32")
        rc = lib.tfmpc_lqr_forward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), T * m * n, _hip.ptr(flat["k"]), T * m,
                                       _hip.ptr(x0d), _hip.ptr(flat["states"]), _hip.ptr(flat["actions"]), _hip.ptr(flat["costs"]),
                                       _hip.stream())
        _hip.check(rc, "tfmpc_lqr_forward_f32")
    else:
        rc = lib.tfmpc_lqr_solve_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(x0d), *(_hip.ptr(flat[key]) for key in TRAJ),
                                     None, None, None, _hip.ptr(status), None, 0, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_solve_f32")
    torch.cuda.synchronize()
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][B * r:]).all(), (idx, T, key, "guard row behind the batch")
        out[key] = flat[key][:B * r].reshape(B, r, w)
    assert int(status[B]) == -1, (idx, T, "guard behind the status")
    return out, status[:B]


def _check_ratios(out, idx, ref64, ref32, what):
    for key in TRAJ:
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


def _partner_changes_nothing(n, m, T, split=False):
    """Instances a = 0 and b = 1 as [a, b], [b, a], [a] and [a, b, a]."""
    problem, ref64, ref32 = _case(n, m, T)
    what = f"({n}, {m}) T={T}"
    ab, ba, a, aba = (_launch(problem, idx, T, split) for idx in ((0, 1), (1, 0), (0,), (0, 1, 0)))
    for got in (ab, ba, a, aba):
        assert int(got[1].abs().sum()) == 0, what
    _check_ratios(ab[0], (0, 1), ref64, ref32, what)
    _same_bits(ab, 0, a, 0, (what, "a: first wave of a pair against alone in the odd last block"))
    _same_bits(ba, 1, a, 0, (what, "a: second wave of a pair"))
    _same_bits(aba, 0, a, 0, (what, "a: first of three"))
    _same_bits(aba, 2, a, 0, (what, "a: alone in the odd last block behind a pair"))
    _same_bits(ba, 0, ab, 1, (what, "b: first wave against second"))
    _same_bits(aba, 1, ab, 1, (what, "b: second of three"))
    return ab


@pytest.mark.parametrize("T", HORIZONS)
def test_a_partner_changes_nothing(T):
    _partner_changes_nothing(16, 8, T)


@pytest.mark.parametrize("B", [1, 3, 5])
def test_odd_batches(B):
    """The second wave of the last block has no instance: nothing lands behind the batch (the guard rows are checked in _launch),
    the instances are right, and the last one -- alone in its block -- has the bits it has with a partner behind it."""
    T = 5
    problem, ref64, ref32 = _case(16, 8, T)
    got = _launch(problem, range(B), T)
    assert int(got[1].abs().sum()) == 0
    _check_ratios(got[0], range(B), ref64, ref32, f"B={B} T={T}")
    even = _launch(problem, list(range(B)) + [0], T)
    for pos in range(B):
        _same_bits(got, pos, even, pos, (B, "odd batch against the same batch with a partner for the last instance", pos))


@pytest.mark.parametrize("order", ["good_bad", "bad_good"])
def test_status_isolation(order):
    """A partner whose Q_uu is not positive definite (C_uu negated) reports it; the good instance next to it, whose system is
    eliminated by the same instructions, keeps the bits it has when solved alone and status 0."""
    n, m, T = 16, 8, 5
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


@pytest.mark.parametrize("T", HORIZONS)
def test_variant_f32_products(T):
    with _hip.option("TFMPC_LQR_MFMA", "f32"):
        f32 = _partner_changes_nothing(16, 8, T)
    # the option reached the kernel: fp32 FMA chains and bf16x3 round differently
    bf3 = _launch(_case(16, 8, T)[0], (0, 1), T)
    assert not torch.equal(f32[0]["K"], bf3[0]["K"]), (T, "TFMPC_LQR_MFMA=f32 gave the bits of the default products")


@pytest.mark.parametrize("T", HORIZONS)
def test_variant_four_waves(T):
    """... and the four-wave instantiation gives the bits of the five-wave one."""
    with _hip.option("TFMPC_LQR_WAVES", "4"):
        four = _partner_changes_nothing(16, 8, T)
    five = _launch(_case(16, 8, T)[0], (0, 1), T)
    for pos in (0, 1):
        _same_bits(four, pos, five, pos, (T, "four waves against five", pos))


@pytest.mark.parametrize("T", HORIZONS)
def test_variant_split_entry_points(T):
    """Backward without value outputs, then forward: the bits of the fused launch."""
    split = _partner_changes_nothing(16, 8, T, split=True)
    fused = _launch(_case(16, 8, T)[0], (0, 1), T)
    for pos in (0, 1):
        _same_bits(split, pos, fused, pos, (T, "backward + forward against fused", pos))


@pytest.mark.parametrize("n,m", [(5, 3), (7, 8)])
def test_variant_padded_shapes(n, m):
    _partner_changes_nothing(n, m, 6)
    _partner_changes_nothing(n, m, 6, split=True)

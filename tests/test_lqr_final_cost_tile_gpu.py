"""The final cost of the matrix-core LQR rollout rides in the last chunk's cost tiles (lqr_mfma16x8.hip; ``-m gpu``): row tc of
the chunk buffer holds x_T, its action part is zeroed, and ``chunk_costs`` prices tc + 1 rows, sixteen per tile, instead of a
tile of its own for the one row (bookkeeping: lqr_final_cost_tile_ref.py, test_lqr_final_cost_tile_cpu.py).

Horizons (the chunk is 52 rows, a tile 16): T = 1 the peeled step alone, the final row is row 1; 15 the final row is the last
of a tile; 16 it opens a tile; 17 one past that edge; 48 the same edge nearer the chunk's end; 50 the headline; 52 a full
chunk, the final row is the buffer's last; 53 a second chunk of one step, whose row 1 holds a stale action of the first; 68 a
second chunk of 16 rows; 104 two full chunks.  Shapes: (16, 8) at each, the zero-padded (5, 3) and (7, 8) at T = 1, 16, 53.
B = 5: the odd last block runs with its idle wave.

* costs (final column included), states, actions and gains against ``oracle.c_oracle`` by the accuracy rule of
  test_lqr_pair_solve_gpu.py: per instance the ratio of |gpu - fp64 oracle| to |fp32 oracle - fp64 oracle| (floored at 1e-6 of
  the tensor's scale) has median <= 2.5, 0.9 quantile <= 2 BUDGET, max <= 10 BUDGET; all finite, guard rows intact.
* costs[:, T] and costs[:, :T] are the same bits from the fused launch without value outputs, the fused launch with value
  outputs (one-wave blocks) and the split backward + forward entry points.
* Under TFMPC_LQR_MFMA=f32 and TFMPC_LQR_WAVES = 4 and 6 every output at T = 16 and 53 has the bits of the default budget of
  the same product mode.
* An instance whose x0 holds a NaN reports TFMPC_ST_NAN -- from the value the storing lane holds, nothing is read back --
  and its neighbours in the same and in the next block keep status 0 and their bits."""

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
HORIZONS = (1, 15, 16, 17, 48, 50, 52, 53, 68, 104)
PADDED = [(n, m, T) for (n, m) in ((5, 3), (7, 8)) for T in (1, 16, 53)]
CASES = [(16, 8, T) for T in HORIZONS] + PADDED
BUDGET_CASES = [(n, m, T) for (n, m) in ((16, 8), (5, 3), (7, 8)) for T in (16, 53)]


@functools.lru_cache(maxsize=None)
def _case(n, m, T):
    """Five instances and their two oracle solves, made once per shape and horizon."""
    problem = problems.make_lqr_batch_spd(NINST, n, m, seed=31 * n + m)
    F, f, C, c, x0 = problem
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True)
    for arr in problem:
        arr.setflags(write=False)
    for r in (ref64, ref32):
        for key in TRAJ:
            r[key].setflags(write=False)
    return problem, ref64, ref32


def _launch(problem, T, how="fused"):
    """One solve of the whole batch into NaN-filled buffers with a guard row behind the batch and behind the status.
    ``how``: "fused" (no value outputs: two-wave blocks), "value" (V, v, const requested: one-wave blocks) or "split" (backward
    without value outputs, then tfmpc_lqr_forward_f32).  Returns {key: [B, rows, width]}, status [B]."""
    lib = _hip.require_gpu()
    F, f, C, c, x0 = problem
    B, n, m = F.shape[0], F.shape[1], F.shape[2] - F.shape[1]
    assert lib.tfmpc_lqr_kernel_name(n, m, T).startswith(b"mfma_16x8")
    lqr = LQR(F, f, C, c)
    x0d = lqr._prep_x0(x0)
    dev = x0d.device
    rows = dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m))
    if how == "value":
        rows.update(V=(T, n * n), v=(T, n), cst=(T, 1))
    flat = {key: torch.full((B * r + 1, w), float("nan"), device=dev) for key, (r, w) in rows.items()}
    status = torch.full((B + 1,), -1, dtype=torch.int32, device=dev)
    if how == "split":
        rc = lib.tfmpc_lqr_backward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), _hip.ptr(flat["k"]), None, None, None,
                                        _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_backward_f32")
        rc = lib.tfmpc_lqr_forward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), T * m * n, _hip.ptr(flat["k"]), T * m,
                                       _hip.ptr(x0d), _hip.ptr(flat["states"]), _hip.ptr(flat["actions"]), _hip.ptr(flat["costs"]),
                                       _hip.stream())
        _hip.check(rc, "tfmpc_lqr_forward_f32")
    else:
        value = [_hip.ptr(flat[key]) for key in ("V", "v", "cst")] if how == "value" else [None, None, None]
        rc = lib.tfmpc_lqr_solve_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(x0d), *(_hip.ptr(flat[key]) for key in TRAJ),
                                     *value, _hip.ptr(status), None, 0, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_solve_f32")
    torch.cuda.synchronize()
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][B * r:]).all(), (T, how, key, "guard row behind the batch")
        out[key] = flat[key][:B * r].reshape(B, r, w)
    assert int(status[B]) == -1, (T, how, "guard behind the status")
    return out, status[:B]


def _check_ratios(out, ref64, ref32, what):
    for key in TRAJ:
        got = out[key].detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (what, key)
        ratios = []
        for b in range(got.shape[0]):
            want = ref64[key][b].reshape(got[b].shape)
            scale = np.abs(want).max()
            e32 = max(np.abs(ref32[key][b].astype(np.float64).reshape(want.shape) - want).max(), 1e-6 * scale)
            ratios.append(np.abs(got[b] - want).max() / e32)
        med, q9, top = np.median(ratios), np.quantile(ratios, 0.9), max(ratios)
        print(f"{what} {key}: median {med:.2f} q0.9 {q9:.2f} max {top:.2f}")
        assert med <= 2.5 and q9 <= 2 * BUDGET and top <= 10 * BUDGET, (what, key, med, q9, top)
    # the final cost by itself: one number per instance, so the rule's maximum is what applies to it
    got = out["costs"][:, -1, 0].detach().cpu().numpy().astype(np.float64)
    for b in range(got.shape[0]):
        want = ref64["costs"][b].reshape(-1)
        e32 = max(abs(float(ref32["costs"][b].reshape(-1)[-1]) - want[-1]), 1e-6 * np.abs(want).max())
        ratio = abs(got[b] - want[-1]) / e32
        print(f"{what} final cost of instance {b}: ratio {ratio:.2f}")
        assert ratio <= 10 * BUDGET, (what, "final cost", b, ratio)


def _same_bits(got, want, what, keys=TRAJ, rows=None):
    (out, status), (wout, wstatus) = got, want
    rows = range(status.shape[0]) if rows is None else rows
    for b in rows:
        for key in keys:
            assert torch.equal(out[key][b], wout[key][b]), (what, key, b)
        assert int(status[b]) == int(wstatus[b]), (what, "status", b)


@pytest.mark.parametrize("n,m,T", CASES)
def test_costs_against_the_oracle_and_across_entry_points(n, m, T):
    problem, ref64, ref32 = _case(n, m, T)
    what = f"({n}, {m}) T={T}"
    fused = _launch(problem, T)
    assert int(fused[1].abs().sum()) == 0, what
    _check_ratios(fused[0], ref64, ref32, what)
    for how in ("value", "split"):
        other = _launch(problem, T, how)
        assert int(other[1].abs().sum()) == 0, (what, how)
        assert torch.equal(other[0]["costs"][:, T], fused[0]["costs"][:, T]), (what, how, "the final cost")
        assert torch.equal(other[0]["costs"][:, :T], fused[0]["costs"][:, :T]), (what, how, "the stage costs")
        _same_bits(other, fused, (what, how))


@pytest.mark.parametrize("products", ["bf16x3", "f32"])
@pytest.mark.parametrize("n,m,T", BUDGET_CASES)
def test_register_budgets_give_the_same_bits(n, m, T, products):
    problem, _, _ = _case(n, m, T)
    with _hip.option("TFMPC_LQR_MFMA", products):
        base = _launch(problem, T)
        split = _launch(problem, T, "split")
        for waves in ("4", "6"):
            with _hip.option("TFMPC_LQR_WAVES", waves):
                _same_bits(_launch(problem, T), base, (n, m, T, products, waves, "fused"))
                _same_bits(_launch(problem, T, "split"), split, (n, m, T, products, waves, "split"))
    if products == "f32":     # the option reached the kernel: fp32 FMA chains and bf16x3 round differently
        assert not torch.equal(base[0]["K"], _launch(problem, T)[0]["K"]), (n, m, T)


@pytest.mark.parametrize("n,m,T", [(16, 8, 1), (16, 8, 16), (16, 8, 50), (16, 8, 53), (5, 3, 16), (7, 8, 53)])
@pytest.mark.parametrize("how", ["fused", "value", "split"])
def test_nan_in_x0_is_reported_and_stays_with_its_instance(n, m, T, how):
    """Instance 2 (first wave of the second block) starts from a state with a NaN: every cost of it is NaN, the final one included.
    An input value, not a fault: the solve runs to its end."""
    problem, _, _ = _case(n, m, T)
    clean = _launch(problem, T, how)
    x0 = problem[4].copy()
    x0[2, n - 1] = np.nan
    got = _launch(problem[:4] + (x0,), T, how)
    if how != "split":        # (the forward entry point takes no status)
        assert int(got[1][2]) == _hip.ST_NAN, (n, m, T, how, int(got[1][2]))
    assert torch.isnan(got[0]["costs"][2, T]).all()
    # the sweep does not depend on x0
    assert torch.equal(got[0]["K"][2], clean[0]["K"][2]) and torch.equal(got[0]["k"][2], clean[0]["k"][2])
    # its partner in the block (3), the block behind it (4, alone with the idle wave) and the block ahead (0, 1)
    _same_bits(got, clean, (n, m, T, how, "neighbours"), rows=(0, 1, 3, 4))
    assert int(got[1][[0, 1, 3, 4]].abs().sum()) == 0

"""The address paths of the matrix-core LQR kernel (lqr_mfma16x8.hip) that the rollout trim changed (``-m gpu``):

* the rollout's gain ring reads step ``min(t + 4, T - 1)`` through a wave-uniform base and a fixed lane offset; the turns of
  the ring run in a loop without exits and the last ``T mod 4`` steps behind it -- horizons below, at and just past the ring
  depth, and on both sides of the chunk length 52;
* the sweep stores its gains the same way (base moving down by one step);
* the chunk epilogue of the exact shape stores 16 bytes per lane, four lanes per state row, two per action row, and must
  store exactly the chunk's rows;
* the instance's bases come from the block index: first and last instance of B = 1 and B = 65.

Rule of ``test_lqr_sweep_trim_gpu.py``: per instance the ratio of |gpu - fp64 oracle| to |fp32 oracle - fp64 oracle| (floored
at 1e-6 of the tensor's scale) has median <= 2.5, 0.9 quantile <= 2 BUDGET, max <= 10 BUDGET; its generator, F scaled by 0.4.

Guard rows.  The kernel's instance stride is the instance's size, so a batched launch has room for a guard only behind its
last instance; a guard behind EVERY instance is had by solving each instance in a launch of its own (B = 1) into its slot of
a buffer with one spare row per instance.  Both are done, everything is NaN before the launch, and the two must agree bit for bit."""

import functools

import numpy as np
import pytest
import torch

import problems
from oracle import c_oracle
from tfmpc import _hip
from tfmpc.solvers.lqr import LQR, Policy

pytestmark = pytest.mark.gpu
BUDGET = 5.0
TRAJ = ("states", "actions", "costs", "K", "k")
VALUE = ("V", "v", "const")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(B, n, m, T):
    """Problem and its two oracle solves, made once per case."""
    F, f, C, c, x0 = problems.make_lqr_batch_fast(B, n, m, seed=41 * n + 7 * m + T)
    F *= 0.4
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True, want_value=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True, want_value=True)
    return (F, f, C, c, x0), ref64, ref32


def _check_ratios(out, ref64, ref32, keys, what):
    B = ref64["states"].shape[0]
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


def _solve_checked(B, n, m, T):
    """The launch without value outputs (the headline instantiation at (16, 8)) against the oracle; the one with them, bit for bit."""
    (F, f, C, c, x0), ref64, ref32 = _case(B, n, m, T)
    assert _hip.require_gpu().tfmpc_lqr_kernel_name(n, m, T).startswith(b"mfma_16x8")
    lqr = LQR(F, f, C, c)
    lean = lqr.solve_device(x0, T, want_policy=True)
    full = lqr.solve_device(x0, T, want_policy=True, want_value=True)
    torch.cuda.synchronize()
    what = f"B={B} ({n}, {m}) T={T}"
    for out in (lean, full):
        assert int(out["status"].abs().sum()) == 0, what
    _check_ratios(lean, ref64, ref32, TRAJ, what)
    for key in TRAJ:
        assert torch.equal(lean[key], full[key]), (what, "value outputs", key)
    return lqr, x0, lean, full, ref64, ref32


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8])
def test_ring_clamp_at_short_horizons(T):
    """T < ring depth, T = ring depth, just past it: the last gain loaded is step T - 1."""
    _solve_checked(3, 16, 8, T)


@pytest.mark.parametrize("T", [51, 52, 53, 105])
def test_chunk_boundary(T):
    """One row short of a chunk, a whole chunk, one row into the second, one row into the third: the bases carry across chunks and the
    epilogue's last partial iteration stores exactly the chunk's rows."""
    _solve_checked(2, 16, 8, T)


@pytest.mark.parametrize("B", [1, 65])
def test_first_and_last_instance(B):
    _solve_checked(B, 16, 8, 6)


def _raw_solve(lqr, x0, T, states, actions, costs, K, k, status, B):
    """tfmpc_lqr_solve_f32 into caller-owned buffers (views allowed: the entry takes addresses)."""
    lib = _hip.require_gpu()
    n, m = lqr.state_size, lqr.action_size
    rc = lib.tfmpc_lqr_solve_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(x0), _hip.ptr(states), _hip.ptr(actions), _hip.ptr(costs),
                                 _hip.ptr(K), _hip.ptr(k), None, None, None, _hip.ptr(status), None, 0, _hip.stream())
    _hip.check(rc, "tfmpc_lqr_solve_f32")


@pytest.mark.parametrize("n,m", [(5, 3), (16, 3), (7, 8), (16, 8)])
def test_guard_rows_stay_untouched(n, m):
    """Zero-padded shapes (and the exact one, whose stores are the widened ones): nothing is written outside an instance's rows."""
    B, T = 3, 6
    (F, f, C, c, x0), ref64, ref32 = _case(B, n, m, T)
    lqr = LQR(F, f, C, c)
    x0d = lqr._prep_x0(x0)
    dev = x0d.device
    rows = dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m))
    nan = float("nan")

    # (a) one launch, guard row behind the last instance
    flat = {key: torch.full((B * r + 1, w), nan, device=dev) for key, (r, w) in rows.items()}
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    _raw_solve(lqr, x0d, T, *(flat[key] for key in TRAJ), status, B)
    # (b) one launch per instance, guard row behind every instance
    slots = {key: torch.full((B, r + 1, w), nan, device=dev) for key, (r, w) in rows.items()}
    status1 = torch.full((B,), -1, dtype=torch.int32, device=dev)
    for b in range(B):
        one = LQR(F[b:b + 1], f[b:b + 1], C[b:b + 1], c[b:b + 1])
        _raw_solve(one, x0d[b:b + 1].contiguous(), T, *(slots[key][b] for key in TRAJ), status1[b:b + 1], 1)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0 and int(status1.abs().sum()) == 0
    what = f"({n}, {m}) T={T} guarded"
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][B * r:]).all(), (what, key, "guard behind the batch")
        assert torch.isnan(slots[key][:, r:]).all(), (what, key, "guard behind every instance")
        out[key] = flat[key][:B * r].reshape(B, r, w)
        assert torch.equal(out[key], slots[key][:, :r]), (what, key, "batched launch against single launches")
    _check_ratios(out, ref64, ref32, TRAJ, what)


@pytest.mark.parametrize("T", [5, 53])
def test_backward_then_forward_is_the_fused_launch(T):
    lqr, x0, lean, full, ref64, ref32 = _solve_checked(3, 16, 8, T)
    policy, value = lqr.backward(T)
    states, actions, costs = lqr.forward(Policy(policy.K, policy.k), x0, T)
    torch.cuda.synchronize()
    assert int(lqr.last_status.abs().sum()) == 0
    split = dict(states=states, actions=actions, costs=costs, K=policy.K, k=policy.k, V=value.V, v=value.v, const=value.const)
    for key in TRAJ + VALUE:
        assert torch.equal(split[key].reshape(full[key].shape), full[key]), (T, "backward + forward", key)


def test_value_and_16_bit_outputs():
    """One launch with value outputs against the oracle, one with 16-bit policy outputs against the fp32 launch."""
    T = 5
    lqr, x0, lean, full, ref64, ref32 = _solve_checked(3, 16, 8, T)
    _check_ratios(full, ref64, ref32, VALUE, f"(16, 8) T={T} value outputs")
    out16 = lqr.solve_device(x0, T, want_policy=True, storage_bf16=True)
    torch.cuda.synchronize()
    assert int(out16["status"].abs().sum()) == 0
    for key in ("states", "actions", "costs"):
        assert torch.equal(out16[key], lean[key]), ("16-bit outputs", key)
    for key in ("K", "k"):
        assert out16[key].dtype == torch.bfloat16
        assert torch.equal(out16[key], lean[key].to(torch.bfloat16)), ("16-bit outputs", key)


def test_four_and_five_waves_agree():
    T = 53
    lqr, x0, lean, full, ref64, ref32 = _solve_checked(3, 16, 8, T)
    with _hip.option("TFMPC_LQR_WAVES", "4"):
        lean4 = lqr.solve_device(x0, T, want_policy=True)
    torch.cuda.synchronize()
    for key in TRAJ:
        assert torch.equal(lean4[key], lean[key]), ("four waves", key)

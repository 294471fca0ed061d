"""How the paired sweep of the matrix-core LQR kernel is scheduled (lqr_mfma16x8.hip, wave_ldlt8_pair.h; ``-m gpu``).  None of
it may change a bit of any output:

* the register budget: ``TFMPC_LQR_WAVES`` = 4, 5, 6 and unset run instantiations sized for four, five and six resident waves
  per SIMD (six exists for the paired kernels only) -- the same instruction stream up to register allocation;
* the LDS overlay: the rollout's chunk buffer starts at float 0 of the wave's slice, on top of the sweep's elimination input,
  K~ and transpose staging.  A fused launch must give what the backward launch followed by the forward launch gives (where
  nothing is overlaid: each kernel uses one of the two layouts), past one rollout chunk (T = 53) and past two (T = 105), where
  the carried row and the reused slice meet; for the paired launch and for the one with value outputs (one wave per block, the
  same slice constants);
* the grouped wait states of the pair solve (one ``s_nop 1`` per group of broadcasts): a broadcast that read a stale lane would
  give an instance values that depend on what rides in the other rows of the wave, so at B = 6 every instance must keep its K and
  k whoever its block partner is and whichever wave it sits in;
* accuracy rule of ``test_lqr_rollout_trim_gpu.py`` against ``oracle.c_oracle``: per instance the ratio of |gpu - fp64 oracle| to
  |fp32 oracle - fp64 oracle| (floored at 1e-6 of the tensor's scale) has median <= 2.5, 0.9 quantile <= 2 BUDGET, max <=
  10 BUDGET.  The fp32 oracle is finite on every case used here (asserted).

Instances: ``problems.make_lqr_batch_spd``.  Every launch writes into NaN-filled buffers with a guard row behind the batch."""

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
NINST = 6


@functools.lru_cache(maxsize=None)
def _problem(n, m):
    arrays = problems.make_lqr_batch_spd(NINST, n, m, seed=23 * n + m)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _oracle(n, m, T):
    """The two oracle solves of the six instances, made once per shape and horizon."""
    F, f, C, c, x0 = _problem(n, m)
    ref64 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    ref32 = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float32, want_policy=True)
    for r in (ref64, ref32):
        for key in TRAJ:
            r[key].setflags(write=False)
    return ref64, ref32


def _launch(n, m, idx, T, mode="fused"):
    """Instances ``idx`` of the shape's problem (in that order).  ``mode``: "fused" (one launch without value outputs: paired blocks),
    "split" (backward without value outputs, then forward), "value" (one launch with value outputs: one wave per block),
    "value_split" (backward with value outputs, then forward).  Returns ({key: [B, rows, width]}, status [B]); checks the guards."""
    lib = _hip.require_gpu()
    idx = list(idx)
    B = len(idx)
    F, f, C, c, x0 = (np.ascontiguousarray(a[idx]) for a in _problem(n, m))
    assert lib.tfmpc_lqr_kernel_name(n, m, T).startswith(b"mfma_16x8")
    lqr = LQR(F, f, C, c)
    x0d = lqr._prep_x0(x0)
    dev = x0d.device
    rows = dict(states=(T + 1, n), actions=(T, m), costs=(T + 1, 1), K=(T, m * n), k=(T, m))
    value = mode.startswith("value")
    if value:
        rows.update(V=(T, n * n), v=(T, n), const=(T, 1))
    flat = {key: torch.full((B * r + 1, w), float("nan"), device=dev) for key, (r, w) in rows.items()}
    status = torch.full((B + 1,), -1, dtype=torch.int32, device=dev)
    vptr = [_hip.ptr(flat[key]) if value else None for key in VALUE]
    if mode.endswith("split"):
        rc = lib.tfmpc_lqr_backward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), _hip.ptr(flat["k"]), *vptr,
                                        _hip.ptr(status), _hip.stream())
        _hip.check(rc, "tfmpc_lqr_backward_f32")
        rc = lib.tfmpc_lqr_forward_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(flat["K"]), T * m * n, _hip.ptr(flat["k"]), T * m,
                                       _hip.ptr(x0d), _hip.ptr(flat["states"]), _hip.ptr(flat["actions"]), _hip.ptr(flat["costs"]),
                                       _hip.stream())
        _hip.check(rc, "tfmpc_lqr_forward_f32")
    else:
        rc = lib.tfmpc_lqr_solve_f32(B, n, m, T, *lqr._ptr_args(), _hip.ptr(x0d), *(_hip.ptr(flat[key]) for key in TRAJ),
                                     *vptr, _hip.ptr(status), None, 0, _hip.stream())
        _hip.check(rc, "tfmpc_lqr_solve_f32")
    torch.cuda.synchronize()
    out = {}
    for key, (r, w) in rows.items():
        assert torch.isnan(flat[key][B * r:]).all(), (idx, T, mode, key, "guard row behind the batch")
        out[key] = flat[key][:B * r].reshape(B, r, w)
        assert torch.isfinite(out[key]).all(), (idx, T, mode, key, "an output element was not written")
    assert int(status[B]) == -1, (idx, T, mode, "guard behind the status")
    assert int(status[:B].abs().sum()) == 0, (idx, T, mode, status[:B].tolist())
    return out, status[:B]


def _same_bits(got, pos, want, wpos, what, keys=TRAJ):
    (out, status), (wout, wstatus) = got, want
    for key in keys:
        assert torch.equal(out[key][pos], wout[key][wpos]), (what, key)
    assert int(status[pos]) == int(wstatus[wpos]), (what, "status")


@pytest.mark.parametrize("mfma", [None, "f32"])
@pytest.mark.parametrize("T", [1, 2, 5, 53])
@pytest.mark.parametrize("n,m", [(16, 8), (5, 3)])
def test_register_budgets_give_equal_bits(n, m, T, mfma):
    """B = 5: two paired blocks and an odd last one."""
    idx = range(5)
    with _hip.option("TFMPC_LQR_MFMA", mfma):
        got = {}
        for waves in ("4", "5", "6", None):
            with _hip.option("TFMPC_LQR_WAVES", waves):
                got[waves] = _launch(n, m, idx, T)
    for waves in ("5", "6", None):
        for pos in idx:
            _same_bits(got[waves], pos, got["4"], pos, ((n, m), T, mfma, waves, "against four waves", pos))


@pytest.mark.parametrize("mode", ["fused", "value"])
@pytest.mark.parametrize("T", [53, 105])
def test_lds_overlay_fused_equals_split(T, mode):
    """The fused launch runs sweep and rollout on ONE slice; backward then forward run each on a slice of its own."""
    idx = range(5)
    keys = TRAJ + (VALUE if mode == "value" else ())
    for n, m in ((16, 8), (5, 3)):
        fused = _launch(n, m, idx, T, mode)
        split = _launch(n, m, idx, T, mode + "_split" if mode == "value" else "split")
        for pos in idx:
            _same_bits(fused, pos, split, pos, ((n, m), T, mode, "fused against backward + forward", pos), keys)
        if mode == "value":      # ... and the paired launch and the one-wave launch agree on what both compute
            paired = _launch(n, m, idx, T, "fused")
            for pos in idx:
                _same_bits(paired, pos, fused, pos, ((n, m), T, "paired against value outputs", pos))


@pytest.mark.parametrize("mfma", [None, "f32"])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_partner_and_wave_change_nothing(T, mfma):
    """Six instances in three blocks; then every instance with another partner, in the other wave, and both."""
    n, m = 16, 8
    orders = ((0, 1, 2, 3, 4, 5),      # blocks (0, 1) (2, 3) (4, 5)
              (0, 3, 2, 5, 4, 1),      # same waves, other partners
              (1, 0, 3, 2, 5, 4),      # same partners, other waves
              (3, 0, 5, 2, 1, 4))      # other partners and other waves
    with _hip.option("TFMPC_LQR_MFMA", mfma):
        runs = [(order, _launch(n, m, order, T)) for order in orders]
    base_order, base = runs[0]
    for order, got in runs[1:]:
        for inst in range(NINST):
            _same_bits(got, order.index(inst), base, base_order.index(inst), (T, mfma, order, "instance", inst))


@pytest.mark.parametrize("T", [5, 53])
@pytest.mark.parametrize("n,m", [(16, 8), (5, 3)])
def test_accuracy_against_the_oracle(n, m, T):
    ref64, ref32 = _oracle(n, m, T)
    out, _ = _launch(n, m, range(NINST), T)
    what = f"({n}, {m}) T={T}"
    for key in TRAJ:
        assert np.isfinite(ref32[key]).all() and np.isfinite(ref64[key]).all(), (what, key, "the oracle itself")
        got = out[key].detach().cpu().numpy().astype(np.float64)
        ratios = []
        for b in range(NINST):
            want = ref64[key][b].reshape(got[b].shape)
            scale = np.abs(want).max()
            e32 = max(np.abs(ref32[key][b].astype(np.float64).reshape(want.shape) - want).max(), 1e-6 * scale)
            ratios.append(np.abs(got[b] - want).max() / e32)
        med, q9, top = np.median(ratios), np.quantile(ratios, 0.9), max(ratios)
        print(f"{what} {key}: median {med:.2f} q0.9 {q9:.2f} max {top:.2f}")
        assert med <= 2.5 and q9 <= 2 * BUDGET and top <= 10 * BUDGET, (what, key, med, q9, top)

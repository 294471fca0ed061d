"""The ground under tests/test_lqr_long_horizon_gpu.py, checked without a GPU:

* the numpy rollout of tests/lqr_rollout_ref.py is pinned to the existing oracles (``oracle/lqr_ref.py``, the C restatement);
* its workload is SAFE for the reference: under the per-step gains every shape stays bounded and finite in fp64 and in
  fp32 over the longest horizon, and the fp32 budget is near the 1e-6 floor, so it cannot hide a kernel error;
* the workload SEES the faults the GPU tests are for: an off-by-one in the gain index or in the carried state row at any
  chunk boundary moves the states by >= 1000 x the budget (100 x the largest ratio the GPU test lets through), while the
  same faults under the solver's own gains in mid-horizon move them by <= 1e-3 of it -- which is why the GPU tests do not
  simply call ``solve`` at a long horizon;
* the chunk lengths and ring depth the horizons are derived from are the ones in the kernel sources.
"""

import os
import re

import numpy as np
import pytest

import lqr_rollout_ref as ref
from oracle import c_oracle, lqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tf-mpc_amd", "csrc")
SHAPES = sorted(ref.SHAPES)
B = 8


def test_constants_are_the_kernel_sources():
    src16 = open(os.path.join(CSRC, "lqr_mfma16x8.hip")).read()
    src32 = open(os.path.join(CSRC, "lqr_mfma32x16.hip")).read()
    (tc,) = re.findall(r"^#define\s+TFMPC_LQR_TC\s+(\d+)\s*$", src16, flags=re.M)
    (ring,) = re.findall(r"^#define\s+TFMPC_LQR_RING\s+(\d+)\s*$", src16, flags=re.M)
    (tc32,) = re.findall(r"^constexpr\s+int\s+kTC\s*=\s*(\d+)\s*;", src32, flags=re.M)
    assert (int(tc), int(ring), int(tc32)) == (ref.CHUNK["mfma_16x8"], ref.RING, ref.CHUNK["mfma_32x16"])
    # the build does not override them
    assert not re.search(r"TFMPC_LQR_(TC|RING)", open(os.path.join(CSRC, "Makefile")).read())
    # every horizon family crosses a boundary, and the solve horizons put one inside the final transient
    for c in ref.CHUNK.values():
        assert c % ref.RING == 0
        hs = ref.rollout_horizons(c)
        assert len(set(hs)) == len(hs) == 10 and min(hs) == c - 1 and all(ref.boundaries(c, T) for T in hs if T > c)
        assert [T - ref.boundaries(c, T)[-1] for T in ref.solve_horizons(c)[:4]] == [1, 2, ref.RING, 9]
        assert all(ref.boundaries(c, T - T1) and T1 < T for T1, T in ref.split_points(c))


@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (24, 12)])
def test_rollout_is_pinned_to_the_oracles(n, m):
    T = 60
    F, f, C, c, x0 = ref.workload(4, n, m, seed=3)
    sol = c_oracle.lqr_solve(F, f, C, c, x0, T, dtype=np.float64, want_policy=True)
    for b in range(4):
        got = ref.rollout(F[b], f[b], C[b], c[b], sol["K"][b], sol["k"][b], x0[b], T)
        for name in ref.FIELDS:
            assert np.abs(got[name] - sol[name][b]).max() <= 1e-12 * np.abs(sol[name][b]).max(), (name, b)
    # ... and under gains that are NOT the solver's, to the numpy restatement of the reference's forward pass
    K, k = ref.per_step_gains(sol["K"][0, 0], T, np.random.default_rng(5))
    got = ref.rollout(F[0], f[0], C[0], c[0], K, k, x0[0], T)
    xs, us, cs = lqr_ref.forward(F[0], f[0], C[0], c[0], [(K[t], k[t][:, None]) for t in range(T)], x0[0], T)
    for name, want in zip(ref.FIELDS, (xs[..., 0], us[..., 0], cs.reshape(-1))):
        assert np.abs(got[name] - want).max() <= 1e-12 * np.abs(want).max(), name
    # the fp32 restatement computes in fp32
    assert all(v.dtype == np.float32 for v in ref.rollout(F[0], f[0], C[0], c[0], K, k, x0[0], 3, np.float32).values())


@pytest.mark.parametrize("n,m", SHAPES)
def test_workload_is_safe_for_the_reference(n, m):
    """The GPU tests' own case (same seeds; their horizons are prefixes of this one)."""
    case = ref.case(n, m, B)
    T = max(ref.rollout_horizons(ref.chunk(n, m)))
    assert case["K"].shape[1] >= T + ref.EXTRA_STEPS
    r64 = ref.rollout_batch(*case["problem"][:4], case["K"], case["k"], case["problem"][4], T, np.float64)
    r32 = ref.rollout_batch(*case["problem"][:4], case["K"], case["k"], case["problem"][4], T, np.float32)
    for b in range(B):
        for name in ref.FIELDS:
            assert np.isfinite(r64[b][name]).all() and np.isfinite(r32[b][name]).all(), (name, b)
        scale = np.abs(r64[b]["states"]).max()
        assert 1.0 <= scale <= 1e3, (b, scale)
        # the state keeps moving to the end (nothing settles into a fixed point that would hide a step)
        assert np.abs(np.diff(r64[b]["states"][-100:], axis=0)).max(axis=1).min() >= 1e-2 * scale, b
        # the budget is fp32 rounding, not an instability: a kernel 10 x the budget off is still within 1e-4 of scale
        e32 = np.abs(r32[b]["states"].astype(np.float64) - r64[b]["states"]).max()
        assert e32 <= 1e-5 * scale, (b, e32 / scale)
    print(f"({n}, {m}): max|x| {max(np.abs(r['states']).max() for r in r64):.1f}")


@pytest.mark.parametrize("n,m", SHAPES)
def test_solve_workload_is_safe_and_its_gains_still_change_at_the_boundary(n, m):
    """The full-solve case of the GPU file: the fp32 oracle is finite and within 1e-4 of scale of the fp64 one at the
    longest horizon (so the budget is rounding), and at the four short horizons the gains on the two sides of the chunk
    boundary differ by far more than rounding (so taking the wrong one is seen)."""
    c = ref.chunk(n, m)
    F, f, C, cc, x0 = ref.solve_case(n, m, 37)
    T = max(ref.solve_horizons(c))
    s64 = c_oracle.lqr_solve(F, f, C, cc, x0, T, dtype=np.float64, nthreads=8, want_policy=True, want_value=True)
    s32 = c_oracle.lqr_solve(F, f, C, cc, x0, T, dtype=np.float32, nthreads=8, want_policy=True, want_value=True)
    assert s64["status"] == 0 and s32["status"] == 0
    for key in ("states", "actions", "costs", "K", "k", "V", "v", "const"):
        a, b = s64[key].reshape(37, -1), s32[key].astype(np.float64).reshape(37, -1)
        assert np.isfinite(b).all() and (np.abs(a - b).max(axis=1) <= 1e-4 * np.abs(a).max(axis=1)).all(), key
    assert np.abs(s64["states"]).max() <= 1e3
    steps = {}
    for T in ref.solve_horizons(c)[:4]:
        K = c_oracle.lqr_solve(F, f, C, cc, x0, T, dtype=np.float64, want_policy=True)["K"]
        steps[T - c] = np.abs(K[:, c] - K[:, c - 1]).reshape(37, -1).max(axis=1) / np.abs(K[:, 0]).reshape(37, -1).max(axis=1)
    # boundary one or two steps before the end: K changes by percents of its size on EVERY instance; a ring turn before
    # the end: on the median instance by 1e-3 or more.  Nine steps before the end the sweep has converged on some
    # instances (measured: median 1e-6 .. 3e-4 of |K|, smallest 2e-10 at (5, 3)): that horizon adds little on its own.
    assert steps[1].min() >= 1e-2 and steps[2].min() >= 1e-2, (steps[1].min(), steps[2].min())
    assert np.median(steps[ref.RING]) >= 1e-3, np.median(steps[ref.RING])


def _faulted_states(F, f, K, k, truth, t, kind, T, tail=8):
    """States t+1 .. of the fp64 rollout with ONE wrong step t: ``gain`` uses step t + 1's gains, ``carry`` takes the
    previous row x_{t-1} for the state (what a chunk's row 0 holds when the carry copies the wrong row)."""
    n = F.shape[0]
    x = truth["states"][t - 1] if kind == "carry" else truth["states"][t]
    g = t + 1 if kind == "gain" else t
    out = []
    for s in range(t, min(T, t + 1 + tail)):
        u = K[g] @ x + k[g]
        x = F @ np.concatenate([x, u]) + f
        out.append(x)
        g = s + 1
    assert len(out[0]) == n
    return np.array(out)


def _fault_ratio(F, f, K, k, r64, r32, t, kind, T):
    bad = _faulted_states(F, f, K, k, r64, t, kind, T)
    ref_x = r64["states"]
    budget = max(np.abs(r32["states"].astype(np.float64) - ref_x).max(), 1e-6 * np.abs(ref_x).max())
    return np.abs(bad - ref_x[t + 1:t + 1 + len(bad)]).max() / budget


@pytest.mark.parametrize("n,m", SHAPES)
def test_workload_sees_an_off_by_one_at_every_chunk_boundary(n, m):
    c = ref.chunk(n, m)
    case = ref.case(n, m, B)
    F, f, C, cc, x0 = case["problem"]
    worst = np.inf
    for T in ref.rollout_horizons(c):
        if not ref.boundaries(c, T):
            continue
        r64 = ref.rollout_batch(F, f, C, cc, case["K"], case["k"], x0, T, np.float64)
        r32 = ref.rollout_batch(F, f, C, cc, case["K"], case["k"], x0, T, np.float32)
        for t in ref.boundaries(c, T):
            for kind in ("carry", "gain"):
                if kind == "gain" and t + 1 >= T:      # the last step has no next gain: the kernels clamp the prefetch to it
                    continue
                for b in range(B):
                    r = _fault_ratio(F[b], f[b], case["K"][b], case["k"][b], r64[b], r32[b], t, kind, T)
                    assert r >= 1000.0, (T, t, kind, b, r)
                    worst = min(worst, r)
    print(f"({n}, {m}): smallest fault / budget {worst:.3g}")


@pytest.mark.parametrize("n,m", SHAPES)
def test_the_solvers_own_gains_hide_the_same_faults_in_mid_horizon(n, m):
    c = ref.chunk(n, m)
    F, f, C, cc, x0 = ref.case(n, m, B)["problem"]
    for T in (2 * c + 1, 257, 1000):
        s64 = c_oracle.lqr_solve(F, f, C, cc, x0, T, dtype=np.float64, want_policy=True)
        s32 = c_oracle.lqr_solve(F, f, C, cc, x0, T, dtype=np.float32, want_policy=True)
        for b in range(B):
            r64, r32 = dict(states=s64["states"][b]), dict(states=s32["states"][b])
            for kind in ("carry", "gain"):
                r = _fault_ratio(F[b], f[b], s64["K"][b], s64["k"][b], r64, r32, c, kind, T)
                assert r <= 1e-3, (T, kind, b, r)

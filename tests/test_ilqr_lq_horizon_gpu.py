"""The three matrix-core iLQR kernels of the LQ env at their horizon edges and past T = 50 (``-m gpu``): ``lq_mfma``
(tf-mpc_amd/csrc/ilqr_lq_mfma.hip: trajectories in LDS up to T = 187, gain rings 4 and 2 deep), ``lq_box_mfma`` (ilqr_lq_box_mfma.hip:
bounded actions, up to T = 148, ring 4 deep) and ``lq_mfma32`` (ilqr_lq_mfma32.hip: any T, LDS chunks of 48 steps, ring 4 / 1 deep).

Horizons: below every ring depth (1, 2, 3), T mod 4 = 1 (5, 9, 13, 53), one ring turn around the chunk of 48 (47 .. 52, 97, 99, 145),
on the LDS caps (186, 187; 147, 148), one past them (188, 149: the wave kernel, pinned by name), 257 and 1000.  Workload, references
and budget rule: tests/ilqr_lq_horizon_ref.py -- every solve against the fp64 restatement of ilqr.py per instance, budget the fp32
restatement's own error floored at 1e-6 of scale, median over instances of error / budget <= 2.5 and every instance <= 10 (the rule of
tests/test_tvlqr_gpu.py).  tests/test_ilqr_lq_horizon_cpu.py shows on this very workload that ONE wrong step at any of these horizons'
ring ends or chunk starts moves the solution by >= 100 x the budget (and lists the mid-horizon chunk starts whose carried row cannot be
seen by any tolerance).

Every case runs with TFMPC_ILQR_LQ_REUSE unset and = 0, at the default tolerance and with ``atol = 1e-12, max_iterations = 4`` (every
instance makes all four passes: three gain-reusing vector recursions in a row).  Iterations: the fp64 restatement's on every instance;
under the unreachable tolerance 1 .. 3 -- fp64 reaches 1e-12 and stops at 1, an fp32 program iterates on rounding noise and its count
follows no reference (``test_the_unreachable_tolerance_is_reachable_in_fp64`` in the CPU file); the trajectory is held to fp64 all the same.  Every test prints its ratios (``-s``)."""

import numpy as np
import pytest
import torch

import ilqr_lq_horizon_ref as ref
from tfmpc import _hip
from tfmpc.envs.lq import LQEnv
from tfmpc.solvers.ilqr import iLQR

pytestmark = pytest.mark.gpu

OPTIONS = ("TFMPC_ILQR_KERNEL", "TFMPC_ILQR_LQ_REUSE")
NAMES = {"lq_mfma": "lq_mfma (matrix cores)", "lq_mfma32": "lq_mfma32 (matrix cores, 2 x 2 tiles)",
         "lq_box_mfma": "lq_box_mfma (matrix cores, control-limited)", "wave": "wave"}
CONFIGS = ((), ref.ATOL_CONFIG)
TRACE_ROWS = 6


@pytest.fixture(autouse=True)
def options_restored():
    before = {name: _hip.get_option(name) for name in OPTIONS}
    yield
    for name, value in before.items():
        _hip.set_option(name, value)


def _solve(kernel, n, m, T, B, bound=None, config=(), reuse=None, form="exact", trace_rows=0):
    """One launch on the case's problem -> per-instance host dicts, the raw outputs."""
    F, f, C, c, x0, u0 = ref.workload(B, n, m, ref.seed_of(n, m), T, bound)
    box = {} if bound is None else dict(low=-bound, high=bound)
    solver = iLQR(LQEnv(F, f, C, c, **box), **dict(config))
    with _hip.option("TFMPC_ILQR_KERNEL", "lq_generic" if form == "generic" and (n, m) == (16, 8) else None), \
            _hip.option("TFMPC_ILQR_LQ_REUSE", reuse):
        out = solver.solve_device(x0.astype(np.float32)[..., None], T, u_init=u0.astype(np.float32)[..., None], trace_rows=trace_rows)
        torch.cuda.synchronize()
    assert solver.last_kernel.startswith(NAMES[kernel]), (solver.last_kernel, kernel, n, m, T)      # no case runs on another kernel
    host = {name: out[name].float().cpu().numpy().astype(np.float64) for name in ref.FIELDS}
    got = [dict(states=host["states"][b, :, :, 0], actions=host["actions"][b, :, :, 0], costs=host["costs"][b]) for b in range(B)]
    assert all(np.isfinite(g[name]).all() for g in got for name in ref.FIELDS)
    assert np.array_equal(host["states"][:, 0, :, 0], x0)
    return got, out


def _unbounded_case(kernel, n, m, T, form="exact", B=None, fields=ref.FIELDS, configs=CONFIGS):
    B = ref.batch_of(T) if B is None else B
    lines = []
    for config in configs:
        r64, r32 = ref.oracle(n, m, T, ref.seed_of(n, m), B, None, config)
        want = [a["iterations"] for a in r64]
        assert all(a["iterations"] == 1 for a in r64)
        traces = {}
        for reuse in (None, "0"):
            got, out = _solve(kernel, n, m, T, B, None, config, reuse, form, trace_rows=TRACE_ROWS)
            what = (kernel, form, n, m, T, dict(config), reuse)
            assert int(out["status"].abs().sum()) == 0, what
            its = out["iterations"].cpu().tolist()
            if config:              # passes on rounding noise: no fewer than fp64 makes, no more than allowed (see the CPU file)
                assert all(w <= i <= 3 for i, w in zip(its, want)), (what, its)
            else:
                assert its == want, (what, its, want)
                assert out["trace_len"].cpu().tolist() == [w + 1 for w in want], what
            report = {}
            try:
                ref.check_budget(got, r64, r32, what, fields, report=report)
            finally:
                lines.append(f"{'atol' if config else 'default'} reuse={reuse}: " + ", ".join(f"{k} {a:.2f}/{b:.2f}" for k, (a, b) in report.items()))
            traces[reuse] = out["trace"][:, 0].nan_to_num(-7.0)
        # the first pass is the same code with and without gain reuse: its trace row is the same bits (an instance that one of the two
        # hands to the wave kernel at the noise floor of the unreachable tolerance has its rows rewritten: tests/test_ilqr_lq_mfma_gpu.py)
        same = (traces[None] == traces["0"]).all(dim=1).float().mean()
        assert float(same) >= (0.9 if config else 1.0), (kernel, n, m, T, float(same))
    print(f"\n{kernel} {form} ({n}, {m}) T={T} B={B} (median/max): " + "; ".join(lines))


# ------------------------------------------------------------------------------------------------------------------- lq_mfma --
@pytest.mark.parametrize("form,n,m,T", [("exact", 16, 8, T) for T in ref.T_LQ_EXACT] +
                         [("generic", n, m, T) for n, m in ref.SHAPES_LQ_GENERIC for T in ref.T_LQ_GENERIC])
def test_lq_mfma_horizons(form, n, m, T):
    _unbounded_case("lq_mfma", n, m, T, form)


# ----------------------------------------------------------------------------------------------------------------- lq_mfma32 --
@pytest.mark.parametrize("n,m,T", [(n, m, T) for n, m in ref.SHAPES_MFMA32 for T in ref.T_MFMA32])
def test_lq_mfma32_horizons(n, m, T):
    _unbounded_case("lq_mfma32", n, m, T)


def test_lq_mfma32_thousand_steps():
    """The one unbounded matrix-core kernel that admits T = 1000 (21 chunks): states and costs."""
    _unbounded_case("lq_mfma32", 32, 16, ref.T_LONG, fields=("states", "costs"), configs=((),))


# ---------------------------------------------------------------------------------------------------------------- the switch --
def test_the_lds_cap_switches_lq_mfma_to_the_wave_kernel_after_187_steps():
    n, m = 16, 8
    _unbounded_case("lq_mfma", n, m, ref.T_SWITCH_LQ, configs=((),))
    T = ref.T_SWITCH_LQ + 1
    B = ref.batch_of(T)
    r64, r32 = ref.oracle(n, m, T, ref.seed_of(n, m), B)
    got, out = _solve("wave", n, m, T, B)
    assert int(out["status"].abs().sum()) == 0 and out["iterations"].cpu().tolist() == [a["iterations"] for a in r64]
    report = {}
    ref.check_budget(got, r64, r32, ("wave", T), report=report)
    print(f"\nwave (16, 8) T={T}: {report}")


def _bounded_case(kernel, n, m, T):
    bound, B = ref.BOUND, ref.batch_of(T, True)
    F, f, C, c, x0, u0 = ref.workload(B, n, m, ref.seed_of(n, m), T, bound)
    r64, r32 = ref.oracle(n, m, T, ref.seed_of(n, m), B, bound)
    got, out = _solve(kernel, n, m, T, B, bound)
    assert int((out["status"] & (_hip.ST_NAN | _hip.ST_MAX_ATTEMPTS)).sum()) == 0
    its = out["iterations"].cpu().tolist()
    for b in range(B):
        st, ac, total = got[b]["states"], got[b]["actions"], got[b]["costs"].sum()
        c64, c32 = r64[b]["costs"].sum(), float(r32[b]["costs"].astype(np.float64).sum())
        near64 = abs(total - c64) <= 2e-3 * np.abs(r64[b]["costs"]).sum()
        near32 = abs(total - c32) <= 2e-3 * np.abs(r64[b]["costs"]).sum()
        assert near64 or near32, (T, b, total, c64, c32)
        assert np.abs(ac).max() <= bound + 1e-6, (T, b)
        pred = np.concatenate([st[:-1], ac], axis=1) @ F[b].T + f[b]                 # the rollout obeys x' = F z + f
        assert np.abs(pred - st[1:]).max() <= 2e-5 * max(np.abs(st).max(), 1.0), (T, b)
    same = [b for b in range(B) if its[b] == r64[b]["iterations"]]
    report = {}
    try:
        assert len(same) >= 0.8 * B, (T, its, [a["iterations"] for a in r64])
        ref.check_budget(got, r64, r32, (kernel, n, m, T), ("states",), idx=same, report=report)
    finally:
        on_bound = np.mean([np.mean(np.abs(g["actions"]) >= bound - 1e-6) for g in got])
        print(f"\n{kernel} ({n}, {m}) T={T} B={B}: iterations as fp64 on {len(same)}, {on_bound:.2f} of the actions on the bound, states median/max {report.get('states')}")


def test_the_lds_cap_switches_lq_box_mfma_to_the_wave_kernel_after_148_steps():
    _bounded_case("lq_box_mfma", 16, 8, ref.T_SWITCH_BOX)
    _bounded_case("wave", 16, 8, ref.T_SWITCH_BOX + 1)


# --------------------------------------------------------------------------------------------------------------- lq_box_mfma --
@pytest.mark.parametrize("n,m,T", [(n, m, T) for n, m in ref.SHAPES_BOX for T in ref.T_BOX])
def test_lq_box_mfma_horizons(n, m, T):
    _bounded_case("lq_box_mfma", n, m, T)

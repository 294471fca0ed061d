"""The double-precision control-limited time-varying LQR solve on the MI355X: tfmpc_tvlqr_box_solve_f64
(tfmpc.solvers.tvlqr_box_solve(dtype=torch.float64)) against the longdouble restatement.

Budget, the project's double rule (tests/tvlqr_box_f64_ref.py): per instance and per output (states, actions, costs),
the kernel's error against the longdouble run divided by max(the fp64 numpy restatement's error on that instance,
2^-48 max(1, |ref|_inf)); median <= 2.5 and every instance <= 10.  What the rule relies on -- both restatements
converged, their held sets equal, the share of clear instances -- is asserted without a GPU by
tests/test_tvlqr_box_f64_cpu.py."""
import numpy as np
import pytest
import torch

import tvlqr_box_f64_ref as dref
import tvlqr_box_solve_ref as sref
from tfmpc import _hip

pytestmark = pytest.mark.gpu

F64 = torch.float64
OUTPUTS = dref.OUTPUTS
ST_NOT_PD = 2
NAMES = ("F", "f", "C", "c", "low", "high")


def _t(a, dtype=F64):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype, device="cuda")


def _solve(ops, dtype=F64, **kw):
    """ops: numpy arrays (F f C c x0 low high Cfin cfin) or tensors -> numpy outputs with the batch axis kept."""
    from tfmpc.solvers import tvlqr_box_solve
    # (numpy vectors go in with their trailing column axis: at n = 1 or m = 1 and T = 1 a [B, 1, 1] vector would be read
    # as [T, 1] with a dropped column axis)
    p = {k: (_t(v[..., None] if k in ("f", "c", "low", "high") and v.ndim >= 2 else v) if isinstance(v, np.ndarray) else v)
         for k, v in ops.items()}
    kw = {k: (_t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    res = tvlqr_box_solve(p["F"], p["f"], p["C"], p["c"], p["x0"], p["low"], p["high"], C_final=p.get("Cfin"),
                          c_final=p.get("cfin"), dtype=dtype, **kw)
    torch.cuda.synchronize()
    want = torch.float32 if dtype in (None, torch.float32) else F64
    assert all(t.dtype == want for t in res)
    info = res.info
    out = dict(states=res[0][..., 0], actions=res[1][..., 0], costs=res[2][..., 0, 0], iterations=info.last_iterations,
               status=info.last_status, reason=info.last_reason, clamped=info.last_clamped)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _converged(got, r64=None):
    assert not got["status"].any(), got["status"]
    assert not got["reason"].any(), got["reason"]
    if r64 is not None:                        # sweep counts differ by at most one between precisions and summation orders
        assert np.abs(got["iterations"] - r64["iterations"]).max() <= 1, (got["iterations"], r64["iterations"])


def _held_sets(got, ops, sol):
    """info.last_clamped is the set read off the actions' bits, and on clear instances the exact set."""
    held = dref.held_from_actions(got["actions"], ops["low"], ops["high"])
    assert np.array_equal(got["clamped"], held)
    clear = sol["clear"]
    assert np.array_equal(held[clear], sol["clamped"][clear])
    lo, hi = np.broadcast_to(ops["low"], held.shape), np.broadcast_to(ops["high"], held.shape)
    assert (got["actions"] >= lo).all() and (got["actions"] <= hi).all()


@pytest.mark.parametrize("n,m,T,width", dref.CASES)
def test_shapes_and_horizons(n, m, T, width):
    """Models per instance and per step; (1, 1) the smallest, m > n, the wave16 edge and the first wave32 shapes, the full
    mask word (with every control held: width 1e-3), and LDS above 64 KiB."""
    lib = _hip.load()
    assert lib.tfmpc_tvlqr_box_solve_kernel_name_f64(n, m, T).decode() == ("tv_box_f64_wave16" if max(n, m) <= 16 else "tv_box_f64_wave32")
    ops, sol, rld, r64 = dref.case(n, m, T, width)
    got = _solve(ops)
    print(f"f64 box {n}x{m} T={T} sweeps", got["iterations"].tolist(), "restatement", r64["iterations"].tolist())
    _converged(got, r64)
    dref.check(got, r64, rld, f"{n}x{m} T={T} width={width}")
    _held_sets(got, ops, sol)
    if width < 1.0:
        assert got["clamped"].all()


@pytest.mark.parametrize("which", ["batch", "time", "both"])
def test_stride_zero_operands_give_the_bits_of_materialised_copies(which):
    """Shared and unbatched operands, a time axis of 1 and an expanded one: read with stride 0, no copy, the same bits."""
    n, m, T = 12, 6, 8
    B = dref.BATCH
    ops = dref.case(n, m, T)[0]
    full = {k: _t(ops[k]) for k in NAMES}
    full["F"] = 0.6 * full["F"]                                      # (one step's draw held for T steps: keep it stable)
    if which in ("batch", "both"):
        full = {k: v[:1].expand(B, *v.shape[1:]) for k, v in full.items()}
    if which in ("time", "both"):
        full = {k: v[:, :1].expand(v.shape[0], T, *v.shape[2:]) for k, v in full.items()}
    thin = dict(full)
    if which in ("time", "both"):
        thin = {k: (v if k == "high" else v[:, :1]) for k, v in thin.items()}     # a time axis of 1 (one operand carries T)
    if which in ("batch", "both"):
        thin = {k: v[0] for k, v in thin.items()}                     # no batch axis
    a = _solve(dict(thin, x0=ops["x0"]))
    b = _solve(dict({k: v.contiguous() for k, v in full.items()}, x0=ops["x0"]))
    c = _solve(dict(full, x0=ops["x0"]))                              # expanded views: stride 0, no copy
    assert not a["status"].any() and a["iterations"].max() > 1
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    # against the restatement on the materialised problem
    mat = {k: v.contiguous().cpu().numpy() for k, v in full.items()}
    mat["x0"] = ops["x0"]
    sol, rld, r64 = dref.references(mat)
    _converged(b, r64)
    dref.check(b, r64, rld, f"stride 0 ({which})")


def test_a_scalar_and_a_per_step_infinite_bound():
    n, m, T = 5, 3, 20
    ops = dref.case(n, m, T)[0]
    high = ops["high"][0].copy()                                      # [T, m], shared by the batch
    high[::3, 0] = np.inf
    high[5:9] = np.inf
    mat = dict(ops, low=np.full_like(ops["low"], -np.inf), high=np.broadcast_to(high, ops["high"].shape).copy())
    sol, rld, r64 = dref.references(mat)
    got = _solve(dict(ops, low=-np.inf, high=high))
    _converged(got, r64)
    assert got["clamped"].any() and not got["clamped"].all()
    dref.check(got, r64, rld, "infinite bounds")
    _held_sets(got, mat, sol)


def test_an_explicit_final_cost_equal_to_the_default_gives_the_same_bits():
    n, m, T = 5, 3, 20
    ops = dref.case(n, m, T)[0]
    base = _solve(ops)
    same = _solve(dict(ops, Cfin=np.ascontiguousarray(ops["C"][:, -1, :n, :n]), cfin=np.ascontiguousarray(ops["c"][:, -1, :n])))
    for k in base:
        assert np.array_equal(base[k], same[k]), k


def test_numpy_inputs_and_non_contiguous_tensors_give_the_same_bits():
    from tfmpc.solvers import tvlqr_box_solve
    n, m, T = 5, 3, 20
    ops = dref.case(n, m, T)[0]
    base = _solve(ops)
    res = tvlqr_box_solve(*(ops[k] for k in ("F", "f", "C", "c", "x0", "low", "high")), dtype=F64)      # numpy, on the default device
    assert all(t.dtype == F64 and t.is_cuda for t in res)
    assert np.array_equal(res[0][..., 0].cpu().numpy(), base["states"]) and np.array_equal(res[1][..., 0].cpu().numpy(), base["actions"])
    # a transposed inner block and a padded last axis (copied), a strided time axis (kept: the per-step block is dense)
    odd = {k: _t(ops[k]) for k in NAMES}
    odd["C"] = odd["C"].transpose(-1, -2).contiguous().transpose(-1, -2)
    pad = torch.zeros(*odd["F"].shape[:-1], n + m + 3, dtype=F64, device="cuda")
    pad[..., :n + m] = odd["F"]
    odd["F"] = pad[..., :n + m]
    two = torch.zeros(odd["c"].shape[0], 2 * T, n + m, dtype=F64, device="cuda")
    two[:, ::2] = odd["c"]
    odd["c"] = two[:, ::2]
    assert not odd["C"].is_contiguous() and not odd["F"].is_contiguous() and not odd["c"].is_contiguous()
    got = _solve(dict(odd, x0=ops["x0"]))
    for k in base:
        assert np.array_equal(base[k], got[k]), k


def test_a_start_at_the_rounded_optimum_and_a_pinned_box():
    n, m, T = 16, 8, 50
    ops, sol, rld, r64 = dref.case(n, m, T)
    warm = _solve(ops, u_init=rld["actions"].astype(np.float64))
    print("f64 warm sweeps", warm["iterations"].tolist())
    _converged(warm)
    assert (warm["iterations"] <= 2).all()
    dref.check(warm, r64, rld, "warm start")
    _held_sets(warm, ops, sol)
    shared = _solve(ops, u_init=rld["actions"][0].astype(np.float64))          # one start for the batch: [T, m]
    assert np.array_equal(shared["actions"][0], warm["actions"][0])
    # low == high: no sweep, the bound's own double bits
    got = _solve(dict(ops, high=ops["low"]))
    assert not got["iterations"].any() and not got["status"].any() and not got["reason"].any() and not got["clamped"].any()
    assert np.array_equal(got["actions"], ops["low"])
    pin = sref.solve_batch(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["low"], ops["low"], dtype=np.float64)
    pld = sref.solve_batch(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["low"], ops["low"], dtype=dref.LD, tol=dref.LD_TOL)
    dref.check(got, pin, pld, "pinned box")


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 20)])
def test_without_bounds_it_is_the_double_tvlqr_solve(n, m, T):
    """The same rule with TimeVaryingLQR(dtype=torch.float64)'s own error as the budget, and with the restatement's."""
    from tfmpc.solvers import TimeVaryingLQR
    ops = dref.case(n, m, T)[0]
    B = dref.BATCH
    free = dict(ops, low=np.full_like(ops["low"], -np.inf), high=np.full_like(ops["high"], np.inf))
    _, rld, r64 = dref.references(free)
    got = _solve(dict(ops, low=-np.inf, high=np.inf))
    _converged(got, r64)
    assert (got["iterations"] <= 2).all() and not got["clamped"].any()
    dref.check(got, r64, rld, f"unbounded {n}x{m}")
    tv = TimeVaryingLQR(ops["F"], ops["f"], ops["C"], ops["c"], device="cuda", dtype=F64)
    out = tv.solve_device(_t(ops["x0"][..., None]))
    torch.cuda.synchronize()
    plain = dict(states=out["states"][..., 0].cpu().numpy(), actions=out["actions"][..., 0].cpu().numpy(),
                 costs=out["costs"].reshape(B, -1).cpu().numpy())
    dref.check(plain, r64, rld, f"tfmpc_tvlqr_solve_f64 {n}x{m}")
    dref.check(got, plain, rld, f"unbounded {n}x{m} against tfmpc_tvlqr_solve_f64")


@pytest.mark.parametrize("rho,width", dref.RESCUED)
def test_the_rescued_class(rho, width):
    """Problems the fp32 kernel's arithmetic cannot solve (its restatement flags NOT_PD, tests/test_tvlqr_box_f64_cpu.py):
    status 0, reason 0 and the rule, on the instances whose fp64 restatement converges by the step norm."""
    ops, rld, r64, _ = dref.rescued(rho, width)
    got = _solve(ops)
    good = r64["reason"] == 0
    print("rescued", rho, width, "sweeps", got["iterations"].tolist(), "reasons", got["reason"].tolist(), "compared", good.tolist())
    assert not got["status"][good].any() and not got["reason"][good].any()
    assert np.abs(got["iterations"] - r64["iterations"])[good].max() <= 1
    assert all(np.isfinite(got[k][good]).all() for k in OUTPUTS)
    dref.check(got, r64, rld, f"rescued rho={rho}", pick=good)
    assert np.array_equal(got["clamped"][good], r64["clamped"][good])


def test_statuses_are_per_instance():
    n, m, T = 5, 3, 6
    ops, sol, _, _ = dref.case(n, m, T)
    bad = {k: (None if v is None else v.copy()) for k, v in ops.items()}
    s, i = np.argwhere(~sol["clamped"][2])[0]
    bad["C"][2, s, n + i, n + i] = -50.0                              # an indefinite C_uu at one step
    got = _solve(bad)
    rest = [0, 1, 3]
    assert got["status"][2] & ST_NOT_PD and not got["status"][rest].any() and got["reason"][2] == sref.REASON_FAILED
    for k in OUTPUTS:
        assert np.isnan(got[k][2]).all() and np.isfinite(got[k][rest]).all(), k
    alone = _solve({k: (None if v is None else v[rest]) for k, v in ops.items()})
    for k in alone:
        assert np.array_equal(got[k][rest], alone[k]), k


def test_the_default_dtype_with_double_inputs_gives_todays_fp32_bits():
    n, m, T = 5, 3, 20
    ops = dref.case(n, m, T)[0]
    cast = {k: (None if v is None else _t(v, torch.float32)) for k, v in ops.items()}
    want = _solve(cast, dtype=torch.float32)
    for dtype in (None, torch.float32):
        got = _solve({k: (None if v is None else _t(v)) for k, v in ops.items()}, dtype=dtype)       # double tensors in
        for k in want:
            assert np.array_equal(want[k], got[k]), (k, dtype)
    assert not want["status"].any() and want["states"].dtype == np.float32

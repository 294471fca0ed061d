"""The double-precision control-limited time-varying LQR solve without a GPU: the yardstick of
tests/test_tvlqr_box_f64_gpu.py (tests/tvlqr_box_f64_ref.py) pinned -- every condition that test relies on is asserted
here -- then the C ABI's declarations, bindings and argument rules, the Python front end's routing against a recorder,
and the kernels' register budget from the gfx950 assembly.

The tests up to test_the_rescued_class_is_ill_conditioned_not_ill_posed run numpy only; the ones after test the FEATURE."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import tvlqr_box_f64_ref as dref
import tvlqr_box_solve_ref as sref
import tvlqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc import solvers  # noqa: E402

EXPORTS = ("tfmpc_tvlqr_box_solve_workspace_bytes_f64", "tfmpc_tvlqr_box_solve_kernel_name_f64", "tfmpc_tvlqr_box_solve_f64")


# ------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("n,m,T,width", dref.CASES)
def test_both_restatements_converge_to_the_same_held_sets(n, m, T, width):
    ops, sol, rld, r64 = dref.case(n, m, T, width)
    for r in (rld, r64):
        assert (r["status"] == 0).all() and (r["reason"] == sref.REASON_CONVERGED).all(), (r["status"], r["reason"])
    assert np.array_equal(rld["clamped"], r64["clamped"])
    assert np.abs(rld["iterations"] - r64["iterations"]).max() <= 1            # (12 sweeps against 11 at 16 x 8, T = 50)
    clear = sol["clear"]
    assert clear.mean() >= dref.CLEAR_SHARE_EACH, clear
    for r in (rld, r64):
        held = dref.held_from_actions(r["actions"].astype(np.float64), ops["low"], ops["high"])
        assert np.array_equal(held[clear], sol["clamped"][clear]) and np.array_equal(r["clamped"][clear], sol["clamped"][clear])
    # the operands are no fp32 numbers: a path through fp32 cannot meet the double budget
    for k in ("F", "f", "C", "c", "x0", "low", "high"):
        assert (ops[k] != ops[k].astype(np.float32)).mean() > 0.9, k
    assert np.array_equal(ops["C"], np.swapaxes(ops["C"], -1, -2))
    # the fp64 restatement is at the rule's floor: 2^-48 is 3.6e-15
    for name in dref.OUTPUTS:
        scale = np.maximum(1.0, np.abs(rld[name].reshape(dref.BATCH, -1)).max(1).astype(np.float64))
        assert (dref.instance_error(r64[name], rld[name]) <= 4 * dref.FLOOR * scale).all(), name
    if width < 1.0:
        assert sol["clamped"].all()                                           # the tight box: every control held


def test_the_share_of_clear_instances():
    clear = np.concatenate([dref.case(*cs)[1]["clear"] for cs in dref.CASES])
    assert clear.mean() >= dref.CLEAR_SHARE_ALL, clear.mean()


def test_a_rounding_through_fp32_misses_the_rule_by_orders():
    """The rule has teeth: the same restatement on operands rounded to fp32 is 1e5 budgets away."""
    ops, _, rld, r64 = dref.case(5, 3, 20)
    low = {k: (None if v is None else v.astype(np.float32).astype(np.float64)) for k, v in ops.items()}
    bad = sref.solve_batch(low["F"], low["f"], low["C"], low["c"], low["x0"], low["low"], low["high"], dtype=np.float64)
    for name in dref.OUTPUTS:
        assert np.median(dref.ratios(bad[name], r64[name], rld[name])) > 1e5, name


@pytest.mark.parametrize("rho,width", dref.RESCUED)
def test_the_rescued_class_is_ill_conditioned_not_ill_posed(rho, width):
    ops, rld, r64, r32 = dref.rescued(rho, width)
    for k in ("F", "f", "C", "c", "x0", "low", "high"):
        assert np.array_equal(ops[k], ops[k].astype(np.float32)), k          # fp32 is handed the very same problem
    flagged = (r32["status"] & sref.ST_NOT_PD) != 0
    print("rescued", rho, width, "fp32 flags", flagged.tolist(), "fp64 reasons", r64["reason"].tolist(), "sweeps",
          r64["iterations"].tolist(), "max |x| %.3g" % np.nanmax(np.abs(r64["states"])))
    assert not r64["status"].any() and not rld["status"].any()
    assert np.array_equal(r64["reason"], rld["reason"]) and np.array_equal(r64["clamped"], rld["clamped"])
    good = r64["reason"] == sref.REASON_CONVERGED
    if (rho, width) == dref.RESCUED[0]:
        assert flagged.mean() >= 0.5 and good.all()
    else:
        assert flagged.any() and good.sum() >= 5 and set(r64["reason"].tolist()) <= {0, 1}
        cl = r64["clamped"].reshape(len(good), -1)
        assert (cl.any(1) & ~cl.all(1)).any()                                 # held and free controls in one instance
    for name in dref.OUTPUTS:
        scale = np.maximum(1.0, np.abs(rld[name].reshape(len(good), -1)).max(1).astype(np.float64))
        assert (dref.instance_error(r64[name], rld[name])[good] <= 4 * dref.FLOOR * scale[good]).all(), name


# ------------------------------------------------------------------------- the feature
def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    f32, f64 = (_hip._SIGNATURES["tfmpc_tvlqr_box_solve_" + s] for s in ("f32", "f64"))
    assert f64[0] == f32[0] and len(f64[1]) == len(f32[1]) == 4 + 16 + 6 + 5 + 7 + 3
    differ = [i for i, (a, b) in enumerate(zip(f32[1], f64[1])) if a is not b]
    assert differ == [30] and f32[1][30] is ctypes.c_float and f64[1][30] is ctypes.c_double      # tol


def test_kernel_name_and_workspace_per_shape():
    lib = _hip.load()
    name = lambda n, m: lib.tfmpc_tvlqr_box_solve_kernel_name_f64(n, m, 50).decode()      # noqa: E731
    assert name(16, 8) == name(16, 16) == name(1, 1) == "tv_box_f64_wave16"
    assert name(17, 8) == name(16, 17) == name(32, 32) == name(8, 32) == "tv_box_f64_wave32"
    assert name(16, 33) == name(200, 8) == name(33, 1) == "unsupported" and name(0, 3) == name(3, 0) == "invalid"
    assert lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64(2, 16, 8, 50) == 8 * 2 * (50 * 8 * 17 + 51 * 16 + 50 * 8 + 51)
    assert lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64(2, 16, 8, 50) == 2 * lib.tfmpc_tvlqr_box_solve_workspace_bytes(2, 16, 8, 50)
    assert lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64(0, 16, 8, 50) == 0
    assert lib.tfmpc_tvlqr_box_solve_workspace_bytes_f64(-1, 16, 8, 50) == 0


def test_abi_argument_errors_return_before_any_launch():
    """tests/test_tvlqr_box_solve_cpu.py's list, in its order, against the double entry point."""
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4, dtype=torch.float64))

    def call(B=1, n=3, m=2, T=4, s=0, F=p, Cfin=None, cfin=None, low=p, high=p, x0=p, su=0, max_iter=0, tol=0.0, states=p,
             iterations=p, status=p, ws=p, ws_bytes=1 << 20):
        return lib.tfmpc_tvlqr_box_solve_f64(B, n, m, T, F, s, s, p, s, s, p, s, s, p, s, s, Cfin, 0, cfin, 0, low, s, s, high, s, s,
                                             x0, None, su, max_iter, tol, states, p, p, iterations, status, None, None, ws,
                                             ws_bytes, None)

    assert call(B=-1) == -1 and call(n=0) == -1 and call(m=0) == -1 and call(T=0) == -1
    assert call(max_iter=-1) == -1 and call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(F=None) == -1 and call(low=None) == -1 and call(high=None) == -1 and call(x0=None) == -1
    assert call(Cfin=p) == -1 and call(cfin=p) == -1                      # both or neither
    assert call(s=-3) == -1 and call(su=-1) == -1
    assert call(states=None) == -1 and call(iterations=None) == -1 and call(status=None) == -1
    assert call(m=33) == -2 and call(n=200, m=8) == -2 and call(n=33) == -2 and call(B=0, m=33) == -2
    assert call(ws=None) == -4 and call(ws_bytes=8 * (4 * 2 * 4 + 5 * 3 + 4 * 2 + 5) - 1) == -4
    assert call(B=0, F=None, low=None, high=None, x0=None, states=None, iterations=None, status=None, ws=None) == 0   # a no-op
    assert call(B=-1, m=33) == -1 and call(m=33, ws=None) == -2          # the order: argument, shape, workspace


class _Recorder:
    """Stands in for the library: keeps the launch's symbol and arguments, returns TFMPC_OK."""

    def __init__(self):
        self.calls = []

    def tfmpc_tvlqr_box_solve_workspace_bytes(self, B, n, m, T):
        return 4 * B * (T * m * (n + 1) + (T + 1) * n + T * m + T + 1)

    def tfmpc_tvlqr_box_solve_workspace_bytes_f64(self, B, n, m, T):
        return 8 * B * (T * m * (n + 1) + (T + 1) * n + T * m + T + 1)

    def tfmpc_tvlqr_box_solve_f32(self, *args):
        self.calls.append(("f32", args))
        return 0

    def tfmpc_tvlqr_box_solve_f64(self, *args):
        self.calls.append(("f64", args))
        return 0


def _value(p):
    return p.value if isinstance(p, ctypes.c_void_p) else p


@pytest.fixture
def recorder(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_hip, "require_gpu", lambda: lib)
    monkeypatch.setattr(_hip, "stream", lambda: None)
    monkeypatch.setattr(_hip, "default_device", lambda: torch.device("cpu"))
    return lib


def _problem(B=3, T=4, n=3, m=2):
    F, f, C, c = (torch.as_tensor(a, dtype=torch.float64) for a in tvlqr_ref.make_models(n, m, T, B, seed=3))
    x0 = torch.as_tensor(tvlqr_ref.make_x0(n, B), dtype=torch.float64)
    return F, f, C, c, x0


def test_float64_routes_to_the_double_symbol_with_element_strides(recorder):
    B, T, n, m = 3, 4, 3, 2
    d = n + m
    F, f, C, c, x0 = _problem(B, T, n, m)
    low, high = -torch.ones(B, T, m, dtype=torch.float64), torch.ones(B, T, m, dtype=torch.float64)
    out = solvers.tvlqr_box_solve(F, f, C, c, x0, low, high, max_iter=7, tol=1e-13, dtype=torch.float64)
    assert all(t.dtype == torch.float64 for t in out)
    assert tuple(out[0].shape) == (B, T + 1, n, 1) and tuple(out[1].shape) == (B, T, m, 1) and tuple(out[2].shape) == (B, T + 1, 1, 1)
    sym, a = recorder.calls[-1]
    assert sym == "f64" and a[:4] == (B, n, m, T)
    assert _value(a[4]) == F.data_ptr() and a[5:7] == (T * n * d, n * d)              # the caller's doubles: no copy, ELEMENT strides
    assert _value(a[7]) == f.data_ptr() and _value(a[10]) == C.data_ptr() and _value(a[13]) == c.data_ptr()
    assert a[8:10] == (T * n, n) and a[11:13] == (T * d * d, d * d) and a[14:16] == (T * d, d)
    assert a[16] is None and a[18] is None
    assert _value(a[20]) == low.data_ptr() and _value(a[23]) == high.data_ptr() and _value(a[26]) == x0.data_ptr()
    assert a[21:23] == (T * m, m) and a[24:26] == (T * m, m)
    assert a[27] is None and a[28] == 0 and a[29] == 7 and a[30] == 1e-13              # tol: no fp32 rounding
    assert a[-2] >= recorder.tfmpc_tvlqr_box_solve_workspace_bytes_f64(B, n, m, T)
    info = out.info
    assert tuple(info.last_clamped.shape) == (B, T, m) and info.last_reason.dtype == torch.int32
    assert tuple(info.last_iterations.shape) == (B,) and tuple(info.last_status.shape) == (B,)

    # shared by the batch, constant in time (an axis of 1 and an expanded axis), scalar and [m] bounds, a final cost, u_init
    Fx = F[0, :1].expand(T, n, d)
    u0 = torch.zeros(T, m, dtype=torch.float64)
    out = solvers.tvlqr_box_solve(Fx, f[:1, :, :, None], C[:, :1], c[0], x0, -0.5, torch.ones(m, dtype=torch.float64),
                                  C_final=torch.eye(n, dtype=torch.float64).expand(B, n, n), c_final=torch.zeros(n), u_init=u0,
                                  dtype=torch.float64)
    sym, a = recorder.calls[-1]
    assert sym == "f64" and a[:4] == (B, n, m, T)
    assert _value(a[4]) == F.data_ptr() and a[5:7] == (0, 0)
    assert a[8:10] == (0, n) and a[11:13] == (T * d * d, 0) and a[14:16] == (0, d)
    assert a[17] == n * n and a[19] == 0 and a[16] is not None and a[18] is not None
    assert a[21:23] == (0, 0) and a[24:26] == (0, 0)
    assert _value(a[27]) == u0.data_ptr() and a[28] == 0 and a[29] == 0 and a[30] == 0.0

    # numpy and fp32 operands are taken to double
    out = solvers.tvlqr_box_solve(F.numpy(), f.float(), C.numpy(), c, x0.numpy(), -1.0, 1.0, dtype=torch.float64)
    assert recorder.calls[-1][0] == "f64" and out[0].dtype == torch.float64

    # no batch axis anywhere: one instance, unbatched results
    out = solvers.tvlqr_box_solve(F[0], f[0], C[0], c[0], x0[0], -1.0, 1.0, dtype=torch.float64)
    assert recorder.calls[-1][1][0] == 1 and tuple(out[0].shape) == (T + 1, n, 1) and not out.info.batched


def test_the_default_dtype_still_calls_the_fp32_symbol(recorder):
    F, f, C, c, x0 = _problem()
    for kw in ({}, dict(dtype=None), dict(dtype=torch.float32)):
        out = solvers.tvlqr_box_solve(F, f, C, c, x0, -1.0, 1.0, **kw)           # fp64 inputs: cast to fp32, as before
        sym, a = recorder.calls[-1]
        assert sym == "f32" and out[0].dtype == torch.float32 and _value(a[4]) != F.data_ptr()
        assert a[-2] >= recorder.tfmpc_tvlqr_box_solve_workspace_bytes(3, 3, 2, 4)


def test_float64_refuses_gradients_and_other_dtypes_are_refused(recorder):
    F, f, C, c, x0 = _problem()
    low = torch.full((2,), -1.0, dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32"):
        solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32"):
        solvers.tvlqr_box_solve(F.clone().requires_grad_(), f, C, c, x0, -1.0, 1.0, dtype=torch.float64)
    assert not recorder.calls
    with torch.no_grad():                                                      # nothing records: a plain double solve
        assert solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0, dtype=torch.float64)[0].dtype == torch.float64
    for bad in (torch.float16, torch.bfloat16, torch.int32, "float64", np.float64):
        with pytest.raises(ValueError, match="dtype"):
            solvers.tvlqr_box_solve(F, f, C, c, x0, -1.0, 1.0, dtype=bad)
    assert len(recorder.calls) == 1
    # the fp32 path keeps its autograd graph
    out = solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0)
    assert all(t.requires_grad for t in out)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_kernels_use_no_scratch_fit_the_register_file_and_run_on_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_box_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 2 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    for name, private, vgprs, spills in found:
        assert "tvlqr_box_solve_f64_kernel" in name
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        body = re.search(r"^" + re.escape(name) + r":.*?\n(.*?)^\s*\.amdhsa_kernel\s+" + re.escape(name), text, flags=re.S | re.M).group(1)
        assert "v_mfma_f64_16x16x4_f64" in body and "v_mfma_f32" not in body, name

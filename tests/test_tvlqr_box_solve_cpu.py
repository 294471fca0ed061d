"""The control-limited time-varying LQR forward without a GPU: the numpy restatement
(tests/tvlqr_box_solve_ref.py) pinned against the exact fp64 optimum, the plain TV-LQR solve and the pinned box; the C
ABI's declarations, bindings and argument rules; the Python front end's routing, stride mapping and validation against
a recorder; and the kernel's register budget from the gfx950 assembly.

The first four tests pin the YARDSTICK of tests/test_tvlqr_box_solve_gpu.py and run numpy only; the tests from
test_every_new_export_is_declared_bound_and_exported on test the FEATURE."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import lqr_box_grad_ref as bref
import tvlqr_box_solve_ref as sref
import tvlqr_ref
from test_lqr_box_grad_cpu import GPU_TV_BATCH, GPU_TV_HORIZONS, GPU_TV_SHAPES, tv_final

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc import solvers  # noqa: E402

EXPORTS = ("tfmpc_tvlqr_box_solve_workspace_bytes", "tfmpc_tvlqr_box_solve_kernel_name", "tfmpc_tvlqr_box_solve_f32")
CASES = [(n, m, T) for (n, m) in GPU_TV_SHAPES for T in GPU_TV_HORIZONS]


@pytest.mark.parametrize("n,m,T", CASES)
def test_the_restatement_in_fp64_is_the_exact_optimum(n, m, T):
    ops, sol, _ = sref.case(n, m, T, GPU_TV_BATCH, tv_final(T))
    got = sref.solve_batch(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["low"], ops["high"], ops["Cfin"], ops["cfin"],
                           dtype=np.float64)
    assert (got["status"] == 0).all() and (got["reason"] == 0).all()
    for name in ("states", "actions", "costs"):
        scale = np.maximum(1.0, np.abs(sol[name]).reshape(GPU_TV_BATCH, -1).max(1))
        assert (sref.instance_error(got[name], sol[name]) <= 1e-9 * scale).all(), name
    held = (got["actions"] == ops["low"]) | (got["actions"] == ops["high"])
    assert np.array_equal(held, sol["clamped"]) and np.array_equal(got["clamped"], sol["clamped"])


@pytest.mark.parametrize("n,m,T", CASES)
def test_the_restatement_in_fp32_converges_to_the_exact_held_set(n, m, T):
    ops, sol, r32 = sref.case(n, m, T, GPU_TV_BATCH, tv_final(T))
    assert (r32["status"] == 0).all() and (r32["reason"] == sref.REASON_CONVERGED).all()
    assert (r32["iterations"] < sref.DEFAULT_PASSES).all()
    held = sref.held_from_actions(r32["actions"], ops["low"], ops["high"])
    clear = sol["clear"]
    assert np.array_equal(held[clear], sol["clamped"][clear]) and np.array_equal(r32["clamped"][clear], sol["clamped"][clear])
    assert (r32["actions"] >= ops["low"].astype(np.float32)).all() and (r32["actions"] <= ops["high"].astype(np.float32)).all()


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-10), (np.float32, 2e-5)])
def test_without_bounds_the_restatement_is_the_tvlqr_solve(dtype, tol):
    ops, _ = bref.tv_case(5, 3, 20, 3)
    for b in range(3):
        got = sref.solve(ops["F"][b], ops["f"][b], ops["C"][b], ops["c"][b], ops["x0"][b], -np.inf, np.inf, dtype=dtype)
        ref = tvlqr_ref.solve(ops["F"][b], ops["f"][b], ops["C"][b], ops["c"][b], ops["x0"][b][:, None])
        assert got["status"] == 0 and got["reason"] == 0 and got["iterations"] <= 2 and not got["clamped"].any()
        for name in ("states", "actions", "costs"):
            assert np.abs(got[name] - ref[name]).max() <= tol * max(1.0, np.abs(ref[name]).max()), name


def test_a_pinned_box_returns_the_bounds_bits_after_zero_sweeps():
    ops, _ = bref.tv_case(5, 3, 6, 2)
    for b in range(2):
        got = sref.solve(ops["F"][b], ops["f"][b], ops["C"][b], ops["c"][b], ops["x0"][b], ops["low"][b], ops["low"][b])
        assert got["iterations"] == 0 and got["status"] == 0 and got["reason"] == 0
        assert np.array_equal(got["actions"], ops["low"][b].astype(np.float32))


# ------------------------------------------------------------------------- the feature
def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    # B n m T, the model (16), low high (6), x0 u_init su_b max_iter tol, 3 + 4 outputs, workspace bytes stream
    assert len(_hip._SIGNATURES["tfmpc_tvlqr_box_solve_f32"][1]) == 4 + 16 + 6 + 5 + 7 + 3
    assert callable(solvers.tvlqr_box_solve) and "tvlqr_box_solve" in dir(solvers)


def test_kernel_name_and_workspace_per_shape():
    lib = _hip.load()
    name = lambda n, m: lib.tfmpc_tvlqr_box_solve_kernel_name(n, m, 50).decode()      # noqa: E731
    assert name(16, 8) == name(32, 32) == name(3, 5) == name(1, 1) == "tv_box_wave"
    assert name(16, 33) == name(200, 8) == "unsupported" and name(0, 3) == "invalid"
    assert lib.tfmpc_tvlqr_box_solve_workspace_bytes(2, 16, 8, 50) == 4 * 2 * (50 * 8 * 17 + 51 * 16 + 50 * 8 + 51)
    assert lib.tfmpc_tvlqr_box_solve_workspace_bytes(0, 16, 8, 50) == 0


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4))

    def call(B=1, n=3, m=2, T=4, s=0, F=p, Cfin=None, cfin=None, low=p, high=p, x0=p, su=0, max_iter=0, tol=0.0, states=p,
             iterations=p, status=p, ws=p, ws_bytes=1 << 20):
        return lib.tfmpc_tvlqr_box_solve_f32(B, n, m, T, F, s, s, p, s, s, p, s, s, p, s, s, Cfin, 0, cfin, 0, low, s, s, high, s, s,
                                             x0, None, su, max_iter, tol, states, p, p, iterations, status, None, None, ws,
                                             ws_bytes, None)

    assert call(B=-1) == -1 and call(n=0) == -1 and call(m=0) == -1 and call(T=0) == -1
    assert call(max_iter=-1) == -1 and call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(F=None) == -1 and call(low=None) == -1 and call(high=None) == -1 and call(x0=None) == -1
    assert call(Cfin=p) == -1 and call(cfin=p) == -1                      # both or neither
    assert call(s=-3) == -1 and call(su=-1) == -1
    assert call(states=None) == -1 and call(iterations=None) == -1 and call(status=None) == -1
    assert call(m=33) == -2 and call(n=200, m=8) == -2 and call(B=0, m=33) == -2
    assert call(ws=None) == -4 and call(ws_bytes=15) == -4
    assert call(B=0, F=None, low=None, high=None, x0=None, states=None, iterations=None, status=None, ws=None) == 0   # a no-op
    assert call(B=-1, m=33) == -1 and call(m=33, ws=None) == -2          # the order: argument, shape, workspace


class _Recorder:
    """Stands in for the library: keeps the launch's arguments, returns TFMPC_OK."""

    def __init__(self):
        self.calls = []

    def tfmpc_tvlqr_box_solve_workspace_bytes(self, B, n, m, T):
        return 4 * B * (T * m * (n + 1) + (T + 1) * n + T * m + T + 1)

    def tfmpc_tvlqr_box_solve_f32(self, *args):
        self.calls.append(args)
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
    F, f, C, c = (torch.as_tensor(a) for a in tvlqr_ref.make_models(n, m, T, B, seed=3))
    x0 = torch.as_tensor(tvlqr_ref.make_x0(n, B))
    return F, f, C, c, x0


def test_shapes_and_strides_up_to_the_launch(recorder):
    B, T, n, m = 3, 4, 3, 2
    d = n + m
    F, f, C, c, x0 = _problem(B, T, n, m)
    low, high = -torch.ones(B, T, m), torch.ones(B, T, m)
    out = solvers.tvlqr_box_solve(F, f, C, c, x0, low, high, max_iter=7, tol=1e-5)
    assert tuple(out[0].shape) == (B, T + 1, n, 1) and tuple(out[1].shape) == (B, T, m, 1) and tuple(out[2].shape) == (B, T + 1, 1, 1)
    a = recorder.calls[-1]
    assert a[:4] == (B, n, m, T)
    assert _value(a[4]) == F.data_ptr() and a[5:7] == (T * n * d, n * d)               # F: no copy, its own strides
    assert a[8:10] == (T * n, n) and a[11:13] == (T * d * d, d * d) and a[14:16] == (T * d, d)
    assert a[16] is None and a[18] is None                                               # the default final cost
    assert a[21:23] == (T * m, m) and a[24:26] == (T * m, m)                            # low, high
    assert a[27] is None and a[28] == 0 and a[29] == 7 and a[30] == pytest.approx(1e-5)
    assert a[-2] >= recorder.tfmpc_tvlqr_box_solve_workspace_bytes(B, n, m, T)
    info = out.info
    assert tuple(info.last_clamped.shape) == (B, T, m) and info.last_reason.dtype == torch.int32
    assert tuple(info.last_iterations.shape) == (B,) and tuple(info.last_status.shape) == (B,)

    # shared by the batch, constant in time (an axis of 1 and an expanded axis), scalar and [m] bounds, a final cost, u_init
    Fx = F[0, :1].expand(T, n, d)
    u0 = torch.zeros(T, m)
    out = solvers.tvlqr_box_solve(Fx, f[:1, :, :, None], C[:, :1], c[0], x0, -0.5, torch.ones(m), C_final=torch.eye(n).expand(B, n, n),
                                  c_final=torch.zeros(n), u_init=u0)
    a = recorder.calls[-1]
    assert a[:4] == (B, n, m, T)
    assert _value(a[4]) == F.data_ptr() and a[5:7] == (0, 0)
    assert a[8:10] == (0, n) and a[11:13] == (T * d * d, 0) and a[14:16] == (0, d)     # (C[:, :1] keeps its batch stride)
    assert a[17] == n * n and a[19] == 0 and a[16] is not None and a[18] is not None
    assert a[21:23] == (0, 0) and a[24:26] == (0, 0)
    assert _value(a[27]) == u0.data_ptr() and a[28] == 0 and a[29] == 0 and a[30] == 0.0
    assert tuple(out[0].shape) == (B, T + 1, n, 1)

    # a start with a batch axis of 1 beside a larger batch is shared, as every other operand is
    u1 = torch.zeros(1, T, m)
    solvers.tvlqr_box_solve(F, f, C, c, x0, low, high, u_init=u1)
    a = recorder.calls[-1]
    assert a[0] == B and _value(a[27]) == u1.data_ptr() and a[28] == 0

    # no batch axis anywhere: one instance, unbatched results
    out = solvers.tvlqr_box_solve(F[0], f[0], C[0], c[0], x0[0], -1.0, 1.0, u_init=torch.zeros(1, T, m)[0])
    assert recorder.calls[-1][0] == 1 and tuple(out[0].shape) == (T + 1, n, 1) and tuple(out[2].shape) == (T + 1, 1, 1)
    assert not out.info.batched


def test_a_result_that_needs_gradients_is_in_the_autograd_graph(recorder):
    F, f, C, c, x0 = _problem()
    low = torch.full((2,), -1.0, requires_grad=True)
    out = solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0)
    assert all(t.requires_grad for t in out)
    assert type(out[0].grad_fn.next_functions[0][0]).__name__.startswith("TvBoxSolveFunction")
    plain = solvers.tvlqr_box_solve(F, f, C, c, x0, low.detach(), 1.0)
    assert not any(t.requires_grad for t in plain)
    with torch.no_grad():
        assert not solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0)[0].requires_grad


@pytest.mark.parametrize("bad", ["F2d", "m0", "m33", "f_size", "C_size", "horizons", "batches", "low_size", "low_above_high",
                                 "nan_bound", "final_one", "final_size", "x0_size", "u_init_T", "max_iter", "tol"])
def test_bad_inputs_raise_before_any_launch(bad, monkeypatch):
    monkeypatch.setattr(_hip, "require_gpu", lambda: pytest.fail("a launch was prepared"))
    monkeypatch.setattr(_hip, "default_device", lambda: torch.device("cpu"))
    F, f, C, c, x0 = _problem()
    low, high, kw = -1.0, 1.0, {}
    if bad == "F2d":
        F = F[0, 0]
    elif bad == "m0":
        F = F[..., :3]
    elif bad == "m33":
        F, C, c = torch.zeros(4, 3, 36), torch.zeros(4, 36, 36), torch.zeros(4, 36)
    elif bad == "f_size":
        f = f[..., :2]
    elif bad == "C_size":
        C = C[..., :4, :4]
    elif bad == "horizons":
        C = C[:, :3]
    elif bad == "batches":
        c = torch.cat([c, c])
    elif bad == "low_size":
        low = -torch.ones(3)
    elif bad == "low_above_high":
        low = torch.tensor([-1.0, 2.0])
    elif bad == "nan_bound":
        high = torch.tensor([1.0, float("nan")])
    elif bad == "final_one":
        kw = dict(C_final=torch.eye(3))
    elif bad == "final_size":
        kw = dict(C_final=torch.eye(4), c_final=torch.zeros(4))
    elif bad == "x0_size":
        x0 = x0[:, :2]
    elif bad == "u_init_T":
        kw = dict(u_init=torch.zeros(5, 2))
    elif bad == "max_iter":
        kw = dict(max_iter=-1)
    elif bad == "tol":
        kw = dict(tol=float("nan"))
    with pytest.raises(ValueError):
        solvers.tvlqr_box_solve(F, f, C, c, x0, low, high, **kw)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_kernel_uses_no_scratch_and_fits_the_register_file():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_box.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 1 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    for name, private, vgprs, spills in found:
        assert "tvlqr_box_solve_kernel" in name
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)

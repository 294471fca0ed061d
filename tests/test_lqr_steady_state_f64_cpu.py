"""Double-precision infinite-horizon LQR without a GPU: the 80-bit restatement of
tests/lqr_steady_state_f64_ref.py pinned against the LAPACK restatement and scipy, the row exchanges the GPU test's
inputs produce, the C ABI's declarations, bindings and argument errors, the Python front end's validation, and the
kernels' register budget.

The first four tests (the 80-bit format, the restatement against LAPACK and scipy, the row exchanges, the flagged
instances) pin the YARDSTICK of tests/test_lqr_steady_state_f64_gpu.py: they run numpy only and do not depend on the
feature.  The tests from test_every_new_export_is_declared_bound_and_exported on test the FEATURE: the exports, the
argument rules, the front end and the kernels' assembly."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.linalg
import torch

import lqr_steady_state_f64_ref as ref64
import lqr_steady_state_ref as ssref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import lqr_steady_state  # noqa: E402
from tfmpc.solvers.lqr import LQR  # noqa: E402

EXPORTS = ("tfmpc_lqr_steady_state_kernel_name_f64", "tfmpc_lqr_steady_state_f64")
# the parity shapes of tests/test_lqr_steady_state_f64_gpu.py with more than one row
PIVOT_SHAPES = [(3, 2), (12, 6), (16, 8), (16, 16), (17, 8), (16, 17), (22, 3), (32, 16), (32, 32)]


def test_longdouble_is_the_80_bit_format():
    assert np.finfo(np.longdouble).nmant == 63


@pytest.mark.parametrize("kind", ["make_lqr", "damped"])
@pytest.mark.parametrize("n,m", [(3, 2), (16, 8), (32, 16)])
def test_the_80_bit_restatement_is_the_lapack_one_and_scipy(n, m, kind):
    B = 3
    F, f, C, c = ref64.operands(kind, n, m, B, seed=10 * n + m)
    for b in range(B):
        ld = ref64.steady_state_ld(F[b], f[b], C[b], c[b])
        la = ssref.steady_state(F[b], f[b], C[b], c[b], dtype=np.float64)
        gj = ref64.steady_state_gj(F[b], f[b], C[b], c[b])
        assert ld["status"] == 0 and la["status"] == 0 and gj["status"] == 0
        assert ld["P"].dtype == np.longdouble and gj["P"].dtype == np.float64
        for name in ref64.FIELDS:
            assert ref64.error(la[name], ld[name]) <= 1e-10 * ref64.scale_of(ld[name]), (name, b)
        P = scipy.linalg.solve_discrete_are(F[b][:, :n], F[b][:, n:], C[b][:n, :n], C[b][n:, n:], s=C[b][:n, n:])
        assert ref64.error(P, ld["P"]) <= 1e-9 * ref64.scale_of(ld["P"]), b
        assert abs(gj["iterations"] - ld["iterations"]) <= 1, (gj["iterations"], ld["iterations"])


@pytest.mark.parametrize("n,m", PIVOT_SHAPES)
def test_the_gpu_tests_inputs_exchange_rows_in_both_pivoted_solves(n, m):
    F, f, C, c = ref64.operands("make_lqr", n, m, 6, seed=10 * n + m)
    got = [ref64.steady_state_gj(F[b], f[b], C[b], c[b]) for b in range(6)]
    assert all(g["status"] == 0 for g in got)
    assert sum(g["exchanges_sda"] for g in got) >= 1
    assert sum(g["exchanges_p"] for g in got) >= 1


def test_the_restatement_flags_what_the_lapack_one_flags():
    F, f, C, c = ref64.operands("make_lqr", 5, 3, 2, seed=3)
    F0, C0 = F[0].copy(), C[0].copy()
    F0[0, :] = 0.0
    F0[:, 0] = 0.0
    F0[0, 0] = 1.5
    C0[0, 1:] = 0.0
    C0[1:, 0] = 0.0
    got = ref64.steady_state_gj(F0, f[0], C0, c[0])
    assert got["status"] == ssref.ST_NOT_STABILISING and np.isnan(got["K"]).all()
    C1 = C[1].copy()
    C1[5:, 5:] = -np.eye(3)
    got = ref64.steady_state_gj(F[1], f[1], C1, c[1])
    assert got["status"] == ssref.ST_NOT_PD and got["iterations"] == 0


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    assert len(_hip._SIGNATURES["tfmpc_lqr_steady_state_f64"][1]) == len(_hip._SIGNATURES["tfmpc_lqr_steady_state_f32"][1])


def test_kernel_names_per_shape():
    name = lambda n, m: _hip.load().tfmpc_lqr_steady_state_kernel_name_f64(n, m).decode()   # noqa: E731
    assert name(16, 8) == name(16, 16) == name(1, 1) == "ss_f64_wave16"
    assert name(17, 8) == name(16, 17) == name(32, 32) == "ss_f64_wave32"
    assert name(33, 1) == "unsupported"
    assert name(0, 3) == "invalid"


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4, dtype=torch.float64))
    st = p

    def call(B=1, n=3, m=2, F=p, f=p, C=p, c=p, s=0, max_iter=0, tol=0.0, status=st):
        return lib.tfmpc_lqr_steady_state_f64(B, n, m, F, s, f, s, C, s, c, s, max_iter, tol, p, p, p, p, None, status, None)

    assert call(B=-1) == -1
    assert call(n=0) == -1 and call(m=0) == -1
    assert call(max_iter=-1) == -1
    assert call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(C=None) == -1 and call(c=None) == -1
    assert call(status=None) == -1
    assert call(s=-3) == -1
    assert call(n=33) == -2 and call(m=33) == -2 and call(B=0, n=40, m=40) == -2
    assert call(B=0, F=None, f=None, C=None, c=None, status=None) == 0          # B == 0: a no-op, nothing is read


def _operands(n=3, m=2, B=2):
    return ref64.operands("make_lqr", n, m, B, seed=5)


def test_a_dtype_that_is_not_served_is_refused():
    F, f, C, c = _operands()
    for dtype in (torch.float16, torch.bfloat16, np.float64, "float64"):
        with pytest.raises(ValueError):
            lqr_steady_state(F, f, C, c, dtype=dtype)
        with pytest.raises(ValueError):
            LQR(F, f, C, c, device="cpu").steady_state(dtype=dtype)


def test_gradients_in_double_are_refused_before_any_launch(monkeypatch):
    monkeypatch.setattr(_hip, "require_gpu", lambda: pytest.fail("a launch was prepared"))
    F, f, C, c = (torch.as_tensor(a) for a in _operands())
    with pytest.raises(NotImplementedError):
        lqr_steady_state(F.clone().requires_grad_(), f, C, c, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        LQR(F.clone().requires_grad_(), f, C, c, device="cpu").steady_state(dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        LQR(F, f, C, c, device="cpu").steady_state(dtype=torch.float64, differentiable=True)


def test_symmetry_is_checked_to_1e_12_in_double():
    F, f, C, c = _operands()
    C = C.copy()
    C[1, 0, 4] += 1e-9 * np.abs(C[1]).max()
    with pytest.raises(NotImplementedError, match="symmetric"):
        lqr_steady_state(F, f, C, c, dtype=torch.float64)
    assert LQR(F, f, C, c, device="cpu").symmetric_cost           # the fp32 default takes it


class _Recorder:
    """Stands in for the library: keeps the launch's arguments and a copy of the F it points to, returns TFMPC_OK."""

    def __init__(self):
        self.calls, self.F = [], []

    def tfmpc_lqr_steady_state_f64(self, *args):
        B, n, m, F, stride = args[:5]
        count = (B * stride if stride else n * (n + m))
        self.F.append(np.ctypeslib.as_array(ctypes.cast(F, ctypes.POINTER(ctypes.c_double)), shape=(count,)).copy())
        self.calls.append(args)
        return 0


def test_shapes_and_dtypes_up_to_the_launch(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_hip, "require_gpu", lambda: lib)
    monkeypatch.setattr(_hip, "stream", lambda: None)
    monkeypatch.setattr(_hip, "default_device", lambda: torch.device("cpu"))
    n, m, B = 3, 2, 2
    F, f, C, c = _operands(n, m, B)
    batched = lqr_steady_state(F, torch.as_tensor(f), C, c, dtype=torch.float64)
    for name, shape in (("K", (B, m, n)), ("k", (B, m, 1)), ("P", (B, n, n)), ("p", (B, n, 1))):
        t = getattr(batched, name)
        assert tuple(t.shape) == shape and t.dtype == torch.float64, name
    assert tuple(batched.status.shape) == (B,) and batched.status.dtype == torch.int32
    assert batched.iterations.dtype == torch.int32
    args = lib.calls[-1]
    assert args[:3] == (B, n, m) and args[4] == n * (n + m) and args[6] == n and args[11:13] == (0, 0.0)
    # the operands reach the launch in double: F's bits, which fp32 cannot hold
    assert np.array_equal(lib.F[-1], F.reshape(-1)) and not np.array_equal(F.astype(np.float32).astype(np.float64), F)

    one = lqr_steady_state(F[0], f[0], C[0], c[0], max_iter=7, tol=1e-9, dtype=torch.float64)
    assert tuple(one.K.shape) == (m, n) and tuple(one.k.shape) == (m, 1) and tuple(one.P.shape) == (n, n)
    assert tuple(one.p.shape) == (n, 1) and one.status.dim() == 0 and one.K.dtype == torch.float64
    assert lib.calls[-1][0] == 1 and lib.calls[-1][11:13] == (7, 1e-9) and lib.calls[-1][4] == 0

    lqr = LQR(F, f, C, c, device="cpu")
    ss = lqr.steady_state(dtype=torch.float64)
    assert ss.K.dtype == torch.float64 and tuple(ss.K.shape) == (B, m, n) and lqr.last_status is ss.status
    assert np.array_equal(lib.F[-1], F.astype(np.float32).astype(np.float64).reshape(-1))      # the fp32 operands the LQR stores, upcast
    assert tuple(ss.policy(4).K.shape) == (B, 4, m, n)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_f64_kernels_use_no_scratch_and_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "lqr_steady_state_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 2 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    for name, private, vgprs, spills in found:
        assert "lqr_steady_state_f64_kernel" in name
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    assert "v_mfma_f64_16x16x4" in text

"""Infinite-horizon LQR without a GPU: the numpy restatement of tests/lqr_steady_state_ref.py pinned against scipy's
discrete Riccati solver and against the finite recursion of oracle/lqr_ref.py, the C ABI's declarations, bindings and
argument errors, the Python front end's validation, and the new kernels' register budget."""
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

import lqr_steady_state_ref as ssref
from oracle import lqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402
from tfmpc.solvers.lqr import LQR, Policy, SteadyState  # noqa: E402

EXPORTS = ("tfmpc_lqr_steady_state_kernel_name", "tfmpc_lqr_steady_state_f32")


def _workload(kind, n, m, B, seed=0):
    if kind == "make_lqr":
        return ssref.make_lqr_batch(n, m, B, seed=seed)
    return ssref.damped_workload(n, m, B, seed=seed)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


CASES = [("make_lqr", 16, 8), ("make_lqr", 5, 3), ("make_lqr", 32, 16), ("damped", 16, 8)]


@pytest.mark.parametrize("kind,n,m", CASES)
def test_restatement_is_scipy_solve_discrete_are(kind, n, m):
    F, f, C, c = _workload(kind, n, m, 3, seed=n + m)
    for b in range(3):
        F64, C64 = F[b].astype(np.float64), C[b].astype(np.float64)
        A, Bm = F64[:, :n], F64[:, n:]
        Q, S, R = C64[:n, :n], C64[:n, n:], C64[n:, n:]
        P = scipy.linalg.solve_discrete_are(A, Bm, Q, R, s=S)
        K = -np.linalg.solve(R + Bm.T @ P @ Bm, Bm.T @ P @ A + S.T)
        got = ssref.steady_state(F[b], f[b], C[b], c[b])
        assert got["status"] == 0
        assert _rel(got["P"], P) <= 1e-10, _rel(got["P"], P)
        assert _rel(got["K"], K) <= 1e-10, _rel(got["K"], K)
        assert np.abs(np.linalg.eigvals(A + Bm @ got["K"])).max() < 1.0


@pytest.mark.parametrize("kind,n,m", CASES)
def test_restatement_is_the_limit_of_the_finite_recursion(kind, n, m):
    """K, k, P, p are backward(T)'s K_0, k_0, V_0, v_0 at a horizon long enough to converge (the affine terms converge at
    the closed loop's rate: the damped workload needs thousands of steps)."""
    F, f, C, c = _workload(kind, n, m, 1, seed=n * m)
    T = 10000 if kind == "damped" else 200
    policy, value_fn = lqr_ref.backward(F[0], f[0][:, None], C[0], c[0][:, None], T)
    got = ssref.steady_state(F[0], f[0], C[0], c[0])
    assert got["status"] == 0
    for name, ref in (("K", policy[0][0]), ("k", policy[0][1][:, 0]), ("P", value_fn[0][0]), ("p", value_fn[0][1][:, 0])):
        assert _rel(got[name], ref) <= 1e-9, (name, _rel(got[name], ref))


def test_damped_workload_converges_in_few_doublings_where_the_recursion_needs_thousands():
    F, f, C, c = ssref.damped_workload(16, 8, 4, seed=1)
    for b in range(4):
        r64 = ssref.steady_state(F[b], f[b], C[b], c[b])
        r32 = ssref.steady_state(F[b], f[b], C[b], c[b], dtype=np.float32)
        assert r64["status"] == 0 and r32["status"] == 0
        assert r32["iterations"] <= 16
        rho = np.abs(np.linalg.eigvals(F[b][:, :16].astype(np.float64) + F[b][:, 16:] @ r64["K"])).max()
        assert 0.98 < rho < 1.0


def unstabilisable(F, C):
    """Mode 0 of the plant made unstable (1.5) and unreachable: no input, no coupling to the other states."""
    F, C = F.copy(), C.copy()
    F[0, :] = 0.0
    F[:, 0] = 0.0
    F[0, 0] = 1.5
    C[0, 1:] = 0.0
    C[1:, 0] = 0.0
    return F, C


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_unstabilisable_system_is_reported(dtype):
    F, f, C, c = ssref.make_lqr_batch(5, 3, 1, seed=3)
    F0, C0 = unstabilisable(F[0], C[0])
    got = ssref.steady_state(F0, f[0], C0, c[0], dtype=dtype)
    assert got["status"] == ssref.ST_NOT_STABILISING
    assert all(np.isnan(got[name]).all() for name in ("K", "k", "P", "p"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_k_going_to_zero_is_not_enough(dtype):
    """The same unreachable unstable mode, coupled to the rest through A and the cost: H_k grows to a huge finite
    value whose (I + GH)^-1 drives A_k to zero.  The instance is still flagged (by R + B'PB or the closed-loop
    certificate), never reported as solved."""
    F, f, C, c = ssref.make_lqr_batch(5, 3, 1, seed=3)
    F0 = F[0].copy()
    F0[0, :] = 0.0
    F0[0, 0] = 1.5
    got = ssref.steady_state(F0, f[0], C[0], c[0], dtype=dtype)
    assert got["status"] != 0
    assert all(np.isnan(got[name]).all() for name in ("K", "k", "P", "p"))


def test_r_not_positive_definite_is_reported():
    F, f, C, c = ssref.make_lqr_batch(5, 3, 1, seed=4)
    C = C[0].copy()
    C[5:, 5:] = -np.eye(3)
    got = ssref.steady_state(F[0], f[0], C, c[0], dtype=np.float32)
    assert got["status"] == ssref.ST_NOT_PD and got["iterations"] == 0


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define TFMPC_ST_NOT_STABILISING 0x80\b", header)
    assert _hip.ST_NOT_STABILISING == 0x80 == ssref.ST_NOT_STABILISING
    assert lib.tfmpc_version() == 320
    assert len(_hip._SIGNATURES["tfmpc_lqr_steady_state_f32"][1]) == 3 + 8 + 2 + 4 + 3


def test_kernel_names_per_shape():
    name = lambda n, m: _hip.load().tfmpc_lqr_steady_state_kernel_name(n, m).decode()   # noqa: E731
    assert name(16, 8) == name(16, 16) == name(16, 1) == "ss_mfma_16"
    assert name(5, 3) == name(12, 6) == name(1, 16) == "ss_mfma_16 (padded)"
    assert name(20, 10) == name(32, 16) == name(16, 17) == name(32, 32) == "ss_wave_32"
    assert name(33, 1) == name(8, 33) == "unsupported"
    assert name(0, 3) == name(3, 0) == "invalid"


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4))
    st = p

    def call(B=1, n=3, m=2, F=p, f=p, C=p, c=p, s=0, max_iter=0, tol=0.0, status=st):
        return lib.tfmpc_lqr_steady_state_f32(B, n, m, F, s, f, s, C, s, c, s, max_iter, tol, p, p, p, p, None, status, None)

    assert call(B=-1) == -1
    assert call(n=0) == -1 and call(m=0) == -1
    assert call(max_iter=-1) == -1
    assert call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(C=None) == -1 and call(c=None) == -1
    assert call(status=None) == -1
    assert call(s=-3) == -1
    assert call(n=33) == -2 and call(m=33) == -2 and call(B=0, n=40, m=40) == -2
    assert call(B=0, F=None, f=None, C=None, c=None, status=None) == 0          # B == 0: a no-op, nothing is read


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_steady_state_kernels_use_no_scratch():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "lqr_steady_state.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*lqr_steady_state_kernel\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 2 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    assert "v_mfma_f32_16x16x4" in text and "v_mfma_f64" not in text      # every product on the f32 matrix cores
    assert not re.search(r"\b(scratch_|buffer_atomic|global_atomic|flat_atomic|ds_add|ds_max|ds_min)\w*", text)


def _lqr(n=3, m=2, B=2, **kw):
    F, f, C, c = ssref.make_lqr_batch(n, m, B, seed=5)
    return LQR(F, f, C, c, device="cpu", **kw)


@pytest.mark.parametrize("bad,exc", [("asym", NotImplementedError), ("grad", NotImplementedError), ("max_iter0", ValueError),
                                     ("max_iter_frac", ValueError), ("tol_neg", ValueError), ("tol_nan", ValueError),
                                     ("too_large", ValueError)])
def test_python_validation_errors_are_raised_without_a_device(bad, exc):
    kw = {}
    if bad == "asym":
        F, f, C, c = ssref.make_lqr_batch(3, 2, 2, seed=5)
        C = C.copy()
        C[1, 0, 4] += 1.0
        lqr = LQR(F, f, C, c, device="cpu")
    elif bad == "grad":
        F, f, C, c = (torch.as_tensor(a) for a in ssref.make_lqr_batch(3, 2, 2, seed=5))
        lqr = LQR(F.requires_grad_(), f, C, c, device="cpu")
    elif bad == "too_large":
        lqr = _lqr(33, 2, 1)
    else:
        lqr = _lqr()
        kw = {"max_iter0": dict(max_iter=0), "max_iter_frac": dict(max_iter=2.5), "tol_neg": dict(tol=-1e-6),
              "tol_nan": dict(tol=float("nan"))}[bad]
    with pytest.raises(exc):
        lqr.steady_state(**kw)


def test_steady_state_policy_is_an_expanded_view():
    B, n, m, T = 3, 4, 2, 7
    K, k = torch.randn(B, m, n), torch.randn(B, m, 1)
    ss = SteadyState(K, k, torch.eye(n).expand(B, n, n), torch.zeros(B, n, 1), torch.zeros(B, dtype=torch.int32),
                     torch.zeros(B, dtype=torch.int32))
    pol = ss.policy(T)
    assert isinstance(pol, Policy) and len(pol) == T
    assert tuple(pol.K.shape) == (B, T, m, n) and tuple(pol.k.shape) == (B, T, m, 1)
    assert pol.K.stride(1) == 0 and pol.K.data_ptr() == K.data_ptr()
    assert torch.equal(pol[T - 1][0], K)
    one = SteadyState(K[0], k[0], None, None, None, None).policy(T)
    assert tuple(one.K.shape) == (T, m, n) and one.K.stride(0) == 0


def test_from_lqr_takes_an_explicit_final_cost():
    lqr = _lqr(3, 2, 2)
    P = np.stack([np.eye(3, dtype=np.float32)] * 2)
    p = np.ones((2, 3), np.float32)
    tv = TimeVaryingLQR.from_lqr(lqr, 5, P, p)
    assert tv.C_final is not None and tuple(tv.c_final.shape) == (2, 3, 1)
    assert TimeVaryingLQR.from_lqr(lqr, 5).C_final is None
    P[1, 0, 2] = 0.5
    with pytest.raises(ValueError):
        TimeVaryingLQR.from_lqr(lqr, 5, P, p)
    with pytest.raises(ValueError):
        TimeVaryingLQR.from_lqr(lqr, 5, P)
    nan = np.full((2, 3, 3), np.nan, np.float32)          # a flagged steady state: symmetric NaN rows pass through
    assert TimeVaryingLQR.from_lqr(lqr, 5, nan, p).C_final is not None

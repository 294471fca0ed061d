"""Gradients of the infinite-horizon LQR without a GPU: the fp64 closed form of tests/lqr_steady_state_grad_ref.py
pinned against central differences of the fp64 steady state and against torch autograd through the finite recursion,
the C ABI's declarations, bindings and argument errors, the Python front end's routing and validation, and the new
kernels' register budget."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import lqr_steady_state_grad_ref as gref
import lqr_steady_state_ref as ssref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip, solvers  # noqa: E402
from tfmpc.solvers import lqr_steady_state  # noqa: E402
from tfmpc.solvers.lqr import LQR, SteadyState  # noqa: E402

EXPORTS = ("tfmpc_lqr_steady_state_vjp_workspace_bytes", "tfmpc_lqr_steady_state_vjp_kernel_name",
           "tfmpc_lqr_steady_state_vjp_f32")
GRADS = ("dF", "df", "dC", "dc")


def _upstream(n, m, seed=0):
    rng = np.random.default_rng(seed)
    return dict(gK=rng.normal(size=(m, n)), gk=rng.normal(size=m), gP=rng.normal(size=(n, n)), gp=rng.normal(size=n))


@pytest.mark.parametrize("kind,n,m", [("make_lqr", 5, 3), ("make_lqr", 3, 5), ("make_lqr", 2, 1), ("damped", 4, 2)])
def test_closed_form_is_central_differences(kind, n, m):
    """S != 0 (make_spd_matrix C), f != 0, m > n included."""
    F, f, C, c = (ssref.make_lqr_batch if kind == "make_lqr" else ssref.damped_workload)(n, m, 1, seed=n + 2 * m)
    F, f, C, c = (a[0].astype(np.float64) for a in (F, f, C, c))
    if kind == "make_lqr":
        assert np.abs(C[:n, n:]).max() > 0.01
    up = _upstream(n, m, seed=n * m)
    got = gref.vjp(F, f, C, c, **up)
    assert got["status"] == 0
    fd = gref.steady_state_grad_fd(F, f, C, c, *up.values())
    for name in GRADS:
        scale = max(1.0, float(np.abs(fd[name]).max()))
        assert np.abs(got[name] - fd[name]).max() <= 1e-6 * scale, (name, np.abs(got[name] - fd[name]).max(), scale)


def _finite_recursion(F, f, C, c, T):
    """backward(T)'s K_0, k_0, V_0, v_0 in torch (oracle/lqr_ref.py's recursion, default final cost)."""
    n = F.shape[0]
    V, v = C[:n, :n], c[:n]
    for _ in range(T):
        FV = F.T @ V
        Q = C + FV @ F
        q = c + FV @ f + F.T @ v
        K = -torch.linalg.solve(Q[n:, n:], Q[n:, :n])
        k = -torch.linalg.solve(Q[n:, n:], q[n:])
        V = Q[:n, :n] + Q[:n, n:] @ K
        V = 0.5 * (V + V.T)
        v = q[:n] + Q[:n, n:] @ k
    return K, k, V, v


@pytest.mark.parametrize("kind,n,m,T", [("make_lqr", 5, 3, 300), ("damped", 6, 3, 12000)])
def test_closed_form_is_autograd_through_the_finite_recursion(kind, n, m, T):
    """The gradients of backward(T)'s first-step outputs converge to the steady state's as T grows: the damped
    workload (closed-loop radius ~0.998) needs a horizon in the thousands."""
    F, f, C, c = (ssref.make_lqr_batch if kind == "make_lqr" else ssref.damped_workload)(n, m, 1, seed=2)
    ops = [torch.tensor(a[0], dtype=torch.float64, requires_grad=True) for a in (F, f, C, c)]
    up = _upstream(n, m, seed=1)
    outs = _finite_recursion(*ops, T)
    loss = sum((torch.as_tensor(g) * o).sum() for g, o in zip(up.values(), outs))
    grads = [g.numpy() for g in torch.autograd.grad(loss, ops)]
    grads[2] = 0.5 * (grads[2] + grads[2].T)
    got = gref.vjp(F[0], f[0], C[0], c[0], **up)
    for name, g in zip(GRADS, grads):
        assert np.abs(got[name] - g).max() <= 1e-6 * max(1.0, np.abs(g).max()), (name, np.abs(got[name] - g).max())


def test_fp32_restatement_is_close_and_flags_like_the_forward():
    F, f, C, c = ssref.make_lqr_batch(5, 3, 1, seed=3)
    up = _upstream(5, 3)
    g64 = gref.vjp(F[0], f[0], C[0], c[0], **up)
    g32 = gref.vjp(F[0], f[0], C[0], c[0], **up, dtype=np.float32)
    for name in GRADS:
        assert g32[name].dtype == np.float32
        assert np.abs(g32[name] - g64[name]).max() <= 1e-3 * max(1.0, np.abs(g64[name]).max()), name
    Cb = C[0].copy()
    Cb[5:, 5:] = -np.eye(3)
    bad = gref.vjp(F[0], f[0], Cb, c[0], **up, dtype=np.float32)
    assert bad["status"] == ssref.ST_NOT_PD and all(np.isnan(bad[name]).all() for name in GRADS)
    # a Smith doubling capped before it converges
    Fd, fd, Cd, cd = ssref.damped_workload(16, 8, 1, seed=1)
    capped = gref.vjp(Fd[0], fd[0], Cd[0], cd[0], **_upstream(16, 8), max_iter=3)
    assert capped["status"] == ssref.ST_NOT_STABILISING and np.isnan(capped["dF"]).all()


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320
    assert len(_hip._SIGNATURES["tfmpc_lqr_steady_state_vjp_f32"][1]) == 3 + 8 + 5 + 4 + 2 + 8 + 4
    assert solvers.lqr_steady_state is lqr_steady_state
    assert "lqr_steady_state" in vars(solvers)


def test_kernel_names_per_shape():
    name = lambda n, m: _hip.load().tfmpc_lqr_steady_state_vjp_kernel_name(n, m).decode()   # noqa: E731
    assert name(16, 8) == name(16, 16) == name(16, 1) == "ss_vjp_mfma_16"
    assert name(5, 3) == name(12, 6) == name(1, 1) == name(3, 5) == "ss_vjp_mfma_16 (padded)"
    assert name(20, 10) == name(32, 16) == name(16, 17) == name(32, 32) == "ss_vjp_wave_32"
    assert name(33, 1) == name(8, 33) == "unsupported"
    assert name(0, 3) == name(3, 0) == "invalid"


def test_workspace_bytes():
    ws = _hip.load().tfmpc_lqr_steady_state_vjp_workspace_bytes
    n, m = 16, 8
    d = n + m
    per = n * d + n + d * d + d
    assert ws(65536, n, m) >= 65536 * per * 4
    assert ws(1, n, m) == 0 and ws(0, n, m) == 0          # nothing is summed over a batch of one
    assert ws(4, 33, 1) == 0 and ws(4, 0, 1) == 0


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4))

    def call(B=1, n=3, m=2, F=p, f=p, C=p, c=p, s=0, K=p, k=p, P=p, pv=p, fst=p, max_iter=0, tol=0.0, ds=1, status=p,
             dF=p, ws=None, ws_bytes=0):
        return lib.tfmpc_lqr_steady_state_vjp_f32(B, n, m, F, s, f, s, C, s, c, s, K, k, P, pv, fst, None, None, None, None,
                                                  max_iter, tol, dF, ds, p, ds, p, ds, p, ds, status, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(n=0) == -1 and call(m=0) == -1
    assert call(max_iter=-1) == -1
    assert call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(C=None) == -1 and call(c=None) == -1
    assert call(K=None) == -1 and call(k=None) == -1 and call(P=None) == -1 and call(pv=None) == -1
    assert call(fst=None) == -1 and call(status=None) == -1
    assert call(s=-3) == -1 and call(ds=-3) == -1
    assert call(n=33) == -2 and call(m=33) == -2 and call(B=0, n=40, m=40) == -2
    assert call(B=4, ds=0) == -4                                    # a summed output needs the workspace
    assert call(B=4, ds=0, ws=p, ws_bytes=16) == -4
    assert call(B=0, F=None, f=None, C=None, c=None, K=None, k=None, P=None, pv=None, fst=None, status=None) == 0


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_steady_state_vjp_kernels_use_no_scratch():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "lqr_steady_state_vjp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*(?:ss_vjp_|batch_sum_)\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len([f for f in found if "ss_vjp_kernel" in f[0]]) == 2, found
    assert len(found) == 4, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    assert not re.search(r"\b(scratch_|buffer_atomic|global_atomic|flat_atomic|ds_add|ds_max|ds_min)\w*", text)


def _ops(n=3, m=2, B=2, grad=(), seed=5):
    F, f, C, c = ssref.make_lqr_batch(n, m, B, seed=seed)
    return [torch.as_tensor(a).requires_grad_() if name in grad else a for name, a in zip("FfCc", (F, f, C, c))]


def _fake_launch(lqr, max_iter, tol):
    """A stand-in for the kernel launch on a machine without a GPU: batched outputs of the right shapes."""
    n, m = lqr.state_size, lqr.action_size
    Bk = lqr.batch_size or 1
    i32 = lambda: torch.zeros((Bk,), dtype=torch.int32)        # noqa: E731
    return (torch.zeros(Bk, m, n), torch.zeros(Bk, m, 1), torch.zeros(Bk, n, n), torch.zeros(Bk, n, 1), i32(), i32())


def test_default_call_still_refuses_grad_operands_and_names_the_opt_in():
    lqr = LQR(*_ops(grad="F"), device="cpu")
    with pytest.raises(NotImplementedError, match="differentiable=True"):
        lqr.steady_state()


def test_differentiable_with_an_asymmetric_cost_raises():
    F, f, C, c = ssref.make_lqr_batch(3, 2, 2, seed=5)
    C = C.copy()
    C[1, 0, 4] += 1.0
    lqr = LQR(torch.as_tensor(F).requires_grad_(), f, C, c, device="cpu")
    with pytest.raises(NotImplementedError):
        lqr.steady_state(differentiable=True)
    with pytest.raises(NotImplementedError):
        lqr_steady_state(torch.as_tensor(F).requires_grad_(), f, C, c)


@pytest.mark.parametrize("kw", [dict(max_iter=0), dict(max_iter=2.5), dict(tol=-1e-6), dict(tol=float("nan"))])
def test_differentiable_validation_errors(kw):
    with pytest.raises(ValueError):
        lqr_steady_state(*_ops(grad="F"), **kw)


def test_routing(monkeypatch):
    """numpy operands (or no operand requiring grad) take the plain launch and give no grad; an operand that requires
    grad takes the autograd Function, whose outputs are in the graph and whose status / iterations are not."""
    calls = []

    def fake(self, max_iter, tol):
        calls.append((max_iter, tol))
        return _fake_launch(self, max_iter, tol)

    monkeypatch.setattr(LQR, "_steady_state_launch", fake)
    ss = lqr_steady_state(*_ops(), max_iter=7, tol=1e-4)
    assert isinstance(ss, SteadyState) and calls == [(7, 1e-4)]
    assert not any(getattr(ss, name).requires_grad for name in ("K", "k", "P", "p"))
    ss = LQR(*_ops(grad="C"), device="cpu").steady_state(differentiable=True)
    assert all(getattr(ss, name).requires_grad for name in ("K", "k", "P", "p"))
    assert not ss.status.requires_grad and not ss.iterations.requires_grad
    assert calls[-1] == (0, 0.0)
    with torch.no_grad():
        ss = LQR(*_ops(grad="C"), device="cpu").steady_state(differentiable=True)
    assert not ss.K.requires_grad
    one = LQR(*(a[0] for a in _ops(B=1, grad="F")), device="cpu").steady_state(differentiable=True)
    assert tuple(one.K.shape) == (2, 3) and tuple(one.p.shape) == (3, 1) and one.status.dim() == 0 and one.K.requires_grad

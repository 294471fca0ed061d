"""Double-precision time-varying LQR without a GPU: the longdouble restatement pinned against the fp64 oracle, the
budget rule shown attainable by the kernel's formulation on the host, the C ABI's declarations, bindings and argument
errors, the Python class's dtype handling, and the kernels' register budget."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import tvlqr_f64_ref as ref64
import tvlqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402

F64_EXPORTS = ("tfmpc_tvlqr_workspace_bytes_f64", "tfmpc_tvlqr_kernel_name_f64", "tfmpc_tvlqr_backward_f64",
               "tfmpc_tvlqr_forward_f64", "tfmpc_tvlqr_solve_f64")


def _problem(n, m, T, count, seed, unscaled=False):
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = make(n, m, T, count, seed=seed)
    return F, f, C, c, tvlqr_ref.make_x0(n, count, seed=seed)


def test_longdouble_is_the_80_bit_format():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("n,m,T", [(3, 2, 50), (16, 8, 50)])
def test_longdouble_restatement_agrees_with_the_fp64_oracle(n, m, T):
    F, f, C, c, x0 = _problem(n, m, T, 2, seed=5)
    for b in range(2):
        ld = ref64.solve_ld(F[b], f[b], C[b], c[b], x0[b])
        r64 = tvlqr_ref.solve(F[b], f[b], C[b], c[b], x0[b], dtype=np.float64)
        for name in ref64.FIELDS:
            assert ld[name].dtype == np.longdouble and ld[name].shape == r64[name].shape, name
            assert ref64.error(r64[name], ld[name]) <= 1e-9 * max(1.0, float(np.abs(ld[name]).max())), name


def test_longdouble_inverse():
    A = np.random.default_rng(0).normal(size=(7, 7))
    A[0, 0] = 0.0                                            # forces a row exchange
    got = ref64.inv_ld(A)
    assert float(np.abs(got @ A.astype(np.longdouble) - np.eye(7)).max()) <= 1e-15


@pytest.mark.parametrize("n,m,T,unscaled", [(3, 2, 50, False), (12, 5, 53, False), (16, 8, 50, False), (16, 16, 53, False),
                                            (32, 16, 20, False), (16, 8, 50, True)])
def test_the_budget_is_attainable_by_the_kernels_formulation(n, m, T, unscaled):
    B = 6
    F, f, C, c, x0 = _problem(n, m, T, B, seed=n * 100 + m, unscaled=unscaled)
    rld, r64 = ref64.references(F, f, C, c, x0)
    got = [ref64.solve_schur(F[b], f[b], C[b], c[b], x0[b]) for b in range(B)]
    got = {name: [g[name] for g in got] for name in ref64.FIELDS}
    ref64.check(got, rld, r64, what=(n, m, T, "unscaled" if unscaled else "scaled"))


def test_every_f64_export_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in F64_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    for call in ("backward", "forward", "solve"):
        f64, f32 = _hip._SIGNATURES[f"tfmpc_tvlqr_{call}_f64"], _hip._SIGNATURES[f"tfmpc_tvlqr_{call}_f32"]
        assert len(f64[1]) == len(f32[1]) and f64[0] is f32[0], call
    assert lib.tfmpc_version() == 320 and _hip.MIN_VERSION == 320


def test_f64_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    dummy = torch.zeros(4, dtype=torch.float64)
    p = _hip.ptr(dummy)
    model = lambda B, n, m, T, s=0: (B, n, m, T, *([p, s, s] * 4), None, 0, None, 0)     # noqa: E731
    bw = lambda *mdl: lib.tfmpc_tvlqr_backward_f64(*mdl, p, p, None, None, None, None, None)   # noqa: E731
    assert bw(*model(1, 3, 2, 0)) == -1                       # T >= 1
    assert bw(*model(1, 0, 2, 4)) == -1
    assert bw(*model(-1, 3, 2, 4)) == -1
    assert bw(*model(1, 3, 2, 4, s=-5)) == -1                 # negative stride
    args = list(model(1, 3, 2, 4))
    args[4] = None                                            # F NULL
    assert bw(*args) == -1
    args = list(model(1, 3, 2, 4))
    args[16] = p                                              # Cfin without cfin
    assert bw(*args) == -1
    assert bw(*model(1, 33, 2, 4)) == -2                      # n beyond the kernel
    assert bw(*model(1, 2, 33, 4)) == -2                      # m beyond the kernel
    assert lib.tfmpc_tvlqr_backward_f64(*model(1, 3, 2, 4), None, p, None, None, None, None, None) == -1   # K NULL
    assert bw(*model(0, 3, 2, 4)) == 0                        # B == 0: no-op
    assert bw(*model(0, 33, 2, 4)) == -2                      # ... after the shape check, as the fp32 call
    fw = lambda *mdl, sK=0: lib.tfmpc_tvlqr_forward_f64(*mdl, p, sK, p, 0, None, p, p, p, None)   # noqa: E731
    assert fw(*model(1, 3, 2, 4)) == -1                       # x0 NULL
    assert lib.tfmpc_tvlqr_forward_f64(*model(1, 3, 2, 4), p, -1, p, 0, p, p, p, p, None) == -1
    # the fused solve without gain outputs needs the workspace
    solve = lambda ws, nbytes: lib.tfmpc_tvlqr_solve_f64(*model(2, 3, 2, 4), p, p, p, p, None, None, None, None, None, None,   # noqa: E731
                                                          ws, nbytes, None)
    need = lib.tfmpc_tvlqr_workspace_bytes_f64(2, 3, 2, 4)
    assert need == 2 * 4 * 2 * 4 * 8
    assert solve(None, 0) == -4 and solve(p, need - 1) == -4
    assert lib.tfmpc_tvlqr_solve_f64(*model(2, 3, 2, 4), None, p, p, p, None, None, None, None, None, None, p, need, None) == -1
    assert lib.tfmpc_tvlqr_workspace_bytes_f64(2, 16, 8, 50) == 2 * 50 * 8 * 17 * 8
    assert lib.tfmpc_tvlqr_workspace_bytes_f64(0, 16, 8, 50) == 0
    name = lambda n, m: lib.tfmpc_tvlqr_kernel_name_f64(n, m, 50).decode()      # noqa: E731
    assert name(16, 16) == "tv_f64_wave16" and name(1, 1) == "tv_f64_wave16"
    assert name(17, 8) == "tv_f64_wave32" and name(16, 17) == "tv_f64_wave32" and name(32, 32) == "tv_f64_wave32"
    assert name(33, 1) == "unsupported" and name(1, 33) == "unsupported"
    assert name(0, 1) == "invalid"


def _model64(B, T, n, m):
    F, f, C, c = (a.astype(np.float64) for a in tvlqr_ref.make_models(n, m, T, max(B, 1), seed=3))
    rng = np.random.default_rng(8)
    F = F + 1e-9 * rng.normal(size=F.shape)                  # not representable in fp32
    if not B:
        F, f, C, c = F[0], f[0], C[0], c[0]
    return F, f, C, c


def test_dtype_and_shapes_are_kept_without_a_device():
    F, f, C, c = _model64(3, 4, 3, 2)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu", dtype=torch.float64)
    assert (tv.state_size, tv.action_size, tv.horizon, tv.batch_size, tv.dtype) == (3, 2, 4, 3, torch.float64)
    for t, a in ((tv.F, F), (tv.f, f[..., None]), (tv.C, C), (tv.c, c[..., None])):
        assert t.dtype == torch.float64 and tuple(t.shape) == a.shape
        assert np.array_equal(t.numpy(), a)                  # no trip through fp32
    Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(3, 3))
    tv = TimeVaryingLQR(torch.as_tensor(F), f, C, torch.as_tensor(c, dtype=torch.float32), Cf, cf, device="cpu", dtype=torch.float64)
    assert tv.C_final.dtype == torch.float64 and tv.c_final.dtype == torch.float64 and tv.c.dtype == torch.float64
    x, u = np.ones((3, 3, 1)), np.zeros((3, 2, 1))
    for out in (tv.transition(x, u, 1), tv.cost(x, u, 1), tv.final_cost(x)):
        assert out.dtype == torch.float64
    np.testing.assert_allclose(tv.transition(x, u, 1).numpy(), F[:, 1, :, :3] @ x + f[:, 1, :, None], rtol=1e-14)
    assert tv._prep_x0(np.ones(3, np.float32)).dtype == torch.float64
    # the symmetry check is the double one: an asymmetry of 1e-9 relative passes in fp32 and is refused in double
    C_bad = C.copy()
    C_bad[1, 2, 0, 1] += 1e-9 * np.abs(C).max()
    TimeVaryingLQR(F, f, C_bad, c, device="cpu")
    with pytest.raises(ValueError):
        TimeVaryingLQR(F, f, C_bad, c, device="cpu", dtype=torch.float64)


def test_the_default_dtype_still_stores_fp32_for_fp64_inputs():
    F, f, C, c = _model64(2, 4, 3, 2)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu")
    assert tv.dtype == torch.float32
    for t, a in ((tv.F, F), (tv.f, f[..., None]), (tv.C, C), (tv.c, c[..., None])):
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), a.astype(np.float32))
    assert tv._prep_x0(np.ones(3)).dtype == torch.float32


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.int64, np.float64, "float64", None])
def test_a_dtype_that_is_not_served_is_refused(dtype):
    F, f, C, c = _model64(0, 4, 3, 2)
    with pytest.raises(ValueError, match="dtype"):
        TimeVaryingLQR(F, f, C, c, device="cpu", dtype=dtype)
    with pytest.raises(ValueError, match="dtype"):
        TimeVaryingLQR.time_invariant(F[0], f[0], C[0], c[0], 5, device="cpu", dtype=dtype)


@pytest.mark.parametrize("batched", [False, True])
def test_time_invariant_is_a_stride_zero_view(batched):
    F, f, C, c = (a[:, 0] if batched else a[0, 0] for a in _model64(2, 1, 3, 2))
    Ft = torch.as_tensor(F)
    tv = TimeVaryingLQR.time_invariant(Ft, f, C, c[..., None], 6, device="cpu", dtype=torch.float64)
    assert (tv.horizon, tv.batch_size, tv.dtype) == (6, 2 if batched else None, torch.float64)
    assert tv.F.data_ptr() == Ft.data_ptr() and tv.F.stride(-3) == 0          # the caller's own storage: no copy
    assert tuple(tv.F.shape) == ((2, 6, 3, 5) if batched else (6, 3, 5)) and tuple(tv.f.shape)[-3:] == (6, 3, 1)
    args = tv._model_args()
    assert [args[i] for i in (2, 5, 8, 11)] == [0, 0, 0, 0]                   # every time stride
    assert args[1] == (15 if batched else 0) and args[7] == (25 if batched else 0)
    # an explicit final cost, and the fp32 default
    Cf, cf = (a[0] for a in tvlqr_ref.make_final(3, 1))
    tv = TimeVaryingLQR.time_invariant(F, f, C, c, 4, Cf, cf, device="cpu")
    assert tv.dtype == torch.float32 and tv.F.dtype == torch.float32 and tv.F.stride(-3) == 0 and tv.C_final is not None
    with pytest.raises(ValueError):
        TimeVaryingLQR.time_invariant(F, f, C, c, 0, device="cpu")


def test_from_lqr_upcasts_the_stored_fp32_operands():
    from tfmpc.solvers.lqr import LQR
    F, f, C, c = (a[0, 0] for a in _model64(1, 1, 3, 2))
    lqr = LQR(F, f, C, c, device="cpu")
    tv = TimeVaryingLQR.from_lqr(lqr, 6, dtype=torch.float64)
    assert tv.dtype == torch.float64 and tv.F.stride(-3) == 0 and tv.horizon == 6
    assert np.array_equal(tv.F[0].numpy(), F.astype(np.float32).astype(np.float64))      # rounded to fp32 before
    assert TimeVaryingLQR.from_lqr(lqr, 6).dtype == torch.float32


@pytest.mark.parametrize("call,which", [("solve", "operand"), ("solve", "x0"), ("solve_tensors", "operand"),
                                        ("solve_tensors", "x0"), ("backward", "operand")])
def test_gradients_are_refused_in_double_before_any_launch(call, which):
    F, f, C, c = _model64(2, 4, 3, 2)
    Ft = torch.as_tensor(F).requires_grad_(which == "operand")
    x0 = torch.ones(2, 3, 1, dtype=torch.float64).requires_grad_(which == "x0")
    tv = TimeVaryingLQR(Ft, f, C, c, device="cpu", dtype=torch.float64)
    if call == "backward":
        with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32"):
            tv.backward(differentiable=True)
    else:
        with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32"):
            getattr(tv, call)(x0)
    with torch.no_grad():                                     # nothing records: the refusal does not apply, the missing GPU does
        with pytest.raises(RuntimeError, match="GPU"):
            tv.solve(x0)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_f64_kernels_use_no_scratch_and_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*tvlqr_f64_kernel\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 6, found                             # {wave16, wave32} x {backward, forward, solve}
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        body = re.search(r"\n" + re.escape(name) + r":.*?\n(.*?)\n\s*\.amdhsa_kernel\s+" + re.escape(name), text, flags=re.S)
        assert body, name
        # every kernel that holds a matrix product, i.e. a backward sweep (<MAXD, true, *>); the rollout-only kernels
        # are matrix-vector work, which stays on the vector unit
        assert ("v_mfma_f64_16x16x4_f64" in body.group(1)) == ("Lb1ELb" in name), name

"""Double-precision gradients of the finite-horizon Riccati recursion without a GPU: the restatements of
tests/tvlqr_backward_grad_f64_ref.py pinned against autograd and central differences, the horizon table, the budget's
attainability on the GPU test's inputs, the C ABI's declarations, bindings and argument errors, the workspace plan, the
Python front end up to the launch, and the kernels' resources.

The restatement, horizon and attainability tests pin the YARDSTICK of tests/test_tvlqr_backward_grad_f64_gpu.py: they run
numpy only.  The tests from test_every_new_export_is_declared_bound_and_exported on test the FEATURE."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import batch_sum_ref
import tvlqr_backward_grad_f64_ref as g64
import tvlqr_backward_grad_ref as gref
import tvlqr_f64_ref as ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip, solvers  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR, tvlqr_backward, tvlqr_backward_vjp  # noqa: E402

EXPORTS = ("tfmpc_tvlqr_backward_vjp_workspace_bytes_f64", "tfmpc_tvlqr_backward_vjp_kernel_name_f64",
           "tfmpc_tvlqr_backward_vjp_f64")
# (n, m, T, seed) of the budget cases of tests/test_tvlqr_backward_grad_f64_gpu.py, B = 4
GPU_CASES = ([(n, m, 7) for n, m in ((1, 1), (3, 2), (3, 5), (16, 8), (16, 16), (17, 8), (16, 17), (5, 20), (20, 10))]
             + [(32, 32, 4)] + [(n, m, T) for n, m in ((16, 8), (12, 5)) for T in (1, 2, 3)])
LDS_BYTES = {16: 4704 * 8, 32: 18112 * 8}


def _case(n, m, T, B=2, seed=0, final=False, unscaled=False):
    if unscaled:
        F, f, C, c = ref64.make_unscaled(n, m, T, B, seed=seed)
        Cf = cf = None
    else:
        F, f, C, c, Cf, cf = gref.problem(n, m, T, B, seed=seed, final=final)
    return g64.as_f64(F, f, C, c, Cf, cf), {k: v.astype(np.float64) for k, v in gref.upstream(n, m, T, B, seed=seed).items()}


@pytest.mark.parametrize("n,m,T", [(3, 2, 5), (5, 3, 2)])
@pytest.mark.parametrize("final", [False, True])
def test_the_restatements_agree_with_autograd(n, m, T, final):
    ops, ups = _case(n, m, T, final=final)
    rld, r64, rag = g64.references(*ops, ups)
    old = gref.closed_form(*ops, **ups)                    # the fp32 tests' oracle of record: the same fp64 numbers
    for name in g64.names_of((rld,)):
        assert r64[name].dtype == np.float64 and rld[name].dtype == np.longdouble
        scale = max(1.0, float(np.abs(rag[name]).max()))
        assert np.abs(r64[name] - rag[name]).max() <= 1e-9 * scale, name
        assert np.abs(np.asarray(rld[name], np.float64) - rag[name]).max() <= 1e-9 * scale, name
        assert np.abs(r64[name] - old[name]).max() <= 1e-12 * scale, name


def test_the_restatements_agree_with_central_differences():
    n, m, T = 3, 2, 3
    ops, ups = _case(n, m, T, B=1, final=True)
    rld, r64, _ = g64.references(*ops, ups)
    names = ("F", "f", "C", "c", "Cfin", "cfin")

    def loss(args):
        out = g64.recursion_np(*args)
        return sum(float((ups["g" + q] * out[q]).sum()) for q in ("K", "k", "V", "v", "const"))

    h = 1e-6
    for i, name in enumerate(names):
        fd = np.zeros_like(ops[i])
        for idx in np.ndindex(*ops[i].shape):
            hi, lo = [a.copy() for a in ops], [a.copy() for a in ops]
            hi[i][idx] += h
            lo[i][idx] -= h
            fd[idx] = (loss(hi) - loss(lo)) / (2 * h)
        if name in ("C", "Cfin"):
            fd = gref._sym(fd)
        scale = max(1.0, float(np.abs(fd).max()))
        assert np.abs(r64["d" + name] - fd.reshape(r64["d" + name].shape)).max() <= 1e-6 * scale, name
        assert np.abs(np.asarray(rld["d" + name], np.float64) - fd.reshape(r64["d" + name].shape)).max() <= 1e-6 * scale, name


def test_the_fp64_closed_form_does_not_degrade_with_the_horizon():
    """Unscaled (16, 8), B = 2, T = 5, 20, 50: the fp64 closed form's error relative to the gradient's scale grows by
    no more than 10 x from T = 5 to T = 50 (measured: 3 x on dF; the 10 is headroom over the reference's own behaviour)."""
    rel = {}
    for T in (5, 20, 50):
        ops, ups = _case(16, 8, T, unscaled=True)
        rld = g64.closed_form(*ops, **ups, dtype=g64.LD)
        r64 = g64.closed_form(*ops, **ups)
        assert not rld["status"].any() and not r64["status"].any()
        rel[T] = {name: ref64.error(r64[name], rld[name]) / float(np.abs(rld[name]).max()) for name in ("dF", "df", "dC", "dc")}
        print(T, {k: f"{v:.2e}" for k, v in rel[T].items()})
    for name in ("dF", "df", "dC", "dc"):
        assert rel[50][name] <= 10 * max(rel[5][name], rel[20][name], 2.0 ** -52), (name, rel)
        assert rel[50][name] <= 1e-11, (name, rel)


@pytest.mark.parametrize("n,m,T", GPU_CASES)
@pytest.mark.parametrize("final", [False, True])
def test_the_budget_is_attainable_on_the_gpu_tests_inputs(n, m, T, final):
    """The fp64 closed form with every product's k-sum reversed -- another admissible fp64 evaluation -- stays under the
    rule on every input of the GPU test's budget cases."""
    ops, ups = _case(n, m, T, B=4, seed=100 * n + m, final=final)
    refs = g64.references(*ops, ups)
    other = g64.closed_form(*ops, **ups, reverse=True)
    g64.check(other, refs, what=f"reversed ({n},{m},{T}) final={final}")


@pytest.mark.parametrize("seed", [0, 1])
def test_the_budget_is_attainable_on_the_long_unscaled_horizon(seed):
    ops, ups = _case(16, 8, 50, B=4, seed=seed, unscaled=True)
    refs = g64.references(*ops, ups)
    g64.check(g64.closed_form(*ops, **ups, reverse=True), refs, what=f"reversed unscaled seed {seed}")


# ---- the feature

def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    assert _hip._SIGNATURES["tfmpc_tvlqr_backward_vjp_f64"] == _hip._SIGNATURES["tfmpc_tvlqr_backward_vjp_f32"]
    assert solvers.tvlqr_backward_vjp is solvers.tvlqr_backward_grad.tvlqr_backward_vjp
    assert "tvlqr_backward_vjp" in vars(solvers)


def test_kernel_names_per_shape():
    name = lambda n, m: _hip.load().tfmpc_tvlqr_backward_vjp_kernel_name_f64(n, m, 5).decode()   # noqa: E731
    assert name(16, 16) == name(1, 1) == name(16, 8) == name(3, 5) == "tvb_vjp_f64_wave16"
    assert name(17, 8) == name(16, 17) == name(5, 20) == name(32, 32) == name(20, 10) == "tvb_vjp_f64_wave32"
    assert name(33, 1) == name(1, 33) == "unsupported"
    assert name(0, 3) == name(3, 0) == "invalid"
    assert _hip.load().tfmpc_tvlqr_backward_vjp_kernel_name_f64(3, 2, 0).decode() == "invalid"


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4, dtype=torch.float64))

    def call(B=1, n=3, m=2, T=2, F=p, f=p, C=p, c=p, s=0, Cfin=None, cfin=None, K=p, k=p, V=p, v=p, fst=p, dsb=1, dst=1,
             dF=p, dCfin=None, dcfin=None, status=p, ws=None, ws_bytes=0):
        return lib.tfmpc_tvlqr_backward_vjp_f64(B, n, m, T, F, s, s, f, s, s, C, s, s, c, s, s, Cfin, s, cfin, s, K, k, V, v, fst,
                                                None, None, None, None, None, dF, dsb, dst, p, dsb, dst, p, dsb, dst, p, dsb, dst,
                                                dCfin, dsb, dcfin, dsb, status, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(n=0) == -1 and call(m=0) == -1 and call(T=0) == -1 and call(n=-2) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(C=None) == -1 and call(c=None) == -1
    assert call(K=None) == -1 and call(k=None) == -1 and call(V=None) == -1 and call(v=None) == -1
    assert call(fst=None) == -1 and call(status=None) == -1
    assert call(Cfin=p) == -1 and call(cfin=p) == -1                 # Cfin without cfin, and the reverse
    assert call(dCfin=p) == -1 and call(dcfin=p) == -1               # dCfin without Cfin
    assert call(s=-3) == -1 and call(dsb=-3) == -1 and call(dst=-1) == -1
    assert call(n=33) == -2 and call(m=33) == -2 and call(B=0, n=40, m=40) == -2
    assert call(B=4, dsb=0) == -4                                    # a summed output needs the workspace
    assert call(B=4, dsb=0, ws=p, ws_bytes=16) == -4
    full = lib.tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(4, 3, 2, 2)
    assert call(B=4, dsb=0, Cfin=p, cfin=p, dCfin=p, dcfin=p, ws=p, ws_bytes=full - 8) == -4      # one double short of the plan
    assert call(B=0, F=None, f=None, C=None, c=None, K=None, k=None, V=None, v=None, fst=None, status=None) == 0


@pytest.mark.parametrize("n,m,T", [(5, 3, 4), (16, 8, 3), (20, 10, 1)])
@pytest.mark.parametrize("B", [0, 1, 2, 64, 65, 131, 16449])
def test_workspace_is_the_plan_in_doubles(B, n, m, T):
    ws = _hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes_f64
    d = n + m
    outputs = [(n * d, T), (n, T), (d * d, T), (d, T), (n * n, 1), (n, 1)]
    want = 0 if B <= 1 else 8 * batch_sum_ref.workspace_floats(B, batch_sum_ref.STEADY_STATE_CHUNK, outputs)
    assert ws(B, n, m, T) == want
    assert ws(4, 33, 1, T) == 0 and ws(4, 0, 1, T) == 0 and ws(4, 3, 2, 0) == 0


# ---- the front end, with a recorder standing in for the library

class _Recorder:
    """Keeps every launch's arguments and a copy of the F it points to; returns TFMPC_OK and writes nothing."""

    def __init__(self):
        self.forward, self.vjp, self.vjp32, self.F = [], [], [], []

    def _keep_F(self, args, kind):
        B, n, m, T, F, sb, st = args[:7]
        count = n * (n + m) * (T if st else 1) * (B if sb else 1)
        self.F.append(np.ctypeslib.as_array(ctypes.cast(F, ctypes.POINTER(kind)), shape=(count,)).copy())

    def tfmpc_tvlqr_backward_f64(self, *args):
        self._keep_F(args, ctypes.c_double)
        self.forward.append(args)
        return 0

    def tfmpc_tvlqr_backward_f32(self, *args):
        self.forward.append(("f32", *args))
        return 0

    def tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(self, B, n, m, T):
        return _hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(B, n, m, T)

    def tfmpc_tvlqr_backward_vjp_workspace_bytes(self, B, n, m, T):
        return _hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes(B, n, m, T)

    def tfmpc_tvlqr_backward_vjp_f64(self, *args):
        self._keep_F(args, ctypes.c_double)
        self.vjp.append(args)
        return 0

    def tfmpc_tvlqr_backward_vjp_f32(self, *args):
        self.vjp32.append(args)
        return 0


@pytest.fixture
def recorder(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_hip, "require_gpu", lambda: lib)
    monkeypatch.setattr(_hip, "stream", lambda: None)
    monkeypatch.setattr(_hip, "default_device", lambda: torch.device("cpu"))
    return lib


def _operands(n=3, m=2, T=4, B=2, final=False):
    ops, _ = _case(n, m, T, B=B, seed=5, final=final)
    return [None if a is None else a * (1.0 + 2.0 ** -40) for a in ops]      # not representable in fp32


# positions in tfmpc_tvlqr_backward_vjp_f64's argument list: B n m T, four (ptr, sb, st), two (ptr, sb), K k V v fst, five
# upstream, four (ptr, sb, st), two (ptr, sb), status ws ws_bytes stream
_IN = dict(F=4, f=7, C=10, c=13, Cfin=16, cfin=18)
_FWD, _UP = slice(20, 25), slice(25, 30)
_OUT = dict(F=30, f=33, C=36, c=39, Cfin=42, cfin=44)
_WS = slice(47, 49)


def test_the_double_dtype_reaches_both_f64_entries_with_fp64_buffers(recorder):
    n, m, T, B = 3, 2, 4, 2
    F, f, C, c, _, _ = _operands(n, m, T, B)
    d = n + m
    assert not np.array_equal(F.astype(np.float32).astype(np.float64), F)
    ops = [torch.as_tensor(a).requires_grad_() for a in (F, f, C, c)]
    K, k, V, v, const = tvlqr_backward(*ops, dtype=torch.float64)
    assert len(recorder.forward) == 1 and not recorder.vjp and not recorder.vjp32
    args = recorder.forward[-1]
    assert args[:4] == (B, n, m, T) and args[5:7] == (T * n * d, n * d)
    assert np.array_equal(recorder.F[-1], F.reshape(-1))                     # the caller's double bits: no pass through fp32
    for t, shape in ((K, (B, T, m, n)), (k, (B, T, m, 1)), (V, (B, T, n, n)), (v, (B, T, n, 1)), (const, (B, T, 1, 1))):
        assert tuple(t.shape) == shape and t.dtype == torch.float64 and t.requires_grad
    (K.sum() + v.float().sum()).backward()                                   # an fp32 upstream gradient is cast to double
    assert len(recorder.vjp) == 1 and not recorder.vjp32
    args = recorder.vjp[-1]
    assert args[:4] == (B, n, m, T) and np.array_equal(recorder.F[-1], F.reshape(-1))
    assert [args[_IN[q] + 1] for q in "FfCc"] == [T * n * d, T * n, T * d * d, T * d]
    assert [args[_IN[q] + 2] for q in "FfCc"] == [n * d, n, d * d, d]
    assert args[_IN["Cfin"]] is None and args[_IN["cfin"]] is None
    gK, gk, gV, gv, gconst = args[_UP]
    assert gK is not None and gv is not None and gk is None and gV is None and gconst is None     # unused outputs: NULL
    assert [args[_OUT[q] + 1] for q in "FfCc"] == [T * n * d, T * n, T * d * d, T * d]
    assert [args[_OUT[q] + 2] for q in "FfCc"] == [n * d, n, d * d, d]
    assert args[_OUT["Cfin"]] is None and args[_OUT["cfin"]] is None
    assert args[_WS][0] is None and args[_WS][1] == 0                        # nothing summed: no workspace
    for t, a in zip(ops, (F, f, C, c)):
        assert t.grad.dtype == torch.float64 and tuple(t.grad.shape) == a.shape


def test_operand_sharing_turns_into_strides_of_zero(recorder):
    n, m, T, B = 3, 2, 4, 5
    d = n + m
    F, f, C, c, Cf, cf = _operands(n, m, T, B, final=True)
    Ft = torch.as_tensor(F[0]).requires_grad_()                  # no batch axis: summed over the batch
    ft = torch.as_tensor(f[:, :1].copy()).requires_grad_()              # a time axis of 1: summed over time
    Ct = torch.as_tensor(C[0, :1].copy()).requires_grad_()              # both
    ct = torch.as_tensor(c).requires_grad_()
    Cft = torch.as_tensor(Cf[0]).requires_grad_()
    cft = torch.as_tensor(cf).requires_grad_()
    K, k, V, v, const = tvlqr_backward(Ft, ft, Ct, ct, Cft, cft, dtype=torch.float64)
    assert tuple(K.shape) == (B, T, m, n)
    (V.sum() + const.sum()).backward()
    args = recorder.vjp[-1]
    assert (args[_IN["F"] + 1], args[_IN["F"] + 2]) == (0, n * d)
    assert (args[_IN["f"] + 1], args[_IN["f"] + 2]) == (n, 0)
    assert (args[_IN["C"] + 1], args[_IN["C"] + 2]) == (0, 0)
    assert args[_IN["Cfin"] + 1] == 0 and args[_IN["cfin"] + 1] == n
    assert (args[_OUT["F"] + 1], args[_OUT["F"] + 2]) == (0, n * d)
    assert (args[_OUT["f"] + 1], args[_OUT["f"] + 2]) == (n, 0)
    assert (args[_OUT["C"] + 1], args[_OUT["C"] + 2]) == (0, 0)
    assert (args[_OUT["c"] + 1], args[_OUT["c"] + 2]) == (T * d, d)
    assert args[_OUT["Cfin"]] is not None and args[_OUT["Cfin"] + 1] == 0 and args[_OUT["cfin"] + 1] == n
    assert args[_UP][2] is not None and args[_UP][4] is not None and args[_UP][0] is None
    assert args[_WS][0] is not None and args[_WS][1] == _hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes_f64(B, n, m, T)
    assert tuple(Ft.grad.shape) == (T, n, d) and tuple(ft.grad.shape) == (B, 1, n) and tuple(Ct.grad.shape) == (1, d, d)
    assert tuple(Cft.grad.shape) == (n, n) and tuple(cft.grad.shape) == (B, n)
    # a batch of one writes in place, with no workspace
    one = tvlqr_backward(Ft, f[0], Ct, c[0], dtype=torch.float64)
    assert tuple(one[0].shape) == (T, m, n)
    one[0].sum().backward()
    assert recorder.vjp[-1][0] == 1 and recorder.vjp[-1][_WS][0] is None and recorder.vjp[-1][_WS][1] == 0


def test_tvlqr_backward_vjp_marshals_its_arguments(recorder):
    n, m, T, B = 3, 2, 4, 4
    d = n + m
    F, f, C, c, Cf, cf = _operands(n, m, T, B, final=True)
    z = lambda *s: np.zeros(s)       # noqa: E731
    fwd = (z(B, T, m, n), z(B, T, m), z(B, T, n, n), z(B, T, n), np.zeros(B, np.int32))
    out = tvlqr_backward_vjp(F[0], f, C[0], c, *fwd, gV=z(B, T, n, n), C_final=Cf, c_final=cf)
    assert len(out) == 7 and not recorder.forward
    dF, df, dC, dc, dCf, dcf, status = out
    assert tuple(dF.shape) == (T, n, d) and tuple(df.shape) == (B, T, n, 1) and tuple(dC.shape) == (T, d, d)
    assert tuple(dc.shape) == (B, T, d, 1) and tuple(dCf.shape) == (B, n, n) and tuple(dcf.shape) == (B, n, 1)
    assert tuple(status.shape) == (B,) and status.dtype == torch.int32
    assert all(g.dtype == torch.float64 for g in (dF, df, dC, dc, dCf, dcf))
    args = recorder.vjp[-1]
    assert args[:4] == (B, n, m, T) and args[_OUT["F"] + 1] == 0 and args[_OUT["f"] + 1] == T * n
    assert all(a is not None for a in args[_FWD])
    assert args[_UP][2] is not None and all(args[_UP][i] is None for i in (0, 1, 3, 4))
    assert args[_WS][0] is not None
    out = tvlqr_backward_vjp(F, f, C, c, *fwd, gconst=z(B, T))           # the default final cost: no dC_final
    assert out[4] is None and out[5] is None and recorder.vjp[-1][_OUT["Cfin"]] is None
    for dtype in (None, torch.float32, torch.float16, np.float64):
        with pytest.raises(ValueError):
            tvlqr_backward_vjp(F, f, C, c, *fwd, dtype=dtype)
    with pytest.raises(ValueError):
        tvlqr_backward_vjp(F, f, C, c, z(B - 1, T, m, n), z(B - 1, T, m), z(B - 1, T, n, n), z(B - 1, T, n), np.zeros(B - 1, np.int32))


def test_other_dtypes_raise_and_no_dtype_is_the_fp32_entry(recorder):
    F, f, C, c, _, _ = _operands()
    Ft = torch.as_tensor(F).requires_grad_()
    for dtype in (torch.float16, torch.bfloat16, np.float64, "float64"):
        with pytest.raises(ValueError):
            tvlqr_backward(Ft, f, C, c, dtype=dtype)
    assert not recorder.forward and not recorder.vjp
    for kw in (dict(), dict(dtype=None), dict(dtype=torch.float32)):
        K = tvlqr_backward(Ft, f, C, c, **kw)[0]
        assert K.dtype == torch.float32 and recorder.forward[-1][0] == "f32"
        K.sum().backward()
    assert len(recorder.vjp32) == 3 and not recorder.vjp
    # without a grad operand the double call is the plain double recursion
    K = tvlqr_backward(F, f, C, c, dtype=torch.float64)[0]
    assert K.dtype == torch.float64 and not K.requires_grad and recorder.forward[-1][0] != "f32"


def test_the_method_form_still_refuses(monkeypatch):
    monkeypatch.setattr(_hip, "require_gpu", lambda: pytest.fail("a launch was prepared"))
    F, f, C, c, _, _ = _operands()
    tv = TimeVaryingLQR(torch.as_tensor(F).requires_grad_(), f, C, c, device="cpu", dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32") as info:
        tv.backward(differentiable=True)
    assert "tvlqr_backward(..., dtype=torch.float64)" in str(info.value)


def test_the_double_gradient_path_asks_for_the_gpu(monkeypatch):
    """Fails without the feature (TypeError: unexpected keyword): on a machine without a GPU the double path gets as far as
    the launch and raises the RuntimeError that names the GPU (a visible GPU is hidden from the front end)."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    F, f, C, c, _, _ = _operands()
    with pytest.raises(RuntimeError, match="GPU"):
        tvlqr_backward(torch.as_tensor(F).requires_grad_(), f, C, c, dtype=torch.float64)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_f64_kernels_use_no_scratch_the_documented_lds_and_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_backward_vjp_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 4 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    kernels = sorted(f[0] for f in found if "tvb_vjp_f64_kernel" in f[0])
    assert len(kernels) == 2 and "ILi16E" in kernels[0] and "ILi32E" in kernels[1], found
    sums = sorted(f[0] for f in found if "batch_sum_" in f[0])
    assert len(sums) == 2 and "batch_sum_stage1" in sums[0] and "batch_sum_stage2_tree" in sums[1], found
    assert all(name.endswith("PKdimPd") for name in sums), sums            # the double overloads
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    # the instance kernels take all their LDS at launch (none static); the launch sizes are the layout's
    static = {name: int(size) for size, name in
              re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.group_segment_fixed_size).*\n)*?\s+\.name:\s+(\S+)\n", text)}
    assert all(static[name] == 0 for name in kernels), static
    source = open(path).read()
    assert "BvLayout<16>::kTotal == 4704 && BvLayout<32>::kTotal == 18112" in source
    assert LDS_BYTES[16] == 37632 and LDS_BYTES[32] == 144896 <= 160 * 1024
    # the f64 matrix-core instruction is in both instance kernels' bodies
    for name in kernels:
        body = text[text.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma_f64_16x16x4" in body, name

"""Double-precision gradients of the infinite-horizon LQR without a GPU: the restatements of
tests/lqr_steady_state_grad_f64_ref.py pinned against central differences and the LAPACK restatement, the row exchanges
the GPU test's inputs produce, the float64 emulation of the batch sum, the C ABI's declarations, bindings and argument
errors, the workspace plan, the Python front end up to the launch, and the kernels' register budget.

The restatement, row-exchange and emulation tests pin the YARDSTICK of tests/test_lqr_steady_state_grad_f64_gpu.py: they
run numpy only.  The tests from test_every_new_export_is_declared_bound_and_exported on test the FEATURE."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import batch_sum_f64_ref as sum64
import batch_sum_ref
import lqr_steady_state_f64_ref as ref64
import lqr_steady_state_grad_f64_ref as g64
import lqr_steady_state_grad_ref as gref
import lqr_steady_state_ref as ssref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip, solvers  # noqa: E402
from tfmpc.solvers import lqr_steady_state  # noqa: E402
from tfmpc.solvers.lqr import LQR  # noqa: E402

EXPORTS = ("tfmpc_lqr_steady_state_vjp_workspace_bytes_f64", "tfmpc_lqr_steady_state_vjp_kernel_name_f64",
           "tfmpc_lqr_steady_state_vjp_f64")
# the shapes of tests/test_lqr_steady_state_grad_f64_gpu.py with more than one row
PIVOT_SHAPES = [(3, 2), (3, 5), (12, 6), (16, 8), (16, 16), (17, 8), (16, 17), (20, 10), (32, 16), (32, 32), (22, 3)]
U64 = 2.0 ** -53                  # fp64 unit roundoff


def _upstream(n, m, seed=0):
    rng = np.random.default_rng(seed)
    return dict(gK=rng.normal(size=(m, n)), gk=rng.normal(size=m), gP=rng.normal(size=(n, n)), gp=rng.normal(size=n))


@pytest.mark.parametrize("kind", ["make_lqr", "damped"])
@pytest.mark.parametrize("n,m", [(3, 2), (3, 5)])
def test_the_restatements_agree_with_central_differences_and_each_other(n, m, kind):
    """S != 0 (make_lqr's C), f != 0; the fp64 vjp_gj against central differences of the fp64 steady state (1e-6) and
    the LAPACK restatement (1e-9), the 80-bit run against both."""
    F, f, C, c = (a[0] for a in ref64.operands(kind, n, m, 1, seed=100 * n + m))
    assert np.abs(f).max() > 0
    if kind == "make_lqr":
        assert np.abs(C[:n, n:]).max() > 0.01
    up = _upstream(n, m, seed=n * m)
    gj = g64.vjp_gj(F, f, C, c, **up)
    ld = g64.vjp_gj(F, f, C, c, **up, dtype=g64.LD)
    la = gref.vjp(F, f, C, c, **up, dtype=np.float64)
    fd = gref.steady_state_grad_fd(F, f, C, c, *up.values())
    assert gj["status"] == ld["status"] == la["status"] == 0
    for name in g64.GRADS:
        assert gj[name].dtype == np.float64 and ld[name].dtype == np.longdouble
        scale = max(1.0, float(np.abs(fd[name]).max()))
        assert np.abs(gj[name] - fd[name]).max() <= 1e-6 * scale, (name, np.abs(gj[name] - fd[name]).max(), scale)
        assert np.abs(gj[name] - la[name]).max() <= 1e-9 * scale, (name, np.abs(gj[name] - la[name]).max(), scale)
        assert ref64.error(gj[name], ld[name]) <= 1e-9 * scale and ref64.error(la[name], ld[name]) <= 1e-9 * scale, name
        assert ref64.error(fd[name], ld[name]) <= 1e-6 * scale, name


@pytest.mark.parametrize("n,m", PIVOT_SHAPES)
def test_the_gpu_tests_inputs_exchange_rows_in_the_pivoted_elimination(n, m):
    """For every GPU-test shape with n >= 2, one of the six instances of either workload exchanges rows in the
    elimination of I - A_cl."""
    exchanges = 0
    for kind in ("make_lqr", "damped"):
        F, f, C, c = ref64.operands(kind, n, m, 6, seed=100 * n + m)
        for b in range(6):
            got = g64.vjp_gj(F[b], f[b], C[b], c[b], **_upstream(n, m, seed=b))
            assert got["status"] == 0 or (kind, n, m) == ("make_lqr", 22, 3), (kind, b, got["status"])
            exchanges += got["exchanges"]
    assert exchanges >= 1


def test_the_restatement_flags_a_flagged_forward_and_a_capped_smith_loop():
    F, f, C, c = (a[0] for a in ref64.operands("damped", 16, 8, 1, seed=1))
    up = _upstream(16, 8)
    full = g64.vjp_gj(F, f, C, c, **up)
    assert full["status"] == 0 and 13 <= full["iterations"] <= 15
    capped = g64.vjp_gj(F, f, C, c, **up, max_iter=1)
    assert capped["status"] == ssref.ST_NOT_STABILISING and all(np.isnan(capped[name]).all() for name in g64.GRADS)
    Cb = C.copy()
    Cb[16:, 16:] = -1e3 * np.eye(8)
    bad = g64.vjp_gj(F, f, Cb, c, **up)
    assert bad["status"] == ssref.ST_NOT_PD and np.isnan(bad["dF"]).all()


@pytest.mark.parametrize("B", [1, 3, 4, 63, 64, 65, 131, 259, 64 * 257 + 1])
def test_the_float64_emulation_is_a_sum(B):
    """Any fp64 order of B terms is within the sequential sum's bound (B - 1) u sum|x| of the exact sum."""
    x = np.random.default_rng(B).normal(size=(B, 7))
    got = sum64.steady_state_sum(x)
    assert got.dtype == np.float64 and got.shape == (7,)
    exact = x.astype(np.longdouble).sum(0)
    bound = (B - 1) * U64 * np.abs(x).astype(np.longdouble).sum(0)
    assert (np.abs(got - exact) <= bound).all(), (B, float(np.abs(got - exact).max()), float(bound.min()))


def test_the_float64_emulation_hand_worked():
    """tests/test_batch_sum_cpu.py's eleven records in chunks of four with H = 2^53, where H + 1 rounds back to H:
      chunk 0: s = [H, 1, 1, -H] -> (H + 1) + (1 - H) = H - (H - 1) = 1;  chunk 1: s = [1, H, -H, 1] -> 1;
      chunk 2: the tail of three goes to s[0], s[1], s[2]: s = [1, 1, H, 0] -> (1 + 1) + (H + 0) = H + 2, exact.
    The tree adds t[0] + t[2] = 1 + (H + 2) = H + 3 -> H + 4 (tie to even) at w = 2, then + t[1] = H + 5 -> H + 4.
    In float32 the same records give 2^53 sums that lose every 1: the emulation does not pass through float32."""
    H = 2.0 ** 53
    rec = np.array([H, 1, 1, -H, 1, H, -H, 1, 1, 1, H]).reshape(11, 1)
    partial = sum64.stage1(rec, 4)
    assert partial.dtype == np.float64 and partial[:, 0].tolist() == [1.0, 1.0, H + 2]
    assert sum64.stage2_tree(partial)[0] == H + 4
    # 259 chunks: threads 0, 1 of the tree add two chunks each (k and k + 256) before the tree
    partial = np.zeros((259, 1))
    partial[0], partial[256], partial[1], partial[257] = H, 1.0, 1.0, 1.0
    assert sum64.stage2_tree(partial)[0] == H + 2          # thread 0: H + 1 -> H; thread 1: 2; H + 2 is exact
    x = np.random.default_rng(0).normal(size=(70, 5)) * (1.0 + 2.0 ** -40)
    assert not np.array_equal(sum64.steady_state_sum(x), batch_sum_ref.steady_state_sum(x).astype(np.float64))


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    assert len(_hip._SIGNATURES["tfmpc_lqr_steady_state_vjp_f64"][1]) == len(_hip._SIGNATURES["tfmpc_lqr_steady_state_vjp_f32"][1])
    assert _hip._SIGNATURES["tfmpc_lqr_steady_state_vjp_f64"][1][21] is ctypes.c_double
    assert solvers.lqr_steady_state_vjp is solvers.steady_state_grad.lqr_steady_state_vjp
    assert "lqr_steady_state_vjp" in vars(solvers)


def test_kernel_names_per_shape():
    name = lambda n, m: _hip.load().tfmpc_lqr_steady_state_vjp_kernel_name_f64(n, m).decode()   # noqa: E731
    assert name(16, 8) == name(16, 16) == name(1, 1) == name(3, 5) == name(12, 6) == "ss_vjp_f64_wave16"
    assert name(17, 8) == name(16, 17) == name(20, 10) == name(32, 16) == name(32, 32) == name(22, 3) == "ss_vjp_f64_wave32"
    assert name(33, 1) == name(8, 33) == "unsupported"
    assert name(0, 3) == name(3, 0) == "invalid"


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4, dtype=torch.float64))

    def call(B=1, n=3, m=2, F=p, f=p, C=p, c=p, s=0, K=p, k=p, P=p, pv=p, fst=p, max_iter=0, tol=0.0, ds=1, status=p,
             dF=p, ws=None, ws_bytes=0):
        return lib.tfmpc_lqr_steady_state_vjp_f64(B, n, m, F, s, f, s, C, s, c, s, K, k, P, pv, fst, None, None, None, None,
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
    full = lib.tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(4, 3, 2)
    assert call(B=4, ds=0, ws=p, ws_bytes=full - 8) == -4           # one double short of the plan
    assert call(B=0, F=None, f=None, C=None, c=None, K=None, k=None, P=None, pv=None, fst=None, status=None) == 0


@pytest.mark.parametrize("n,m", [(5, 3), (16, 8), (20, 10)])
@pytest.mark.parametrize("B", [0, 1, 2, 64, 65, 131, 16449])
def test_workspace_is_the_plan_in_doubles(B, n, m):
    ws = _hip.load().tfmpc_lqr_steady_state_vjp_workspace_bytes_f64
    want = 0 if B <= 1 else batch_sum_ref.steady_state_workspace_bytes(B, n, m) * 2      # nothing is summed over a batch of one
    assert ws(B, n, m) == want
    assert ws(4, 33, 1) == 0 and ws(4, 0, 1) == 0


# ---- the front end, with a recorder standing in for the library

class _Recorder:
    """Keeps every launch's arguments and a copy of the F it points to; returns TFMPC_OK and writes nothing."""

    def __init__(self):
        self.forward, self.vjp, self.F = [], [], []

    def _keep_F(self, args):
        B, n, m, F, stride = args[:5]
        count = (B * stride if stride else n * (n + m))
        self.F.append(np.ctypeslib.as_array(ctypes.cast(F, ctypes.POINTER(ctypes.c_double)), shape=(count,)).copy())

    def tfmpc_lqr_steady_state_f64(self, *args):
        self._keep_F(args)
        self.forward.append(args)
        return 0

    def tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(self, B, n, m):
        return _hip.load().tfmpc_lqr_steady_state_vjp_workspace_bytes_f64(B, n, m)

    def tfmpc_lqr_steady_state_vjp_f64(self, *args):
        self._keep_F(args)
        self.vjp.append(args)
        return 0


@pytest.fixture
def recorder(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_hip, "require_gpu", lambda: lib)
    monkeypatch.setattr(_hip, "stream", lambda: None)
    monkeypatch.setattr(_hip, "default_device", lambda: torch.device("cpu"))
    return lib


def _operands(n=3, m=2, B=2):
    return ref64.operands("make_lqr", n, m, B, seed=5)


# positions in tfmpc_lqr_steady_state_vjp_f64's argument list
_STRIDE_IN = dict(F=4, f=6, C=8, c=10)
_UP, _LIMITS, _OUT, _WS = slice(16, 20), slice(20, 22), dict(F=22, f=24, C=26, c=28), slice(31, 33)


def test_the_opt_in_reaches_both_launches_in_double(recorder):
    n, m, B = 3, 2, 2
    F, f, C, c = _operands(n, m, B)
    assert not np.array_equal(F.astype(np.float32).astype(np.float64), F)
    ops = [torch.as_tensor(a).requires_grad_() for a in (F, f, C, c)]
    ss = lqr_steady_state(*ops, max_iter=9, tol=1e-13, dtype=torch.float64, differentiable=True)
    assert len(recorder.forward) == 1 and not recorder.vjp
    args = recorder.forward[-1]
    assert args[:3] == (B, n, m) and args[4] == n * (n + m) and args[11:13] == (9, 1e-13)
    assert np.array_equal(recorder.F[-1], F.reshape(-1))                    # the caller's double bits
    for name, shape in (("K", (B, m, n)), ("k", (B, m, 1)), ("P", (B, n, n)), ("p", (B, n, 1))):
        t = getattr(ss, name)
        assert tuple(t.shape) == shape and t.dtype == torch.float64 and t.requires_grad, name
    assert not ss.status.requires_grad and not ss.iterations.requires_grad and ss.status.dtype == torch.int32
    (ss.K.sum() + ss.p.float().sum()).backward()                            # an fp32 upstream gradient is cast to double
    args = recorder.vjp[-1]
    assert args[:3] == (B, n, m) and np.array_equal(recorder.F[-1], F.reshape(-1))
    assert [args[i] for i in _STRIDE_IN.values()] == [n * (n + m), n, (n + m) ** 2, n + m]
    assert args[_LIMITS] == (9, 1e-13)
    gK, gk, gP, gp = args[_UP]
    assert gK is not None and gp is not None and gk is None and gP is None      # an unused output's pointer is NULL
    assert [args[i + 1] for i in _OUT.values()] == [n * (n + m), n, (n + m) ** 2, n + m]
    assert args[_WS][0] is None and args[_WS][1] == 0                       # nothing summed: no workspace
    for t, a in zip(ops, (F, f, C, c)):
        assert t.grad.dtype == torch.float64 and tuple(t.grad.shape) == a.shape


def test_an_operand_without_a_batch_axis_is_summed_through_the_workspace(recorder):
    n, m, B = 3, 2, 5
    F, f, C, c = _operands(n, m, B)
    Ft, Ct = torch.as_tensor(F[0]).requires_grad_(), torch.as_tensor(C[0]).requires_grad_()
    ct = torch.as_tensor(c).requires_grad_()
    ss = lqr_steady_state(Ft, f[0], Ct, ct, dtype=torch.float64, differentiable=True)
    assert tuple(ss.K.shape) == (B, m, n) and recorder.forward[-1][4] == 0 and recorder.forward[-1][10] == n + m
    ss.P.sum().backward()
    args = recorder.vjp[-1]
    assert args[_STRIDE_IN["F"]] == 0 and args[_STRIDE_IN["C"]] == 0 and args[_STRIDE_IN["c"]] == n + m
    assert args[_OUT["F"] + 1] == 0 and args[_OUT["C"] + 1] == 0 and args[_OUT["c"] + 1] == n + m
    assert args[_OUT["f"]] is None                                          # numpy f: no gradient asked for
    assert args[_UP][2] is not None and args[_UP][0] is None                # only gP arrives
    assert args[_WS][0] is not None and args[_WS][1] == batch_sum_ref.steady_state_workspace_bytes(B, n, m) * 2
    assert tuple(Ft.grad.shape) == (n, n + m) and tuple(ct.grad.shape) == (B, n + m)
    # a batch of one writes in place, with no workspace
    one = lqr_steady_state(Ft, f[0], Ct, c[0], dtype=torch.float64, differentiable=True)
    assert tuple(one.K.shape) == (m, n) and one.status.dim() == 0
    one.K.sum().backward()
    assert recorder.vjp[-1][0] == 1 and recorder.vjp[-1][_WS][0] is None and recorder.vjp[-1][_WS][1] == 0


def test_lqr_steady_state_vjp_up_to_the_launch(recorder):
    n, m, B = 3, 2, 4
    F, f, C, c = _operands(n, m, B)
    z = lambda *s: np.zeros(s)       # noqa: E731
    out = solvers.lqr_steady_state_vjp(F[0], f, C[0], c, z(B, m, n), z(B, m), z(B, n, n), z(B, n), np.zeros(B, np.int32),
                                       gP=z(B, n, n), max_iter=3)
    assert len(out) == 5 and not recorder.forward
    dF, df, dC, dc, status = out
    assert tuple(dF.shape) == (n, n + m) and tuple(df.shape) == (B, n, 1) and tuple(dC.shape) == (n + m, n + m)
    assert tuple(dc.shape) == (B, n + m, 1) and tuple(status.shape) == (B,) and status.dtype == torch.int32
    assert all(g.dtype == torch.float64 for g in (dF, df, dC, dc))
    args = recorder.vjp[-1]
    assert args[0] == B and args[_LIMITS] == (3, 0.0) and args[_OUT["F"] + 1] == 0 and args[_OUT["f"] + 1] == n
    assert args[_UP][2] is not None and args[_UP][0] is None and args[_UP][1] is None and args[_UP][3] is None
    assert args[_WS][0] is not None
    for dtype in (None, torch.float32, torch.float16, np.float64):
        with pytest.raises(ValueError):
            solvers.lqr_steady_state_vjp(F, f, C, c, z(B, m, n), z(B, m), z(B, n, n), z(B, n), np.zeros(B, np.int32), dtype=dtype)
    with pytest.raises(ValueError):
        solvers.lqr_steady_state_vjp(F, f, C, c, z(B - 1, m, n), z(B - 1, m), z(B - 1, n, n), z(B - 1, n), np.zeros(B - 1, np.int32))


def test_without_the_flag_the_refusal_stays_and_names_the_opt_in(monkeypatch):
    monkeypatch.setattr(_hip, "require_gpu", lambda: pytest.fail("a launch was prepared"))
    F, f, C, c = (torch.as_tensor(a) for a in _operands())
    opt_in = re.escape("lqr_steady_state(..., dtype=torch.float64, differentiable=True)")
    with pytest.raises(NotImplementedError, match=opt_in):
        lqr_steady_state(F.clone().requires_grad_(), f, C, c, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=opt_in):
        LQR(F.clone().requires_grad_(), f, C, c, device="cpu").steady_state(dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=opt_in):
        LQR(F, f, C, c, device="cpu").steady_state(dtype=torch.float64, differentiable=True)


def test_the_fp32_path_ignores_the_flag(monkeypatch):
    calls = []

    def fake(self, max_iter, tol):
        calls.append((max_iter, tol))
        n, m, Bk = self.state_size, self.action_size, self.batch_size or 1
        i32 = lambda: torch.zeros((Bk,), dtype=torch.int32)        # noqa: E731
        return (torch.zeros(Bk, m, n), torch.zeros(Bk, m, 1), torch.zeros(Bk, n, n), torch.zeros(Bk, n, 1), i32(), i32())

    monkeypatch.setattr(LQR, "_steady_state_launch", fake)
    monkeypatch.setattr(_hip, "default_device", lambda: torch.device("cpu"))
    F, f, C, c = ssref.make_lqr_batch(3, 2, 2, seed=5)
    for kw in (dict(), dict(differentiable=True), dict(differentiable=False), dict(dtype=torch.float32, differentiable=True)):
        ss = lqr_steady_state(torch.as_tensor(F).requires_grad_(), f, C, c, **kw)
        assert ss.K.dtype == torch.float32 and ss.K.requires_grad, kw
        plain = lqr_steady_state(F, f, C, c, **kw)
        assert not plain.K.requires_grad, kw
    assert len(calls) == 8


def test_the_flag_without_a_grad_operand_is_the_plain_double_call(recorder):
    F, f, C, c = _operands()
    ss = lqr_steady_state(F, f, C, c, dtype=torch.float64, differentiable=True)
    assert ss.K.dtype == torch.float64 and not ss.K.requires_grad and len(recorder.forward) == 1
    with torch.no_grad():
        ss = lqr_steady_state(torch.as_tensor(F).requires_grad_(), f, C, c, dtype=torch.float64, differentiable=True)
    assert not ss.K.requires_grad


def test_other_dtypes_and_an_asymmetric_cost_are_refused(recorder):
    F, f, C, c = _operands()
    Ft = torch.as_tensor(F).requires_grad_()
    for dtype in (torch.float16, torch.bfloat16, np.float64, "float64"):
        with pytest.raises(ValueError):
            lqr_steady_state(Ft, f, C, c, dtype=dtype, differentiable=True)
    Ca = C.copy()
    Ca[1, 0, 4] += 1e-9 * np.abs(C[1]).max()
    with pytest.raises(NotImplementedError, match="symmetric"):
        lqr_steady_state(Ft, f, Ca, c, dtype=torch.float64, differentiable=True)
    with pytest.raises(ValueError):
        lqr_steady_state(Ft, f, C, c, dtype=torch.float64, differentiable=True, max_iter=0)
    with pytest.raises(ValueError):
        lqr_steady_state(Ft, f, C, c, dtype=torch.float64, differentiable=True, tol=float("nan"))
    assert not recorder.forward and not recorder.vjp


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_f64_vjp_kernels_use_no_scratch_and_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "lqr_steady_state_vjp_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 4 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    assert len([f for f in found if "ss_vjp_f64_kernel" in f[0]]) == 2, found
    sums = sorted(f[0] for f in found if "batch_sum_" in f[0])
    assert len(sums) == 2 and "batch_sum_stage1" in sums[0] and "batch_sum_stage2_tree" in sums[1], found
    assert all(name.endswith("PKdimPd") for name in sums), sums            # the double overloads
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    assert "v_mfma_f64_16x16x4" in text

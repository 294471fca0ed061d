"""The segmented adjoint of the time-parallel double-precision TV-LQR without a GPU: the numpy
restatement against the 80-bit value-function reference and under tests/tvlqr_grad_f64_ref.py's rule, the segment table's
edges, the workspace formula, the C ABI (declarations, bindings, argument errors), the Python opt-in and refusals, and
the kernels' assembly."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import tvlqr_f64_ref as ref64
import tvlqr_grad_f64_ref as g64
import tvlqr_ref
import tvlqr_time_parallel_grad_ref as tpg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR, tvlqr_solve_time_parallel, tvlqr_vjp_time_parallel  # noqa: E402

LD = np.longdouble
EXPORTS = ("tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64", "tfmpc_tvlqr_vjp_time_parallel_f64")
# (n, m, T, segments): the shapes the algorithm was prototyped on, T <= 200
SCALED = [(3, 2, 8, 4), (5, 3, 7, 3), (16, 8, 50, 5), (16, 8, 64, 64), (16, 8, 200, 8), (32, 32, 8, 2)]
UNSCALED = [(16, 8, 50, 5), (17, 8, 12, 3), (16, 8, 200, 8)]
KERNELS = ("tp_vjp_step_kernelILi16E", "tp_vjp_step_kernelILi32E", "tp_vjp_condense_kernelILi16E", "tp_vjp_condense_kernelILi32E",
           "tp_vjp_stitch_back_kernel", "tp_vjp_expand_back_kernel", "tp_vjp_stitch_fwd_kernel", "tp_vjp_expand_fwd_kernel")
_CACHE = {}


def _case(n, m, T, final=False, unscaled=False, B=2):
    """A seeded problem (mixed loss) and tvlqr_grad_f64_ref's three references, computed once."""
    key = (n, m, T, final, unscaled, B)
    if key not in _CACHE:
        make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
        F, f, C, c = (a.astype(np.float64) for a in make(n, m, T, B, seed=n * 100 + m))
        Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B)) if final else (None, None)
        x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
        rng = np.random.default_rng(T)
        g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
        ops = (F, f, C, c, x0, Cf, cf) + g
        _CACHE[key] = (ops, g64.references(*ops))
    return _CACHE[key]


def _agrees_in_longdouble(ops, rld, segments, what):
    got = tpg.grads(*ops, segments, dtype=LD)
    assert set(got) == set(rld)
    for k in rld:
        err, scale = float(np.abs(got[k] - rld[k]).max()), max(1.0, float(np.abs(rld[k]).max()))
        print(f"longdouble {what} d{k}: {err / scale:.3g}")
        assert got[k].dtype == LD and err <= 1e-14 * scale, (what, k, err, scale)


@pytest.mark.parametrize("n,m,T,segments", SCALED)
def test_the_longdouble_restatement_is_the_value_function_reference(n, m, T, segments):
    """A formula error shows at once: in 80-bit the segmented recursions agree with the adjoint SOLVE of
    tvlqr_grad_f64_ref.closed_form to 1e-14 max(1, |ref|) on every output (measured: <= 5.8e-16)."""
    for final in (False, True):
        ops, refs = _case(n, m, T, final)
        _agrees_in_longdouble(ops, refs[0], segments, (n, m, T, segments, final))


@pytest.mark.parametrize("n,m,T,segments", UNSCALED)
def test_the_longdouble_restatement_on_unscaled_models(n, m, T, segments):
    ops, refs = _case(n, m, T, unscaled=True)
    _agrees_in_longdouble(ops, refs[0], segments, ("unscaled", n, m, T, segments))


@pytest.mark.parametrize("n,m,T,segments", SCALED)
def test_the_fp64_restatement_meets_the_rule_unwidened(n, m, T, segments):
    """K, V, v from the fp64 sequential restatement; the budget is tvlqr_grad_f64_ref's own three terms."""
    ops, refs = _case(n, m, T)
    g64.check(tpg.grads(*ops, segments), refs, what=("segmented", n, m, T, segments))


@pytest.mark.parametrize("n,m,T,segments", UNSCALED)
def test_the_fp64_restatement_meets_the_rule_on_unscaled_models(n, m, T, segments):
    ops, refs = _case(n, m, T, unscaled=True)
    g64.check(tpg.grads(*ops, segments), refs, what=("segmented unscaled", n, m, T, segments))


@pytest.mark.parametrize("T,segments,table", [(7, 3, [(0, 3), (3, 6), (6, 7)]), (7, 7, [(t, t + 1) for t in range(7)]),
                                              (7, 50, [(t, t + 1) for t in range(7)]), (7, 1, [(0, 7)]),
                                              (8, 3, [(0, 3), (3, 6), (6, 8)]), (1, 2, [(0, 1)])])
def test_segment_table_edges(T, segments, table):
    """A short last segment, one step per segment, more segments than steps (clamped), one segment: the same gradients
    in 80-bit, and the fp64 restatement under the rule."""
    assert tpg.segment_table(T, segments)[1] == table
    ops, refs = _case(5, 3, T, final=True)
    _agrees_in_longdouble(ops, refs[0], segments, ("edges", T, segments))
    g64.check(tpg.grads(*ops, segments), refs, what=("edges", T, segments))


def test_workspace_formula():
    lib = _hip.load()
    query = lib.tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64
    for B, n, m, T, segments in ((1, 16, 8, 4096, 64), (3, 5, 3, 7, 3), (300, 16, 8, 50, 5), (2, 32, 32, 8, 2), (2, 3, 2, 9, 50),
                                 (257, 17, 8, 12, 3)):
        assert query(B, n, m, T, segments) == tpg.workspace_bytes(B, n, m, T, segments), (B, n, m, T, segments)
    # one segment (asked for, or clamped at T = 1) is the sequential VJP's workspace
    assert query(2, 3, 2, 4, 1) == lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(2, 3, 2, 4)
    assert query(2, 3, 2, 1, 9) == lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(2, 3, 2, 1)
    for bad in ((0, 3, 2, 4, 2), (2, 0, 2, 4, 2), (2, 3, 0, 4, 2), (2, 3, 2, 0, 2), (2, 3, 2, 4, 0), (2, 3, 2, 4, -1)):
        assert query(*bad) == 0, bad


def test_every_new_export_is_declared_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES and hasattr(lib, name) and name in integration, name
    sig = _hip._SIGNATURES["tfmpc_tvlqr_vjp_time_parallel_f64"][1]
    # tfmpc_tvlqr_vjp_f64's arguments and K, V, segments
    assert len(sig) == len(_hip._SIGNATURES["tfmpc_tvlqr_vjp_f64"][1]) + 3
    decl = re.search(r"int tfmpc_tvlqr_vjp_time_parallel_f64\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(sig)
    assert re.search(r"const double \*v,\s*const double \*K, const double \*V,", decl)
    assert re.search(r"int32_t \*status, int segments, void \*workspace", decl)


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    buf = torch.zeros(8, dtype=torch.float64)
    p = _hip.ptr(buf)

    def call(B, n, m, T, segments=2, s=0, model_null=None, outs_fin=False, status=True, ws=p, ws_bytes=1 << 40, so=0, v=True,
             K=True, V=True):
        model = [p, s, s] * 4 + [None, 0, None, 0]
        if model_null is not None:
            model[model_null] = None
        outs = [p, so, so] * 4 + [p if outs_fin else None, 0, p if outs_fin else None, 0, p, 0]
        return lib.tfmpc_tvlqr_vjp_time_parallel_f64(B, n, m, T, *model, p, p, p if v else None, p if K else None,
                                                     p if V else None, None, None, None, *outs, p if status else None, segments,
                                                     ws, ws_bytes, None)

    assert call(1, 3, 2, 0) == -1 and call(1, 0, 2, 4) == -1 and call(-1, 3, 2, 4) == -1
    assert call(1, 33, 2, 4) == -2 and call(1, 2, 33, 4) == -2 and call(1, 200, 200, 4) == -2   # n or m above 32
    assert call(1, 3, 2, 4, segments=0) == -1 and call(1, 3, 2, 4, segments=-3) == -1
    assert call(1, 3, 2, 4, v=False) == -1
    assert call(1, 3, 2, 4, K=False) == -1 and call(1, 3, 2, 4, V=False) == -1             # required with P > 1
    assert call(1, 3, 2, 4, s=-1) == -1 and call(1, 3, 2, 4, so=-1) == -1
    assert call(1, 3, 2, 4, model_null=0) == -1
    assert call(1, 3, 2, 4, outs_fin=True) == -1                                            # dCfin without Cfin
    assert call(1, 3, 2, 4, status=False) == -1
    need = lib.tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64(1, 3, 2, 4, 2)
    assert call(1, 3, 2, 4, ws=None) == -4 and call(1, 3, 2, 4, ws_bytes=need - 1) == -4
    odd = ctypes.c_void_p(buf.data_ptr() + 4)                                               # doubles are carved from it
    assert call(1, 3, 2, 4, ws=odd) == -1
    assert call(0, 3, 2, 4, status=False, ws=None, v=False, K=False, V=False) == 0          # B == 0: no-op
    # one segment forwards to tfmpc_tvlqr_vjp_f64: K and V are not looked at, its workspace rule applies
    need1 = lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(1, 3, 2, 4)
    assert call(1, 3, 2, 4, segments=1, K=False, V=False, ws_bytes=need1 - 1) == -4
    assert call(1, 3, 2, 1, segments=7, K=False, V=False, ws=None) == -4
    assert call(1, 3, 2, 4, segments=1, v=False) == -1


def _double_problem(requires_grad, dtype=np.float64):
    F, f, C, c = (torch.as_tensor(a.astype(dtype)) for a in tvlqr_ref.make_models(3, 2, 4, 2, seed=3))
    F.requires_grad_(requires_grad)
    return F, f, C, c, torch.ones(2, 3, 1, dtype=torch.float64)


def test_the_flag_reaches_the_gpu_and_the_refusal_names_it():
    F, f, C, c, x0 = _double_problem(True)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu", dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"differentiable=True to solve_time_parallel.*solve\(x0, differentiable=True\)"):
        tv.solve_time_parallel(x0, 2)
    with pytest.raises(NotImplementedError, match=r"differentiable=True to solve_time_parallel"):
        tvlqr_solve_time_parallel(F, f, C, c, x0, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        tv.solve_time_parallel(x0, 2, differentiable=True)
    with pytest.raises(RuntimeError, match="GPU"):
        tv.solve_time_parallel(x0, differentiable=True, want_policy=True)
    with pytest.raises(RuntimeError, match="GPU"):
        tvlqr_solve_time_parallel(F, f, C, c, x0, 2, differentiable=True)
    with pytest.raises(RuntimeError, match="GPU"):
        tvlqr_solve_time_parallel(F.detach(), f, C, c, x0.clone().requires_grad_(True), differentiable=True)
    with pytest.raises(ValueError, match="segments"):
        tv.solve_time_parallel(x0, 0, differentiable=True)
    assert tv.default_vjp_segments(2) >= 1


def test_default_vjp_segments_rule():
    F, f, C, c = (a[:, :1].astype(np.float64) for a in tvlqr_ref.make_models(3, 2, 1, 1, seed=3))
    mk = lambda T: TimeVaryingLQR(*(torch.as_tensor(a).expand(1, T, *a.shape[2:]) for a in (F, f, C, c)), device="cpu",     # noqa: E731
                                  dtype=torch.float64, symmetric=True)
    tv = mk(4096)
    assert tv.default_vjp_segments(1) == 93                   # sqrt(2.1 T), between the measured optima 64 and 128 (a tie)
    assert tv.default_vjp_segments(64) == 93 and tv.default_vjp_segments(4096) == 93      # no cap in the batch
    assert mk(512).default_vjp_segments(8) == 33              # measured optimum: 32
    assert mk(8).default_vjp_segments(1) == 4
    assert mk(5).default_vjp_segments(1) == 1 and mk(1).default_vjp_segments(1) == 1      # too short to pay for the launches


def test_fp32_problems_are_refused_with_the_flag_too():
    F, f, C, c, x0 = _double_problem(True)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float64"):
        TimeVaryingLQR(F, f, C, c, device="cpu").solve_time_parallel(x0, 2, differentiable=True)
    F32, f32, C32, c32, _ = _double_problem(True, np.float32)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float64"):
        tvlqr_solve_time_parallel(F32, f32, C32, c32, x0, 2, differentiable=True)


class _Recorder:
    """Stands in for the library: records the calls instead of launching."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.endswith("workspace_bytes_f64"):
            return getattr(_hip.load(), name)

        def record(*a):
            self.calls.append((name, a))
            return 0
        return record


def test_the_backward_passes_the_forwards_tensors_segments_and_strides(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_hip, "require_gpu", lambda: rec)
    monkeypatch.setattr(_hip, "stream", lambda: None)
    F, f, C, c = (a.astype(np.float64) for a in tvlqr_ref.make_models(3, 2, 6, 3, seed=3))
    Ft, ct = torch.as_tensor(F[0]).requires_grad_(True), torch.as_tensor(c[:, :1]).requires_grad_(True)   # shared; a time axis of 1
    x0 = torch.ones(3, 3, 1, dtype=torch.float64, requires_grad=True)
    tv = TimeVaryingLQR(Ft, f, C, ct, device="cpu", dtype=torch.float64)
    traj, K, k = tv.solve_time_parallel(x0, segments=4, want_policy=True, differentiable=True)
    name, a = rec.calls[-1]
    assert name == "tfmpc_tvlqr_solve_time_parallel_f64" and a[30] == 4 and all(a[i] is not None for i in (24, 25, 26, 27))
    assert traj.states.requires_grad and not K.requires_grad and K.shape == (3, 6, 2, 3)
    (traj.states.sum() + traj.costs.sum()).backward()
    name, a = rec.calls[-1]
    assert name == "tfmpc_tvlqr_vjp_time_parallel_f64" and a[:4] == (3, 3, 2, 6)
    assert all(a[i] is not None for i in range(20, 28))              # states actions v K V, the upstream gradients
    assert a[28] is not None and a[29:31] == (0, 3 * 5)             # dF: summed over the batch, a slot per step
    assert a[31] is None and a[34] is None                           # f, C are numpy: no gradient
    assert a[37] is not None and a[38:40] == (5, 0)                  # dc: per instance, summed over time
    assert a[40] is None and a[42] is None and a[44] is not None and a[45] == 3
    assert a[47] == 4 and a[49] >= tpg.workspace_bytes(3, 3, 2, 6, 4)
    assert Ft.grad.shape == Ft.shape and ct.grad.shape == ct.shape and x0.grad.dtype == torch.float64
    assert tv.last_grad_status is not None and tuple(tv.last_grad_status.shape) == (3,)
    # no segments given: the backward asks default_vjp_segments
    Ft.grad = None
    states, _, _ = tvlqr_solve_time_parallel(Ft, f, C, ct, x0, differentiable=True)
    states.sum().backward()
    assert rec.calls[-1][1][47] == tv.default_vjp_segments(3)
    # the functional VJP: every gradient in its operand's shape
    out = tvlqr_vjp_time_parallel(F[0], f, C, c[:, :1], np.zeros((3, 7, 3)), np.zeros((3, 6, 2)), np.zeros((3, 6, 2, 3)),
                                  np.zeros((3, 6, 3, 3)), np.zeros((3, 6, 3)), g_states=np.ones((3, 7, 3)), segments=3)
    dF, df, dC, dc, dCf, dcf, dx0, status = out
    assert dF.shape == (6, 3, 5) and df.shape == (3, 6, 3, 1) and dC.shape == (3, 6, 5, 5) and dc.shape == (3, 1, 5, 1)
    assert dCf is None and dcf is None and dx0.shape == (3, 3, 1) and status.shape == (3,)
    assert rec.calls[-1][1][47] == 3 and rec.calls[-1][1][26] is None


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_kernels_use_no_scratch_and_the_condense_runs_on_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_vjp_time_parallel_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)) == len(found) == len(KERNELS), found
    for stem in KERNELS:
        assert sum(stem in name for name, *_ in found) == 1, (stem, found)
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        body = re.search(r"\n" + re.escape(name) + r":.*?\n(.*?)\n\s*\.amdhsa_kernel\s+" + re.escape(name), text, flags=re.S)
        assert body, name
        assert "v_mfma_f32" not in body.group(1) and "scratch_" not in body.group(1), name
        assert ("v_mfma_f64_16x16x4" in body.group(1)) == ("condense" in name or "step" in name), name

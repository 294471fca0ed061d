"""The time-parallel double-precision time-varying LQR without a GPU: the numpy restatement of its three
phases against the longdouble sequential recursion under the project's double rule, the segment table, the workspace
formula, the C ABI's declarations, bindings and argument errors, the Python refusals, and the kernels' assembly."""
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
import tvlqr_ref
import tvlqr_time_parallel_ref as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR, tvlqr_solve_time_parallel  # noqa: E402

EXPORTS = ("tfmpc_tvlqr_time_parallel_workspace_bytes_f64", "tfmpc_tvlqr_time_parallel_kernel_name_f64",
           "tfmpc_tvlqr_solve_time_parallel_f64")
# (n, m, T, segments): the shapes the algorithm was prototyped on
CASES = [(3, 2, 8, 4), (5, 3, 7, 3), (16, 8, 50, 5), (16, 8, 64, 64), (17, 8, 12, 3), (32, 32, 8, 2), (16, 8, 200, 8)]


def _check(n, m, T, segments, B, make):
    """The fp64 restatement against solve_ld; the budget is the SEQUENTIAL fp64 restatement's error or the 2^-48 floor."""
    F, f, C, c = tp.perturbed(make, n, m, T, B, seed=n * 100 + m)
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    rld, r64 = ref64.references(F, f, C, c, x0)
    got = tp.solve_batch(F, f, C, c, x0, segments)
    ref64.check({name: [g[name] for g in got] for name in tp.FIELDS}, rld, r64, fields=tp.FIELDS, what=(n, m, T, segments))


@pytest.mark.parametrize("n,m,T,segments", CASES)
def test_the_restatement_meets_the_double_rule(n, m, T, segments):
    _check(n, m, T, segments, 2 if n == 32 else 4, tvlqr_ref.make_models)


@pytest.mark.parametrize("n,m,T,segments", [case for case in CASES if -(-case[2] // case[3]) >= 4])
def test_the_restatement_meets_the_double_rule_on_unscaled_models(n, m, T, segments):
    """Segment lengths >= 4: with single-step segments the unscaled costs reach a median above the rule."""
    _check(n, m, T, segments, 2 if n == 32 else 4, ref64.make_unscaled)


def test_the_longdouble_variant_is_the_sequential_recursion():
    """A formula error shows at once: in longdouble the three phases agree with the plain recursion to ~1e-17 relative."""
    n, m, T = 5, 3, 11
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, 1, seed=3)
    x0 = tvlqr_ref.make_x0(n, 1).astype(np.float64)
    Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, 1))
    for segments, final in ((3, False), (11, False), (4, True)):
        fin = (Cf[0], cf[0]) if final else (None, None)
        a = tp.solve(F[0], f[0], C[0], c[0], x0[0], segments, *fin, dtype=np.longdouble)
        b = ref64.solve_ld(F[0], f[0], C[0], c[0], x0[0], *fin)
        for name in tp.FIELDS:
            assert a[name].dtype == np.longdouble
            assert float(np.abs(a[name] - b[name]).max()) <= 1e-15 * max(1.0, float(np.abs(b[name]).max())), (segments, name)
        _, table = tp.segment_table(T, segments)
        for i, (t0, _) in enumerate(table):                 # the stitch's boundaries are the recursion's own
            assert float(np.abs(a["boundary_states"][i] - b["states"][t0]).max()) <= 1e-15
        for i, (_, t1) in enumerate(table[:-1]):
            assert float(np.abs(a["boundary_V"][i] - b["V"][t1]).max()) <= 1e-15 * float(np.abs(b["V"][t1]).max())


def test_segment_table():
    assert tp.segment_table(10, 3) == (4, [(0, 4), (4, 8), (8, 10)])
    assert tp.segment_table(10, 4) == (3, [(0, 3), (3, 6), (6, 9), (9, 10)])
    assert tp.segment_table(9, 4) == (3, [(0, 3), (3, 6), (6, 9)])             # fewer segments than asked for
    assert tp.segment_table(7, 100) == (1, [(t, t + 1) for t in range(7)])      # clamped to T
    assert tp.segment_table(5, 1) == (5, [(0, 5)])
    with pytest.raises(ValueError):
        tp.segment_table(5, 0)


def test_workspace_formula_and_kernel_names():
    lib = _hip.load()
    ws = lib.tfmpc_tvlqr_time_parallel_workspace_bytes_f64
    for B, n, m, T, segments in ((3, 16, 8, 50, 7), (1, 32, 32, 9, 4), (2, 3, 2, 7, 100), (4, 5, 3, 10, 1), (1, 1, 1, 1, 1)):
        assert ws(B, n, m, T, segments) == tp.workspace_bytes(B, n, m, T, segments), (B, n, m, T, segments)
        assert ws(B, n, m, T, segments) >= lib.tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T)
    # B = 2, n = 3, m = 2, T = 7, seven segments: w = 14
    assert ws(2, 3, 2, 7, 100) == 8 * (14 * (36 + 12) + 2 * 7 * 2 * 4) + 4 * (28 + 2)
    assert ws(3, 16, 8, 50, 7) % 8 == 0
    for bad in ((0, 3, 2, 7, 2), (2, 0, 2, 7, 2), (2, 3, 2, 0, 2), (2, 3, 2, 7, 0), (-1, 3, 2, 7, 2)):
        assert ws(*bad) == 0, bad
    name = lambda *a: lib.tfmpc_tvlqr_time_parallel_kernel_name_f64(*a).decode()      # noqa: E731
    assert name(16, 16, 50, 4) == "tv_f64_time_parallel16" and name(1, 1, 2, 2) == "tv_f64_time_parallel16"
    assert name(17, 8, 50, 4) == "tv_f64_time_parallel32" and name(16, 17, 50, 50) == "tv_f64_time_parallel32"
    assert name(16, 8, 50, 1) == "tv_f64_wave16" and name(17, 8, 1, 9) == "tv_f64_wave32"      # one segment: the sequential kernel
    assert name(33, 1, 50, 4) == "unsupported" and name(1, 33, 50, 4) == "unsupported"
    assert name(0, 1, 50, 4) == "invalid" and name(3, 2, 50, 0) == "invalid" and name(3, 2, 0, 2) == "invalid"


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    seq, par = _hip._SIGNATURES["tfmpc_tvlqr_solve_f64"], _hip._SIGNATURES["tfmpc_tvlqr_solve_time_parallel_f64"]
    assert par[0] is seq[0] and len(par[1]) == len(seq[1]) + 1           # tfmpc_tvlqr_solve_f64's arguments plus segments
    assert par[1][:30] == seq[1][:30] and par[1][30] is ctypes.c_int and par[1][31:] == seq[1][30:]
    decl = re.search(r"int tfmpc_tvlqr_solve_time_parallel_f64\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(par[1])
    assert lib.tfmpc_version() == 320 and _hip.MIN_VERSION == 320


def test_argument_errors_return_before_any_launch():
    lib = _hip.load()
    dummy = torch.zeros(4, dtype=torch.float64)
    p = _hip.ptr(dummy)
    model = lambda B, n, m, T, s=0: (B, n, m, T, *([p, s, s] * 4), None, 0, None, 0)     # noqa: E731

    def solve(mdl, segments=2, x0=p, cst=None, ws=p, nbytes=1 << 30):
        return lib.tfmpc_tvlqr_solve_time_parallel_f64(*mdl, x0, p, p, p, None, None, None, None, cst, None, segments, ws, nbytes, None)
    # tfmpc_tvlqr_solve_f64's checks, in its order
    assert solve(model(1, 3, 2, 0)) == -1 and solve(model(1, 0, 2, 4)) == -1 and solve(model(-1, 3, 2, 4)) == -1
    assert solve(model(1, 33, 2, 4)) == -2 and solve(model(1, 2, 33, 4)) == -2
    assert solve(model(0, 33, 2, 4)) == -2                    # ... the shape check comes before the B == 0 no-op
    assert solve(model(1, 3, 2, 4, s=-5)) == -1
    args = list(model(1, 3, 2, 4))
    args[4] = None
    assert solve(args) == -1                                  # F NULL
    args = list(model(1, 3, 2, 4))
    args[16] = p
    assert solve(args) == -1                                  # Cfin without cfin
    # the call's own
    assert solve(model(1, 3, 2, 4), segments=0) == -1 and solve(model(1, 3, 2, 4), segments=-3) == -1
    assert solve(model(1, 3, 2, 4), cst=p) == -1              # the constant term is not carried
    assert solve(model(0, 3, 2, 4)) == 0                      # B == 0: no-op
    assert solve(model(1, 3, 2, 4), x0=None) == -1
    need = lib.tfmpc_tvlqr_time_parallel_workspace_bytes_f64(2, 3, 2, 4, 2)
    assert solve(model(2, 3, 2, 4), ws=None, nbytes=0) == -4 and solve(model(2, 3, 2, 4), nbytes=need - 1) == -4
    odd = ctypes.c_void_p(dummy.data_ptr() + 4)               # doubles are carved from the workspace
    assert solve(model(2, 3, 2, 4), ws=odd) == -1
    # one segment (asked for, or clamped at T = 1) forwards: tfmpc_tvlqr_solve_f64's workspace rule applies
    need1 = lib.tfmpc_tvlqr_workspace_bytes_f64(2, 3, 2, 4)
    assert solve(model(2, 3, 2, 4), segments=1, nbytes=need1 - 1) == -4
    assert solve(model(2, 3, 2, 1), segments=7, ws=None, nbytes=0) == -4


def test_the_phase_option_is_known_documented_and_off_by_default():
    """TFMPC_TVLQR_TP_PHASES stops the solve after a launch for timing; such a call returns TFMPC_TVLQR_TP_STOPPED, which the
    Python front end raises on, so a stopped call is never taken for a result."""
    name = "TFMPC_TVLQR_TP_PHASES"
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    assert name in header and re.search(r"#define TFMPC_TVLQR_TP_STOPPED 1\b", header)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.environ.get(name) is None and _hip.get_option(name) is None          # unset: all four launches
    with _hip.option(name, "2"):
        assert _hip.get_option(name) == "2"
    assert _hip.get_option(name) is None
    assert _hip.TVLQR_TP_STOPPED == 1 and "TFMPC_TVLQR_TP_PHASES" in _hip.ERRORS[1]
    with pytest.raises(RuntimeError, match="TFMPC_TVLQR_TP_PHASES"):
        _hip.check(_hip.TVLQR_TP_STOPPED, "tfmpc_tvlqr_solve_time_parallel_f64")


class _Recorder:
    """Stands in for the library: records the solve call's arguments instead of launching."""

    def __init__(self):
        self.calls = []

    def tfmpc_tvlqr_time_parallel_workspace_bytes_f64(self, *a):
        return _hip.load().tfmpc_tvlqr_time_parallel_workspace_bytes_f64(*a)

    def tfmpc_tvlqr_solve_time_parallel_f64(self, *a):
        self.calls.append(a)
        return 0


def _model64(B, T, n, m):
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, T, max(B, 1), seed=3)
    return (F, f, C, c) if B else (F[0], f[0], C[0], c[0])


def test_the_python_call_passes_segments_strides_and_outputs(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_hip, "require_gpu", lambda: rec)
    monkeypatch.setattr(_hip, "stream", lambda: None)
    F, f, C, c = _model64(3, 6, 3, 2)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu", dtype=torch.float64)
    traj, K, k = tv.solve_time_parallel(np.ones((3, 3, 1)), segments=4, want_policy=True)
    a = rec.calls[-1]
    assert a[:4] == (3, 3, 2, 6) and a[30] == 4 and a[28] is None                    # B n m T, segments, cst
    assert a[24] is not None and a[25] is not None and a[26] is None and a[27] is None          # K k given, V v not
    assert a[32] >= tp.workspace_bytes(3, 3, 2, 6, 4) and a[31] is not None
    assert traj.states.shape == (3, 7, 3) and K.shape == (3, 6, 2, 3) and k.dtype == torch.float64
    assert tv.last_status is not None and tuple(tv.last_status.shape) == (3,)
    traj, V, v = tv.solve_time_parallel(np.ones((3, 3, 1)), segments=50, want_value=True)       # (clamped by the library)
    a = rec.calls[-1]
    assert a[30] == 50 and a[24] is None and a[26] is not None and V.shape == (3, 6, 3, 3) and v.shape == (3, 6, 3, 1)
    # the default is a valid count; one segment is passed on as 1 (the library forwards to the sequential solve)
    tv.solve_time_parallel(np.ones((3, 3, 1)))
    assert rec.calls[-1][30] == tv.default_segments(3) and 1 <= rec.calls[-1][30] <= 6
    tv.solve_time_parallel(np.ones((3, 3, 1)), segments=1)
    assert rec.calls[-1][30] == 1
    # an unbatched problem: outputs lose the batch axis; a shared model has batch stride 0
    tv1 = TimeVaryingLQR(*_model64(0, 6, 3, 2), device="cpu", dtype=torch.float64)
    out = tv1.solve_time_parallel(np.ones(3), segments=2)
    assert out.states.shape == (7, 3) and rec.calls[-1][0] == 1 and rec.calls[-1][5] == 0
    states, actions, costs = tvlqr_solve_time_parallel(F, f, C, c, np.ones((3, 3, 1)), segments=3)
    assert states.shape == (3, 7, 3, 1) and costs.shape == (3, 7, 1, 1) and rec.calls[-1][30] == 3
    with pytest.raises(ValueError, match="segments"):
        tv.solve_time_parallel(np.ones((3, 3, 1)), segments=0)


def test_default_segments_rule():
    F, f, C, c = (a[:, :1] for a in _model64(1, 1, 3, 2))
    mk = lambda T: TimeVaryingLQR(*(torch.as_tensor(a).expand(1, T, *a.shape[2:]) for a in (F, f, C, c)), device="cpu",     # noqa: E731
                                  dtype=torch.float64, symmetric=True)
    tv = mk(4096)
    assert tv.default_segments(1) == 70                       # sqrt(1.2 T): the device's waves are not the limit
    assert tv.default_segments(64) == 20                      # 5 x 256 compute units' resident waves shared by 64 instances
    assert tv.default_segments(320) == 4
    assert tv.default_segments(640) == 1                      # two segments cost more than the sequential sweep
    assert tv.default_segments(1024) == 1                     # the batch fills the device
    assert mk(512).default_segments(8) == 25
    assert mk(20).default_segments(1) == 1                    # too short to pay for the condense and the stitch
    assert mk(40).default_segments(1) == 7


def test_refusals():
    F, f, C, c = _model64(2, 4, 3, 2)
    x0 = torch.ones(2, 3, 1, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float64"):
        TimeVaryingLQR(F, f, C, c, device="cpu").solve_time_parallel(x0, 2)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float64"):
        tvlqr_solve_time_parallel(F.astype(np.float32), f, C, c, x0, 2)
    Ft = torch.as_tensor(F).requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"solve\(x0, differentiable=True\)"):
        TimeVaryingLQR(Ft, f, C, c, device="cpu", dtype=torch.float64).solve_time_parallel(x0, 2)
    with pytest.raises(NotImplementedError, match=r"solve\(x0, differentiable=True\)"):
        TimeVaryingLQR(F, f, C, c, device="cpu", dtype=torch.float64).solve_time_parallel(x0.clone().requires_grad_(True), 2)
    with pytest.raises(NotImplementedError, match=r"solve\(x0, differentiable=True\)"):
        tvlqr_solve_time_parallel(Ft, f, C, c, x0, 2)
    with torch.no_grad():                                     # nothing records: the refusal does not apply, the missing GPU does
        with pytest.raises(RuntimeError, match="GPU"):
            TimeVaryingLQR(Ft, f, C, c, device="cpu", dtype=torch.float64).solve_time_parallel(x0, 2)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
@pytest.mark.parametrize("source,kernels", [("tvlqr_time_parallel_f64.hip", ("tvlqr_tp_condense_kernel", "tvlqr_tp_stitch_kernel",
                                                                            "tvlqr_tp_finish_kernel")),
                                            ("tvlqr_f64.hip", ("tvlqr_expand_f64_kernel",))])
def test_the_kernels_use_no_scratch_and_the_f64_matrix_cores(source, kernels):
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", source)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    found = [row for row in found if any(k in row[0] for k in kernels)]
    assert len(found) == sum(1 if k == "tvlqr_tp_finish_kernel" else 2 for k in kernels), found      # MAXD 16 and 32
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        body = re.search(r"\n" + re.escape(name) + r":.*?\n(.*?)\n\s*\.amdhsa_kernel\s+" + re.escape(name), text, flags=re.S)
        assert body, name
        assert ("v_mfma_f64_16x16x4" in body.group(1)) == ("finish" not in name), name

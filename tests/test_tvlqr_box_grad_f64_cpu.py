"""Double-precision gradients through the control-limited TV-LQR solve without a GPU: the reference of
tests/test_tvlqr_box_grad_f64_gpu.py (tests/tvlqr_box_grad_f64_ref.py) pinned -- against central differences of an exact
box-QP solve, against the fp64 recursion form where that is usable, against the unconstrained double reference -- the
budget rule shown to separate and to be attainable, the GPU test's cases shown to hold 30 - 70 % of their controls, then
the C ABI, the Python front end's routing against a recorder, and the kernels' resources from the gfx950 assembly."""
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
import tvlqr_box_grad_f64_ref as bg
import tvlqr_f64_ref as ref64
import tvlqr_grad_f64_ref as g64
import tvlqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc import solvers  # noqa: E402

LD = np.longdouble
EXPORTS = ("tfmpc_tvlqr_box_vjp_workspace_bytes_f64", "tfmpc_tvlqr_box_vjp_kernel_name_f64", "tfmpc_tvlqr_box_vjp_f64")
SHAPES = [(5, 3, 6), (3, 5, 6)]
# tvlqr_vjp_f64.hip's kernels by their mangled stems (as in tests/test_tvlqr_grad_f64_cpu.py): the folds, the status OR,
# the costates <LOOP, BOX>, the model's batch sums and the bounds' two
F64_VJP_KERNELS = ("15vjp_fold_kernelE", "19box_fold_f64_kernelE", "20box_status_or_kernelE", "18vjp_costate_kernelILb0ELb0EE",
                   "18vjp_costate_kernelILb1ELb0EE", "18vjp_costate_kernelILb0ELb1EE", "18vjp_costate_kernelILb1ELb1EE",
                   "16vjp_reduce_finalIdE", "16vjp_reduce_stepsIdE", "23vjp_reduce_steps_mfma16IdE", "23vjp_reduce_steps_stage2IdE",
                   "17box_reduce_boundsIdE", "16box_reduce_finalIdE")


def _exact_case(n, m, T, B=4):
    ops, sol = bref.tv_case(n, m, T, B, seed=n + T, width=0.6)
    rng = np.random.default_rng(7)
    g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    cl = sol["clamped"]
    assert (cl & sol["at_low"]).any() and (cl & ~sol["at_low"]).any() and (~cl).any()      # both bounds, and free controls
    return ops, sol, g


def _loss(sol, g):
    return sum(float((np.asarray(sol[k]) * w).sum()) for k, w in zip(("states", "actions", "costs"), g))


# ------------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("n,m,T", SHAPES)
def test_the_reference_is_the_central_difference_of_the_box_solve(n, m, T):
    ops, sol, g = _exact_case(n, m, T)
    B = ops["F"].shape[0]
    got = bg.grads(ops, sol["states"], sol["actions"], sol["clamped"], *g, dtype=LD)
    rng = np.random.default_rng(11)
    eps, checked = 1e-5, 0
    for b in range(B):
        if not sol["clear"][b]:
            continue                     # the active set may move inside the difference step
        checked += 1
        for name in ("F", "f", "C", "c", "x0", "low", "high"):
            for _ in range(3):
                direction = rng.normal(size=ops[name][b].shape)
                if name == "C":
                    direction = 0.5 * (direction + direction.swapaxes(-1, -2))
                vals = []
                for sgn in (1.0, -1.0):
                    p = {k: (None if v is None else v[b]) for k, v in ops.items()}
                    p[name] = p[name] + sgn * eps * direction
                    s = bref.solve_box(p["F"], p["f"], p["C"], p["c"], p["x0"], p["low"], p["high"])
                    assert np.array_equal(s["clamped"], sol["clamped"][b])
                    vals.append(_loss(s, [w[b] for w in g]))
                fd = (vals[0] - vals[1]) / (2 * eps)
                an = float((got[name][b] * direction).sum())
                assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd), abs(an)), (name, b, fd, an)
    assert checked >= 2


@pytest.mark.parametrize("n,m,T", SHAPES)
def test_the_value_form_agrees_with_the_recursion_form_where_that_is_usable(n, m, T):
    ops, sol, g = _exact_case(n, m, T)
    got = bg.grads(ops, sol["states"], sol["actions"], sol["clamped"], *g, dtype=LD)
    want = bref.closed_form(ops["F"], ops["f"], ops["C"], ops["c"], ops["low"], ops["high"], sol["states"], sol["actions"],
                            sol["clamped"], sol["at_low"], None, None, *g)
    assert set(want) == set(got)
    for k in want:
        w = want[k].numpy()
        assert float(np.abs(got[k] - w).max()) <= 1e-9 * max(1.0, float(np.abs(w).max())), k
    # and with its own recursion form, in the same dtype
    rec = bg.grads(ops, sol["states"], sol["actions"], sol["clamped"], *g, dtype=LD, costates="recursion")
    for k in got:
        assert float(np.abs(got[k] - rec[k]).max()) <= 1e-12 * max(1.0, float(np.abs(got[k]).max())), k


@pytest.mark.parametrize("n,m,T", SHAPES)
def test_infinite_bounds_give_the_unconstrained_double_reference(n, m, T):
    ops, _, g = _exact_case(n, m, T)
    for b in range(2):
        args = (ops["F"][b], ops["f"][b], ops["C"][b], ops["c"][b])
        fwd = ref64.solve_ld(*args, ops["x0"][b])
        want = g64.closed_form(*args, ops["x0"][b], None, None, *(w[b] for w in g), dtype=LD)
        none = np.zeros((T, m), bool)
        got = bg.closed_form(*args, -np.inf, fwd["states"], fwd["actions"], none, None, None, *(w[b] for w in g), dtype=LD)
        assert not got["low"].any() and not got["high"].any()
        for k in want:
            assert float(np.abs(got[k] - want[k]).max()) <= 1e-15 * max(1.0, float(np.abs(want[k]).max())), k


# ------------------------------------------------------------------------- the rule
def _unscaled20():
    full, _, states, actions, held = bg.unscaled_case(T=20)
    assert 0.3 <= held.mean() <= 0.7
    w = bg.weights(actions.shape[0], states.shape[2], actions.shape[2], 20, "mixed")
    return full, states, actions, held, w, bg.references(full, states, actions, held, *w)


def test_the_rule_separates_the_recursion_form_from_the_value_form():
    """Unscaled (16, 8), T = 20, about half of the controls held: the RECURSION form in fp64 misses the budget by more than
    1e4 on every gradient that a costate enters -- in the rule's own two statistics, the median over instances against
    2.5 and the worst instance against 10."""
    full, states, actions, held, w, refs = _unscaled20()
    rec = bg.grads(full, states, actions, held, *w, dtype=np.float64, costates="recursion")
    for k in ("F", "f", "x0", "low", "high"):
        r = bg.ratios(rec[k], refs, k)
        print(f"recursion form in fp64, unscaled T = 20, d{k}: median {np.median(r):.3g} min {r.min():.3g} max {r.max():.3g}")
        assert np.median(r) > 1e4 * g64.MEDIAN_BOUND and r.max() > 1e4 * g64.MAX_BOUND, (k, r)


def test_the_rule_is_attainable_in_another_summation_order():
    full, states, actions, held, w, refs = _unscaled20()
    rev = bg.grads(full, states, actions, held, *w, dtype=np.float64, reverse=True)
    for k in rev:
        r = bg.ratios(rev[k], refs, k)
        print(f"value form in fp64, reversed sums, unscaled T = 20, d{k}: median {np.median(r):.3g} max {r.max():.3g}")
        assert np.median(r) <= 2.5 and r.max() <= 10.0, (k, r)


# ------------------------------------------------------------------------- the GPU test's cases are sound
def _both(held):
    """Every control is held at some step and free at some step."""
    h = held.reshape(-1, held.shape[-1])
    return h.any(0).all() and (~h).any(0).all()


@pytest.mark.parametrize("kw", bg.gpu_cases(), ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k not in ("shared", "const")))
def test_gpu_cases_hold_30_to_70_percent_of_their_controls(kw):
    full, user, states, actions, held = bg.forward_case(**kw)
    assert 0.3 <= held.mean() <= 0.7 and _both(held), held.mean()
    for k in ("F", "f", "C", "c", "x0", "low", "high"):                       # no fp32 numbers
        assert (full[k] != full[k].astype(np.float32)).mean() > 0.9, k
    at_low = held & (actions == full["low"])
    if held.size >= 16:
        assert at_low.any() and (held & ~at_low).any()                         # both bounds


def test_the_other_gpu_cases():
    for kw in bg.ALL_HELD:
        assert bg.forward_case(**kw)[4].all()
    for kw in bg.NONE_HELD:
        assert not bg.forward_case(**kw)[4].any()
    # the rescued class of the issue, (1.35, 0.02): every control is held -- the 30 - 70 % cannot hold there
    import tvlqr_box_f64_ref as dref
    ops, _, r64, _ = dref.rescued(*dref.RESCUED[0])
    assert dref.held_from_actions(r64["actions"].astype(np.float64), ops["low"], ops["high"]).all()
    ops, _, r64, _ = dref.rescued(*dref.RESCUED[1])
    h = dref.held_from_actions(r64["actions"].astype(np.float64), ops["low"], ops["high"]).reshape(6, -1)
    assert (h.any(1) & ~h.all(1)).any()
    held = bg.unscaled_case()[4]
    assert 0.3 <= held.mean() <= 0.7 and _both(held), held.mean()
    # the gradcheck case: no difference step moves the held set
    full, _, _, actions, held = bg.forward_case(**bg.GRADCHECK)
    sol = bref.solve_box_batch(full["F"], full["f"], full["C"], full["c"], full["x0"], full["low"], full["high"])
    assert np.array_equal(sol["clamped"], held) and sol["multiplier"].min() > 1e-2 and sol["slack"].min() > 1e-2
    assert float(np.abs(sol["actions"] - actions).max()) <= 1e-10


# ------------------------------------------------------------------------- the feature: ABI
def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    f32, f64 = (_hip._SIGNATURES["tfmpc_tvlqr_box_vjp_" + s] for s in ("f32", "f64"))
    assert f64[0] == f32[0] and len(f64[1]) == len(f32[1]) and all(a is b for a, b in zip(f32[1], f64[1]))
    for s in ("workspace_bytes", "kernel_name"):
        assert _hip._SIGNATURES[f"tfmpc_tvlqr_box_vjp_{s}_f64"] == _hip._SIGNATURES[f"tfmpc_tvlqr_box_vjp_{s}"]


def test_kernel_name_and_workspace_per_shape():
    lib = _hip.load()
    name = lambda n, m: lib.tfmpc_tvlqr_box_vjp_kernel_name_f64(n, m, 50).decode()      # noqa: E731
    assert name(16, 8) == name(16, 16) == name(1, 1) == "tv_masked_f64_wave16"
    assert name(17, 8) == name(16, 17) == name(32, 32) == name(8, 32) == "tv_masked_f64_wave32"
    assert name(33, 8) == name(8, 33) == name(200, 8) == "unsupported" and name(0, 3) == name(3, 0) == "invalid"
    ws = lib.tfmpc_tvlqr_box_vjp_workspace_bytes_f64
    up = lambda x: (x + 63) // 64 * 64                                                 # noqa: E731
    B, n, m, T = 3, 5, 3, 7
    extra = up((B * T + 1) // 2) + up((B + 1) // 2) + 3 * up(B * T * m) + 2 * up(B * T * n) + up(B * T * (n + m))
    assert ws(B, n, m, T) == lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(B, n, m, T) + 8 * extra
    assert ws(0, 16, 8, 50) == 0 and ws(-1, 16, 8, 50) == 0 and ws(2, 0, 8, 50) == 0
    for B in (1, 2, 255, 256, 257, 1000):                                              # monotone in B and in T
        assert ws(B, 16, 8, 50) <= ws(B + 1, 16, 8, 50) and ws(B, 16, 8, 50) <= ws(B, 16, 8, 51)
    assert ws(1, 16, 8, 50) < ws(65, 16, 8, 50) < ws(257, 16, 8, 50) and ws(4, 16, 8, 1) < ws(4, 16, 8, 50)


def test_abi_argument_errors_return_before_any_launch():
    """tests/test_lqr_box_grad_cpu.py's checks, in the fp32 entry point's order, against the double one."""
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4, dtype=torch.float64))

    def call(B=1, n=3, m=2, T=4, s=0, F=p, f=p, Cfin=None, cfin=None, low=p, high=p, sl=0, states=p, actions=p, dCfin=None, sd=0,
             sdl=0, status=p, ws=p, ws_bytes=1 << 24):
        return lib.tfmpc_tvlqr_box_vjp_f64(B, n, m, T, F, s, s, f, s, s, p, s, s, p, s, s, Cfin, 0, cfin, 0, low, sl, sl, high, sl, sl,
                                           states, actions, None, None, None, p, sd, sd, p, sd, sd, p, sd, sd, p, sd, sd, dCfin, 0,
                                           None, 0, p, sd, p, sdl, sdl, p, sdl, sdl, None, status, ws, ws_bytes, None)

    assert call(B=-1) == -1 and call(n=0) == -1 and call(m=0) == -1 and call(T=0) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(states=None) == -1 and call(actions=None) == -1 and call(status=None) == -1
    assert call(Cfin=p) == -1 and call(cfin=p) == -1 and call(dCfin=p) == -1      # both or neither; no dCfin without Cfin
    assert call(low=None) == -1 and call(high=None) == -1
    assert call(s=-3) == -1 and call(sl=-1) == -1 and call(sd=-2) == -1 and call(sdl=-1) == -1
    assert call(n=33, m=8) == -2 and call(n=8, m=33) == -2 and call(B=0, m=33) == -2 and call(T=65536) == -2
    assert call(ws=None) == -4 and call(ws_bytes=lib.tfmpc_tvlqr_box_vjp_workspace_bytes_f64(1, 3, 2, 4) - 1) == -4
    assert call(B=0, F=None, f=None, low=None, high=None, states=None, actions=None, status=None, ws=None) == 0      # a no-op
    assert call(B=-1, m=33) == -1 and call(m=33, ws=None) == -2 and call(F=None, ws=None) == -1      # argument, shape, workspace


# ------------------------------------------------------------------------- the feature: Python
class _Recorder:
    """Stands in for the library: keeps the launch's symbol and arguments, returns TFMPC_OK."""

    def __init__(self):
        self.calls = []

    def tfmpc_tvlqr_box_vjp_workspace_bytes(self, B, n, m, T):
        return 4 * 1024

    def tfmpc_tvlqr_box_vjp_workspace_bytes_f64(self, B, n, m, T):
        return 8 * 1024

    def tfmpc_tvlqr_box_solve_workspace_bytes(self, B, n, m, T):
        return 4 * 1024

    def tfmpc_tvlqr_box_solve_workspace_bytes_f64(self, B, n, m, T):
        return 8 * 1024

    def _record(name):                                                                   # noqa: N805
        def method(self, *args):
            self.calls.append((name, args))
            return 0
        return method

    tfmpc_tvlqr_box_vjp_f32 = _record("vjp_f32")
    tfmpc_tvlqr_box_vjp_f64 = _record("vjp_f64")
    tfmpc_tvlqr_box_solve_f32 = _record("solve_f32")
    tfmpc_tvlqr_box_solve_f64 = _record("solve_f64")


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


def test_float64_reaches_the_double_symbol_with_the_callers_doubles(recorder):
    B, T, n, m = 3, 4, 3, 2
    d = n + m
    F, f, C, c, _ = _problem(B, T, n, m)
    low, high = -torch.ones(B, T, m, dtype=torch.float64), torch.ones(m, dtype=torch.float64)
    states, actions = torch.zeros(B, T + 1, n, dtype=torch.float64), torch.zeros(B, T, m, dtype=torch.float64)
    gx = torch.ones(B, T + 1, n, dtype=torch.float64)
    got = solvers.tvlqr_box_vjp(F, f, C, c, low, high, states, actions, gx, dtype=torch.float64)
    sym, a = recorder.calls[-1]
    assert sym == "vjp_f64" and a[:4] == (B, n, m, T)
    assert _value(a[4]) == F.data_ptr() and a[5:7] == (T * n * d, n * d)              # the caller's doubles: no copy, ELEMENT strides
    assert _value(a[7]) == f.data_ptr() and _value(a[10]) == C.data_ptr() and _value(a[13]) == c.data_ptr()
    assert a[16] is None and a[18] is None
    assert _value(a[20]) == low.data_ptr() and a[21:23] == (T * m, m) and _value(a[23]) == high.data_ptr() and a[24:26] == (0, 0)
    assert _value(a[26]) == states.data_ptr() and _value(a[27]) == actions.data_ptr() and _value(a[28]) == gx.data_ptr()
    assert a[29] is None and a[30] is None
    assert a[-2] >= 8 * 1024
    for k in ("F", "f", "C", "c", "x0", "low", "high"):
        assert got[k].dtype == torch.float64, k
    assert got["F"].shape == F.shape and got["low"].shape == low.shape and got["high"].shape == (1, m) and got["x0"].shape == (B, n)
    assert got["clamped"].shape == (B, T, m) and got["status"].shape == (B,)
    # numpy and fp32 operands are taken to double
    got = solvers.tvlqr_box_vjp(F.numpy(), f.float(), C, c, -1.0, 1.0, states, actions, gx, dtype=torch.float64)
    assert recorder.calls[-1][0] == "vjp_f64" and got["F"].dtype == torch.float64
    for bad in (torch.float16, "float64", np.float64):
        with pytest.raises(ValueError, match="dtype"):
            solvers.tvlqr_box_vjp(F, f, C, c, low, high, states, actions, gx, dtype=bad)


def test_the_default_dtype_still_reaches_the_fp32_symbol(recorder):
    F, f, C, c, _ = _problem()
    states, actions = torch.zeros(3, 5, 3, dtype=torch.float64), torch.zeros(3, 4, 2, dtype=torch.float64)
    for kw in ({}, dict(dtype=None), dict(dtype=torch.float32)):
        got = solvers.tvlqr_box_vjp(F, f, C, c, -1.0, 1.0, states, actions, **kw)     # fp64 inputs: cast to fp32, as before
        sym, a = recorder.calls[-1]
        assert sym == "vjp_f32" and got["F"].dtype == torch.float32 and _value(a[4]) != F.data_ptr() and a[-2] >= 4 * 1024


def test_differentiable_puts_the_double_result_in_the_graph(recorder):
    F, f, C, c, x0 = _problem()
    F.requires_grad_()
    low = torch.full((2,), -1.0, dtype=torch.float64, requires_grad=True)
    out = solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0, dtype=torch.float64, differentiable=True)
    assert recorder.calls[-1][0] == "solve_f64" and _value(recorder.calls[-1][1][4]) == F.data_ptr()
    assert all(t.dtype == torch.float64 and t.requires_grad for t in out)
    (out[0].sum() + out[2].sum()).backward()
    sym, a = recorder.calls[-1]
    assert sym == "vjp_f64" and _value(a[4]) == F.data_ptr()
    assert F.grad.dtype == torch.float64 and F.grad.shape == F.shape and low.grad.shape == low.shape
    assert f.grad is None and out.info.last_grad_status is not None
    # nothing requires grad: a plain solve, flag or no flag
    n_calls = len(recorder.calls)
    out = solvers.tvlqr_box_solve(F.detach(), f, C, c, x0, -1.0, 1.0, dtype=torch.float64, differentiable=True)
    assert not out[0].requires_grad and len(recorder.calls) == n_calls + 1 and recorder.calls[-1][0] == "solve_f64"


def test_without_the_flag_the_refusal_stays_and_fp32_ignores_the_flag(recorder):
    F, f, C, c, x0 = _problem()
    low = torch.full((2,), -1.0, dtype=torch.float64, requires_grad=True)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32") as info:
        solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0, dtype=torch.float64)
    assert "differentiable=True" in str(info.value) and not recorder.calls
    for flag in (False, True):
        out = solvers.tvlqr_box_solve(F, f, C, c, x0, low, 1.0, differentiable=flag)
        assert recorder.calls[-1][0] == "solve_f32" and all(t.dtype == torch.float32 and t.requires_grad for t in out)
        out[0].sum().backward()
        assert recorder.calls[-1][0] == "vjp_f32"


# ------------------------------------------------------------------------- the feature: resources
def _assembly(source):
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", source)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M))
    bodies = {name: re.search(r"^" + re.escape(name) + r":.*?\n(.*?)^\s*\.amdhsa_kernel\s+" + re.escape(name), text, flags=re.S | re.M).group(1)
              for name, *_ in found}
    return found, bodies


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_new_kernels_use_no_scratch_and_fit_the_register_file():
    found, bodies = _assembly("tvlqr_vjp_f64.hip")
    assert len(found) == len(F64_VJP_KERNELS), found
    for stem in F64_VJP_KERNELS:          # exactly this set: the file holds the plain and the control-limited VJP
        assert sum(stem in name for name, *_ in found) == 1, (stem, found)
    assert sum("vjp_" in name for name, *_ in found) == 9 and sum("box_" in name for name, *_ in found) == 4, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        assert "v_mfma_f32" not in bodies[name], name
        assert ("v_mfma_f64_16x16x4" in bodies[name]) == ("mfma16" in name), name
    found, bodies = _assembly("tvlqr_f64.hip")
    masked = [row for row in found if "tvlqr_masked_f64_sweep" in row[0]]
    assert len(masked) == 4, found       # {wave16, wave32} x {solve, backward only}
    for name, private, vgprs, spills in masked:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        assert "v_mfma_f64_16x16x4_f64" in bodies[name] and "v_mfma_f32" not in bodies[name], name

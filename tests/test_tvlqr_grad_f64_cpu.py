"""Gradients of the double-precision time-varying LQR without a GPU: the value-function costates against §3.8's recursion
in 80-bit, the fp64 restatement under the budget rule, the instability of the recursion on unscaled models (why the
kernel is not a type swap of tvlqr_vjp.hip), the C ABI (declarations, bindings, argument errors), the register budget of
the kernels and the Python opt-in."""
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
import tvlqr_grad_ref as gref
import tvlqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402

LD = np.longdouble
EXPORTS = ("tfmpc_tvlqr_vjp_workspace_bytes_f64", "tfmpc_tvlqr_vjp_f64")
LOSSES = ("states", "actions", "costs", "mixed")
SCALED = [(3, 2, 1), (4, 3, 2), (5, 2, 9), (16, 8, 8)]
# tvlqr_vjp_f64.hip's kernels by their mangled stems: the folds, the status OR, the costates <LOOP, BOX>, the model's batch
# sums (final records, per step scalar and matrix-core, stage 2) and the bounds' two
F64_VJP_KERNELS = ("15vjp_fold_kernelE", "19box_fold_f64_kernelE", "20box_status_or_kernelE", "18vjp_costate_kernelILb0ELb0EE",
                   "18vjp_costate_kernelILb1ELb0EE", "18vjp_costate_kernelILb0ELb1EE", "18vjp_costate_kernelILb1ELb1EE",
                   "16vjp_reduce_finalIdE", "16vjp_reduce_stepsIdE", "23vjp_reduce_steps_mfma16IdE", "23vjp_reduce_steps_stage2IdE",
                   "17box_reduce_boundsIdE", "16box_reduce_finalIdE")


def _problem(n, m, T, B, final, seed=0, loss="mixed", unscaled=False):
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = make(n, m, T, B, seed=seed)
    Cf, cf = tvlqr_ref.make_final(n, B) if final else (None, None)
    x0 = tvlqr_ref.make_x0(n, B)
    rng = np.random.default_rng(seed + 5)
    g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    g = tuple(a if loss in (name, "mixed") else None for a, name in zip(g, LOSSES))
    return (F, f, C, c, x0, Cf, cf) + g


_REFS = {}


def _refs(*key):
    """The three references of a seeded problem, computed once."""
    if key not in _REFS:
        _REFS[key] = (_problem(*key), g64.references(*_problem(*key)))
    return _REFS[key]


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n,m,T", SCALED)
def test_value_function_costates_are_the_recursions_in_80_bit(n, m, T, final, loss):
    ops, (rld, _, _) = _refs(n, m, T, 2, final, n * 10 + T, loss)
    rec = g64.grads(*ops, dtype=LD, costates="recursion")
    assert set(rec) == set(rld) == {"F", "f", "C", "c", "x0"} | ({"Cfin", "cfin"} if final else set())
    for k in rld:
        assert rld[k].dtype == LD and rec[k].shape == rld[k].shape, k
        scale = max(1.0, float(np.abs(rld[k]).max()))
        assert float(np.abs(rec[k] - rld[k]).max()) <= 1e-15 * scale, (k, float(np.abs(rec[k] - rld[k]).max()), scale)


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("n,m,T", SCALED)
def test_fp64_restatement_is_fp64_autograd_within_the_rule(n, m, T, final, loss):
    """Under the rule both fp64 restatements are in the budget, so each passes it by construction (checked: the plumbing
    of ``check``).  What is pinned beyond that: they agree -- the error of each against 80-bit is at most 10 x
    max(the other's, the floor) in every instance."""
    _, refs = _refs(n, m, T, 2, final, n * 10 + T, loss)
    g64.check(refs[1], refs, what=("fp64 value form", n, m, T))
    g64.check(refs[2], refs, what=("fp64 autograd", n, m, T))
    _, (rld, r64, auto) = _refs(n, m, T, 2, final, n * 10 + T, loss)
    for k in rld:
        for b in range(2):
            floor = g64.FLOOR * max(1.0, float(np.abs(rld[k][b]).max()))
            ea, eb = g64._err(r64[k][b], rld[k][b]), g64._err(auto[k][b], rld[k][b])
            assert ea <= g64.MAX_BOUND * max(eb, floor) and eb <= g64.MAX_BOUND * max(ea, floor), (k, b, ea, eb, floor)


@pytest.mark.parametrize("T", [20, 50])
def test_unscaled_models_the_value_function_form_holds_and_the_recursion_does_not(T):
    """Why the kernel is not a type swap of tvlqr_vjp.hip.  Measured at T = 20: recursion 5e-2 against a budget of 1e-10."""
    key = (16, 8, T, 4, False, 0, "mixed", True)
    ops, refs = _refs(*key)
    g64.check(refs[1], refs, what=("unscaled fp64 value form", T))
    rec = gref.closed_form(*ops, dtype=torch.float64)
    for k in ("F", "f", "x0"):
        budgets = g64.term_budgets(refs, k)
        errs = np.array([g64._err(rec[k][b].numpy(), refs[0][k][b]) for b in range(4)])
        print(f"unscaled T={T} fp64 recursion d{k}: error {errs.max():.3g}, budget {budgets.max():.3g}, ratio {(errs / budgets).min():.3g}")
        if T == 20:
            assert (errs >= 1e6 * budgets).all(), (k, errs, budgets)


@pytest.mark.parametrize("key", [(16, 8, 8, 2, False, 168, "mixed"), (5, 2, 9, 2, True, 59, "mixed"),
                                 (16, 8, 20, 4, False, 0, "mixed", True), (16, 8, 50, 4, False, 0, "mixed", True)])
def test_the_rule_is_attainable_in_another_summation_order(key):
    ops, refs = _refs(*key)
    got = g64.grads(*ops, dtype=np.float64, reverse=True)
    assert any(not np.array_equal(got[k], refs[1][k]) for k in got)         # not the restatement itself
    g64.check(got, refs, what=("reversed sums", key[:3]))


def test_every_new_export_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert hasattr(lib, name), name
    assert "There are no f64 gradient calls" not in header
    # the f32 call's arguments and v
    assert len(_hip._SIGNATURES["tfmpc_tvlqr_vjp_f64"][1]) == len(_hip._SIGNATURES["tfmpc_tvlqr_vjp_f32"][1]) + 1
    decl = re.search(r"int tfmpc_tvlqr_vjp_f64\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_hip._SIGNATURES["tfmpc_tvlqr_vjp_f64"][1])


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    buf = torch.zeros(4, dtype=torch.float64)
    p = _hip.ptr(buf)

    def call(B, n, m, T, s=0, model_null=None, cfin=None, outs_fin=False, status=True, ws=True, ws_bytes=None, so=0, v=True):
        model = [p, s, s] * 4 + [None, 0, None, 0]
        if model_null is not None:
            model[model_null] = None
        if cfin:
            model[12], model[14] = p, p
        outs = [p, so, so] * 4 + [p if outs_fin else None, 0, p if outs_fin else None, 0, p, 0]
        nbytes = ws_bytes if ws_bytes is not None else 1 << 40
        return lib.tfmpc_tvlqr_vjp_f64(B, n, m, T, *model, p, p, p if v else None, None, None, None, *outs,
                                       p if status else None, p if ws else None, nbytes, None)

    assert call(1, 3, 2, 0) == -1                     # T >= 1
    assert call(1, 0, 2, 4) == -1
    assert call(-1, 3, 2, 4) == -1
    assert call(1, 3, 2, 4, s=-1) == -1               # negative model stride
    assert call(1, 3, 2, 4, so=-1) == -1              # negative output stride
    assert call(1, 3, 2, 4, model_null=0) == -1       # F NULL
    assert call(1, 3, 2, 4, outs_fin=True) == -1      # final-cost gradients without an explicit final cost
    assert call(1, 3, 2, 4, status=False) == -1
    assert call(1, 3, 2, 4, v=False) == -1            # the forward's v is required
    assert call(1, 200, 200, 4) == -2                 # beyond the f64 solve
    assert call(1, 33, 2, 4) == -2 and call(1, 2, 33, 4) == -2
    assert call(1, 3, 2, 4, ws=False) == -4
    assert call(1, 3, 2, 4, ws_bytes=16) == -4
    assert call(0, 3, 2, 4, status=False, ws=False, v=False) == 0     # B == 0: no-op
    assert lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(0, 3, 2, 4) == 0
    # the header's formula
    up = lambda x: (x + 63) // 64 * 64            # noqa: E731
    B, n, m, T = 300, 16, 8, 50
    d, chunks = n + m, 2
    doubles = (up(B * T * d) + 2 * up(B * n) + up(B * n * n) + up(B * (T + 1) * n) + up(B * T * m) + up(B * (T + 1))
               + up(B * T * m * (n + 1)) + up(B * T * n * n) + up(B * T * n) + up(2 * B * T * n)
               + up(chunks * T * (n * d + n + d * d + d)))
    assert lib.tfmpc_tvlqr_vjp_workspace_bytes_f64(B, n, m, T) == 8 * doubles


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_f64_vjp_kernels_use_no_scratch_and_the_f64_matrix_cores():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_vjp_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)) == len(found) == len(F64_VJP_KERNELS), found
    for stem in F64_VJP_KERNELS:          # exactly this set: the file holds the plain and the control-limited VJP
        assert sum(stem in name for name, *_ in found) == 1, (stem, found)
    assert sum("vjp_" in name for name, *_ in found) == 9 and sum("box_" in name for name, *_ in found) == 4, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        body = re.search(r"\n" + re.escape(name) + r":.*?\n(.*?)\n\s*\.amdhsa_kernel\s+" + re.escape(name), text, flags=re.S)
        assert body, name
        assert "v_mfma_f32" not in body.group(1), name
        assert ("v_mfma_f64_16x16x4" in body.group(1)) == ("mfma16" in name), name


def _double_problem(requires_grad):
    F, f, C, c = (torch.as_tensor(a, dtype=torch.float64) for a in tvlqr_ref.make_models(3, 2, 4, 2, seed=3))
    F.requires_grad_(requires_grad)
    return F, f, C, c, torch.ones(2, 3, 1, dtype=torch.float64)


def test_the_opt_in_reaches_the_gpu_and_the_refusal_stays_without_it():
    from tfmpc.solvers import TimeVaryingLQR, tvlqr_solve
    F, f, C, c, x0 = _double_problem(True)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu", dtype=torch.float64)
    for call in (tv.solve, tv.solve_tensors):
        with pytest.raises(NotImplementedError, match=r"differentiable=True.*dtype=torch\.float32"):
            call(x0)
        with pytest.raises(RuntimeError, match="GPU"):
            call(x0, differentiable=True)
    with pytest.raises(RuntimeError, match="GPU"):
        tvlqr_solve(F, f, C, c, x0, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match=r"dtype=torch\.float32"):
        tv.backward(differentiable=True)                      # the Riccati gradients stay fp32
    with pytest.raises(ValueError, match="dtype"):
        tvlqr_solve(F, f, C, c, x0, dtype=torch.float16)


def test_the_flag_changes_nothing_for_fp32_problems():
    from tfmpc.solvers import TimeVaryingLQR
    F, f, C, c, x0 = _double_problem(True)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu")
    assert tv.dtype == torch.float32
    for flag in (False, True):
        with pytest.raises(RuntimeError, match="GPU"):
            tv.solve_tensors(x0, differentiable=flag)

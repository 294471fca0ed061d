"""Gradients of the control-limited LQR without a GPU: the fp64 closed form (tests/lqr_box_grad_ref.py) against central
differences of an exact box-QP solve, its unconstrained limit, the held-set statistics of the workloads the GPU tests use,
the C ABI of tfmpc_tvlqr_box_vjp_f32 and the register budget of its kernels."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import lqr_box_grad_ref as bref
import tvlqr_grad_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402

BOX_EXPORTS = ("tfmpc_tvlqr_box_vjp_workspace_bytes", "tfmpc_tvlqr_box_vjp_kernel_name", "tfmpc_tvlqr_box_vjp_f32")
GPU_TV_SHAPES = [(16, 8), (5, 3), (12, 6), (20, 10)]
GPU_TV_HORIZONS = [1, 2, 50]
GPU_TV_BATCH = 8


def tv_final(T):
    """The GPU tests' time-varying cases: an explicit final cost at T = 2, the default one at T = 1 and T = 50."""
    return T == 2


def _loss(sol, g):
    return sum(float((np.asarray(sol[k]) * w).sum()) for k, w in zip(("states", "actions", "costs"), g))


@pytest.mark.parametrize("n,m,T,final", [(4, 2, 12, True), (2, 3, 2, False), (3, 2, 1, False), (2, 3, 12, False), (4, 2, 2, True)])
def test_closed_form_is_the_central_difference_of_the_box_solve(n, m, T, final):
    B = 4
    ops, sol = bref.tv_case(n, m, T, B, final=final, seed=n + T, width=0.6)
    rng = np.random.default_rng(7)
    g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    cl = sol["clamped"]
    assert (cl & sol["at_low"]).any() and (cl & ~sol["at_low"]).any() and (~cl).any()      # both bounds, and free controls
    got = bref.closed_form(ops["F"], ops["f"], ops["C"], ops["c"], ops["low"], ops["high"], sol["states"], sol["actions"],
                           cl, sol["at_low"], ops["Cfin"], ops["cfin"], *g)
    names = ["F", "f", "C", "c", "x0", "low", "high"] + (["Cfin", "cfin"] if final else [])
    eps = 1e-5
    checked = 0
    for b in range(B):
        if not sol["clear"][b]:
            continue                     # the active set may move inside the difference step
        checked += 1
        for name in names:
            for _ in range(3):
                direction = rng.normal(size=ops[name][b].shape)
                if name in ("C", "Cfin"):
                    direction = 0.5 * (direction + np.swapaxes(direction, -1, -2))
                vals = []
                for sgn in (1.0, -1.0):
                    p = {k: (None if v is None else v[b]) for k, v in ops.items()}
                    p[name] = p[name] + sgn * eps * direction
                    s = bref.solve_box(p["F"], p["f"], p["C"], p["c"], p["x0"], p["low"], p["high"], p["Cfin"], p["cfin"])
                    assert np.array_equal(s["clamped"], cl[b])
                    vals.append(_loss(s, [w[b] for w in g]))
                fd = (vals[0] - vals[1]) / (2 * eps)
                an = float((got[name][b].numpy() * direction).sum())
                assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd), abs(an)), (name, b, fd, an)
    assert checked >= 2


@pytest.mark.parametrize("n,m,T,final", [(4, 2, 6, True), (3, 4, 3, False)])
def test_infinite_bounds_give_the_unconstrained_closed_form(n, m, T, final):
    B = 3
    ops, _ = bref.tv_case(n, m, T, B, final=final)
    rng = np.random.default_rng(3)
    g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    t64 = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    want = gref.closed_form(ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["Cfin"], ops["cfin"], *g)
    xs, us, _ = gref.solve(*(t64(ops[k]) for k in ("F", "f", "C", "c", "x0")), t64(ops["Cfin"]), t64(ops["cfin"]))
    none = np.zeros((B, T, m), bool)
    got = bref.closed_form(ops["F"], ops["f"], ops["C"], ops["c"], -np.inf, np.inf, xs, us, none, none, ops["Cfin"], ops["cfin"], *g)
    assert float(got["low"].abs().max()) == 0.0 and float(got["high"].abs().max()) == 0.0
    for k in want:
        assert float((want[k] - got[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max())), k


@pytest.mark.parametrize("n,m,T", [(16, 8, 50), (5, 3, 20)])
def test_the_end_to_end_workload_has_mixed_and_clear_instances(n, m, T):
    F, f, C, c, x0, lo, hi = bref.workload_numbers(32, n, m)
    sol = bref.solve_box_batch(*(bref.tile_time(a, T) for a in (F, f, C, c)), x0, lo, hi)
    assert bref.mixed(sol).mean() >= 0.75 and sol["clear"].mean() >= 0.75, (bref.mixed(sol).mean(), sol["clear"].mean())


@pytest.mark.parametrize("T", GPU_TV_HORIZONS)
@pytest.mark.parametrize("n,m", GPU_TV_SHAPES)
def test_the_time_varying_workload_has_mixed_and_clear_instances(n, m, T):
    _, sol = bref.tv_case(n, m, T, GPU_TV_BATCH, final=tv_final(T))      # the cases of tests/test_lqr_box_grad_gpu.py
    assert bref.mixed(sol).mean() >= 0.75 and sol["clear"].mean() >= 0.75, (bref.mixed(sol).mean(), sol["clear"].mean())


def test_every_new_export_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in BOX_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert hasattr(lib, name), name
    # the VJP's arguments + low high (pointer, two strides each) + dlow dhigh (likewise) + clamp_mask
    assert len(_hip._SIGNATURES["tfmpc_tvlqr_box_vjp_f32"][1]) == len(_hip._SIGNATURES["tfmpc_tvlqr_vjp_f32"][1]) + 6 + 6 + 1
    assert lib.tfmpc_version() == 320
    from tfmpc.solvers import box_lqr_solve, tvlqr_box_vjp  # noqa: F401


def test_kernel_names_and_workspace():
    lib = _hip.load()
    name = lambda n, m: lib.tfmpc_tvlqr_box_vjp_kernel_name(n, m, 10).decode()      # noqa: E731
    assert name(16, 8) == "tv_masked_16x8"
    assert name(5, 3) == name(16, 1) == "tv_masked_16x8 (zero-padded)"
    assert name(20, 10) == name(12, 9) == "tv_masked_generic_wave"
    assert name(200, 200) == "unsupported"            # beyond one wave's LDS
    assert name(8, 33) == "unsupported"               # one 32-bit held-set word per step
    assert name(0, 3) == "invalid"
    for B, n, m, T in ((65536, 16, 8, 50), (1, 16, 8, 1), (64, 5, 3, 20), (7, 20, 10, 50), (3, 2, 1, 1)):
        extra = lib.tfmpc_tvlqr_box_vjp_workspace_bytes(B, n, m, T) - lib.tfmpc_tvlqr_vjp_workspace_bytes(B, n, m, T)
        assert 0 < extra <= B * T * (4 + 8 * m) + 4096, (B, n, m, T, extra)      # no masked copy of the model
    assert lib.tfmpc_tvlqr_box_vjp_workspace_bytes(0, 3, 2, 4) == 0


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    buf = torch.zeros(4)
    p = _hip.ptr(buf)

    def call(B, n, m, T, s=0, model_null=None, low=True, high=True, sb=0, outs_fin=False, status=True, ws=True, ws_bytes=None, so=0):
        model = [p, s, s] * 4 + [None, 0, None, 0]
        if model_null is not None:
            model[model_null] = None
        bounds = [p if low else None, sb, sb, p if high else None, sb, sb]
        outs = [p, 0, 0] * 4 + [p if outs_fin else None, 0, p if outs_fin else None, 0, p, 0] + [p, so, so, p, so, so]
        nbytes = ws_bytes if ws_bytes is not None else 1 << 40
        return lib.tfmpc_tvlqr_box_vjp_f32(B, n, m, T, *model, *bounds, p, p, None, None, None, *outs, None,
                                           p if status else None, p if ws else None, nbytes, None)

    assert call(1, 3, 2, 0) == -1
    assert call(1, 0, 2, 4) == -1
    assert call(-1, 3, 2, 4) == -1
    assert call(1, 3, 2, 4, s=-1) == -1
    assert call(1, 3, 2, 4, sb=-1) == -1              # negative bound stride
    assert call(1, 3, 2, 4, so=-1) == -1              # negative bound-gradient stride
    assert call(1, 3, 2, 4, model_null=0) == -1
    assert call(1, 3, 2, 4, low=False) == -1
    assert call(1, 3, 2, 4, high=False) == -1
    assert call(1, 3, 2, 4, outs_fin=True) == -1
    assert call(1, 3, 2, 4, status=False) == -1
    assert call(1, 200, 200, 4) == -2
    assert call(1, 8, 33, 4) == -2                    # more than 32 controls
    assert call(1, 3, 2, 4, ws=False) == -4
    assert call(1, 3, 2, 4, ws_bytes=lib.tfmpc_tvlqr_vjp_workspace_bytes(1, 3, 2, 4)) == -4     # the plain VJP's size is too small
    assert call(0, 3, 2, 4, status=False, ws=False, low=False) == 0      # B == 0: no-op


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
@pytest.mark.parametrize("src,pattern,count", [("tvlqr_vjp.hip", r"box_\w+", 4), ("tvlqr_mfma16x8.hip", r"tvlqr_masked16x8_sweep", 4),
                                               ("tvlqr_generic.hip", r"tvlqr_generic_masked_sweep", 1)])
def test_the_new_kernels_use_no_scratch(src, pattern, count):
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*" + pattern + r"\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == count, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
        if "tvlqr_masked16x8_sweepILb1E" in name:      # the exact shape keeps four waves per SIMD
            assert int(vgprs) <= 128, (name, vgprs)


def test_box_lqr_solve_names_its_limits():
    from tfmpc.solvers import box_lqr_solve
    F, f, C, c, x0, lo, hi = bref.workload_numbers(2, 3, 2)
    with pytest.raises(ValueError, match="time-invariant"):
        box_lqr_solve(bref.tile_time(F, 4), f, C, c, x0, lo, hi, 4)
    with pytest.raises(ValueError, match="shared by the batch"):
        box_lqr_solve(F, f, C, c, x0, np.full((2, 2), -0.5), hi, 4)
    with pytest.raises(ValueError, match="finite"):
        box_lqr_solve(F, f, C, c, x0, -np.inf, hi, 4)

"""Gradients of the periodic infinite-horizon LQR in double (tfmpc_tvlqr_periodic_vjp_f64) without a GPU:
the numpy restatement of tests/tvlqr_periodic_grad_ref.py against the brute-force tiled recursion and against central
differences of the periodic solve, across segment counts, against the stationary gradients at N = 1, and the
attainability of the budget rule on every input of the GPU accuracy test; then the C ABI's workspace formula, kernel
names and argument checks, none of which launches anything, and the kernels' resources from their device assembly.

The budget rule is DESIGN.md 3.14 / 3.23's: per gradient and instance, error against the longdouble restatement over
max(budget, 2^-48 max(1, |ref|)); median over instances <= 2.5 and every instance <= 10."""
import ctypes
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import lqr_steady_state_grad_f64_ref as ss64
import tvlqr_f64_ref as ref64
import tvlqr_periodic_grad_ref as pg
import tvlqr_periodic_ref as pr
import tvlqr_ref
import tvlqr_time_parallel_ref as tp
from tfmpc import _hip, solvers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402
LD = np.longdouble
B = 3
GRADS = pg.GRADS
# longdouble restatement against the brute-force tiled recursion, relative to max(1, |brute|): the worst case measured over
# SMALL (three instances each, all four upstream gradients) was 1.59e-18 (dF at (16, 8, 6, 3)); the bound is four times
# that
BRUTE_BOUND = 4 * 1.59e-18
SMALL = [(3, 2, 4, 2), (5, 3, 7, 3), (16, 8, 6, 3)]
# central differences of the longdouble periodic solve at h = 1e-7 against the longdouble restatement, relative to
# max(1, |gradient entry|): the truncation error h^2 f''' / 6 of the differences.  Measured worst case 2.62e-11 (at
# (4, 2, 1)); the bound is four times that
DIFF_H = LD(1e-7)
DIFF_BOUND = 4 * 2.62e-11


@functools.lru_cache(maxsize=None)
def _case(n, m, N, segments, count=B, unscaled=False):
    """Operands, upstream gradients, both forwards and both restatements, computed once; no test writes to them."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = tp.perturbed(make, n, m, N, count, seed=n * 100 + m)
    ups = pg.upstream(n, m, N, count, seed=7)
    fld, f64 = pr.solve_batch(F, f, C, c, segments, dtype=LD), pr.solve_batch(F, f, C, c, segments)
    return F, f, C, c, ups, fld, f64, pg.references(F, f, C, c, ups, segments, fld, f64)


@pytest.mark.parametrize("n,m,N,segments", SMALL)
def test_the_longdouble_restatement_is_the_brute_force_limit(n, m, N, segments):
    F, f, C, c, ups, _, _, refs = _case(n, m, N, segments)
    br = pg.brute(F, f, C, c, ups)
    worst = max(float(np.abs(refs[0][name] - br[name]).max() / max(1.0, float(np.abs(br[name]).max()))) for name in GRADS)
    print(f"longdouble restatement against {br['tiles']} tiled periods ({n}, {m}, {N}, {segments}): {worst:.3g} relative")
    assert worst <= BRUTE_BOUND
    # (X*, y*) reproduces itself under one more lap to longdouble rounding: 64 eps for a lap's few dozen roundings
    assert float(refs[0]["residual"].max()) <= 64 * float(np.finfo(LD).eps)


def _loss(F, f, C, c, ups, segments):
    r = pr.solve(F, f, C, c, segments, dtype=LD)
    assert r["status"] == 0
    return sum((np.asarray(ups[g], dtype=LD) * r[o]).sum() for g, o in zip(pg.UPS, pg.FWD))


@pytest.mark.parametrize("n,m,N,segments", [(3, 2, 4, 2), (4, 2, 1, 1)])
def test_the_longdouble_restatement_against_central_differences_of_the_periodic_solve(n, m, N, segments):
    F, f, C, c, ups, _, _, refs = _case(n, m, N, segments)
    rng = np.random.default_rng(5)
    worst = 0.0
    for b in range(2):
        ops = dict(F=F[b], f=f[b], C=C[b], c=c[b])
        up = pg.upstream_of(ups, b)
        for name, key in zip("FfCc", GRADS):
            for _ in range(3):
                idx = tuple(int(rng.integers(s)) for s in ops[name].shape)
                steps = []
                for sign in (1, -1):
                    a = np.asarray(ops[name], dtype=LD).copy()
                    a[idx] += sign * DIFF_H
                    if name == "C" and idx[1] != idx[2]:       # C stays symmetric: the derivative is dC_ij + dC_ji
                        a[idx[0], idx[2], idx[1]] += sign * DIFF_H
                    steps.append(_loss(*(a if k == name else ops[k] for k in "FfCc"), up, segments))
                fd = (steps[0] - steps[1]) / (2 * DIFF_H)
                want = refs[0][key][b][idx] * (2 if name == "C" and idx[1] != idx[2] else 1)
                worst = max(worst, float(abs(fd - want) / max(1.0, abs(want))))
    print(f"central differences ({n}, {m}, {N}): {worst:.3g} relative")
    assert worst <= DIFF_BOUND


@pytest.mark.parametrize("n,m,N", [(3, 2, 4), (5, 3, 7), (16, 8, 6)])
def test_segment_counts_agree(n, m, N):
    F, f, C, c, ups, fld, f64, refs = _case(n, m, N, 1)
    for segments in (2, N):
        for dtype, fwd in ((LD, fld), (np.float64, f64)):
            got = pg.vjp_batch(F, f, C, c, fwd, ups, segments, dtype=dtype)
            assert not got["status"].any()
            pg.check(got, refs, what=(n, m, N, segments, np.dtype(dtype).name))


@pytest.mark.parametrize("n,m", [(16, 8), (5, 3)])
def test_one_step_periods_agree_with_the_stationary_gradients(n, m):
    """N = 1 is the stationary problem: dF, df, dC, dc of tests/lqr_steady_state_grad_f64_ref.py (gP = gV, gp = gv)."""
    F, f, C, c, ups, _, _, refs = _case(n, m, 1, 1)
    got = {name: [] for name in GRADS}
    for b in range(B):
        r = ss64.vjp_gj(F[b, 0], f[b, 0], C[b, 0], c[b, 0], gK=ups["gK"][b, 0], gk=ups["gk"][b, 0], gP=ups["gV"][b, 0],
                        gp=ups["gv"][b, 0])
        assert r["status"] == 0
        for name in GRADS:
            got[name].append(r[name][None])
    pg.check({name: np.stack(a) for name, a in got.items()}, refs, what=(n, m, "N = 1"))


# the inputs of tests/test_tvlqr_periodic_grad_gpu.py's accuracy test (its instance counts included)
GPU_CASES = [(3, 2, 4, 2, 4, False), (5, 3, 7, 3, 4, False), (16, 8, 6, 3, 4, False), (16, 8, 1, 1, 4, False),
             (17, 8, 5, 2, 3, False), (16, 17, 3, 1, 3, False), (8, 32, 4, 4, 3, False), (32, 32, 3, 2, 3, False),
             (16, 8, 50, 5, 3, False), (17, 8, 5, 2, 3, True), (16, 8, 6, 3, 4, True)]


@pytest.mark.parametrize("n,m,N,segments,count,unscaled", GPU_CASES)
def test_the_rule_is_attainable_in_fp64(n, m, N, segments, count, unscaled):
    """Another admissible fp64 evaluation -- every product's k-sum reversed -- meets the rule the kernel is held to."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = tp.perturbed(make, n, m, N, count, seed=n * 100 + m)
    ups = pg.upstream(n, m, N, count, seed=n + m)
    f64 = pr.solve_batch(F, f, C, c, segments)
    refs = pg.references(F, f, C, c, ups, segments, pr.solve_batch(F, f, C, c, segments, dtype=LD), f64)
    got = pg.vjp_batch(F, f, C, c, f64, ups, segments, reverse=True)
    assert not got["status"].any()
    pg.check(got, refs, what=(n, m, N, segments, "unscaled" if unscaled else "scaled", "reversed"))


def test_the_restatement_names_the_cause():
    n, m, N, segments = 5, 3, 4, 2
    F, f, C, c, ups, _, f64, _ = _case(n, m, N, segments)
    up = pg.upstream_of(ups, 0)
    flagged = pg.vjp(F[0], f[0], C[0], c[0], dict(f64[0], status=pr.ST_NOT_PD), up, segments)
    assert flagged["status"] == pr.ST_NOT_PD and np.isnan(flagged["dF"]).all() and np.isnan(flagged["residual"])
    Fu = F[0].copy()
    Fu[:, :, :n] = 1.3 * np.eye(n)
    unstable = pg.vjp(Fu, f[0], C[0], c[0], dict(f64[0], K=np.zeros_like(f64[0]["K"])), up, segments)
    assert unstable["status"] == pr.ST_NOT_STABILISING and np.isnan(unstable["dC"]).all()
    Vbad = dict(f64[0], V=-1e6 * np.broadcast_to(np.eye(n), (N, n, n)))
    assert pg.vjp(F[0], f[0], C[0], c[0], Vbad, up, segments)["status"] == pr.ST_NOT_PD


# ---- the C ABI, without a launch -----------------------------------------------------------------------------------------

EXPORTS = ("tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64", "tfmpc_tvlqr_periodic_vjp_kernel_name_f64",
           "tfmpc_tvlqr_periodic_vjp_f64")


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION
    assert solvers.tvlqr_periodic_vjp is solvers.tvlqr_grad.tvlqr_periodic_vjp


@pytest.mark.parametrize("n,m,N,segments", [(3, 2, 4, 2), (16, 8, 6, 3), (17, 8, 5, 2), (32, 32, 3, 2), (16, 8, 512, 33),
                                            (16, 8, 1, 4), (8, 32, 4, 9)])
@pytest.mark.parametrize("Bk", [1, 2, 64, 65, 131])
def test_workspace_formula(Bk, n, m, N, segments):
    lib = _hip.load()
    assert lib.tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(Bk, n, m, N, segments) == pg.workspace_bytes(Bk, n, m, N, segments) > 0
    for bad in ((0, n, m, N, segments), (Bk, 0, m, N, segments), (Bk, n, 0, N, segments), (Bk, n, m, 0, segments),
                (Bk, n, m, N, 0), (Bk, 33, m, N, segments), (Bk, n, 33, N, segments)):
        assert lib.tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(*bad) == pg.workspace_bytes(*bad) == 0


def test_kernel_names_per_shape():
    name = lambda *a: _hip.load().tfmpc_tvlqr_periodic_vjp_kernel_name_f64(*a).decode()      # noqa: E731
    assert name(16, 8, 6, 3) == name(16, 16, 1, 1) == name(1, 1, 1, 1) == "tvp_vjp_f64_wave16"
    assert name(17, 8, 5, 2) == name(16, 17, 3, 1) == name(32, 32, 3, 2) == "tvp_vjp_f64_wave32"
    assert name(33, 1, 4, 2) == name(1, 33, 4, 2) == "unsupported"
    assert name(0, 3, 4, 2) == name(3, 0, 4, 2) == name(3, 2, 0, 2) == name(3, 2, 4, 0) == "invalid"


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4, dtype=torch.float64))
    full = lib.tfmpc_tvlqr_periodic_vjp_workspace_bytes_f64(4, 3, 2, 2, 2)
    odd = ctypes.c_void_p(p.value + 4)                                                        # not 8-byte aligned

    def call(B=1, n=3, m=2, N=2, F=p, f=p, C=p, c=p, s=0, K=p, k=p, V=p, v=p, fst=p, dsb=1, dst=1, dF=p, status=p, segments=2,
             max_iter=0, tol=0.0, ws=p, ws_bytes=1 << 30):
        return lib.tfmpc_tvlqr_periodic_vjp_f64(B, n, m, N, F, s, s, f, s, s, C, s, s, c, s, s, K, k, V, v, fst, None, None, None,
                                                None, dF, dsb, dst, p, dsb, dst, p, dsb, dst, p, dsb, dst, None, None, status,
                                                segments, max_iter, tol, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(n=0) == -1 and call(m=0) == -1 and call(N=0) == -1 and call(n=-2) == -1
    assert call(n=33) == -2 and call(m=33) == -2 and call(B=0, n=40, m=40) == -2
    assert call(segments=0) == -1 and call(max_iter=-1) == -1 and call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(C=None) == -1 and call(c=None) == -1
    assert call(K=None) == -1 and call(k=None) == -1 and call(V=None) == -1 and call(v=None) == -1
    assert call(fst=None) == -1 and call(status=None) == -1
    assert call(s=-3) == -1 and call(dsb=-3) == -1 and call(dst=-1) == -1
    assert call(ws=None) == -4 and call(ws_bytes=16) == -4             # the workspace is always required
    assert call(B=4, dsb=0, ws_bytes=full - 8) == -4                   # one double short with every output summed
    assert call(ws=odd) == -1
    assert call(B=0, F=None, f=None, C=None, c=None, K=None, k=None, V=None, v=None, fst=None, status=None, ws=None) == 0


def test_the_refusal_names_the_flag():
    """Before any launch: no GPU is needed to be refused."""
    F, f, C, c, _, _, _, _ = _case(3, 2, 4, 2)
    leaves = [torch.as_tensor(a).requires_grad_() for a in (F, f[..., None], C, c[..., None])]
    with pytest.raises(NotImplementedError, match="gradients") as err:
        solvers.tvlqr_periodic_steady_state(*leaves)
    assert "differentiable=True" in str(err.value)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_f64_kernels_use_no_scratch_no_static_lds_and_the_f64_matrix_cores():
    """The periodic file's counterpart of tests/test_tvlqr_backward_grad_f64_cpu.py's resource test: the exact set of 13
    kernels -- the shared sweep tvb_vjp_f64_kernel (tvlqr_backward_vjp_body.h) at both widths in its three passes, the four
    stitches, the finish, the two double batch-sum stages."""
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_periodic_vjp_f64.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == 13 == len(re.findall(r"^\s*\.amdhsa_kernel\s", text, flags=re.M)), found
    names = [f[0] for f in found]
    sweeps = sorted(name for name in names if "tvb_vjp_f64_kernel" in name)
    assert len(set(sweeps)) == 6, found
    assert all(sum(f"ILi{np_}ENS0_8PeriodicILi{p}EEE" in name for name in sweeps) == 1 for np_ in (16, 32) for p in (0, 1, 2)), sweeps
    stitches = sorted(name for name in names if "tvp_vjp_f64_stitch_kernel" in name)
    assert len(set(stitches)) == 4, found
    assert all(sum(f"ILi{np_}ELi{mode}EEE" in name for name in stitches) == 1 for np_ in (16, 32) for mode in (0, 1)), stitches
    assert sum("tvp_vjp_f64_finish_kernel" in name for name in names) == 1, found
    sums = sorted(name for name in names if "batch_sum_" in name)
    assert len(sums) == 2 and "batch_sum_stage1" in sums[0] and "batch_sum_stage2_tree" in sums[1], found
    assert all(name.endswith("PKdimPd") for name in sums), sums            # the double overloads
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    # the sweeps take all their LDS at launch (none static); the launch sizes are the layout's
    static = {name: int(size) for size, name in
              re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.group_segment_fixed_size).*\n)*?\s+\.name:\s+(\S+)\n", text)}
    assert all(static[name] == 0 for name in sweeps), static
    assert "BvLayout<16>::total(kPassA) == 4976 && BvLayout<32>::total(kPassA) == 19168" in open(path).read()
    assert 19168 * 8 <= 160 * 1024
    # the f64 matrix-core instruction is in every sweep and stitch body
    for name in sweeps + stitches:
        body = text[text.index(name + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma_f64_16x16x4" in body, name

"""Time-varying LQR without a GPU: the numpy restatement (tests/tvlqr_ref.py) pinned two independent ways, the
Python class's shape validation, the C ABI's declarations and bindings, and the new kernels' register budget."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import tvlqr_ref
from oracle import lqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR  # noqa: E402
from tfmpc.solvers.lqr import LQR  # noqa: E402

TV_EXPORTS = ("tfmpc_tvlqr_workspace_bytes", "tfmpc_tvlqr_kernel_name", "tfmpc_tvlqr_backward_f32",
              "tfmpc_tvlqr_forward_f32", "tfmpc_tvlqr_solve_f32")


@pytest.mark.parametrize("n,m,T", [(3, 2, 7), (16, 8, 5)])
def test_restatement_with_equal_steps_is_the_lqr_oracle(n, m, T):
    np.random.seed(4)
    F, f, C, c = lqr_ref.make_lqr(n, m)
    x0 = np.random.default_rng(0).normal(size=(n, 1))
    x, u, cs, policy, value_fn = lqr_ref.solve(F, f, C, c, x0, T)
    tile = lambda a: np.repeat(a[None], T, axis=0)      # noqa: E731
    got = tvlqr_ref.solve(tile(F), tile(f), tile(C), tile(c), x0)
    for name, ref in (("states", x), ("actions", u), ("costs", cs)):
        np.testing.assert_allclose(got[name], ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()), err_msg=name)
    for t in range(T):
        np.testing.assert_allclose(got["K"][t], policy[t][0], rtol=0, atol=1e-12 * max(1.0, np.abs(policy[t][0]).max()))
        np.testing.assert_allclose(got["V"][t], value_fn[t][0], rtol=0, atol=1e-12 * max(1.0, np.abs(value_fn[t][0]).max()))
        assert abs(got["const"][t] - value_fn[t][2][0, 0]) <= 1e-12 * max(1.0, abs(value_fn[t][2][0, 0]))


@pytest.mark.parametrize("n,m,T,final", [(2, 1, 1, False), (3, 2, 6, False), (4, 3, 9, True), (5, 2, 12, True)])
def test_restatement_is_the_minimiser_of_the_dense_qp(n, m, T, final):
    F, f, C, c = (a[0].astype(np.float64) for a in tvlqr_ref.make_models(n, m, T, 1, seed=n + T))
    Cf, cf = (a[0].astype(np.float64) for a in tvlqr_ref.make_final(n, 1)) if final else (None, None)
    x0 = tvlqr_ref.make_x0(n, 1)[0].astype(np.float64)
    got = tvlqr_ref.solve(F, f, C, c, x0, Cf, cf)
    xs, us, total = tvlqr_ref.kkt_solve(F, f, C, c, x0, Cf, cf)
    scale = max(1.0, np.abs(xs).max())
    np.testing.assert_allclose(got["states"], xs, rtol=0, atol=1e-9 * scale)
    np.testing.assert_allclose(got["actions"], us, rtol=0, atol=1e-9 * max(1.0, np.abs(us).max()))
    assert abs(got["costs"].sum() - total) <= 1e-9 * max(1.0, abs(total))
    # and the value function at t = 0 prices the whole trajectory: 1/2 x0' V0 x0 + v0' x0 + const0
    v0 = 0.5 * x0 @ got["V"][0] @ x0 + got["v"][0] @ x0 + got["const"][0]
    assert abs(v0 - total) <= 1e-9 * max(1.0, abs(total))


def _model(B, T, n, m):
    d = n + m
    F, f, C, c = tvlqr_ref.make_models(n, m, T, 1, seed=3)
    bt = lambda a: np.repeat(a, B, axis=0) if B else a[0]      # noqa: E731
    return bt(F), bt(f), bt(C), bt(c), d


def test_shapes_and_properties_without_a_device():
    F, f, C, c, d = _model(3, 4, 3, 2)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu")
    assert (tv.state_size, tv.action_size, tv.n_dim, tv.horizon, tv.batch_size) == (3, 2, 5, 4, 3)
    # shared model, column vectors, a time axis of 1 broadcast with stride 0
    Fs, fs, Cs, cs, _ = _model(0, 4, 3, 2)
    tv = TimeVaryingLQR(Fs, fs[..., None], Cs[:1], cs[:1, :, None], device="cpu")
    assert (tv.horizon, tv.batch_size) == (4, None)
    args = tv._model_args()
    assert args[2] == 3 * 5 and args[1] == 0          # F: time stride n*d, no batch stride
    assert args[7] == 0 and args[8] == 0               # C: shared, constant in time
    x = torch.ones(3, 1)
    u = torch.zeros(2, 1)
    np.testing.assert_allclose(tv.transition(x, u, 2).numpy(), Fs[2][:, :3] @ np.ones((3, 1)) + fs[2][:, None], rtol=1e-6)
    np.testing.assert_allclose(tv.cost(x, u, 3).item(), lqr_ref.cost(Cs[0], cs[0][:, None], np.ones((3, 1)), np.zeros((2, 1))).item(),
                               rtol=1e-5)
    np.testing.assert_allclose(tv.final_cost(x).item(), lqr_ref.final_cost(Cs[0], cs[0][:, None], np.ones((3, 1))).item(), rtol=1e-5)


def test_from_lqr_is_a_stride_zero_view():
    np.random.seed(0)
    F, f, C, c = lqr_ref.make_lqr(3, 2)
    C = 0.5 * (C + C.T)
    lqr = LQR(np.stack([F] * 2), np.stack([f] * 2), np.stack([C] * 2), np.stack([c] * 2), device="cpu")
    tv = TimeVaryingLQR.from_lqr(lqr, 6)
    assert (tv.horizon, tv.batch_size) == (6, 2)
    assert tv.F.data_ptr() == lqr.F.data_ptr() and tv.F.stride(1) == 0
    args = tv._model_args()
    assert args[1] == lqr.F[0].numel() and args[2] == 0


@pytest.mark.parametrize("bad", [
    "F2d", "m0", "f_size", "C_size", "c_size", "horizons", "batches", "final_one", "final_size", "asym", "asym_final"])
def test_validation_errors_are_raised_without_a_device(bad):
    F, f, C, c, d = _model(2, 4, 3, 2)
    kw = {}
    if bad == "F2d":
        F = F[0, 0]
    elif bad == "m0":
        F = F[..., :3]
    elif bad == "f_size":
        f = f[..., :2]
    elif bad == "C_size":
        C = C[..., :4, :4]
    elif bad == "c_size":
        c = c[..., :4]
    elif bad == "horizons":
        C = C[:, :3]
    elif bad == "batches":
        c = np.concatenate([c, c], axis=0)
    elif bad == "final_one":
        kw = dict(C_final=np.eye(3, dtype=np.float32))
    elif bad == "final_size":
        kw = dict(C_final=np.eye(4, dtype=np.float32), c_final=np.zeros(4, np.float32))
    elif bad == "asym":
        C = C.copy()
        C[1, 2, 0, 1] += 1.0
    elif bad == "asym_final":
        Cf = np.eye(3, dtype=np.float32)
        Cf[0, 2] = 0.5
        kw = dict(C_final=Cf, c_final=np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        TimeVaryingLQR(F, f, C, c, device="cpu", **kw)


def test_every_new_export_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    for name in TV_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
    assert re.search(r"tfmpc_version\(void\) \{ return 320; \}", open(os.path.join(ROOT, "tf-mpc_amd", "csrc", "lqr_dispatch.hip")).read())
    # model arguments: B n m T, then (pointer, batch stride, time stride) x 4, then Cfin, its stride, cfin, its stride
    args = _hip._SIGNATURES["tfmpc_tvlqr_solve_f32"][1]
    assert len(args) == 4 + 12 + 4 + 13


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
@pytest.mark.parametrize("src,kernel,count", [("tvlqr_mfma16x8.hip", "tvlqr_mfma16x8_kernel", 20),
                                              ("tvlqr_generic.hip", "tvlqr_generic_kernel", 3)])
def test_the_tvlqr_kernels_use_no_scratch(src, kernel, count):
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*" + kernel + r"\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(found) == count, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    dummy = torch.zeros(4)
    p = _hip.ptr(dummy)
    model = lambda B, n, m, T, s=0: (B, n, m, T, *([p, s, s] * 4), None, 0, None, 0)     # noqa: E731
    bw = lambda *mdl: lib.tfmpc_tvlqr_backward_f32(*mdl, p, p, None, None, None, None, None)   # noqa: E731
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
    assert bw(*model(1, 200, 200, 4)) == -2                   # beyond one wave's LDS
    assert lib.tfmpc_tvlqr_backward_f32(*model(0, 3, 2, 4), None, None, None, None, None, None, None) == 0   # B == 0: no-op
    # solve without K / k and without a workspace
    assert lib.tfmpc_tvlqr_solve_f32(*model(1, 3, 2, 4), p, p, p, p, None, None, None, None, None, None, None, 0, None) == -4
    assert lib.tfmpc_tvlqr_workspace_bytes(2, 16, 8, 50) == 2 * 50 * 8 * 17 * 4
    assert lib.tfmpc_tvlqr_kernel_name(200, 200, 4) == b"unsupported"

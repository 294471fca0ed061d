"""Gradients of the finite-horizon Riccati recursion without a GPU: the fp64 closed form of
tests/tvlqr_backward_grad_ref.py pinned against fp64 autograd through the recursion, the fp32 closed form's error next
to fp32 autograd's on the GPU tests' seeded problems, the C ABI's declarations, bindings and argument errors, the
Python front end's routing, and the new kernels' register budget."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import tvlqr_backward_grad_ref as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip, solvers  # noqa: E402
from tfmpc.solvers import TimeVaryingLQR, tvlqr_backward  # noqa: E402
from tfmpc.solvers.lqr import LQR, Policy, ValueFn  # noqa: E402

EXPORTS = ("tfmpc_tvlqr_backward_vjp_workspace_bytes", "tfmpc_tvlqr_backward_vjp_kernel_name",
           "tfmpc_tvlqr_backward_vjp_f32")


@pytest.mark.parametrize("only", [None] + [(name,) for name in bref.UPS])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("final", [True, False])
def test_closed_form_is_autograd_in_fp64(final, T, only):
    n, m, B = 3, 2, 2
    F, f, C, c, Cf, cf = bref.problem(n, m, T, B, seed=10 + T, final=final)
    up = bref.upstream(n, m, T, B, seed=T, only=only)
    got = bref.closed_form(F, f, C, c, Cf, cf, **up)
    ref = bref.autograd_grads(F, f, C, c, Cf, cf, **up)
    assert (got["status"] == 0).all()
    for name in bref.GRADS:
        if ref[name] is None:
            assert got[name] is None and not final
            continue
        err = np.abs(got[name] - ref[name]).max() / max(1.0, np.abs(ref[name]).max())
        assert err <= 1e-10, (name, err)


def test_fp32_closed_form_errs_like_fp32_autograd():
    """Both are fp32 evaluations of the same gradient in different operation orders, so their errors against fp64 are
    of one size: per shape, seed and operand the ratio (closed form / autograd) of the max-abs errors is held to the
    project's budget rule, median <= 2.5 and worst <= 10 (measured with these seeds: median 0.74 - 1.12 per shape, worst 2.34)."""
    ratios = []
    for n, m, T in ((3, 2, 5), (5, 3, 2), (16, 8, 20), (16, 8, 50)):
        per_shape = []
        for seed in range(4):
            F, f, C, c, Cf, cf = bref.problem(n, m, T, 1, seed=seed, final=bool(seed & 1))
            up = bref.upstream(n, m, T, 1, seed=seed)
            g64 = bref.closed_form(F, f, C, c, Cf, cf, **up)
            g32 = bref.closed_form(F, f, C, c, Cf, cf, **up, dtype=np.float32)
            a32 = bref.autograd_grads(F, f, C, c, Cf, cf, **up, dtype=torch.float32)
            for name in bref.GRADS:
                if g64[name] is None:
                    continue
                assert g32[name].dtype == np.float32
                floor = 1e-7 * max(1.0, np.abs(g64[name]).max())
                per_shape.append(max(np.abs(g32[name] - g64[name]).max(), floor) / max(np.abs(a32[name] - g64[name]).max(), floor))
        print((n, m, T), "closed form / autograd fp32 error: median %.2f worst %.2f" % (np.median(per_shape), max(per_shape)))
        ratios += per_shape
    assert np.median(ratios) <= 2.5 and max(ratios) <= 10.0, (np.median(ratios), max(ratios))


def test_restatement_flags_an_indefinite_step():
    n, m, T, B = 3, 2, 4, 3
    F, f, C, c, _, _ = bref.problem(n, m, T, B, seed=2)
    C = C.copy()
    C[1, 2, n:, n:] = -np.eye(m)
    got = bref.closed_form(F, f, C, c, **bref.upstream(n, m, T, B), dtype=np.float32)
    assert list(got["status"]) == [0, bref.ST_NOT_PD, 0]
    assert np.isnan(got["dF"][1]).all() and np.isfinite(got["dF"][[0, 2]]).all()


def test_every_new_export_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.tfmpc_version() == 320 and _hip.MIN_VERSION == 320
    # B n m T, the model (12 + 4), K k V v fwd_status, five upstream gradients, dF df dC dc (x3), dCfin dcfin (x2), tail
    assert len(_hip._SIGNATURES["tfmpc_tvlqr_backward_vjp_f32"][1]) == 4 + 16 + 5 + 5 + 12 + 4 + 4
    assert solvers.tvlqr_backward is tvlqr_backward and "tvlqr_backward" in vars(solvers)


def test_kernel_names_per_shape():
    name = lambda n, m, T=5: _hip.load().tfmpc_tvlqr_backward_vjp_kernel_name(n, m, T).decode()   # noqa: E731
    assert name(16, 8) == name(16, 16) == "tvb_vjp_mfma_16"
    assert name(5, 3) == name(1, 1) == name(16, 1) == name(3, 16) == "tvb_vjp_mfma_16 (padded)"
    assert name(17, 8) == name(32, 16) == name(20, 1) == "tvb_vjp_mfma_32"
    assert name(33, 1) == name(33, 16) == "unsupported"
    assert name(8, 17) == name(32, 17) == "unsupported"
    assert name(0, 3) == name(3, 0) == name(3, 2, 0) == "invalid"


def test_workspace_bytes():
    ws = _hip.load().tfmpc_tvlqr_backward_vjp_workspace_bytes
    n, m, T = 16, 8, 50
    d = n + m
    per = T * (n * d + n + d * d + d) + n * n + n
    assert ws(65536, n, m, T) >= 65536 * per * 4
    assert ws(1, n, m, T) == 0 and ws(0, n, m, T) == 0          # nothing is summed over a batch of one
    assert ws(4, 33, 1, T) == 0 and ws(4, 8, 17, T) == 0 and ws(4, 0, 1, T) == 0 and ws(4, n, m, 0) == 0


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    p = _hip.ptr(torch.zeros(4))

    def call(B=1, n=3, m=2, T=4, F=p, f=p, C=p, c=p, s=0, Cfin=None, cfin=None, K=p, k=p, V=p, v=p, fst=p, dF=p, ds=1,
             dCfin=None, dcfin=None, status=p, ws=None, ws_bytes=0):
        return lib.tfmpc_tvlqr_backward_vjp_f32(B, n, m, T, F, s, s, f, s, s, C, s, s, c, s, s, Cfin, s, cfin, s, K, k, V, v, fst,
                                                None, None, None, None, None, dF, ds, ds, p, ds, ds, p, ds, ds, p, ds, ds,
                                                dCfin, ds, dcfin, ds, status, ws, ws_bytes, None)

    assert call(B=-1) == -1
    assert call(n=0) == -1 and call(m=0) == -1 and call(T=0) == -1
    assert call(F=None) == -1 and call(f=None) == -1 and call(C=None) == -1 and call(c=None) == -1
    assert call(K=None) == -1 and call(k=None) == -1 and call(V=None) == -1 and call(v=None) == -1
    assert call(fst=None) == -1
    assert call(status=None) == -1                                   # NULL status
    assert call(s=-3) == -1 and call(ds=-3) == -1
    assert call(Cfin=p) == -1 and call(cfin=p) == -1                 # give both, or neither
    assert call(dCfin=p) == -1 and call(dcfin=p) == -1               # the default final cost's gradient is in dC, dc
    assert call(n=33) == -2 and call(m=17) == -2 and call(B=0, n=40, m=40) == -2      # a bad shape
    assert call(B=4, ds=0) == -4                                     # a summed output needs the workspace
    assert call(B=4, ds=0, ws=p, ws_bytes=16) == -4                  # a short workspace
    assert call(B=0, F=None, f=None, C=None, c=None, K=None, k=None, V=None, v=None, fst=None, status=None) == 0


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_backward_vjp_kernels_use_no_scratch():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_backward_vjp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*(?:tvb_vjp_|bvjp_|batch_sum_)\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len([f for f in found if "tvb_vjp_kernel" in f[0]]) == 2, found
    assert len(found) == 4, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)
    assert "v_mfma_f32_16x16x4_f32" in text or "v_mfma_f32_16x16x4f32" in text
    assert not re.search(r"\b(scratch_|buffer_atomic|global_atomic|flat_atomic|ds_add|ds_max|ds_min)\w*", text)


# ---- the Python front end, with the launch replaced by a stand-in ---------------------------------------------------------

def _fake(Bk, T, n, m):
    return (torch.zeros(Bk, T, m, n), torch.zeros(Bk, T, m, 1), torch.zeros(Bk, T, n, n), torch.zeros(Bk, T, n, 1),
            torch.zeros(Bk, T, 1, 1), torch.zeros(Bk, dtype=torch.int32))


def _tv_ops(grad=(), B=2, T=4, n=3, m=2):
    F, f, C, c, _, _ = bref.problem(n, m, T, B, seed=5)
    return [torch.as_tensor(a).requires_grad_() if name in grad else a for name, a in zip("FfCc", (F, f, C, c))]


def test_routing_of_the_time_varying_front_end(monkeypatch):
    monkeypatch.setattr(TimeVaryingLQR, "_backward_launch", lambda self: _fake(self.batch_size or 1, self.horizon, 3, 2))
    pol, val = TimeVaryingLQR(*_tv_ops(grad="F"), device="cpu").backward()
    assert isinstance(pol, Policy) and isinstance(val, ValueFn)
    assert pol.K.grad_fn is None and val.V.grad_fn is None                     # the default: no graph
    pol, val = TimeVaryingLQR(*_tv_ops(grad="F"), device="cpu").backward(differentiable=True)
    assert all(t.requires_grad for t in (pol.K, pol.k, val.V, val.v, val.const))
    assert tuple(pol.K.shape) == (2, 4, 2, 3) and tuple(val.const.shape) == (2, 4, 1, 1)
    pol, val = TimeVaryingLQR(*_tv_ops(), device="cpu").backward(differentiable=True)
    assert pol.K.grad_fn is None                                               # nothing requires grad
    with torch.no_grad():
        pol, _ = TimeVaryingLQR(*_tv_ops(grad="C"), device="cpu").backward(differentiable=True)
    assert not pol.K.requires_grad
    outs = tvlqr_backward(*(a[0] for a in _tv_ops(grad="c")))                  # unbatched
    assert len(outs) == 5 and tuple(outs[0].shape) == (4, 2, 3) and all(t.requires_grad for t in outs)


def test_routing_of_the_lqr_front_end(monkeypatch):
    monkeypatch.setattr(LQR, "_backward_launch", lambda self, T: _fake(self.batch_size or 1, T, 3, 2))
    F, f, C, c = (a[:, 0] for a in _tv_ops())
    Ft = torch.as_tensor(F).requires_grad_()
    pol, val = LQR(Ft, f, C, c, device="cpu").backward(6)
    assert pol.K.grad_fn is None and tuple(pol.K.shape) == (2, 6, 2, 3)
    pol, val = LQR(Ft, f, C, c, device="cpu").backward(6, differentiable=True)
    assert pol.K.requires_grad and val.const.requires_grad and len(pol) == 6
    pol, _ = LQR(F, f, C, c, device="cpu").backward(6, differentiable=True)
    assert pol.K.grad_fn is None
    Ca = C.copy()
    Ca[1, 0, 4] += 1.0
    with pytest.raises(NotImplementedError):
        LQR(Ft, f, Ca, c, device="cpu").backward(6, differentiable=True)
    LQR(Ft, f, Ca, c, device="cpu").backward(6)                                 # the default serves a general C as before

"""Gradients of the time-varying LQR without a GPU: the torch restatement (tests/tvlqr_grad_ref.py) against the numpy
one, the closed-form adjoint against autograd and gradcheck, the VJP's C ABI (declarations, bindings, argument
errors) and the register budget of its kernels."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import tvlqr_grad_ref as gref
import tvlqr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ring_waits  # noqa: E402

from tfmpc import _hip  # noqa: E402

VJP_EXPORTS = ("tfmpc_tvlqr_vjp_workspace_bytes", "tfmpc_tvlqr_vjp_f32")


def _problem(n, m, T, B, final, seed=0):
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=seed)
    Cf, cf = tvlqr_ref.make_final(n, B) if final else (None, None)
    x0 = tvlqr_ref.make_x0(n, B)
    rng = np.random.default_rng(seed + 5)
    g = (rng.normal(size=(B, T + 1, n)), rng.normal(size=(B, T, m)), rng.normal(size=(B, T + 1)))
    return (F, f, C, c, x0, Cf, cf), g


@pytest.mark.parametrize("n,m,T,final", [(3, 2, 1, False), (4, 2, 6, True), (16, 8, 4, False)])
def test_torch_restatement_is_the_numpy_one(n, m, T, final):
    (F, f, C, c, x0, Cf, cf), _ = _problem(n, m, T, 2, final)
    d64 = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64)     # noqa: E731
    xs, us, cs = gref.solve(*(d64(a) for a in (F, f, C, c, x0, Cf, cf)))
    for b in range(2):
        ref = tvlqr_ref.solve(F[b], f[b], C[b], c[b], x0[b], None if Cf is None else Cf[b], None if cf is None else cf[b])
        for name, got in (("states", xs[b]), ("actions", us[b]), ("costs", cs[b])):
            np.testing.assert_allclose(got.numpy(), ref[name], rtol=0, atol=1e-12 * max(1.0, np.abs(ref[name]).max()), err_msg=name)


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("loss", ["states", "actions", "costs", "mixed"])
@pytest.mark.parametrize("n,m,T", [(3, 2, 1), (4, 3, 2), (5, 2, 9)])
def test_closed_form_is_autograd(n, m, T, final, loss):
    ops, (gx, gu, gc) = _problem(n, m, T, 3, final, seed=n * 10 + T)
    gx, gu, gc = (g if loss in (name, "mixed") else None for g, name in ((gx, "states"), (gu, "actions"), (gc, "costs")))
    auto = gref.autograd_grads(*ops, gx, gu, gc)
    closed = gref.closed_form(*ops, gx, gu, gc)
    assert set(auto) == set(closed)
    for k in auto:
        scale = max(1.0, float(auto[k].abs().max()))
        assert float((auto[k] - closed[k]).abs().max()) <= 1e-10 * scale, k


@pytest.mark.parametrize("final", [False, True])
def test_gradcheck_of_the_restatement(final):
    (F, f, C, c, x0, Cf, cf), _ = _problem(2, 1, 3, 1, final, seed=3)
    ops = [torch.as_tensor(a, dtype=torch.float64).requires_grad_() for a in (F, f, c, x0)]
    Cs = torch.as_tensor(C, dtype=torch.float64)
    extra = [] if Cf is None else [torch.as_tensor(a, dtype=torch.float64).requires_grad_() for a in (Cf, cf)]

    def fn(F, f, c, x0, *fin):
        xs, us, cs = gref.solve(F, f, Cs, c, x0, *(fin or (None, None)))
        return xs.sum() + 0.5 * (us ** 2).sum() + cs.sum()

    assert torch.autograd.gradcheck(fn, (*ops, *extra))
    # C through its symmetric parametrisation: the closed form's dC is the gradient with respect to sym(A)
    A = torch.as_tensor(C, dtype=torch.float64).requires_grad_()
    assert torch.autograd.gradcheck(lambda A: gref.solve(ops[0].detach(), ops[1].detach(), gref.sym(A), ops[2].detach(),
                                                           ops[3].detach())[2].sum(), (A,))


def test_every_new_export_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tfmpc_hip.h")).read()
    lib = _hip.load()
    for name in VJP_EXPORTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _hip._SIGNATURES, name
        assert hasattr(lib, name), name
    # model (4 + 12 + 4), states actions, 3 upstream, 4 x (out, sb, st), 3 x (out, sb), status workspace bytes stream
    assert len(_hip._SIGNATURES["tfmpc_tvlqr_vjp_f32"][1]) == 20 + 2 + 3 + 12 + 6 + 4


def test_abi_argument_errors_return_before_any_launch():
    lib = _hip.load()
    buf = torch.zeros(4)
    p = _hip.ptr(buf)

    def call(B, n, m, T, s=0, model_null=None, cfin=None, outs_fin=False, status=True, ws=True, ws_bytes=None, so=0):
        model = [p, s, s] * 4 + [None, 0, None, 0]
        if model_null is not None:
            model[model_null] = None
        if cfin:
            model[12], model[14] = p, p
        outs = [p, so, so] * 4 + [p if outs_fin else None, 0, p if outs_fin else None, 0, p, 0]
        nbytes = ws_bytes if ws_bytes is not None else 1 << 40
        return lib.tfmpc_tvlqr_vjp_f32(B, n, m, T, *model, p, p, None, None, None, *outs, p if status else None,
                                       p if ws else None, nbytes, None)

    assert call(1, 3, 2, 0) == -1                     # T >= 1
    assert call(1, 0, 2, 4) == -1
    assert call(-1, 3, 2, 4) == -1
    assert call(1, 3, 2, 4, s=-1) == -1               # negative model stride
    assert call(1, 3, 2, 4, so=-1) == -1              # negative output stride
    assert call(1, 3, 2, 4, model_null=0) == -1       # F NULL
    assert call(1, 3, 2, 4, outs_fin=True) == -1      # final-cost gradients without an explicit final cost
    assert call(1, 3, 2, 4, status=False) == -1
    assert call(1, 200, 200, 4) == -2                 # beyond one wave's LDS
    assert call(1, 3, 2, 4, ws=False) == -4
    assert call(1, 3, 2, 4, ws_bytes=16) == -4
    assert call(0, 3, 2, 4, status=False, ws=False) == 0     # B == 0: no-op
    assert lib.tfmpc_tvlqr_vjp_workspace_bytes(0, 3, 2, 4) == 0
    assert lib.tfmpc_tvlqr_vjp_workspace_bytes(2, 16, 8, 50) >= lib.tfmpc_tvlqr_workspace_bytes(2, 16, 8, 50)


@pytest.mark.skipif(check_ring_waits.hipcc_path() is None, reason="needs the device compiler (hipcc) to produce the assembly")
def test_the_vjp_kernels_use_no_scratch():
    path = os.path.join(ROOT, "tf-mpc_amd", "csrc", "tvlqr_vjp.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([check_ring_waits.hipcc_path(), *check_ring_waits.FLAGS, "--cuda-device-only", "-S", path, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*(?:vjp_|batch_sum_)\S*)\n\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    # vjp_fold_kernel, vjp_sweep_kernel, vjp_reduce_final, vjp_reduce_steps, vjp_reduce_steps_mfma16, vjp_reduce_steps_stage2
    assert len(found) == 6, found
    for name, private, vgprs, spills in found:
        assert int(private) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, private, vgprs, spills)


def test_operands_that_need_no_grad_keep_the_plain_path():
    from tfmpc.solvers import TimeVaryingLQR, tvlqr_grad
    (F, f, C, c, x0, _, _), _ = _problem(3, 2, 4, 2, False)
    tv = TimeVaryingLQR(F, f, C, c, device="cpu")
    assert not tvlqr_grad.wants_grad(*tv._sources, x0)
    Ft = torch.as_tensor(F).requires_grad_()
    tv = TimeVaryingLQR(Ft, f, C, c, device="cpu")
    assert tv.F.requires_grad is False and tv._sources[0] is Ft
    assert tvlqr_grad.wants_grad(*tv._sources, x0)
    with torch.no_grad():
        assert not tvlqr_grad.wants_grad(*tv._sources, x0)

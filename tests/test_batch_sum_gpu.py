"""The shared batch sum (tf-mpc_amd/csrc/batch_sum.h) on the MI355X, bit for bit: a gradient whose batch
stride is 0 must be the emulated order of tests/batch_sum_ref.py applied to the per-instance gradients of the same problem.

Each case runs one problem twice.  With the shared operands replicated into real [B, ...] tensors the instance kernel
stores its gradients per instance; with them shared it stores the same values as records and the two reduction stages add
them up.  The instance kernels have no cross-instance communication, so the records are the per-instance run's bits and
only the order of the sum is under test.  Inputs are O(1) normals, nowhere near denormals.

The trajectory VJP (tfmpc_tvlqr_vjp_f32) computes its records on the fly, so there is no per-instance path to emulate
from: its shared final cost and x0, whose chunks the shared in-order stage 2 adds, are held to two calls giving the same
bits and to the fp64 budget of tests/tvlqr_grad_batch_ref.py."""
import numpy as np
import pytest
import torch

import batch_sum_ref as ref
import lqr_steady_state_ref as ssref
import tvlqr_backward_grad_ref as bref
import tvlqr_grad_batch_ref as batch
from test_tvlqr_grad_gpu import _kernel_grads as _trajectory_grads
from tfmpc.solvers import lqr_steady_state, tvlqr_backward

pytestmark = pytest.mark.gpu


def _grads(solve, ops, weights):
    """ops: name -> fp32 numpy operand (None: absent); every operand is a leaf.  The loss is sum(w * out) over the outputs
    that have a weight.  -> (fp32 gradients by name, the solver's return value)."""
    leaves = {k: (None if a is None else torch.as_tensor(a, device="cuda").requires_grad_()) for k, a in ops.items()}
    res = solve(*leaves.values())
    total = 0
    for out, w in weights(res):
        total = total + (out * torch.as_tensor(w, device="cuda").reshape(out.shape)).sum()
    total.backward()
    torch.cuda.synchronize()
    return {k: t.grad.cpu().numpy() for k, t in leaves.items() if t is not None}, res


# 131: two full chunks of 64 and a tail of 3; 65 on the 32-wide kernel: one chunk and 1; 64 * 257 + 1: 258 chunks, more than
# the 256 threads of the tree stage 2
@pytest.mark.parametrize("n,m,B", [(5, 3, 131), (20, 10, 65), (2, 1, 64 * 257 + 1)])
def test_steady_state_vjp_sums_in_the_emulated_order(n, m, B):
    F, f, C, _ = ssref.make_lqr_batch(n, m, 1, seed=13)
    rng = np.random.default_rng(B)
    c = rng.normal(size=(B, n + m)).astype(np.float32)
    w = [rng.normal(size=s).astype(np.float32) for s in ((B, m, n), (B, m), (B, n, n), (B, n))]
    weights = lambda ss: zip((ss.K, ss.k, ss.P, ss.p), w)          # noqa: E731
    rep = lambda a: np.repeat(a, B, axis=0)                        # noqa: E731
    per, ss = _grads(lqr_steady_state, dict(F=rep(F), f=rep(f), C=rep(C), c=c), weights)
    assert (ss.status.cpu().numpy() == 0).all()
    shared, ss = _grads(lqr_steady_state, dict(F=F[0], f=f[0], C=C[0], c=c), weights)
    assert (ss.status.cpu().numpy() == 0).all()
    assert np.array_equal(shared["c"], per["c"])
    for name in ("F", "f", "C"):
        assert per[name].shape == (B,) + shared[name].shape and np.isfinite(per[name]).all(), name
        assert np.array_equal(shared[name], ref.steady_state_sum(per[name])), name


# 259: one chunk of 256 and a tail of 3
@pytest.mark.parametrize("time_shared", [False, True], ids=["per step", "time shared"])
@pytest.mark.parametrize("n,m", [(5, 3), (20, 10)])
def test_riccati_vjp_sums_in_the_emulated_order(n, m, time_shared):
    """F, f, C and C_final shared by the batch (c, which sets the horizon, and c_final per instance).  ``time_shared``: they
    also have a time axis of 1 in BOTH runs, so each instance accumulates over time in place and only the batch sum differs."""
    T, B = 3, 259
    F, f, C, _, Cf, _ = bref.problem(n, m, 1 if time_shared else T, 1, seed=5 + n, final=True)
    rng = np.random.default_rng(n)
    c = rng.normal(size=(B, T, n + m)).astype(np.float32)
    cf = rng.normal(size=(B, n)).astype(np.float32)
    up = bref.upstream(n, m, T, B, seed=9)
    weights = lambda outs: zip(outs, (up[name] for name in bref.UPS))          # noqa: E731
    rep = lambda a: np.repeat(a, B, axis=0)                                     # noqa: E731
    per, _ = _grads(tvlqr_backward, dict(F=rep(F), f=rep(f), C=rep(C), c=c, Cfin=rep(Cf), cfin=cf), weights)
    shared, _ = _grads(tvlqr_backward, dict(F=F[0], f=f[0], C=C[0], c=c, Cfin=Cf[0], cfin=cf), weights)
    assert np.array_equal(shared["c"], per["c"]) and np.array_equal(shared["cfin"], per["cfin"])
    for name in ("F", "f", "C", "Cfin"):
        assert per[name].shape == (B,) + shared[name].shape and np.isfinite(per[name]).all(), name
        assert name == "Cfin" or shared[name].shape[0] == (1 if time_shared else T), name
        assert np.array_equal(shared[name], ref.riccati_sum(per[name])), name


def test_trajectory_vjp_shared_final_cost_and_x0():
    case = (5, 3, 3, 259, "final")
    user, full, w = batch.problem(*case)
    g64, budget = batch.oracle(*case)
    got, again = _trajectory_grads(user, w), _trajectory_grads(user, w)
    names = batch.summed_names(user, full)
    assert set(names) == {"Cfin", "cfin", "x0"}
    for k in got:
        assert np.array_equal(got[k].numpy(), again[k].numpy()), k
    for k in names:
        assert got[k].shape == g64[k].shape and bool(torch.isfinite(got[k]).all()), k
        ratio = batch.ratio(got[k], g64[k], budget[k])
        print(batch.case_id(case), k, "ratio", ratio)
        assert ratio <= 2.5, (k, ratio)          # one instance: the rule's median and max coincide

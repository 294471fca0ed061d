"""The shape-generic LQR kernels past 64 columns and at row exchanges (lqr_generic.hip, lqr_block.hip over wave_ops.h and
block_ops.h; ``-m gpu``).  Shapes, instances, the exchange counts they rest on and the launch helpers are in
tests/wide_shapes_ref.py; the conditions are asserted without a GPU in test_lqr_wide_shapes_cpu.py.

Every launch goes through the C ABI into NaN-filled buffers with a guard row behind the batch and a guard behind status:
every element inside the batch comes back finite, every guard stays NaN / -1 (wide_shapes_ref.launch).

* Accuracy, per shape, for the wave kernel (TFMPC_LQR_KERNEL=generic), the block kernel (=block) and the default choice
  (the kernel name is asserted): states, actions, costs, K, k, V, v, const of the fused solve against the fp64 oracle under
  the rule of test_lqr_block_gpu.py -- per instance |gpu - fp64| / max(|fp32 oracle - fp64|, 1e-6 of scale): median <= 2,
  0.9 quantile <= BUDGET = 5, max <= 5 BUDGET.  The measured statistics are recorded in DESIGN.md 3.2a.
* Backward, then forward, give the bits of the fused launch; an instance keeps its bits at another batch index, in a batch
  of one, and between neighbours that exchange no rows; a shared model (batch stride 0) gives the bits of the tiled one.
* The support boundary at m = 24: the largest supported n (found at run time) solves with TFMPC_OK and meets the rule -- the
  largest dynamic LDS this library launches; at n + 1 every entry point returns TFMPC_ERR_UNSUPPORTED and writes nothing.
* A system that cannot be solved without exchanging rows (C_uu = P D, zero diagonal) through tfmpc_lqr_*_general_f32,
  with an exactly singular neighbour.
"""

import numpy as np
import pytest
import torch

import wide_shapes_ref as ws
from oracle import lqr_ref
from tfmpc import _hip
from tfmpc.solvers.lqr import LQR

pytestmark = pytest.mark.gpu

BOUNDARY = ("boundary", ws.BOUNDARY_M, 4)
ACCURACY_SHAPES = ws.SHAPES + (BOUNDARY,) + ws.EXTRA_PIVOTED + ((33, 3, 4),)      # (33, 3): the block kernel's register path
# {(n, m, kernel, tensor): factor on the rule, with the cause} -- never across the board
LOOSE = {}


def _resolve(n, m):
    return (ws.boundary_n(_hip.require_gpu(), m), m) if n == "boundary" else (n, m)


def _expected_name(n, m, kernel):
    """What tfmpc_lqr_kernel_name says under the override: the block kernel wherever its LDS fits (it needs a little more
    than the wave kernel, so at the support boundary the wave kernel serves alone)."""
    block_fits = (n, m) != (ws.boundary_n(_hip.require_gpu(), ws.BOUNDARY_M), ws.BOUNDARY_M)
    return b"generic_wave" if kernel == "generic" or not block_fits else b"block_mfma_f32"


@pytest.mark.parametrize("kernel", ["generic", "block", None])
@pytest.mark.parametrize("n,m,T", ACCURACY_SHAPES)
def test_fused_solve_against_the_fp64_oracle(n, m, T, kernel):
    lib = _hip.require_gpu()
    n, m = _resolve(n, m)
    problem, ref64, ref32 = ws.case(n, m, T)
    idx = range(ws.NINST)
    with _hip.option("TFMPC_LQR_KERNEL", kernel):
        assert lib.tfmpc_lqr_kernel_name(n, m, T) == _expected_name(n, m, kernel)
        out, status = ws.launch(problem, idx, T)
    assert status.tolist() == [0] * ws.NINST
    loose = {key: LOOSE[n, m, kernel, key] for key in ws.FIELDS if (n, m, kernel, key) in LOOSE}
    ws.check_ratios(out, idx, ref64, ref32, f"({n}, {m}) T={T} {kernel or 'default'}", loose=loose)


@pytest.mark.parametrize("kernel", ["generic", "block"])
@pytest.mark.parametrize("n,m,T", [(49, 16, 4), (8, 66, 4), (70, 4, 4)])
def test_backward_then_forward_gives_the_bits_of_the_fused_solve(n, m, T, kernel):
    problem, _, _ = ws.case(n, m, T)
    idx = range(ws.NINST)
    with _hip.option("TFMPC_LQR_KERNEL", kernel):
        fused = ws.launch(problem, idx, T)
        split = ws.launch(problem, idx, T, split=True)
    for pos in idx:
        ws.same_bits(split, pos, fused, pos, ((n, m), kernel, "backward + forward against fused", pos))


@pytest.mark.parametrize("kernel", ["generic", "block"])
@pytest.mark.parametrize("n,m,T", [(56, 24, 4), (8, 66, 4)])
def test_an_instance_keeps_its_bits_wherever_it_sits(n, m, T, kernel):
    problem, _, _ = ws.case(n, m, T)
    order = (3, 0, 4, 1, 2)
    with _hip.option("TFMPC_LQR_KERNEL", kernel):
        full = ws.launch(problem, range(ws.NINST), T)
        moved = ws.launch(problem, order, T)
        alone = ws.launch(problem, (2,), T)
        # one model for the whole batch (batch stride 0) against the same model stored per instance
        shared = ws.launch(problem, (1, 3, 0), T, shared=True)
        F, f, C, c, x0 = problem
        tiled = ws.launch((F[[1, 1, 1]], f[[1, 1, 1]], C[[1, 1, 1]], c[[1, 1, 1]], x0[[1, 3, 0]]), range(3), T)
    for pos, b in enumerate(order):
        ws.same_bits(moved, pos, full, b, ((n, m), kernel, "instance", b, "at index", pos))
    ws.same_bits(alone, 0, full, 2, ((n, m), kernel, "a batch of one"))
    for pos in range(3):
        ws.same_bits(shared, pos, tiled, pos, ((n, m), kernel, "shared model against tiled", pos))
    ws.same_bits(shared, 0, full, 1, ((n, m), kernel, "shared model, its own initial state"))


@pytest.mark.parametrize("kernel", ["generic", "block"])
def test_an_exchanging_instance_between_neighbours_that_do_not_exchange(kernel):
    """Instance `mid` exchanges rows, its neighbours in the batch do not (asserted on the CPU): the bits of the batch of one."""
    n, m, T, (left, mid, right) = ws.NEIGHBOURS
    problem, ref64, ref32 = ws.case(n, m, T)
    with _hip.option("TFMPC_LQR_KERNEL", kernel):
        three = ws.launch(problem, (left, mid, right), T)
        alone = ws.launch(problem, (mid,), T)
    assert three[1].tolist() == [0, 0, 0]
    ws.same_bits(three, 1, alone, 0, (kernel, "the exchanging instance"))
    ws.check_ratios(three[0], (left, mid, right), ref64, ref32, f"neighbours {kernel}")


def test_one_state_past_the_support_boundary_is_refused_and_nothing_is_written():
    lib = _hip.require_gpu()
    m, T, B = ws.BOUNDARY_M, 4, 2
    n = ws.boundary_n(lib, m) + 1
    assert lib.tfmpc_lqr_kernel_name(n, m, T) == b"unsupported"
    F, f, C, c, x0 = ws.make_problem(n, m, B=B, seed=3)
    for kernel in (None, "generic", "block"):
        for general in (False, True):
            lqr = LQR(F, f, C, c, symmetric=not general)
            x0d = lqr._prep_x0(x0)
            for mode in ("solve", "backward", "forward"):
                flat, status = ws.nan_buffers(B, n, m, T, x0d.device)
                with _hip.option("TFMPC_LQR_KERNEL", kernel):
                    rc = ws.launch_raw(lqr, x0d, B, T, flat, status, mode, general)
                torch.cuda.synchronize()
                what = (kernel, "general" if general else "symmetric", mode)
                assert rc == ws.ERR_UNSUPPORTED, (what, rc)
                for key, buf in flat.items():
                    assert torch.isnan(buf).all(), (what, key, "written although the shape was refused")
                assert status.tolist() == [-1] * (B + 1), what


@pytest.mark.parametrize("m", [8, 24, 66])      # 8, 24: the ballot pivot search; 66: the sequential one
def test_general_inverse_of_a_permuted_diagonal_with_a_singular_neighbour(m):
    """F_u = 0 and C_uu = P D (cyclic permutation times a positive diagonal: zero diagonal, non-symmetric): Q_uu = C_uu at every
    step, every pivot but the last needs a row exchange, and K_t = -D^-1 P' C_ux.  An exchange that loses or swaps a
    multiplier gives an error of order one.  Rule of test_non_symmetric_cost_takes_the_reference_recursion: within five times
    the fp32 restatement's own error (floored at 1e-6 of scale) of oracle.lqr_ref.solve in fp64.  Instance 1 of the batch has
    two equal rows in C_uu (its pivot column is exactly zero): it reports TFMPC_ST_SINGULAR, its neighbours keep status 0
    and the bits they have without it."""
    n, T = 8, 3
    F, f, C, c, x0, D, perm = ws.make_permuted(n, m, B=3, seed=m)
    ins = lambda a: np.insert(a, 1, a[0], axis=0)              # noqa: E731  (a copy of instance 0 at index 1)
    F4, f4, C4, c4, x04 = (ins(a) for a in (F, f, C, c, x0))
    C4[1, n + 3] = C4[1, n + 2]                                # two equal rows of [C_ux | C_uu]: column n + 4 of C_uu is zero
    problem = (F4, f4, C4, c4, x04)
    good = (0, 2, 3)
    out, status = ws.launch(problem, range(4), T, general=True)
    assert int(status[1]) & _hip.ST_SINGULAR, status.tolist()
    assert [int(status[b]) for b in good] == [0, 0, 0], status.tolist()
    without = ws.launch(problem, good, T, general=True)
    for pos, b in enumerate(good):
        ws.same_bits((out, status), b, without, pos, (m, "next to the singular instance", b))
    split = ws.launch(problem, good, T, split=True, general=True)
    for pos in range(3):
        ws.same_bits(split, pos, without, pos, (m, "backward + forward against fused", pos))
    for b in good:
        x, u, cs, pol, _ = lqr_ref.solve(F4[b], f4[b], C4[b], c4[b], x04[b], T)
        x32, u32, c32, pol32, _ = lqr_ref.solve(F4[b], f4[b], C4[b], c4[b], x04[b], T, dtype=np.float32)
        stack = lambda p, i: np.stack([s[i] for s in p]).astype(np.float64)        # noqa: E731
        want_K = -(C4[b, n:, :n] / D[good.index(b)][:, None])[perm]
        assert np.abs(stack(pol, 0) - want_K).max() <= 1e-12
        for key, r64, r32 in (("states", x, x32), ("actions", u, u32), ("costs", cs, c32), ("K", stack(pol, 0), stack(pol32, 0)),
                              ("k", stack(pol, 1), stack(pol32, 1))):
            got = out[key][b].cpu().numpy().astype(np.float64).reshape(r64.shape)
            allowed = 5 * max(np.abs(r32.astype(np.float64) - r64).max(), 1e-6 * np.abs(r64).max())
            err = np.abs(got - r64).max()
            print(f"m={m} instance {b} {key}: error {err:.3g}, allowed {allowed:.3g}")
            assert err <= allowed, (m, b, key, err, allowed)

"""The non-symmetric recursion (tfmpc_lqr_*_general_f32: the wave kernel in the reference's term order, lqr.py:74-105) at the
shapes the symmetric dispatcher hands to OTHER kernels (``-m gpu``): (3, 2) at B = 40 (lane), (5, 3) and (16, 8) (matrix-core
16 x 8), (32, 16) (2 x 2 tiles), (33, 3) (block), (49, 16) and (8, 66) (wide).  A general solve that was routed by shape
instead of by entry point would symmetrise.

Instances as test_non_symmetric_cost_takes_the_reference_recursion builds them: a well-conditioned symmetric C plus a skew
part (the same quadratic form, a non-symmetric matrix).  Rule of that test: states, actions, costs and K within five times
the fp32 restatement's own error (floored at 1e-6 of scale) of oracle.lqr_ref.solve in fp64.  Launches go through the C ABI
into NaN-filled guarded buffers (wide_shapes_ref.launch).
"""

import functools

import numpy as np
import pytest

import problems
import wide_shapes_ref as ws
from oracle import lqr_ref
from tfmpc import _hip

pytestmark = pytest.mark.gpu

# (n, m, T, B, the symmetric dispatcher's kernel)
CASES = ((3, 2, 6, 40, b"lane (batch >= 32) / generic_wave"), (5, 3, 6, 3, b"mfma_16x8 (zero-padded)"),
         (16, 8, 6, 3, b"mfma_16x8"), (16, 8, 53, 3, b"mfma_16x8"), (32, 16, 6, 3, b"mfma_32x16"),
         (33, 3, 6, 3, b"block_mfma_f32"), (49, 16, 6, 3, b"block_mfma_f32"), (8, 66, 6, 3, b"block_mfma_f32"))


@functools.lru_cache(maxsize=None)
def _case(n, m, T, B):
    """(symmetric problem, non-symmetric problem, per-instance fp64 and fp32 restatements of the non-symmetric one)"""
    F, f, C, c, x0 = problems.make_lqr_batch_fast(B, n, m, seed=31 * n + m)
    F *= 1.2 / np.sqrt(n)                                      # 0.3 at n = 16, as the existing test
    skew = np.random.default_rng(11).normal(size=(B, n + m, n + m)) * 0.05
    Cn = C + (skew - np.swapaxes(skew, 1, 2))
    refs = []
    stack = lambda p, i: np.stack([s[i] for s in p]).astype(np.float64)            # noqa: E731
    for b in range(B):
        r = []
        for dtype in (np.float64, np.float32):
            x, u, cs, pol, val = lqr_ref.solve(F[b], f[b], Cn[b], c[b], x0[b], T, dtype=dtype)
            r.append(dict(states=x.astype(np.float64), actions=u.astype(np.float64), costs=cs.astype(np.float64),
                          K=stack(pol, 0), V0=val[0][0].astype(np.float64)))
        refs.append(tuple(r))
    return (F, f, C, c, x0), (F, f, Cn, c, x0), refs


@pytest.mark.parametrize("n,m,T,B,symmetric_kernel", CASES)
def test_general_entry_points_at_shapes_other_kernels_serve(n, m, T, B, symmetric_kernel):
    lib = _hip.require_gpu()
    assert lib.tfmpc_lqr_kernel_name(n, m, T) == symmetric_kernel
    sym, gen, refs = _case(n, m, T, B)
    idx = range(B)
    out, status = ws.launch(gen, idx, T, general=True)
    assert status.tolist() == [0] * B
    worst = {}
    for b in idx:
        r64, r32 = refs[b]
        for key in ("states", "actions", "costs", "K"):
            got = out[key][b].cpu().numpy().astype(np.float64).reshape(r64[key].shape)
            allowed = 5 * max(np.abs(r32[key] - r64[key]).max(), 1e-6 * np.abs(r64[key]).max())
            err = np.abs(got - r64[key]).max()
            worst[key] = max(worst.get(key, 0.0), err / allowed)
            assert err <= allowed, ((n, m, T), b, key, err, allowed)
        # V of the reference recursion is not symmetric here -- in the restatement and on the device
        V0 = out["V"][b, 0].cpu().numpy().reshape(n, n)
        assert np.abs(r64["V0"] - r64["V0"].T).max() > 1e-4 * np.abs(r64["V0"]).max()
        assert np.abs(V0 - V0.T).max() > 1e-4 * np.abs(V0).max(), ((n, m, T), b, "V_0 came back symmetric")
    print(f"({n}, {m}) T={T} B={B}: worst error / allowed " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    # the general entry point was taken: the symmetrised problem's gains differ by far more than rounding
    sym_out, sym_status = ws.launch(sym, idx, T)
    assert sym_status.tolist() == [0] * B
    for b in idx:
        assert (out["K"][b] - sym_out["K"][b]).abs().max() > 1e-3, ((n, m, T), b, "the gains of the symmetrised problem")
    # backward + forward: the bits of solve
    split = ws.launch(gen, idx, T, split=True, general=True)
    for b in idx:
        ws.same_bits(split, b, (out, status), b, ((n, m, T), "backward + forward against fused", b))
    # a batch-shared C (and model) against the tiled one
    F, f, Cn, c, x0 = gen
    pick = [0, B - 1, 1]
    shared = ws.launch((F, f, Cn, c, x0), pick, T, general=True, shared=True)
    tiled = ws.launch((F[[0, 0, 0]], f[[0, 0, 0]], Cn[[0, 0, 0]], c[[0, 0, 0]], x0[pick]), range(3), T, general=True)
    for pos in range(3):
        ws.same_bits(shared, pos, tiled, pos, ((n, m, T), "shared model against tiled", pos))
    ws.same_bits(shared, 0, (out, status), 0, ((n, m, T), "shared model, its own initial state"))

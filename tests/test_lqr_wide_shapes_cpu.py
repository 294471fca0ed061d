"""The conditions the wide-shape GPU tests (test_lqr_wide_shapes_gpu.py, test_tvlqr_wide_shapes_gpu.py) rest on, from the
references alone -- no GPU:

* both oracle precisions are finite at every shape of tests/wide_shapes_ref.py, and the fp32 oracle's error against fp64
  (the accuracy rule's denominator) is printed per tensor;
* the library names every shape as supported, for the LQR and for the time-varying LQR, and the support boundary at
  m = 24 is where the LDS sizes put it;
* at every shape whose elimination is pivoted in the block kernel (m > 16 or m + 1 + n > 64 -- every shape of the table)
  at least three of the five instances perform a row exchange on their fp64 Q_uu sequence.  The count is a condition of the
  GPU tests, not a measurement of the kernel.  m = 1 is the exception the arithmetic forces: a 1 x 1 system has no second
  row, so (65, 1) is asserted to have none.

Counts found with the seeds of wide_shapes_ref.SEEDS (instances 0..4, exchanges summed over the T = 4 steps; T = 53 at
(48, 16)):  (49, 16) 0/2/3/4/0   (56, 24) 6/1/2/5/2   (70, 4) 1/2/0/1/0   (8, 66) 25/4/12/15/9   (1, 65) 47/20/44/25/50
(65, 1) none   (48, 16) 0/4/2/4/2   (63, 24) 1/1/7/0/4   (24, 24) 1/6/0/8/0.
"""

import numpy as np
import pytest

import wide_shapes_ref as ws
from tfmpc import _hip


@pytest.mark.parametrize("n,m,T", ws.SHAPES + (("boundary", ws.BOUNDARY_M, 4),))
def test_oracles_are_finite_and_the_library_names_the_shape_supported(n, m, T):
    lib = _hip.load()
    if n == "boundary":
        n = ws.boundary_n(lib)
    assert lib.tfmpc_lqr_kernel_name(n, m, T) not in (b"unsupported", b"invalid"), (n, m)
    assert lib.tfmpc_tvlqr_kernel_name(n, m, T) == b"tv_generic_wave", (n, m)
    _, ref64, ref32 = ws.case(n, m, T)
    assert ref64["status"] == 0 and ref32["status"] == 0
    for key in ws.FIELDS:
        assert np.isfinite(ref64[key]).all() and np.isfinite(ref32[key]).all(), (n, m, key)
        scale = np.abs(ref64[key]).max()
        err = np.abs(ref32[key].astype(np.float64) - ref64[key]).max()
        print(f"({n}, {m}) T={T} {key}: scale {scale:.3g}, fp32 oracle error {err / scale:.2e} of scale")


def test_support_boundary_at_m_24():
    """The wave kernel's LDS need decides what is supported; at the largest n the block kernel no longer fits, so
    the wave kernel is the default there and one more state is refused."""
    lib = _hip.load()
    n = ws.boundary_n(lib)
    assert n == 63
    assert lib.tfmpc_lqr_kernel_name(n, ws.BOUNDARY_M, 4) == b"generic_wave"
    assert lib.tfmpc_lqr_kernel_name(n + 1, ws.BOUNDARY_M, 4) == b"unsupported"
    assert lib.tfmpc_lqr_kernel_name(n - 1, ws.BOUNDARY_M, 4) == b"block_mfma_f32"


@pytest.mark.parametrize("n,m,T", ws.SHAPES + (("boundary", ws.BOUNDARY_M, 4),) + ws.EXTRA_PIVOTED)
def test_pivoted_shapes_exchange_rows(n, m, T):
    if n == "boundary":
        n = ws.boundary_n(_hip.load())
    assert ws.pivoted(n, m), (n, m)
    problem, ref64, _ = ws.case(n, m, T)
    counts = ws.exchange_counts(problem, ref64["V"])
    print(f"({n}, {m}) T={T} seed {ws.seed_of(n, m)}: row exchanges per instance {counts}")
    if m == 1:
        assert counts == [0] * ws.NINST            # nothing to exchange with
    else:
        assert sum(c > 0 for c in counts) >= 3, (n, m, counts, "choose another seed (wide_shapes_ref.SEEDS)")


def test_the_neighbours_case_has_one_exchanging_instance_between_two_that_do_not():
    problem, ref64, _ = ws.case(*ws.NEIGHBOURS[:3])
    counts = ws.exchange_counts(problem, ref64["V"])
    left, mid, right = ws.NEIGHBOURS[3]
    assert counts[left] == 0 and counts[right] == 0 and counts[mid] > 0, counts


def test_the_register_path_shape_and_the_old_generator_do_not_exchange():
    """(33, 3) never leaves the block kernel's register elimination (no pivoting there); and the generator of
    test_lqr_block_gpu.py (eigenvalues of C in [1, 2]) exchanges nothing at the shapes that test runs pivoted -- the gap
    the spd instances close."""
    import problems
    from oracle import c_oracle
    assert not ws.pivoted(33, 3)
    for n, m in ((24, 24), (49, 16)):
        F, f, C, c, x0 = problems.make_lqr_batch_fast(ws.NINST, n, m, seed=97 * n + m)
        F *= 1.5 / np.sqrt(n)
        ref64 = c_oracle.lqr_solve(F, f, C, c, x0, 4, dtype=np.float64, want_policy=True, want_value=True)
        assert ws.exchange_counts((F, f, C, c, x0), ref64["V"]) == [0] * ws.NINST


def test_exchange_counter_on_known_matrices():
    assert ws.exchanges(np.eye(5)) == 0
    assert ws.exchanges(np.array([[0.0, 1.0], [1.0, 0.0]])) == 1
    assert ws.exchanges(np.array([[1.0, 2.0], [-1.0, 0.0]])) == 0           # a tie: the first row of maximal |entry| stays
    P = np.roll(np.eye(6), 1, axis=0) * np.arange(1.0, 7.0)                   # cyclic permutation times a diagonal
    assert ws.exchanges(P) == 5


@pytest.mark.parametrize("m", [8, 24, 66])
def test_permuted_diagonal_instances(m):
    """The instances of the general-inverse test: C_uu = P D has a zero diagonal, every pivot but the last needs an exchange,
    and K_t = -D^-1 P' C_ux at every step (F_u = 0)."""
    from oracle import lqr_ref
    n, T = 8, 3
    F, f, C, c, x0, D, perm = ws.make_permuted(n, m, B=2, seed=m)
    for b in range(2):
        Cuu = C[b, n:, n:]
        assert (np.diag(Cuu) == 0).all() and np.abs(Cuu - Cuu.T).max() > 0.5
        assert ws.exchanges(Cuu) == m - 1
        *_, pol, _ = lqr_ref.solve(F[b], f[b], C[b], c[b], x0[b], T)
        want = -(C[b, n:, :n] / D[b][:, None])[perm]                # row j of the gain: row perm[j] of C_ux over D[perm[j]]
        for t in range(T):
            np.testing.assert_allclose(pol[t][0], want, rtol=0, atol=1e-12)
        r32 = lqr_ref.solve(F[b], f[b], C[b], c[b], x0[b], T, dtype=np.float32)
        assert all(np.isfinite(a).all() for a in r32[:3])

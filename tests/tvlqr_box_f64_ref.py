"""TEST INFRASTRUCTURE ONLY -- the yardstick of the double-precision control-limited solve (``tfmpc_tvlqr_box_solve_f64``,
DESIGN.md §3.18): genuinely double operands, the restatement of tests/tvlqr_box_solve_ref.py run in fp64 (the budget)
and in x86 80-bit longdouble with ``tol = 1e-17`` (the reference), the exact held sets, and the project's double budget
rule (tests/test_tvlqr_f64_gpu.py): per output and instance, the error against the longdouble run over max(the fp64
restatement's error against it, 2^-48 max(1, |ref|_inf)); the median over instances <= 2.5 and every instance <= 10.

Every case is computed once per process and is read-only.
"""

import functools

import numpy as np

import lqr_box_grad_ref as bref
import tvlqr_box_solve_ref as sref

LD = np.longdouble
FLOOR = 2.0 ** -48
MEDIAN_BOUND, MAX_BOUND = 2.5, 10.0
LD_TOL = 1e-17
OUTPUTS = ("states", "actions", "costs")
SEED, BATCH = 5, 4
PERTURBATION = 1e-9

# (n, m, T, width of the bounds): the shapes and horizons of the GPU test.  The last one holds every control of every
# step, the `held == all_held` exit of the box-QP at the full 32-bit mask word.
CASES = [(1, 1, 1, 1.0), (5, 3, 2, 1.0), (5, 3, 20, 1.0), (3, 5, 20, 1.0), (16, 8, 50, 1.0), (16, 16, 4, 1.0), (17, 8, 4, 1.0),
         (16, 17, 4, 1.0), (8, 32, 4, 1.0), (32, 32, 4, 1.0), (8, 32, 4, 1e-3)]
# the share of instances whose held set is `clear` (multipliers and slacks above lqr_box_grad_ref.CLEAR), over all CASES
# and in every single case
CLEAR_SHARE_ALL, CLEAR_SHARE_EACH = 0.9, 0.5
# the rescued class: (mean spectral radius of the state block, width of the bounds)
RESCUED = [(1.35, 0.02), (1.25, 0.05)]


def perturb(ops, seed=SEED):
    """Every entry times (1 + 1e-9 N(0, 1)), C (and an explicit C_fin) re-symmetrised: operands that are no fp32 numbers,
    so that a path which rounds through fp32 misses the double budget by seven orders."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in ("F", "f", "C", "c", "x0", "low", "high", "Cfin", "cfin"):
        a = ops.get(k)
        if a is None:
            out[k] = None
            continue
        a = a * (1.0 + PERTURBATION * rng.standard_normal(a.shape))
        if k in ("C", "Cfin"):
            a = 0.5 * (a + np.swapaxes(a, -1, -2))
        out[k] = a
    return out


def references(ops, u_init=None):
    """-> (exact solution of ``solve_box_batch``, longdouble restatement, fp64 restatement) of batched operands."""
    args = (ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["low"], ops["high"], ops.get("Cfin"), ops.get("cfin"))
    sol = bref.solve_box_batch(*args)
    rld = sref.solve_batch(*args, u_init=u_init, dtype=LD, tol=LD_TOL)
    r64 = sref.solve_batch(*args, u_init=u_init, dtype=np.float64)
    return sol, rld, r64


@functools.lru_cache(maxsize=None)
def case(n, m, T, width=1.0, B=BATCH, final=False):
    """``lqr_box_grad_ref.tv_case`` perturbed: (operands, exact solution, longdouble restatement, fp64 restatement)."""
    ops, _ = bref.tv_case(n, m, T, B, final=final, width=width)
    ops = perturb(ops)
    return (ops, *references(ops))


@functools.lru_cache(maxsize=None)
def rescued_operands(rho, width, n=16, m=8, T=50, B=6):
    """``tv_case(16, 8, 50, 6, width)`` with each instance's state block F[..., :n] scaled so that its spectral radius,
    averaged over t, is ``rho``; fp32-representable.  Along stretches where every control is held V grows like
    rho^(2 (T - t)) and fp32 loses C_uu in the rounding of F^T V F."""
    ops, _ = bref.tv_case(n, m, T, B, width=width)
    F = ops["F"].copy()
    for b in range(B):
        radius = np.mean([np.abs(np.linalg.eigvals(F[b, t, :, :n])).max() for t in range(T)])
        F[b, :, :, :n] *= rho / radius
    return dict(ops, F=F.astype(np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def rescued(rho, width):
    """-> (operands, longdouble restatement, fp64 restatement, fp32 restatement)."""
    ops = rescued_operands(rho, width)
    args = (ops["F"], ops["f"], ops["C"], ops["c"], ops["x0"], ops["low"], ops["high"])
    return (ops, sref.solve_batch(*args, dtype=LD, tol=LD_TOL), sref.solve_batch(*args, dtype=np.float64),
            sref.solve_batch(*args, dtype=np.float32))


def held_from_actions(actions, low, high):
    """A control is held iff it carries a bound's (double) bits."""
    a = np.asarray(actions, dtype=np.float64)
    return (a == np.broadcast_to(low, a.shape)) | (a == np.broadcast_to(high, a.shape))


def instance_error(got, ref):
    """Per instance: max |got - ref| over everything behind the batch axis, taken in longdouble."""
    B = ref.shape[0]
    return np.abs(np.asarray(got, dtype=LD).reshape(B, -1) - np.asarray(ref, dtype=LD).reshape(B, -1)).max(1).astype(np.float64)


def ratios(got, r64, rld):
    """The budget rule's ratio per instance for one output."""
    B = rld.shape[0]
    floor = FLOOR * np.maximum(1.0, np.abs(rld.reshape(B, -1)).max(1).astype(np.float64))
    err = instance_error(got, rld)
    assert np.isfinite(err).all(), err
    return err / np.maximum(instance_error(r64, rld), floor)


def check(got, r64, rld, what, pick=None):
    """Assert the rule on states, actions and costs; -> {output: (median, max)}."""
    out = {}
    for name in OUTPUTS:
        r = ratios(got[name], r64[name], rld[name])
        if pick is not None:
            r = r[pick]
        out[name] = (float(np.median(r)), float(r.max()))
        print(f"budget {what} {name}: median {out[name][0]:.3g} max {out[name][1]:.3g}")
        assert out[name][0] <= MEDIAN_BOUND and out[name][1] <= MAX_BOUND, (what, name, out[name])
    return out

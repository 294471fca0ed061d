"""The periodic infinite-horizon LQR in double (tfmpc_tvlqr_periodic_steady_state_f64) without a GPU: the
numpy restatement of tests/tvlqr_periodic_ref.py against the brute-force recursion, against the stationary solver at
N = 1, across segment counts and on the status cases; then the C ABI's workspace formula, kernel names and argument
checks, none of which launches anything.

The budget rule is tvlqr_f64_ref's: per output and instance, error against the longdouble restatement over
max(budget, 2^-48 max(1, |ref|)); median over instances <= 2.5 and every instance <= 10."""
import ctypes
import functools

import numpy as np
import pytest

import lqr_steady_state_ref as ssref
import tvlqr_f64_ref as ref64
import tvlqr_periodic_ref as pr
import tvlqr_ref
import tvlqr_time_parallel_ref as tp
from tfmpc import _hip

LD = np.longdouble
B = 3
# longdouble restatement against the brute-force recursion, relative to max(1, |brute|): the worst case measured over
# SMALL (three instances each) was 1.28e-18; the bound is four times that
BRUTE_BOUND = 4 * 1.28e-18
SMALL = [(3, 2, 4, 2), (5, 3, 7, 3), (16, 8, 6, 3)]


@functools.lru_cache(maxsize=None)
def _case(n, m, N, segments, unscaled=False):
    """Operands and both restatements, computed once; no test writes to them."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = tp.perturbed(make, n, m, N, B, seed=n * 100 + m)
    rld = pr.solve_batch(F, f, C, c, segments, dtype=LD)
    r64 = pr.solve_batch(F, f, C, c, segments)
    return F, f, C, c, rld, r64


def _floor_only(rld):
    """A budget of zero: the rule's floor alone."""
    return [{name: r[name] for name in pr.FIELDS} for r in rld]


@pytest.mark.parametrize("n,m,N,segments", SMALL)
def test_the_longdouble_restatement_is_the_brute_force_fixed_point(n, m, N, segments):
    F, f, C, c, rld, _ = _case(n, m, N, segments)
    worst = 0.0
    for b in range(B):
        assert rld[b]["status"] == 0
        br = pr.brute(F[b], f[b], C[b], c[b])
        assert br["periods"] <= 4096                      # (the cost of the brute force is capped: small scaled shapes only)
        for name in pr.FIELDS:
            rel = float(np.abs(rld[b][name] - br[name]).max() / max(1.0, float(np.abs(br[name]).max())))
            worst = max(worst, rel)
    print(f"longdouble restatement against brute force ({n}, {m}, {N}, {segments}): {worst:.3g} relative")
    assert worst <= BRUTE_BOUND


@pytest.mark.parametrize("n,m,N,segments", SMALL + [(16, 8, 1, 1), (17, 8, 5, 2), (16, 17, 3, 1), (8, 32, 4, 4)])
def test_the_fp64_restatement_is_within_the_floor_of_the_longdouble_one(n, m, N, segments):
    """On scaled models the fp64 restatement's error is a fraction of the floor 2^-48 max(1, |ref|) (0.1 - 1.5 floors
    measured): it is held to the rule with the floor alone as the budget."""
    _, _, _, _, rld, r64 = _case(n, m, N, segments)
    assert all(r["status"] == 0 for r in rld + r64)
    got = {name: [r[name] for r in r64] for name in pr.FIELDS}
    pr.check(got, rld, _floor_only(rld), what=(n, m, N, segments))
    for a, b in zip(rld, r64):
        assert abs(a["iterations"] - b["iterations"]) <= 1 and 1 <= b["iterations"] <= 10
        assert np.isfinite(b["residual"]) and b["residual"] >= 0.0


@pytest.mark.parametrize("n,m", [(16, 8), (5, 3)])
def test_one_step_periods_agree_with_the_stationary_solver(n, m):
    F, f, C, c, rld, r64 = _case(n, m, 1, 1)
    got = dict(K=[], k=[], V=[], v=[])
    for b in range(B):
        ss = ssref.steady_state(F[b, 0], f[b, 0], C[b, 0], c[b, 0])
        assert ss["status"] == 0
        for name, key in zip(pr.FIELDS, ("K", "k", "P", "p")):
            got[name].append(ss[key][None])
    pr.check(got, rld, r64, what=("stationary", n, m))


@pytest.mark.parametrize("n,m,N", [(5, 3, 7), (16, 8, 6)])
def test_the_result_does_not_depend_on_the_segment_count(n, m, N):
    F, f, C, c, rld, r64 = _case(n, m, N, 1)
    for segments in (1, 2, N, N + 3):
        res = pr.solve_batch(F, f, C, c, segments)
        got = {name: [r[name] for r in res] for name in pr.FIELDS}
        pr.check(got, rld, r64, what=(n, m, N, segments))


# ---- status ----------------------------------------------------------------------------------------------------------------

def _with_mode(F, C, multipliers, observed):
    """The 'unstab' construction of tests/test_lqr_steady_state_f64_gpu.py (state 0 cut off from the inputs and from the
    other states, its cost decoupled) at EVERY step of one instance's period, step t multiplying the mode by
    ``multipliers[t]``; ``observed=False`` also zeroes the mode's own cost."""
    F, C = F.copy(), C.copy()
    for t, mult in enumerate(multipliers):
        F[t, 0, :] = 0.0
        F[t, :, 0] = 0.0
        F[t, 0, 0] = mult
        C[t, 0, 1:] = 0.0
        C[t, 1:, 0] = 0.0
        if not observed:
            C[t, 0, 0] = 0.0
    return F, C


@pytest.mark.parametrize("observed", [True, False])
@pytest.mark.parametrize("n,m,N,segments", [(5, 3, 4, 2), (16, 8, 3, 1)])
def test_an_uncontrollable_unstable_mode_is_not_stabilising(n, m, N, segments, observed):
    F, f, C, c, _, _ = _case(n, m, N, segments)
    Fb, Cb = _with_mode(F[0], C[0], [1.5] * N, observed)
    for dtype in (np.float64, LD):
        r = pr.solve(Fb, f[0], Cb, c[0], segments, dtype=dtype)
        assert r["status"] == pr.ST_NOT_STABILISING, r["status"]
        assert all(np.isnan(r[name]).all() for name in pr.FIELDS) and np.isnan(r["residual"])


@pytest.mark.parametrize("observed", [True, False])
def test_one_expanding_step_in_a_contracting_period_is_solved(observed):
    n, m, N, segments = 5, 3, 4, 2
    F, f, C, c, _, _ = _case(n, m, N, segments)
    Fb, Cb = _with_mode(F[0], C[0], [0.5, 1.5, 0.5, 0.5], observed)
    r64 = pr.solve(Fb, f[0], Cb, c[0], segments)
    rld = pr.solve(Fb, f[0], Cb, c[0], segments, dtype=LD)
    assert r64["status"] == 0 and rld["status"] == 0
    got = {name: [r64[name]] for name in pr.FIELDS}
    pr.check(got, [rld], _floor_only([rld]), what="expanding step")


def test_a_non_positive_definite_R_at_one_step_is_not_pd():
    n, m, N, segments = 5, 3, 7, 3
    F, f, C, c, _, _ = _case(n, m, N, segments)
    Cb = C[0].copy()
    Cb[4, n:, n:] = -np.eye(m)
    r = pr.solve(F[0], f[0], Cb, c[0], segments)
    assert r["status"] == pr.ST_NOT_PD and np.isnan(r["V"]).all()


def test_one_doubling_step_is_not_enough_for_a_slow_instance():
    n, m = 16, 8
    F, f, C, c = (a.astype(np.float64) for a in ssref.damped_workload(n, m, 1, seed=3, dtype=np.float64))
    slow = pr.solve(F, f, C, c, 1)
    assert slow["status"] == 0 and slow["iterations"] >= 8
    r = pr.solve(F, f, C, c, 1, max_iter=1)
    assert r["status"] == pr.ST_NOT_STABILISING and r["iterations"] == 1


# ---- the C ABI, without a launch -------------------------------------------------------------------------------------------

def test_workspace_formula_and_kernel_names():
    lib = _hip.load()
    assert lib.tfmpc_version() == 320 == _hip.MIN_VERSION         # additive exports
    for (Bk, n, m, N, segments) in [(1, 3, 2, 4, 2), (4, 5, 3, 7, 3), (3, 16, 8, 50, 5), (2, 32, 32, 3, 2), (5, 16, 8, 1, 1),
                                    (3, 8, 32, 4, 9), (7, 17, 8, 5, 2), (0, 3, 2, 4, 2), (2, 3, 2, 4, 0), (2, 0, 2, 4, 1)]:
        assert lib.tfmpc_tvlqr_periodic_workspace_bytes_f64(Bk, n, m, N, segments) == pr.workspace_bytes(Bk, n, m, N, segments)
    name = lambda *a: lib.tfmpc_tvlqr_periodic_kernel_name_f64(*a).decode()          # noqa: E731
    assert name(16, 8, 6, 3) == name(16, 16, 1, 1) == name(1, 1, 1, 1) == "tv_f64_periodic16"
    assert name(17, 8, 5, 2) == name(16, 17, 3, 1) == name(32, 32, 3, 2) == "tv_f64_periodic32"
    assert name(33, 8, 5, 2) == name(8, 33, 5, 2) == "unsupported"
    assert name(0, 8, 5, 2) == name(8, 8, 0, 2) == name(8, 8, 5, 0) == "invalid"


def test_argument_checks_come_before_any_launch():
    lib = _hip.load()
    fn = lib.tfmpc_tvlqr_periodic_steady_state_f64
    buf = (ctypes.c_double * 8)()                  # host memory: a call that got past its checks would not survive it
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(Bk=2, n=3, m=2, N=4, F=p, strides=(0, 0), segments=2, max_iter=0, tol=0.0, status=p, ws=p, ws_bytes=1 << 30):
        model = [F, *strides, p, 0, 0, p, 0, 0, p, 0, 0]
        return fn(Bk, n, m, N, *model, segments, max_iter, tol, None, None, None, None, None, None, status, ws, ws_bytes, None)
    ERR_ARG, ERR_UNSUPPORTED = -1, -2
    assert call(Bk=-1) == ERR_ARG and call(n=0) == ERR_ARG and call(m=0) == ERR_ARG and call(N=0) == ERR_ARG
    assert call(n=33) == ERR_UNSUPPORTED and call(m=33) == ERR_UNSUPPORTED
    assert call(n=33, segments=0) == ERR_UNSUPPORTED            # the model's checks come first
    assert call(F=None) == ERR_ARG and call(strides=(-1, 0)) == ERR_ARG and call(strides=(0, -1)) == ERR_ARG
    assert call(segments=0) == ERR_ARG and call(max_iter=-1) == ERR_ARG and call(tol=-1e-9) == ERR_ARG
    assert call(tol=float("nan")) == ERR_ARG
    assert call(Bk=0, F=None, status=None, ws=None, ws_bytes=0) == 0          # a no-op
    assert call(Bk=0, segments=0) == ERR_ARG
    assert call(status=None) == ERR_ARG
    need = pr.workspace_bytes(2, 3, 2, 4, 2)
    assert call(ws=None) == ERR_ARG and call(ws_bytes=need - 1) == ERR_ARG
    assert call(ws=ctypes.c_void_p(p.value + 4)) == ERR_ARG                   # doubles are carved from it

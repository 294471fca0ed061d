"""Double-precision infinite-horizon LQR on the MI355X (tfmpc_lqr_steady_state_f64 through
tfmpc.solvers.lqr_steady_state(dtype=torch.float64) and LQR.steady_state(dtype=torch.float64)) against
the 80-bit restatement of tests/lqr_steady_state_f64_ref.py, which tests/test_lqr_steady_state_f64_cpu.py pins to the
LAPACK restatement and to scipy.  The budget is that helper's one-precision-up rule.

Operands are the two workloads of tests/lqr_steady_state_ref.py in float64 with F multiplied by 1 + 1e-9 N(0, 1): no
entry of F is representable in fp32, so a path that rounds through fp32 anywhere misses the budget by about 1e6."""

import numpy as np
import pytest
import torch

import lqr_steady_state_f64_ref as ref64
import lqr_steady_state_ref as ssref
import tvlqr_ref
from tfmpc import _hip
from tfmpc.envs import make_lqr_linear_navigation
from tfmpc.solvers import TimeVaryingLQR, lqr_steady_state
from tfmpc.solvers.lqr import LQR

pytestmark = pytest.mark.gpu

FIELDS = ref64.FIELDS
F64 = torch.float64


def _run(F, f, C, c, **kw):
    ss = lqr_steady_state(F, f, C, c, dtype=F64, **kw)
    torch.cuda.synchronize()
    return ss


def _host(ss):
    """Outputs as numpy, batch-major, vectors flat."""
    got = {name: getattr(ss, name).cpu().numpy() for name in FIELDS + ("iterations", "status")}
    got["k"], got["p"] = got["k"][..., 0], got["p"][..., 0]
    return got


_CACHE = {}


def _problem(kind, n, m, B, seed):
    """(operands, references) of a workload, computed once per session; no test writes to them."""
    key = (kind, n, m, B, seed)
    if key not in _CACHE:
        ops = ref64.operands(kind, n, m, B, seed=seed)
        _CACHE[key] = (ops, ref64.references(*ops))
    return _CACHE[key]


SHAPES = [(1, 1, "ss_f64_wave16"), (3, 2, "ss_f64_wave16"), (12, 6, "ss_f64_wave16"), (16, 8, "ss_f64_wave16"),
          (16, 16, "ss_f64_wave16"), (17, 8, "ss_f64_wave32"), (16, 17, "ss_f64_wave32"), (22, 3, "ss_f64_wave32"),
          (32, 16, "ss_f64_wave32"), (32, 32, "ss_f64_wave32")]


@pytest.mark.parametrize("kind", ["make_lqr", "damped"])
@pytest.mark.parametrize("n,m,kernel", SHAPES)
def test_parity_with_the_80_bit_restatement(n, m, kernel, kind):
    assert _hip.load().tfmpc_lqr_steady_state_kernel_name_f64(n, m).decode() == kernel
    (F, f, C, c), refs = _problem(kind, n, m, 6, 10 * n + m)
    ss = _run(F, f, C, c)
    assert all(getattr(ss, name).dtype == F64 for name in FIELDS)
    got = _host(ss)
    assert (got["status"] == 0).all(), got["status"]
    assert all(r["status"] == 0 for r in refs[0])
    ref64.check(got, refs, what=(kind, n, m))
    for j, gj in enumerate(refs[1]):
        assert abs(int(got["iterations"][j]) - gj["iterations"]) <= 1, (j, got["iterations"][j], gj["iterations"])


@pytest.mark.parametrize("kind", ["make_lqr", "damped"])
def test_double_is_worth_having(kind):
    """Per instance, on K and P: the fp32 path's error against the 80-bit result is at least 1e4 times the double
    path's (floored at 2^-48 of the output's scale)."""
    n, m = 16, 8
    (F, f, C, c), refs = _problem(kind, n, m, 6, 10 * n + m)
    got64 = _host(_run(F, f, C, c))
    ss32 = LQR(F, f, C, c, device="cuda").steady_state()
    torch.cuda.synchronize()
    got32 = _host(ss32)
    assert (got64["status"] == 0).all() and (got32["status"] == 0).all()
    for name in ("K", "P"):
        gain = []
        for b, ld in enumerate(refs[0]):
            err64 = max(ref64.error(got64[name][b], ld[name]), ref64.FLOOR * ref64.scale_of(ld[name]))
            gain.append(ref64.error(got32[name][b], ld[name]) / err64)
        print(f"fp32 error / fp64 error, {kind} {name}: min {min(gain):.3g} median {np.median(gain):.3g}")
        assert min(gain) >= 1e4, (kind, name, gain)


@pytest.mark.parametrize("n,m", [(16, 8), (12, 6), (20, 10)])
def test_fixed_point_of_the_double_time_varying_solver(n, m):
    """TimeVaryingLQR.from_lqr(lqr, 20, P, p, dtype=float64) -- another kernel -- returns K, k, P, p at every step.
    Budget: the larger of the steady state's and the error of the fp64 TV restatement started from the 80-bit P, p."""
    B, T = 6, 20
    F, f, C, c = ssref.make_lqr_batch(n, m, B, seed=21)
    lqr = LQR(F, f, C, c, device="cuda")
    ss = lqr.steady_state(dtype=F64)
    assert lqr.last_status is ss.status and int(ss.status.abs().sum()) == 0 and ss.P.dtype == F64
    tv = TimeVaryingLQR.from_lqr(lqr, T, ss.P, ss.p, dtype=F64)
    policy, value = tv.backward()
    torch.cuda.synchronize()
    assert int(tv.last_status.abs().sum()) == 0
    Kt, kt, Vt, vt = (a.cpu().numpy() for a in (policy.K, policy.k[..., 0], value.V, value.v[..., 0]))
    ops = tuple(a.astype(np.float64) for a in (F, f, C, c))
    refs = ref64.references(*ops)
    rep = lambda a: np.repeat(a[None], T, axis=0)          # noqa: E731
    tv64 = [tvlqr_ref.backward(*(rep(a[b]) for a in ops), refs[0][b]["P"].astype(np.float64),
                               refs[0][b]["p"].astype(np.float64), dtype=np.float64) for b in range(B)]
    for t in (0, T // 2, T - 1):
        got = dict(K=Kt[:, t], k=kt[:, t], P=Vt[:, t], p=vt[:, t])
        extra = []
        for b in range(B):
            pol, val = tv64[b]
            rec = dict(K=pol[t][0], k=pol[t][1].reshape(-1), P=val[t][0], p=val[t][1].reshape(-1))
            extra.append({name: ref64.error(rec[name], refs[0][b][name]) for name in FIELDS})
        ref64.check(got, refs, what=("tv", n, m, t), extra=extra)


def test_the_two_entries_agree_on_fp32_representable_operands():
    F, f, C, c = ssref.make_lqr_batch(16, 8, 4, seed=33)
    a = LQR(F, f, C, c, device="cuda").steady_state(dtype=F64)
    b = _run(*(x.astype(np.float64) for x in (F, f, C, c)))
    assert int(a.status.abs().sum()) == 0
    for name in FIELDS + ("iterations", "status"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_the_default_is_untouched():
    F, f, C, c = ssref.make_lqr_batch(16, 8, 4, seed=34)
    lqr = LQR(F, f, C, c, device="cuda")
    a, b = lqr.steady_state(), lqr.steady_state(dtype=torch.float32)
    torch.cuda.synchronize()
    assert int(a.status.abs().sum()) == 0
    for name in FIELDS:
        assert getattr(a, name).dtype == torch.float32 and torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.iterations, b.iterations)


def _batch_with(F, f, C, c, bad):
    """A copy of the batch where instance b of `bad` has been made unstabilisable ('unstab') or given a non-PD R."""
    F, C = F.copy(), C.copy()
    n = F.shape[1]
    for b, kind in bad.items():
        if kind == "unstab":
            F[b, 0, :] = 0.0
            F[b, :, 0] = 0.0
            F[b, 0, 0] = 1.5
            C[b, 0, 1:] = 0.0
            C[b, 1:, 0] = 0.0
        else:
            C[b, n:, n:] = -np.eye(C.shape[1] - n)
    return F, f, C, c


@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (20, 10)])
def test_status_isolation(n, m):
    F, f, C, c = ref64.operands("make_lqr", n, m, 6, seed=41)
    Fb, fb, Cb, cb = _batch_with(F, f, C, c, {1: "unstab", 4: "notpd"})
    got = _host(_run(Fb, fb, Cb, cb))
    assert got["status"][1] == _hip.ST_NOT_STABILISING, got["status"]
    assert got["status"][4] == _hip.ST_NOT_PD, got["status"]
    for b in (1, 4):
        assert all(np.isnan(got[name][b]).all() for name in FIELDS)
    keep = [0, 2, 3, 5]
    assert (got["status"][keep] == 0).all()
    clean = _host(_run(F[keep], f[keep], C[keep], c[keep]))
    for name in FIELDS + ("iterations",):
        assert np.array_equal(got[name][keep], clean[name]), name
    flagged = [ref64.steady_state_gj(Fb[b], fb[b], Cb[b], cb[b])["status"] for b in (1, 4)]
    assert flagged == [ssref.ST_NOT_STABILISING, ssref.ST_NOT_PD]


def test_shared_model_with_per_instance_goals():
    """Navigation: F and C shared by the batch (batch stride 0), c per instance."""
    B, n = 7, 4
    goals = np.random.default_rng(5).normal(size=(B, n, 1))
    lqr = make_lqr_linear_navigation(goals, 0.5, device="cpu")
    F, f, C = (t.numpy().astype(np.float64) for t in (lqr.F, lqr.f[:, 0], lqr.C))
    c = np.concatenate([-2.0 * goals[..., 0], np.zeros((B, n))], axis=1)          # the goals in double
    assert F.ndim == 2 and c.ndim == 2
    got = _host(_run(F, f, C, c))
    assert (got["status"] == 0).all()
    rep = lambda a: np.repeat(a[None], B, axis=0)          # noqa: E731
    ref64.check(got, ref64.references(rep(F), rep(f), rep(C), c), what="navigation")
    for b in range(B):                 # the stationary controller drives every instance to its goal: x* = goal
        xstar = np.linalg.solve(-got["K"][b], got["k"][b])
        assert np.abs(xstar - goals[b, :, 0]).max() <= 1e-12


def test_unbatched_and_mixed_operands():
    n, m = 16, 8
    (F, f, C, c), refs = _problem("make_lqr", n, m, 6, 10 * n + m)
    one = _run(F[0], f[0], C[0], c[0])
    assert tuple(one.K.shape) == (m, n) and tuple(one.k.shape) == (m, 1) and tuple(one.P.shape) == (n, n)
    assert tuple(one.p.shape) == (n, 1) and one.status.dim() == 0 and int(one.status) == 0
    # (the budget rule's median is taken over instances and one instance has none: the un-batched result is held to the
    # bits of instance 0 of the batched call, which the parity test holds to the rule, and to the per-instance bound)
    batched = _run(F, f, C, c)
    for name in FIELDS + ("iterations", "status"):
        assert torch.equal(getattr(one, name), getattr(batched, name)[0]), name
    got = {name: getattr(one, name).cpu().numpy()[None] for name in FIELDS}
    got["k"], got["p"] = got["k"][..., 0], got["p"][..., 0]
    for name in FIELDS:
        assert ref64.ratios(got, tuple(r[:1] for r in refs), name).max() <= ref64.MAX_BOUND, name
    # numpy and tensor operands mixed, with a shared f: same bits as all-numpy with f repeated
    mixed = _run(torch.as_tensor(F, device="cuda"), f[0], C, torch.as_tensor(c))
    plain = _run(F, np.repeat(f[:1], 6, axis=0), C, c)
    for name in FIELDS:
        assert torch.equal(getattr(mixed, name), getattr(plain, name)), name


def test_batch_sizes_zero_and_one_and_null_outputs():
    n, m = 12, 6
    (F, f, C, c), _ = _problem("make_lqr", n, m, 6, 10 * n + m)
    empty = _run(F[:0], f[:0], C[:0], c[:0])
    assert tuple(empty.K.shape) == (0, m, n) and empty.status.numel() == 0 and empty.K.dtype == F64
    single = _run(F[:1], f[:1], C[:1], c[:1])
    pair = _run(F[:2], f[:2], C[:2], c[:2])
    for name in FIELDS + ("iterations", "status"):
        assert torch.equal(getattr(single, name)[0], getattr(pair, name)[0]), name
    # NULL outputs through the raw ABI: only k and status requested
    lib = _hip.load()
    dev = [torch.as_tensor(np.ascontiguousarray(a[:2]), device="cuda") for a in (F, f, C, c)]
    args = []
    for t in dev:
        args += [_hip.ptr(t), t.stride(0)]
    k = torch.empty((2, m), device="cuda", dtype=F64)
    status = torch.empty((2,), dtype=torch.int32, device="cuda")
    rc = lib.tfmpc_lqr_steady_state_f64(2, n, m, *args, 0, 0.0, None, _hip.ptr(k), None, None, None,
                                        _hip.ptr(status), _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(k, pair.k[..., 0]) and torch.equal(status, pair.status)


def test_explicit_max_iter_and_tol():
    F, f, C, c = ref64.operands("damped", 16, 8, 4, seed=71)
    capped = _run(F, f, C, c, max_iter=3)
    assert (capped.status.cpu().numpy() == _hip.ST_NOT_STABILISING).all()
    assert (capped.iterations.cpu().numpy() == 3).all()
    assert all(torch.isnan(getattr(capped, name)).all() for name in FIELDS)
    loose = _run(F, f, C, c, tol=1e-6)
    full = _run(F, f, C, c)
    assert (loose.status.cpu().numpy() == 0).all() and (full.status.cpu().numpy() == 0).all()
    assert (loose.iterations <= full.iterations).all()


def test_reproducible_and_independent_of_batch_position():
    n, m, B = 16, 8, 32
    F, f, C, c = ref64.operands("make_lqr", n, m, B, seed=81)
    a, b = _run(F, f, C, c), _run(F, f, C, c)
    assert int(a.status.abs().sum()) == 0
    for name in FIELDS + ("iterations", "status"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    perm = np.random.default_rng(0).permutation(B)
    shuffled = _run(F[perm], f[perm], C[perm], c[perm])
    for name in FIELDS + ("iterations",):
        assert torch.equal(getattr(shuffled, name), getattr(a, name)[torch.as_tensor(perm, device="cuda")]), name


def test_past_one_round_of_resident_waves():
    """B = 4096 at (16, 8): 256 CUs x 5 waves are resident at once.  A pool of 64 draws, every instance its own copy."""
    B, n, m, pool = 4096, 16, 8, 64
    F, f, C, c = ref64.operands("make_lqr", n, m, pool, seed=91)
    idx = np.arange(B) % pool
    got = _host(_run(F[idx], f[idx], C[idx], c[idx]))
    assert (got["status"] == 0).all(), np.unique(got["status"], return_counts=True)
    sample = np.random.default_rng(1).choice(B, 16, replace=False)
    ref64.check(got, ref64.references(F, f, C, c, idx[sample]), idx=sample, what="B = 4096")
    for name in FIELDS + ("iterations",):          # copies of one draw anywhere in the batch: the same bits
        first = got[name][:pool]
        assert np.array_equal(got[name].reshape(B // pool, *first.shape), np.broadcast_to(first, (B // pool, *first.shape))), name

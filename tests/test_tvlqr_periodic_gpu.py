"""The periodic infinite-horizon LQR in double on the MI355X (tfmpc_tvlqr_periodic_steady_state_f64 through
TimeVaryingLQR.periodic_steady_state and tfmpc.solvers.tvlqr_periodic_steady_state).

Accuracy is the project's double rule with the fp64 restatement's own error as the budget (tests/tvlqr_periodic_ref.py,
which tests/test_tvlqr_periodic_cpu.py pins to the brute-force recursion): per output and instance, the kernel's error
against the longdouble restatement over max(the fp64 restatement's error against it, 2^-48 max(1, |ref|)); median over
instances <= 2.5 and every instance <= 10, on K, k, V, v and the residual, no instance left out.  Strides, batch position,
repetition, NULL outputs, status isolation and stale memory are asserted bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import stale_memory
import tvlqr_f64_ref as ref64
import tvlqr_periodic_ref as pr
import tvlqr_ref
import tvlqr_time_parallel_ref as tp
from tfmpc import _hip
from tfmpc.solvers import PeriodicSteadyState, TimeVaryingLQR, lqr_steady_state, tvlqr_periodic_steady_state
from tfmpc.solvers.lqr import Policy

pytestmark = pytest.mark.gpu

FIELDS = pr.FIELDS
ALL = FIELDS + ("residual", "iterations", "status")
F64 = torch.float64
LD = np.longdouble


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _tv(F, f, C, c, *final, dtype=F64):
    """(f and c as columns: [B, 1, 1] alone would read as [T, n, 1] at n = T = 1)"""
    F, f, C, c, *final = (np.asarray(a, dtype=np.float64) for a in (F, f, C, c, *final))
    return TimeVaryingLQR(F, f[..., None], C, c[..., None], *final, device="cuda", dtype=dtype)


def _host(ss, batched=True):
    """A PeriodicSteadyState as numpy arrays [B, ...], vectors flat."""
    assert isinstance(ss, PeriodicSteadyState)
    torch.cuda.synchronize()
    assert all(getattr(ss, name).dtype == F64 for name in FIELDS + ("residual",))
    assert ss.iterations.dtype == torch.int32 and ss.status.dtype == torch.int32
    got = {name: getattr(ss, name).cpu().numpy() for name in ALL}
    got["k"], got["v"] = got["k"][..., 0], got["v"][..., 0]
    return got if batched else {name: a[None] for name, a in got.items()}


def _solve(F, f, C, c, segments, **kw):
    return _host(_tv(F, f, C, c).periodic_steady_state(segments, **kw))


def _same_bits(a, b, what="", fields=ALL):
    for name in fields:
        assert np.array_equal(a[name], b[name], equal_nan=True), (what, name)


@functools.lru_cache(maxsize=None)
def _case(n, m, N, segments, B, unscaled=False):
    """Operands, the longdouble and the fp64 restatement, computed once; no test writes to them."""
    make = ref64.make_unscaled if unscaled else tvlqr_ref.make_models
    F, f, C, c = tp.perturbed(make, n, m, N, B, seed=n * 100 + m)
    return F, f, C, c, pr.solve_batch(F, f, C, c, segments, dtype=LD), pr.solve_batch(F, f, C, c, segments)


# (n, m, N, segments, B, unscaled): both instantiations, n or m across 16, a one-step period, a short last segment
# ((17, 8, 5, 2): 3 + 2 steps; (16, 8, 50, 5)), len = 1 ((8, 32, 4, 4)), one segment ((16, 17, 3, 1))
CASES = [(3, 2, 4, 2, 4, False), (5, 3, 7, 3, 4, False), (16, 8, 6, 3, 4, False), (16, 8, 1, 1, 4, False),
         (17, 8, 5, 2, 3, False), (16, 17, 3, 1, 3, False), (8, 32, 4, 4, 3, False), (32, 32, 3, 2, 3, False),
         (16, 8, 50, 5, 3, False), (17, 8, 5, 2, 3, True), (16, 8, 6, 3, 4, True)]


@pytest.mark.parametrize("n,m,N,segments,B,unscaled", CASES)
def test_accuracy_against_the_longdouble_restatement(n, m, N, segments, B, unscaled):
    kernel = "tv_f64_periodic16" if n <= 16 and m <= 16 else "tv_f64_periodic32"
    assert _hip.load().tfmpc_tvlqr_periodic_kernel_name_f64(n, m, N, segments).decode() == kernel
    F, f, C, c, rld, r64 = _case(n, m, N, segments, B, unscaled)
    assert all(r["status"] == 0 for r in rld + r64)
    got = _solve(F, f, C, c, segments)
    assert (got["status"] == 0).all(), got["status"]
    what = (n, m, N, segments, "unscaled" if unscaled else "scaled")
    pr.check(got, rld, r64, fields=FIELDS + ("residual",), what=what)
    for b in range(B):
        print(f"residual {what} [{b}]: kernel {got['residual'][b]:.3g} restatement {r64[b]['residual']:.3g}; iterations "
              f"{got['iterations'][b]} / {r64[b]['iterations']}")
    for b in range(B):
        assert 0.0 <= got["residual"][b] <= 64 * r64[b]["residual"], (b, got["residual"][b], r64[b]["residual"])
        assert abs(int(got["iterations"][b]) - r64[b]["iterations"]) <= 1, (b, got["iterations"][b], r64[b]["iterations"])


@pytest.mark.parametrize("n,m,N,segments,B", [(5, 3, 7, 3, 4), (16, 8, 6, 3, 4), (17, 8, 5, 2, 3)])
def test_periodicity_a_finite_sweep_over_one_period_returns_the_cycle(n, m, N, segments, B):
    """TimeVaryingLQR.backward() -- another kernel -- over one period from C_final = V[:, 0], c_final = v[:, 0] returns
    V[:, 0] at step 0 and the periodic gains and values at every step."""
    F, f, C, c, rld, r64 = _case(n, m, N, segments, B)
    ss = _tv(F, f, C, c).periodic_steady_state(segments)
    tv = TimeVaryingLQR(_dev(F), _dev(f[..., None]), _dev(C), _dev(c[..., None]), ss.V[:, 0], ss.v[:, 0], device="cuda", dtype=F64)
    policy, value = tv.backward()
    torch.cuda.synchronize()
    assert int(tv.last_status.abs().sum()) == 0
    got = dict(K=policy.K.cpu().numpy(), k=policy.k.cpu().numpy()[..., 0], V=value.V.cpu().numpy(), v=value.v.cpu().numpy()[..., 0])
    pr.check(got, rld, r64, what=("one period", n, m, N))


@pytest.mark.parametrize("n,m", [(16, 8), (5, 3), (17, 8)])
def test_a_one_step_period_agrees_with_the_stationary_solver(n, m):
    B = 4
    F, f, C, c, rld, r64 = _case(n, m, 1, 1, B)
    ss = lqr_steady_state(F[:, 0], f[:, 0], C[:, 0], c[:, 0], dtype=F64)
    torch.cuda.synchronize()
    assert int(ss.status.abs().sum()) == 0
    got = dict(K=ss.K.cpu().numpy()[:, None], k=ss.k.cpu().numpy()[:, None, :, 0], V=ss.P.cpu().numpy()[:, None],
               v=ss.p.cpu().numpy()[:, None, :, 0])
    pr.check(got, rld, r64, what=("stationary", n, m))
    pr.check(_solve(F, f, C, c, 1), rld, r64, what=("one-step period", n, m))


def test_the_result_composes_with_the_finite_solvers():
    """forward((K, k), x0) rolls one period out; a finite solve over L steps of the tiled model that ends at phase L % N
    with C_final = V[:, L % N], c_final = v[:, L % N] has the periodic gains as its own."""
    n, m, N, segments, B = 16, 8, 6, 3, 4
    F, f, C, c, rld, r64 = _case(n, m, N, segments, B)
    tv = _tv(F, f, C, c)
    ss = tv.periodic_steady_state(segments)
    x0 = _dev(tvlqr_ref.make_x0(n, B)[..., None])
    states, actions, costs = tv.forward((ss.K, ss.k), x0)
    again = tv.forward(Policy(ss.K, ss.k), x0)
    torch.cuda.synchronize()
    assert states.shape == (B, N + 1, n, 1) and actions.shape == (B, N, m, 1)
    assert all(torch.equal(a, b) for a, b in zip((states, actions, costs), again))
    u0 = ss.K[:, 0] @ x0 + ss.k[:, 0]
    assert torch.allclose(actions[:, 0], u0, rtol=1e-12, atol=1e-12)
    L = N + 2
    tile = lambda a: np.concatenate([a, a], axis=1)[:, :L]                   # noqa: E731
    fin = TimeVaryingLQR(_dev(tile(F)), _dev(tile(f)[..., None]), _dev(tile(C)), _dev(tile(c)[..., None]), ss.V[:, L % N],
                         ss.v[:, L % N], device="cuda", dtype=F64)
    policy, value = fin.backward()
    torch.cuda.synchronize()
    assert int(fin.last_status.abs().sum()) == 0
    got = dict(K=policy.K.cpu().numpy(), k=policy.k.cpu().numpy()[..., 0], V=value.V.cpu().numpy(), v=value.v.cpu().numpy()[..., 0])
    tiled = lambda rs: [{name: np.concatenate([r[name], r[name]], axis=0)[:L] for name in FIELDS} for r in rs]      # noqa: E731
    pr.check(got, tiled(rld), tiled(r64), what=("finite solve ending at phase", L % N))


# ---- bits ------------------------------------------------------------------------------------------------------------------

def test_strides_shared_unbatched_numpy_and_noncontiguous_operands_give_the_materialised_bits():
    n, m, N, B, segments = 12, 5, 7, 3, 3
    d = n + m
    # time stride 0 with N > 1: the stationary problem sampled N times, against its materialised copy
    F1, f1, C1, c1 = tp.perturbed(tvlqr_ref.make_models, n, m, 1, B, seed=22)
    views = [_dev(a).expand(B, N, *a.shape[2:]) for a in (F1, f1[..., None], C1, c1[..., None])]
    tv0 = TimeVaryingLQR(*views, device="cuda", dtype=F64)
    assert tv0._model_args()[2] == 0 and tv0.F.data_ptr() == views[0].data_ptr()
    rep = lambda a: np.repeat(a, N, axis=1)                # noqa: E731
    shared_time = _host(tv0.periodic_steady_state(segments))
    assert (shared_time["status"] == 0).all()
    _same_bits(shared_time, _solve(rep(F1), rep(f1), rep(C1), rep(c1), segments), "time stride 0")
    # batch stride 0: one model shared by the batch is an unbatched problem -- the shapes lose the batch axis, the bits are
    # instance 0's
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=23)
    full = _solve(F, f, C, c, segments)
    shared = _tv(F[0], f[0], C[0], c[0])
    assert shared.batch_size is None and shared._model_args()[1] == 0
    ss = shared.periodic_steady_state(segments)
    assert ss.K.shape == (N, m, n) and ss.k.shape == (N, m, 1) and ss.V.shape == (N, n, n) and ss.v.shape == (N, n, 1)
    assert ss.residual.shape == () and ss.iterations.shape == () and ss.status.shape == ()
    one = _host(ss, batched=False)
    for name in ALL:
        assert np.array_equal(one[name][0], full[name][0]), name
    # ... and an operand shared by the batch next to batched ones (F with batch stride 0)
    mixed = TimeVaryingLQR(_dev(F[0]), _dev(f[..., None]), _dev(C), _dev(c[..., None]), device="cuda", dtype=F64)
    assert mixed._model_args()[1] == 0 and mixed.batch_size == B
    _same_bits(_host(mixed.periodic_steady_state(segments)), _solve(np.repeat(F[:1], B, axis=0), f, C, c, segments), "shared F")
    # numpy against non-contiguous tensor views of the same numbers, and the functional form
    Ft = _dev(np.swapaxes(F, -1, -2)).transpose(-1, -2)
    Cw = torch.zeros((B, N, d, 2 * d), dtype=F64, device="cuda")
    Cw[..., ::2] = _dev(C)
    assert not Ft.is_contiguous() and not Cw[..., ::2].is_contiguous()
    tv2 = TimeVaryingLQR(Ft, _dev(f), Cw[..., ::2], _dev(c), device="cuda", dtype=F64)
    _same_bits(_host(tv2.periodic_steady_state(segments)), full, "non-contiguous")
    _same_bits(_host(tvlqr_periodic_steady_state(F, f, C, c, segments)), full, "functional form, numpy")
    _same_bits(_host(tvlqr_periodic_steady_state(_dev(F), _dev(f), _dev(C), _dev(c), segments=segments)), full, "functional form")


@pytest.mark.parametrize("n,m,N,segments", [(16, 8, 11, 4), (20, 10, 5, 5)])
def test_an_instance_alone_gives_its_bits_in_a_batch_and_two_calls_agree(n, m, N, segments):
    B = 3
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=24)
    tv = _tv(F, f, C, c)
    batch, again = _host(tv.periodic_steady_state(segments)), _host(tv.periodic_steady_state(segments))
    assert (batch["status"] == 0).all()
    _same_bits(batch, again, "two calls")
    for b in range(B):
        alone = _solve(F[b:b + 1], f[b:b + 1], C[b:b + 1], c[b:b + 1], segments)
        for name in ALL:
            assert np.array_equal(alone[name][0], batch[name][b]), (name, b)


def test_the_default_segment_count_is_accepted_and_valid():
    n, m, N, B = 5, 3, 200, 2
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=25)
    tv = _tv(F, f, C, c)
    segments = tv.default_segments(B)
    assert 1 < segments <= N
    got = _host(tv.periodic_steady_state())
    assert (got["status"] == 0).all()
    _same_bits(got, _host(tv.periodic_steady_state(segments)), "default")


def _raw(F, f, C, c, segments, want=ALL, fill=None, buffers=None, max_iter=0, tol=0.0):
    """The C entry itself on contiguous [B, N, ...] operands: ``want`` names the outputs that are not NULL; ``fill``
    pre-fills every output and the workspace; ``buffers`` (a dict from an earlier call) is written into again."""
    lib = _hip.require_gpu()
    B, N, n, d = F.shape
    m = d - n
    ops = [_dev(a) for a in (F, f, C, c)]
    shapes = dict(K=(B, N, m, n), k=(B, N, m), V=(B, N, n, n), v=(B, N, n), residual=(B,), iterations=(B,), status=(B,))
    if buffers is None:
        buffers = {name: torch.zeros(shapes[name], device="cuda", dtype=torch.int32 if name in ("iterations", "status") else F64)
                   for name in ALL}
        buffers["workspace"] = torch.zeros(lib.tfmpc_tvlqr_periodic_workspace_bytes_f64(B, n, m, N, segments) // 8, device="cuda", dtype=F64)
    if fill is not None:
        for name, t in buffers.items():
            t.fill_(fill if t.dtype == F64 else stale_memory.NAN_BITS)
    model = []
    for t in ops:
        model += [_hip.ptr(t), t.stride(0), t.stride(1)]
    out = [_hip.ptr(buffers[name]) if name in want else None for name in ALL]
    rc = lib.tfmpc_tvlqr_periodic_steady_state_f64(B, n, m, N, *model, segments, max_iter, tol, *out, _hip.ptr(buffers["workspace"]),
                                                   buffers["workspace"].numel() * 8, _hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {name: buffers[name].cpu().numpy() for name in want}, buffers


def test_null_outputs_leave_the_others_their_bits():
    n, m, N, segments, B = 16, 8, 6, 3, 3
    F, f, C, c, _, _ = _case(n, m, N, segments, B + 1)
    F, f, C, c = F[:B], f[:B], C[:B], c[:B]
    full, _ = _raw(F, f, C, c, segments)
    _same_bits(full, _solve(F, f, C, c, segments), "the C entry and the method")
    optional = ("K", "k", "V", "v", "residual", "iterations")
    subsets = [(), ("K",), ("k", "v"), ("V", "v"), ("K", "k"), ("residual",), ("iterations", "V"), ("K", "V", "residual")]
    for subset in subsets:
        want = tuple(subset) + ("status",)
        got, _ = _raw(F, f, C, c, segments, want=want)
        _same_bits(got, full, subset, fields=want)
    assert set().union(*subsets) == set(optional)


def test_stale_workspace_and_output_memory_is_never_read():
    """Twice into the SAME workspace and outputs, pre-filled with NaN and then with 1e300 -- a clean batch and one with
    flagged instances, whose phases are skipped -- and the front end under tests/stale_memory.py's patch."""
    n, m, N, segments, B = 16, 8, 7, 3, 4
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=27)
    Fb, Cb = _flagged(F, C, {1: "unstab", 2: "notpd"})
    for Fx, Cx in ((F, C), (Fb, Cb)):
        first, buffers = _raw(Fx, f, Cx, c, segments, fill=float("nan"))
        second, _ = _raw(Fx, f, Cx, c, segments, fill=1e300, buffers=buffers)
        _same_bits(first, second, "NaN, then 1e300")
        clean, _ = _raw(Fx, f, Cx, c, segments)
        _same_bits(first, clean, "NaN against zeros")
    tv = _tv(Fb, f, Cb, c)
    ws = _hip.load().tfmpc_tvlqr_periodic_workspace_bytes_f64(B, n, m, N, segments)
    results = []
    for pattern in stale_memory.PATTERNS:
        with stale_memory.StaleMemory(pattern) as mem:
            ss = tv.periodic_steady_state(segments)
        mem.check(ss._asdict(), workspace_bytes=ws)
        results.append(_host(ss))
    for other in results[1:]:
        _same_bits(results[0], other, "patterns")


# ---- status ----------------------------------------------------------------------------------------------------------------

def _flagged(F, C, bad):
    """tests/test_lqr_steady_state_f64_gpu.py's ``_batch_with``: 'unstab' at EVERY step of the instance's period, a
    non-positive-definite R at ONE step."""
    F, C = F.copy(), C.copy()
    n = F.shape[2]
    for b, kind in bad.items():
        if kind == "unstab":
            F[b, :, 0, :] = 0.0
            F[b, :, :, 0] = 0.0
            F[b, :, 0, 0] = 1.5
            C[b, :, 0, 1:] = 0.0
            C[b, :, 1:, 0] = 0.0
        else:
            C[b, F.shape[1] // 2, n:, n:] = -np.eye(C.shape[2] - n)
    return F, C


@pytest.mark.parametrize("n,m,N,segments", [(16, 8, 6, 3), (5, 3, 7, 3), (20, 10, 4, 1)])
def test_status_isolation(n, m, N, segments):
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, 6, seed=41)
    Fb, Cb = _flagged(F, C, {1: "unstab", 4: "notpd"})
    got = _solve(Fb, f, Cb, c, segments)
    assert got["status"][1] == _hip.ST_NOT_STABILISING, got["status"]
    assert got["status"][4] == _hip.ST_NOT_PD, got["status"]
    for b in (1, 4):
        assert all(np.isnan(got[name][b]).all() for name in FIELDS + ("residual",)), b
    keep = [0, 2, 3, 5]
    assert (got["status"][keep] == 0).all()
    clean = _solve(F[keep], f[keep], C[keep], c[keep], segments)
    for name in ALL:
        assert np.array_equal(got[name][keep], clean[name]), name
    flagged = [pr.solve(Fb[b], f[b], Cb[b], c[b], segments)["status"] for b in (1, 4)]
    assert flagged == [pr.ST_NOT_STABILISING, pr.ST_NOT_PD]


def test_an_unobserved_unstable_mode_an_expanding_step_and_a_short_iteration_budget():
    n, m, N, segments, B = 5, 3, 4, 2, 4
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=42)
    Fb, Cb = _flagged(F, C, {0: "unstab", 1: "unstab", 2: "unstab"})
    Cb[1, :, 0, 0] = 0.0                                   # the unstable mode's cost zeroed: unobserved as well
    Fb[2, :, 0, 0] = [0.5, 1.5, 0.5, 0.5]                 # one expanding step, a contracting product
    got = _solve(Fb, f, Cb, c, segments)
    assert list(got["status"]) == [_hip.ST_NOT_STABILISING, _hip.ST_NOT_STABILISING, 0, 0], got["status"]
    refs = [pr.solve_batch(Fb[2:], f[2:], Cb[2:], c[2:], segments, dtype=dt) for dt in (LD, np.float64)]
    pr.check({name: got[name][2:] for name in FIELDS}, *refs, what="expanding step")
    short = _solve(Fb, f, Cb, c, segments, max_iter=1)
    assert (short["status"] == _hip.ST_NOT_STABILISING).all() and (short["iterations"] == 1).all()
    assert np.isnan(short["V"]).all() and np.isnan(short["residual"]).all()


# ---- the front end's refusals ----------------------------------------------------------------------------------------------

def test_fp32_a_final_cost_and_a_grad_operand_are_refused_before_any_launch(monkeypatch):
    n, m, N, B = 5, 3, 4, 2
    F, f, C, c = tp.perturbed(tvlqr_ref.make_models, n, m, N, B, seed=43)
    launched = []
    monkeypatch.setattr(_hip, "require_gpu", lambda: launched.append(1))
    with pytest.raises(NotImplementedError, match="dtype=torch.float64"):
        _tv(F, f, C, c, dtype=torch.float32).periodic_steady_state()
    with pytest.raises(NotImplementedError, match="dtype=torch.float64"):
        tvlqr_periodic_steady_state(F.astype(np.float32), f, C, c)
    Cf, cf = (a.astype(np.float64) for a in tvlqr_ref.make_final(n, B))
    with pytest.raises(ValueError, match="final cost"):
        _tv(F, f, C, c, Cf, cf).periodic_steady_state()
    Fg = _dev(F).requires_grad_()
    with pytest.raises(NotImplementedError, match="[Gg]radients"):
        TimeVaryingLQR(Fg, _dev(f), _dev(C), _dev(c), device="cuda", dtype=F64).periodic_steady_state()
    with pytest.raises(NotImplementedError, match="[Gg]radients"):
        tvlqr_periodic_steady_state(Fg, _dev(f), _dev(C), _dev(c))
    with pytest.raises(ValueError):
        _tv(F, f, C, c).periodic_steady_state(segments=0)
    with pytest.raises(ValueError):
        _tv(F, f, C, c).periodic_steady_state(max_iter=-1)
    assert not launched
    with torch.no_grad():                                  # not recording: the operand's flag asks for nothing
        monkeypatch.undo()
        assert int(TimeVaryingLQR(Fg, _dev(f), _dev(C), _dev(c), device="cuda", dtype=F64).periodic_steady_state(2).status.abs().sum()) == 0

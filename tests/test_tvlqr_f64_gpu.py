"""Double-precision time-varying LQR on the MI355X (tfmpc_tvlqr_*_f64 through TimeVaryingLQR(dtype=torch.float64))
against the longdouble restatement of tests/tvlqr_f64_ref.py.  Budget rule (tvlqr_f64_ref.check): per output and instance,
kernel error against solve_ld over max(error of the fp64 numpy oracle against solve_ld, 2^-48 max(1, |ref|)); the median
over instances <= 2.5 and every instance <= 10, on states, actions, costs, K, k, V, v and const."""
import numpy as np
import pytest
import torch

import tvlqr_f64_ref as ref64
import tvlqr_ref
from tfmpc import _hip
from tfmpc.solvers import TimeVaryingLQR
from tfmpc.solvers.lqr import Policy
from tfmpc.utils.trajectory import Trajectory

pytestmark = pytest.mark.gpu

FIELDS = ref64.FIELDS
F64 = torch.float64


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _host(out):
    got = {k: out[k].cpu().numpy() for k in FIELDS if k in out}
    B = got["states"].shape[0]
    got["states"] = got["states"][..., 0]
    got["actions"] = got["actions"][..., 0]
    got["costs"] = got["costs"].reshape(B, -1)
    if "k" in got:
        got["k"] = got["k"][..., 0]
    if "v" in got:
        got["v"] = got["v"][..., 0]
        got["const"] = got["const"].reshape(B, -1)
    return got


def _tv(F, f, C, c, *final, **kw):
    return TimeVaryingLQR(*(np.asarray(a, dtype=np.float64) for a in (F, f, C, c, *final)), device="cuda", dtype=F64, **kw)


def _solve(tv, x0):
    out = tv.solve_device(_dev(x0[..., None]), want_policy=True, want_value=True)
    torch.cuda.synchronize()
    for name in FIELDS:
        assert out[name].dtype == F64, name
    return out


def _same_bits(a, b, fields=FIELDS, what=""):
    for name in fields:
        assert torch.equal(a[name], b[name]), (what, name)


def _name(n, m):
    return _hip.load().tfmpc_tvlqr_kernel_name_f64(n, m, 50).decode()


# ---- (a) the tile map, exact -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [16, 17, 32])
def test_tile_map_with_exact_integer_data(n):
    """T = 1, C_ux = 0, F_u = 0, C_uu = 2 I: V_0 = C_xx + F_x^T C_fin F_x, all integers far below 2^53 -- every product
    and sum is exact whatever its order, so a wrong row map or edge pad of the f64 matrix instruction cannot pass."""
    m, d = 2, n + 2
    rng = np.random.default_rng(n)
    Fx = rng.integers(-3, 4, size=(n, n))
    assert not np.array_equal(Fx, Fx.T)
    A, Bm = rng.integers(-3, 4, size=(n, n)), rng.integers(-3, 4, size=(n, n))
    Cxx, Cfin = A + A.T, Bm + Bm.T
    F = np.zeros((1, 1, n, d))
    F[0, 0, :, :n] = Fx
    C = np.zeros((1, 1, d, d))
    C[0, 0, :n, :n] = Cxx
    C[0, 0, n:, n:] = 2 * np.eye(m)
    tv = _tv(F, np.zeros((1, 1, n)), C, np.zeros((1, 1, d)), Cfin[None].astype(np.float64), np.zeros((1, n)))
    out = _solve(tv, np.zeros((1, n)))
    assert int(out["status"][0]) == 0
    expect = Cxx + Fx.T @ Cfin @ Fx                            # integer numpy
    got = out["V"][0, 0].cpu().numpy()
    assert (got == expect).all(), np.argwhere(got != expect)[:8]
    assert (out["K"].cpu().numpy() == 0).all() and (out["v"].cpu().numpy() == 0).all()


# ---- (b) shapes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,T,kernel", [(1, 1, 20, "tv_f64_wave16"), (3, 2, 20, "tv_f64_wave16"), (12, 5, 20, "tv_f64_wave16"),
                                          (16, 8, 20, "tv_f64_wave16"), (16, 16, 20, "tv_f64_wave16"),
                                          (17, 8, 20, "tv_f64_wave32"), (16, 17, 20, "tv_f64_wave32"),
                                          (20, 10, 20, "tv_f64_wave32"), (5, 20, 20, "tv_f64_wave32"),
                                          (32, 32, 6, "tv_f64_wave32")])
def test_shapes_per_instance_time_varying(n, m, T, kernel):
    assert _name(n, m) == kernel
    B = 6
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=n * 100 + m)
    x0 = tvlqr_ref.make_x0(n, B)
    out = _solve(_tv(F, f, C, c), x0)
    assert int(out["status"].abs().sum()) == 0
    ref64.check(_host(out), *ref64.references(F, f, C, c, x0), what=(n, m, T))


# ---- (c) horizons (the kernel has no chunk and no ring: one step at a time) ---------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 3, 50, 257])
@pytest.mark.parametrize("n,m", [(16, 8), (12, 5)])
def test_horizons(n, m, T):
    B = 3
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=T)
    x0 = tvlqr_ref.make_x0(n, B, seed=T)
    out = _solve(_tv(F, f, C, c), x0)
    assert int(out["status"].abs().sum()) == 0
    ref64.check(_host(out), *ref64.references(F, f, C, c, x0), what=(n, m, T))


# ---- (d) strides ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_batch_shared_model_and_shared_x0(n, m):
    B, T = 4, 21
    F, f, C, c = (a[0] for a in tvlqr_ref.make_models(n, m, T, 1, seed=7))
    x0 = tvlqr_ref.make_x0(n, B)
    tv = _tv(F, f, C, c)
    assert tv.batch_size is None and tv._model_args()[1] == 0
    out = _solve(tv, x0)
    rep = lambda a: np.repeat(a[None], B, axis=0)          # noqa: E731
    ref64.check(_host(out), *ref64.references(rep(F), rep(f), rep(C), rep(c), x0), what="shared model")
    # one x0 for a batched model
    Fb, fb, Cb, cb = tvlqr_ref.make_models(n, m, T, B, seed=8)
    out = TimeVaryingLQR(*(_dev(a) for a in (Fb, fb, Cb, cb)), device="cuda", dtype=F64).solve_device(
        _dev(x0[0][:, None]), want_policy=True, want_value=True)
    assert out["states"].shape == (B, T + 1, n, 1)
    ref64.check(_host(out), *ref64.references(Fb, fb, Cb, cb, np.repeat(x0[:1], B, axis=0)), what="shared x0")


@pytest.mark.parametrize("n,m", [(16, 8), (3, 2), (20, 10)])
def test_time_stride_zero_and_constant_costs(n, m):
    B, T = 4, 19
    F, f, C, c = tvlqr_ref.make_models(n, m, 1, B, seed=11)
    x0 = tvlqr_ref.make_x0(n, B)
    views = [_dev(a).expand(B, T, *a.shape[2:]) for a in (F, f, C, c)]
    tv = TimeVaryingLQR(*views, device="cuda", dtype=F64)
    assert tv.horizon == T and tv._model_args()[2] == 0 and tv.F.data_ptr() == views[0].data_ptr()
    out = _solve(tv, x0)
    rep = lambda a: np.repeat(a, T, axis=1)                # noqa: E731
    ref64.check(_host(out), *ref64.references(rep(F), rep(f), rep(C), rep(c), x0), what="time stride 0")
    # dynamics varying in time, costs constant (time axis 1)
    Fv, fv, _, _ = tvlqr_ref.make_models(n, m, T, B, seed=12)
    tv = _tv(Fv, fv, C, c)
    assert tv._model_args()[8] == 0 and tv._model_args()[2] != 0
    out = _solve(tv, x0)
    ref64.check(_host(out), *ref64.references(Fv, fv, rep(C), rep(c), x0), what="constant costs")


def test_unbatched_problem():
    n, m, T = 12, 5, 17
    F, f, C, c = (a[0] for a in tvlqr_ref.make_models(n, m, T, 1, seed=13))
    x0 = tvlqr_ref.make_x0(n, 1)
    tv = _tv(F, f, C, c)
    policy, value = tv.backward()
    states, actions, costs = tv.forward(policy, _dev(x0[0][:, None]))
    torch.cuda.synchronize()
    assert states.shape == (T + 1, n, 1) and policy.K.shape == (T, m, n) and value.V.shape == (T, n, n)
    assert all(t.dtype == F64 for t in (states, actions, costs, policy.K, policy.k, value.V, value.v, value.const))
    got = dict(states=states[None], actions=actions[None], costs=costs[None], K=policy.K[None], k=policy.k[None],
               V=value.V[None], v=value.v[None], const=value.const[None])
    ref64.check(_host(got), *ref64.references(F[None], f[None], C[None], c[None], x0), what="unbatched")


@pytest.mark.parametrize("n,m", [(16, 8), (17, 8)])
def test_explicit_final_cost_equal_to_the_default_gives_the_same_bits(n, m):
    B, T = 3, 9
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=14)
    x0 = tvlqr_ref.make_x0(n, B)
    a = _solve(_tv(F, f, C, c), x0)
    b = _solve(_tv(F, f, C, c, C[:, T - 1, :n, :n], c[:, T - 1, :n]), x0)
    _same_bits(a, b, what="final")
    # ... and another final cost is another problem, checked against the restatement
    Cf, cf = tvlqr_ref.make_final(n, B)
    out = _solve(_tv(F, f, C, c, Cf, cf), x0)
    ref64.check(_host(out), *ref64.references(F, f, C, c, x0, Cf, cf), what="final cost")


@pytest.mark.parametrize("n,m,batched", [(16, 8, True), (20, 10, False)])
def test_time_invariant_gives_the_bits_of_the_materialised_model(n, m, batched):
    B, T = 3, 23
    F, f, C, c = (a[:, 0] if batched else a[0, 0] for a in tvlqr_ref.make_models(n, m, 1, B, seed=15))
    F = F.astype(np.float64) + 1e-10                       # not an fp32 problem
    x0 = tvlqr_ref.make_x0(n, B)
    tv = TimeVaryingLQR.time_invariant(F, f, C, c, T, device="cuda", dtype=F64)
    assert tv.dtype == F64 and tv.horizon == T and tv.F.stride(-3) == 0 and tv._model_args()[2] == 0
    tax = 1 if batched else 0
    mat = lambda a: np.repeat(np.expand_dims(np.asarray(a, dtype=np.float64), tax), T, axis=tax)      # noqa: E731
    Fm, fm, Cm, cm = mat(F), mat(f), mat(C), mat(c)
    a, b = _solve(tv, x0), _solve(_tv(Fm, fm, Cm, cm), x0)
    _same_bits(a, b, what="time_invariant")
    full = (lambda x: x) if batched else (lambda x: np.repeat(x[None], B, axis=0))      # noqa: E731
    ref64.check(_host(a), *ref64.references(full(Fm), full(fm), full(Cm), full(cm), x0), what="time_invariant")


# ---- (e) split equals fused ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,T", [(16, 8, 53), (20, 10, 9)])
def test_backward_then_forward_gives_the_bits_of_the_fused_solve(n, m, T):
    B = 4
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=16)
    x0 = _dev(tvlqr_ref.make_x0(n, B)[..., None])
    tv = _tv(F, f, C, c)
    fused = tv.solve_device(x0, want_policy=True, want_value=True)
    policy, value = tv.backward()
    states, actions, costs = tv.forward(policy, x0)
    split = dict(states=states, actions=actions, costs=costs, K=policy.K, k=policy.k, V=value.V, v=value.v, const=value.const)
    lean = tv.solve_device(x0)                              # gains in the workspace
    torch.cuda.synchronize()
    assert "K" not in lean and lean["workspace"].dtype == F64
    assert lean["workspace"].numel() * 8 >= _hip.load().tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T)
    _same_bits(fused, split, what="split")
    _same_bits(fused, lean, fields=("states", "actions", "costs"), what="workspace")
    assert int(fused["status"].abs().sum()) == 0 and int(lean["status"].abs().sum()) == 0 and int(tv.last_status.abs().sum()) == 0


# ---- (f) what double precision buys ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_unscaled_models_gain_four_digits_over_the_fp32_path(seed):
    n, m, T, B = 16, 8, 50, 6
    F, f, C, c = ref64.make_unscaled(n, m, T, B, seed)
    x0 = tvlqr_ref.make_x0(n, B, seed=seed)
    rld, r64 = ref64.references(F, f, C, c, x0)
    out64 = _solve(_tv(F, f, C, c), x0)
    assert int(out64["status"].abs().sum()) == 0
    got64 = _host(out64)
    ref64.check(got64, rld, r64, what=("unscaled", seed))
    out32 = TimeVaryingLQR(F, f, C, c, device="cuda").solve_device(
        torch.as_tensor(x0[..., None], device="cuda"), want_policy=True, want_value=True)
    torch.cuda.synchronize()
    assert out32["states"].dtype == torch.float32 and int(out32["status"].abs().sum()) == 0
    got32 = _host(out32)
    for name in ("states", "actions", "K", "V"):
        for b in range(B):
            e64, e32 = ref64.error(got64[name][b], rld[b][name]), ref64.error(got32[name][b], rld[b][name])
            print(f"unscaled seed {seed} {name}[{b}]: fp64 error {e64:.3g}, fp32 error {e32:.3g}, gain {e32 / max(e64, 1e-300):.3g}")
            assert e64 * 1e4 <= e32, (name, b, e64, e32)


# ---- (g) statuses ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_statuses_are_per_instance(n, m):
    B, T = 4, 11
    F, f, C, c = (a.astype(np.float64) for a in tvlqr_ref.make_models(n, m, T, B, seed=17))
    x0 = tvlqr_ref.make_x0(n, B)
    alone = [_solve(_tv(F[b:b + 1], f[b:b + 1], C[b:b + 1], c[b:b + 1]), x0[b:b + 1]) for b in range(B)]
    C_bad = C.copy()
    C_bad[1, 6, n:, n:] = -1e3 * np.eye(m)                  # Q_uu = C_uu + F_u^T V F_u: indefinite at step 6 of instance 1
    out = _solve(_tv(F, f, C_bad, c), x0)
    status = out["status"].cpu().numpy()
    assert status[1] & _hip.ST_NOT_PD and (status[[0, 2, 3]] == 0).all(), status
    for b in (0, 2, 3):
        for name in FIELDS:
            assert torch.equal(out[name][b], alone[b][name][0]), ("not pd", name, b)
    f_bad = f.copy()
    f_bad[2, 3, 1] = np.nan
    out = _solve(_tv(F, f_bad, C, c), x0)
    status = out["status"].cpu().numpy()
    assert status[2] == _hip.ST_NAN and (status[[0, 1, 3]] == 0).all(), status
    for b in (0, 1, 3):
        for name in FIELDS:
            assert torch.equal(out[name][b], alone[b][name][0]), ("nan", name, b)


# ---- (h) types -----------------------------------------------------------------------------------------------------------------

def test_types_numpy_and_noncontiguous_inputs():
    n, m, T, B = 12, 5, 9, 3
    d = n + m
    F, f, C, c = (a.astype(np.float64) for a in tvlqr_ref.make_models(n, m, T, B, seed=18))
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)
    tv = TimeVaryingLQR(F, f, C, c, device="cuda", dtype=F64)         # numpy fp64
    ref = tv.solve_device(x0[..., None], want_policy=True, want_value=True)
    # the same numbers behind non-contiguous views: F stored transposed, C and x0 as every second element
    Ft = _dev(np.swapaxes(F, -1, -2)).transpose(-1, -2)
    Cw = torch.zeros((B, T, d, 2 * d), dtype=F64, device="cuda")
    Cw[..., ::2] = _dev(C)
    xw = torch.zeros((B, 2 * n, 1), dtype=F64, device="cuda")
    xw[:, ::2] = _dev(x0[..., None])
    assert not Ft.is_contiguous() and not Cw[..., ::2].is_contiguous()
    tv2 = TimeVaryingLQR(Ft, _dev(f), Cw[..., ::2], _dev(c), device="cuda", dtype=F64)
    out = tv2.solve_device(xw[:, ::2], want_policy=True, want_value=True)
    torch.cuda.synchronize()
    _same_bits(ref, out, what="non-contiguous")
    traj = tv.solve(x0[..., None])
    assert isinstance(traj, Trajectory)
    assert traj.states.dtype == np.float64 and traj.actions.dtype == np.float64 and traj.costs.dtype == np.float64
    assert np.array_equal(traj.states, ref["states"][..., 0].cpu().numpy())
    states, actions, costs = tv.solve_tensors(x0[..., None])
    assert states.dtype == F64 and torch.equal(states, ref["states"])
    # the split calls on the same problem
    policy, _ = tv.backward()
    assert isinstance(policy, Policy) and policy.K.dtype == F64
    s2, _, _ = tv.forward(policy, x0[..., None])
    assert torch.equal(s2, ref["states"])


def test_the_default_dtype_with_fp64_inputs_is_the_fp32_path():
    n, m, T, B = 16, 8, 12, 3
    F, f, C, c = (a.astype(np.float64) for a in tvlqr_ref.make_models(n, m, T, B, seed=19))
    F = F * (1.0 + 1e-9)                                    # not representable in fp32
    x0 = tvlqr_ref.make_x0(n, B).astype(np.float64)[..., None]
    a = TimeVaryingLQR(F, f, C, c, device="cuda").solve_device(x0, want_policy=True, want_value=True)
    b = TimeVaryingLQR(*(x.astype(np.float32) for x in (F, f, C, c)), device="cuda").solve_device(
        x0.astype(np.float32), want_policy=True, want_value=True)
    torch.cuda.synchronize()
    assert a["states"].dtype == torch.float32
    _same_bits(a, b, what="default dtype")

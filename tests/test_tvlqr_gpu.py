"""Time-varying LQR on the MI355X (tfmpc_tvlqr_*_f32 through tfmpc.solvers.TimeVaryingLQR) against the fp64
restatement of tests/tvlqr_ref.py.  Budget: the fp32 restatement's own error against fp64 -- per instance, the
median over instances of (kernel error / fp32 error) <= 2.5 and every instance <= 10, on states, actions, costs,
K, k, V, v and const."""
import numpy as np
import pytest
import torch

import tvlqr_ref
from tfmpc import _hip
from tfmpc.envs import make_lqr
from tfmpc.solvers import TimeVaryingLQR

pytestmark = pytest.mark.gpu

FIELDS = ("states", "actions", "costs", "K", "k", "V", "v", "const")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


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


def _refs(F, f, C, c, x0, Cf=None, cf=None, idx=None):
    """fp64 and fp32 restatements per instance; operands [B, T, ...] (Cf, cf [B, ...] or None)."""
    B = x0.shape[0]
    idx = range(B) if idx is None else idx
    r64, r32 = [], []
    for b in idx:
        args = (F[b], f[b], C[b], c[b], x0[b], None if Cf is None else Cf[b], None if cf is None else cf[b])
        r64.append(tvlqr_ref.solve(*args, dtype=np.float64))
        r32.append(tvlqr_ref.solve(*args, dtype=np.float32))
    return r64, r32


def _check(got, r64, r32, idx=None, fields=FIELDS, what=""):
    idx = list(range(len(r64))) if idx is None else list(idx)
    for name in fields:
        ratios = []
        for j, b in enumerate(idx):
            ref = r64[j][name]
            scale = max(1.0, float(np.abs(ref).max()))
            budget = max(float(np.abs(r32[j][name] - ref).max()), 1e-6 * scale)
            err = float(np.abs(got[name][b] - ref).max())
            assert np.isfinite(err), (what, name, b)
            ratios.append(err / budget)
        ratios = np.array(ratios)
        assert np.median(ratios) <= 2.5 and ratios.max() <= 10.0, (what, name, np.median(ratios), ratios.max())


def _solve(tv, x0):
    out = tv.solve_device(_dev(x0[..., None]), want_policy=True, want_value=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,m,kernel", [(16, 8, "tv_mfma_16x8"), (3, 2, "tv_mfma_16x8 (zero-padded)"),
                                        (12, 5, "tv_mfma_16x8 (zero-padded)"), (16, 1, "tv_mfma_16x8 (zero-padded)"),
                                        (20, 10, "tv_generic_wave"), (5, 20, "tv_generic_wave")])
def test_shapes_per_instance_time_varying(n, m, kernel):
    assert _hip.load().tfmpc_tvlqr_kernel_name(n, m, 50).decode() == kernel
    B, T = 6, 50
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=n * 100 + m)
    x0 = tvlqr_ref.make_x0(n, B)
    out = _solve(TimeVaryingLQR(F, f, C, c, device="cuda"), x0)
    assert int(out["status"].abs().sum()) == 0
    r64, r32 = _refs(F, f, C, c, x0)
    _check(_host(out), r64, r32, what=(n, m))


@pytest.mark.parametrize("T", [1, 2, 50, 51, 52, 53, 104, 257])
@pytest.mark.parametrize("n,m", [(16, 8), (12, 5)])
def test_horizons_across_chunk_and_ring_boundaries(n, m, T):
    B = 3
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=T)
    x0 = tvlqr_ref.make_x0(n, B, seed=T)
    out = _solve(TimeVaryingLQR(F, f, C, c, device="cuda"), x0)
    assert int(out["status"].abs().sum()) == 0
    r64, r32 = _refs(F, f, C, c, x0)
    _check(_host(out), r64, r32, what=(n, m, T))


@pytest.mark.parametrize("n,m", [(16, 8), (12, 5), (20, 10)])
def test_batch_shared_time_varying(n, m):
    B, T = 5, 53
    F, f, C, c = (a[0] for a in tvlqr_ref.make_models(n, m, T, 1, seed=7))
    x0 = tvlqr_ref.make_x0(n, B)
    tv = TimeVaryingLQR(F, f, C, c, device="cuda")
    assert tv.batch_size is None and tv._model_args()[1] == 0
    out = _solve(tv, x0)
    rep = lambda a: np.repeat(a[None], B, axis=0)          # noqa: E731
    r64, r32 = _refs(rep(F), rep(f), rep(C), rep(c), x0)
    _check(_host(out), r64, r32, what="shared")


@pytest.mark.parametrize("n,m", [(16, 8), (3, 2), (20, 10)])
def test_per_instance_time_constant(n, m):
    """Time stride 0 through expanded views, and a mixed problem: dynamics varying in time, costs constant (time axis 1)."""
    B, T = 4, 51
    F, f, C, c = tvlqr_ref.make_models(n, m, 1, B, seed=11)
    x0 = tvlqr_ref.make_x0(n, B)
    views = [_dev(a).expand(B, T, *a.shape[2:]) for a in (F, f, C, c)]
    tv = TimeVaryingLQR(*views, device="cuda")
    assert tv.horizon == T and tv._model_args()[2] == 0
    out = _solve(tv, x0)
    rep = lambda a: np.repeat(a, T, axis=1)                # noqa: E731
    r64, r32 = _refs(rep(F), rep(f), rep(C), rep(c), x0)
    _check(_host(out), r64, r32, what="time-constant")
    Fv, fv, _, _ = tvlqr_ref.make_models(n, m, T, B, seed=12)
    out = _solve(TimeVaryingLQR(Fv, fv, C, c, device="cuda"), x0)
    r64, r32 = _refs(Fv, fv, rep(C), rep(c), x0)
    _check(_host(out), r64, r32, what="mixed")


@pytest.mark.parametrize("n,m", [(16, 8), (12, 5), (20, 10)])
def test_explicit_final_cost_versus_default(n, m):
    B, T = 4, 52
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=13)
    Cf, cf = tvlqr_ref.make_final(n, B)
    x0 = tvlqr_ref.make_x0(n, B)
    out = _solve(TimeVaryingLQR(F, f, C, c, Cf, cf, device="cuda"), x0)
    r64, r32 = _refs(F, f, C, c, x0, Cf, cf)
    _check(_host(out), r64, r32, what="explicit final")
    # the default is C_{T-1}[:n,:n], c_{T-1}[:n]: passing exactly that explicitly gives the same bits
    Cd, cd = C[:, T - 1, :n, :n].copy(), c[:, T - 1, :n].copy()
    a = _solve(TimeVaryingLQR(F, f, C, c, device="cuda"), x0)
    b = _solve(TimeVaryingLQR(F, f, C, c, Cd, cd[:, :, None], device="cuda"), x0)
    for k in FIELDS:
        assert torch.equal(a[k], b[k]), k
    # a shared final cost (no batch axis)
    out = _solve(TimeVaryingLQR(F, f, C, c, Cf[0], cf[0], device="cuda"), x0)
    r64, r32 = _refs(F, f, C, c, x0, np.repeat(Cf[:1], B, 0), np.repeat(cf[:1], B, 0))
    _check(_host(out), r64, r32, what="shared final")


@pytest.mark.parametrize("n,m", [(16, 8), (12, 5)])
def test_from_lqr_agrees_with_lqr(n, m):
    B, T = 8, 50
    np.random.seed(3)
    lqr = make_lqr(n, m, batch_size=B)
    lqr.C = 0.5 * (lqr.C + lqr.C.transpose(-1, -2))
    x0 = tvlqr_ref.make_x0(n, B)
    ref = lqr.solve_device(_dev(x0[..., None]), T, want_policy=True, want_value=True)
    tv = TimeVaryingLQR.from_lqr(lqr, T)
    out = _solve(tv, x0)
    F, f, C, c = (t.cpu().numpy() for t in (lqr.F, lqr.f, lqr.C, lqr.c))
    rep = lambda a: np.repeat(a[:, None], T, axis=1)       # noqa: E731
    r64, r32 = _refs(rep(F), rep(f[..., 0]), rep(C), rep(c[..., 0]), x0)
    _check(_host(out), r64, r32, what="from_lqr")
    _check(_host(ref), r64, r32, what="LQR")


@pytest.mark.parametrize("n,m", [(16, 8), (12, 5), (20, 10)])
def test_split_backward_forward_equals_fused_solve_bitwise(n, m):
    B, T = 4, 57
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=17)
    x0 = tvlqr_ref.make_x0(n, B)
    tv = TimeVaryingLQR(F, f, C, c, device="cuda")
    fused = _solve(tv, x0)
    policy, value = tv.backward()
    states, actions, costs = tv.forward(policy, _dev(x0[..., None]))
    torch.cuda.synchronize()
    for name, a in (("K", policy.K), ("k", policy.k), ("V", value.V), ("v", value.v), ("const", value.const),
                    ("states", states), ("actions", actions), ("costs", costs)):
        assert torch.equal(fused[name], a), name
    # and without the value outputs (other instantiations of the same sweep)
    lean = tv.solve_device(_dev(x0[..., None]))
    torch.cuda.synchronize()
    for name in ("states", "actions", "costs"):
        assert torch.equal(fused[name], lean[name]), name


def test_strict_f32_products():
    B, T = 4, 53
    for n, m in ((16, 8), (12, 5)):
        F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=19)
        x0 = tvlqr_ref.make_x0(n, B)
        with _hip.option("TFMPC_LQR_MFMA", "f32"):
            out = _solve(TimeVaryingLQR(F, f, C, c, device="cuda"), x0)
        default = _solve(TimeVaryingLQR(F, f, C, c, device="cuda"), x0)
        assert not torch.equal(out["K"], default["K"])          # the option reached the kernel
        r64, r32 = _refs(F, f, C, c, x0)
        _check(_host(out), r64, r32, what=("f32", n, m))


@pytest.mark.parametrize("n,m", [(16, 8), (12, 5), (20, 10)])
def test_not_pd_at_one_step_of_one_instance(n, m):
    B, T = 4, 20
    F, f, C, c = tvlqr_ref.make_models(n, m, T, B, seed=23)
    C[2, 7, n:, n:] = -1.0e4 * np.eye(m, dtype=np.float32)
    x0 = tvlqr_ref.make_x0(n, B)
    tv = TimeVaryingLQR(F, f, C, c, device="cuda")
    out = _solve(tv, x0)
    st = out["status"].cpu().numpy()
    assert st[2] & _hip.ST_NOT_PD, st
    assert (st[[0, 1, 3]] == 0).all(), st
    assert tv.last_status is out["status"]
    _, _ = tv.backward()
    torch.cuda.synchronize()
    assert (tv.last_status.cpu().numpy() & _hip.ST_NOT_PD).tolist() == [0, 0, _hip.ST_NOT_PD, 0]


@pytest.mark.parametrize("n,m", [(16, 8), (20, 10)])
def test_batch_zero_and_one(n, m):
    T = 9
    F, f, C, c = tvlqr_ref.make_models(n, m, T, 1, seed=29)
    x0 = tvlqr_ref.make_x0(n, 1)
    out = _solve(TimeVaryingLQR(F, f, C, c, device="cuda"), x0)
    r64, r32 = _refs(F, f, C, c, x0)
    _check(_host(out), r64, r32, what="B=1")
    # unbatched operands and x0: outputs without the batch axis
    traj = TimeVaryingLQR(F[0], f[0], C[0], c[0], device="cuda").solve(x0[0][:, None])
    np.testing.assert_array_equal(np.asarray(traj.states), out["states"][0, ..., 0].cpu().numpy())
    empty = TimeVaryingLQR(F[:0], f[:0], C[:0], c[:0], device="cuda")
    assert empty.batch_size == 0
    out0 = empty.solve_device(torch.empty((0, n, 1), device="cuda"), want_policy=True, want_value=True)
    torch.cuda.synchronize()
    assert out0["states"].shape == (0, T + 1, n, 1) and out0["status"].numel() == 0
    lib = _hip.load()
    assert lib.tfmpc_tvlqr_solve_f32(0, n, m, T, *([None, 0, 0] * 4), None, 0, None, 0, *([None] * 10), None, 0, None) == 0


def test_full_size_headline():
    B, n, m, T = 65536, 16, 8, 50
    P = 128                                   # distinct instances; instance b is pool[b % P], stored per instance
    F, f, C, c = tvlqr_ref.make_models(n, m, T, P, seed=31)
    x0p = tvlqr_ref.make_x0(n, P)
    rep = lambda a: _dev(a).repeat(B // P, *([1] * (a.ndim - 1)))     # noqa: E731
    tv = TimeVaryingLQR(rep(F), rep(f), rep(C), rep(c), device="cuda", symmetric=True)
    out = tv.solve_device(rep(x0p)[..., None], want_policy=True, want_value=True)
    torch.cuda.synchronize()
    assert int(out["status"].abs().sum()) == 0
    for k in FIELDS:
        assert bool(torch.isfinite(out[k]).all()), k
    sample = np.random.default_rng(0).choice(B, size=128, replace=False)
    got = _host({k: out[k][torch.as_tensor(sample, device="cuda")] for k in FIELDS})
    r64, r32 = _refs(F, f, C, c, x0p, idx=[b % P for b in sample])
    _check(got, r64, r32, what="full size")

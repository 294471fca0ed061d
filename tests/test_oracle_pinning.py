"""CPU tests that PIN the oracle (``oracle/``) against every known answer the
reference itself holds for the hot path.  These mirror the
reference's own tests; citations are into ``/root/reference/tests``."""

import os
import numpy as np
import pytest

import problems
from oracle import boxqp_ref, c_oracle, envs_ref, ilqr_ref, lqr_ref


# ------------------------------------------------------------ README navlin ---
def test_readme_navlin_known_answer(golden):
    """README.md:75-90: reproduced to the 4 printed decimals by the Riccati
    recursion started from a ZERO terminal value function."""
    g = golden("readme_navlin")
    F, f, C, c = lqr_ref.make_lqr_linear_navigation(g["goal"], float(g["beta"]))
    T = int(g["T"])
    x, u, cs, _, _ = lqr_ref.solve(F, f, C, c, g["x0"], T, terminal="zero")
    assert np.allclose(x[1:], g["next_states"], atol=6e-5)
    assert np.allclose(u, g["actions"], atol=6e-5)
    assert np.allclose(cs[:T], g["costs"], atol=6e-5)
    assert abs(cs[:T].sum() - float(g["total"])) < 5e-4
    assert np.allclose(x[-1], g["final_state"], atol=1e-5)
    # the v0.7.0 terminal condition (lqr.py:67-68) gives a different table
    x2, u2, _, _, _ = lqr_ref.solve(F, f, C, c, g["x0"], T)
    assert abs(u2[0, 0] - 2.8654) < 1e-4 and abs(u2[-1, 0] - 0.0311) < 1e-4


# ------------------------------------------------------------------- box-QP ---
def _kat(golden, i):
    g = golden("boxqp_kats")
    goal, low, high, x_star = (g[f"{k}{i}"] for k in ("goal", "low", "high", "x_star"))
    return 2 * np.eye(len(goal)), -2 * goal, low, high, x_star


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_boxqp_known_answers(golden, case, dtype):
    """test_utils_optimization.py:57-79"""
    H, q, low, high, x_star = _kat(golden, case)
    x, *_ = boxqp_ref.projected_newton_qp(H, q, low, high, x_star, dtype=dtype)
    assert np.all(np.abs(x[:, 0] - x_star) < 1e-4)
    rng = np.random.default_rng(case)
    for _ in range(10):
        x_0 = rng.uniform(low, high)
        x, *_ = boxqp_ref.projected_newton_qp(H, q, low, high, x_0, dtype=dtype)
        assert np.all(np.abs(x[:, 0] - x_star) < 1e-4)
        for bound in (low, high):
            for i in range(len(x_0)):
                xs = x_0.copy()
                xs[i] = bound[i]
                x, *_ = boxqp_ref.projected_newton_qp(H, q, low, high, xs, dtype=dtype)
                assert np.all(np.abs(x[:, 0] - x_star) < 1e-4)


@pytest.mark.parametrize("case", range(6))
def test_boxqp_indices_interior_points_are_free(golden, case):
    """test_utils_optimization.py:30-41"""
    H, q, low, high, _ = _kat(golden, case)
    rng = np.random.default_rng(case)
    for _ in range(10):
        x = rng.uniform(low + 1e-4, high - 1e-4)[:, None]
        g = q[:, None] + H @ x
        free, clamped = boxqp_ref.get_qp_indices(g, low[:, None], high[:, None], x)
        assert free.all() and not clamped.any()


def test_boxqp_dense_kkt(golden):
    """The oracle's dense solutions satisfy the box-QP KKT conditions."""
    g = golden("boxqp_dense")
    for i in range(int(g["n_cases"])):
        H, q, low, high, x = (g[f"{k}{i}"] for k in ("H", "q", "low", "high", "x"))
        grad = H @ x + q
        assert np.all(x >= low - 1e-12) and np.all(x <= high + 1e-12)
        interior = (x > low + 1e-6) & (x < high - 1e-6)
        assert np.all(np.abs(grad[interior]) < 1e-5)
        assert np.all(grad[np.abs(x - low) <= 1e-6] > -1e-5)
        assert np.all(grad[np.abs(x - high) <= 1e-6] < 1e-5)


# ---------------------------------------------------------------------- LQR ---
@pytest.mark.parametrize("seed", range(5))
def test_lqr_invariants(seed):
    """test_lqr.py:51-86: forward consistency and value function == cost-to-go."""
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(2, 10)), int(rng.integers(2, 10))
    F, f, C, c = problems.make_lqr_instance(seed, n, m)
    assert np.allclose(C, C.T) and np.all(np.linalg.eigvalsh(C) > 0)   # test_lqr.py:35-38
    T = 10
    x0 = rng.normal(size=n)
    x, u, cs, pol, val = lqr_ref.solve(F, f, C, c, x0, T)
    assert len(pol) == len(val) == T
    for t in range(T):
        K, k = pol[t]
        assert np.allclose(K @ x[t] + k[:, 0], u[t])
        z = np.concatenate([x[t], u[t]])
        assert np.allclose(F @ z + f, x[t + 1])
        assert np.allclose(0.5 * z @ C @ z + c @ z, cs[t])
        V, v, const = val[t]
        value = const.reshape(()) + 0.5 * x[t] @ V @ x[t] + v[:, 0] @ x[t]
        assert np.allclose(value, cs[t:].sum(), atol=1e-8 * max(1.0, abs(cs[t:].sum())))


def test_lqr_fp32_error_budget():
    """on make_lqr problems the fp32 restatement is 1e-4..1e-3
    (relative to max-abs) away from fp64 at n=16,m=8,T=50 -- the reason the
    1e-5 bar is replaced by "no worse than the fp32 restatement"."""
    errs = []
    for seed in (1000, 1001, 1002):
        F, f, C, c = problems.make_lqr_instance(seed, 16, 8)
        x0 = np.random.default_rng(seed).normal(size=16)
        x64, u64, c64, _, _ = lqr_ref.solve(F, f, C, c, x0, 50)
        x32, u32, c32, _, _ = lqr_ref.solve(F, f, C, c, x0, 50, dtype=np.float32)
        errs.append(max(np.abs(x32 - x64).max() / np.abs(x64).max(), np.abs(u32 - u64).max() / np.abs(u64).max()))
    assert 1e-6 < max(errs) < 1e-2


def test_c_oracle_matches_numpy(golden):
    for name, n, m in (("lqr_cfg1", 3, 2), ("lqr_cfg3", 16, 8)):
        g = golden(name)
        T = int(g["T"])
        for i in range(3):
            out = c_oracle.lqr_solve(g[f"F{i}"], g[f"f{i}"], g[f"C{i}"], g[f"c{i}"], g[f"x0{i}"][None], T,
                                     dtype=np.float64, want_policy=True, want_value=True)
            assert out["status"] == 0
            for key in ("states", "actions", "costs", "K", "k", "V", "v", "const"):
                ref = g[f"{key}{i}"]
                assert np.allclose(out[key][0], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max()), (name, i, key)


def test_c_oracle_shared_operands_and_threads():
    F, f, C, c, x0, goal = problems.make_navlin_batch(33, 5.0)
    a = c_oracle.lqr_solve(F, f, C, c, x0, 20, dtype=np.float64, nthreads=1)
    b = c_oracle.lqr_solve(F, f, C, c, x0, 20, dtype=np.float64, nthreads=4)
    assert np.array_equal(a["states"], b["states"])
    x, u, cs, _, _ = lqr_ref.solve(F, f, C, c[5], x0[5], 20)
    assert np.allclose(a["states"][5], x) and np.allclose(a["costs"][5], cs)


# --------------------------------------------------------------------- envs ---
def _rand_xu(env, rng, T=4, mean=10.0):
    x = rng.normal(mean, 1.0, size=(T, env.state_size, 1))
    u = rng.uniform(size=(T, env.action_size, 1))
    return x, u


def test_env_navigation_lqr_closed_forms():
    """test_env_lqr_navigation.py:28-135"""
    goal, beta = np.array([[5.5], [-9.0]]), 5.0
    env = envs_ref.NavigationLQR(goal, beta)
    x, u = _rand_xu(env, np.random.default_rng(0))
    tm = env.get_linear_transition(x, u)
    cm = env.get_quadratic_cost(x, u)
    I = np.eye(2)
    for t in range(len(x)):
        assert np.array_equal(tm.f_x[t], I) and np.array_equal(tm.f_u[t], I)
        assert np.allclose(cm.l_x[t], 2 * (x[t] - goal)) and np.allclose(cm.l_u[t], 2 * beta * u[t])
        assert np.allclose(cm.l_xx[t], 2 * I) and np.allclose(cm.l_uu[t], 2 * beta * I)
        assert not cm.l_ux[t].any() and not cm.l_xu[t].any()
    fm = env.get_quadratic_final_cost(x[0])
    assert np.allclose(fm.l_x, 2 * (x[0] - goal)) and np.allclose(fm.l_xx, 2 * I)


@pytest.mark.parametrize("zones", [1, 2])
def test_env_navigation_closed_forms(zones):
    """test_env_navigation.py:6-176 (deceleration, f_u = lambda I, f_x formula, cost derivatives)."""
    rng = np.random.default_rng(zones)
    center = rng.normal(size=(zones, 2, 1))
    decay = rng.uniform(0.0, 3.0, size=zones)
    goal = np.array([[8.0], [9.0]])
    env = envs_ref.Navigation(goal, center, decay, [[-1.0], [-1.0]], [[1.0], [1.0]])
    x, u = _rand_xu(env, rng, mean=2.0)
    tm = env.get_linear_transition(x, u)
    cm = env.get_quadratic_cost(x, u)
    for t in range(len(x)):
        r = np.linalg.norm(x[t] - center, axis=(1, 2))
        lam_z = 2.0 / (1.0 + np.exp(-decay * r)) - 1.0
        lam = np.prod(lam_z)
        assert np.allclose(tm.f[t], x[t] + lam * u[t])
        assert np.allclose(tm.f_u[t], lam * np.eye(2), atol=1e-10)
        h = 2.0 * decay * np.exp(-decay * r) / (1.0 + np.exp(-decay * r)) ** 2
        grad = sum(h[z] * (x[t] - center[z]) / r[z] * lam / lam_z[z] for z in range(zones))
        assert np.allclose(tm.f_x[t], np.eye(2) + u[t] @ grad.T, atol=1e-10)
        assert np.allclose(cm.l_x[t], 2 * (x[t] - goal)) and np.allclose(cm.l_xx[t], 2 * np.eye(2))
        assert not cm.l_u[t].any() and not cm.l_uu[t].any() and not cm.l_ux[t].any() and not cm.l_xu[t].any()


def test_env_hvac_closed_forms():
    """test_env_hvac.py:92-98,170-211"""
    cfg = problems.hvac_config(5, seed=3)
    env = envs_ref.HVAC(**cfg)
    rng = np.random.default_rng(0)
    x = rng.normal(20.0, 6.0, size=(6, 5, 1))
    u = rng.uniform(size=(6, 5, 1))
    tm = env.get_linear_transition(x, u)
    cm = env.get_quadratic_cost(x, u)
    cap, air_max = env.capacity, env.air_max
    lo, hi = env.temp_lower_bound, env.temp_upper_bound
    for t in range(len(x)):
        assert np.allclose(tm.f_u[t], np.diag((1.0 / cap * air_max * 1.006 * (40.0 - x[t]))[:, 0]))
        lx = 20000.0 * (-(lo > x[t]).astype(float) + (x[t] > hi).astype(float)) - 10.0 * np.sign((lo + hi) / 2 - x[t])
        assert np.allclose(cm.l_x[t], lx) and np.allclose(cm.l_u[t], air_max)
        for hname in ("l_xx", "l_uu", "l_ux", "l_xu"):
            assert not getattr(cm, hname)[t].any()
        # f_x closed form INCLUDING the -diag(G 1) term the reference's test omits
        A = np.logical_or(env.adj, env.adj.T).astype(float)
        G = A / env.R_wall
        fx = np.eye(5) + np.diag((1.0 / cap)[:, 0]) @ (
            -np.diag((u[t] * air_max * 1.006)[:, 0]) + G - np.diag(G.sum(1))
            - np.diag((env.adj_outside / env.R_outside)[:, 0]) - np.diag((env.adj_hall / env.R_hall)[:, 0]))
        assert np.allclose(tm.f_x[t], fx)


def test_env_reservoir_closed_forms():
    """test_env_reservoir.py:126-233 (mass balance, f_x, f_u, l_x, zero Hessians)."""
    cfg = problems.reservoir_config(4, seed=2)
    env = envs_ref.Reservoir(**cfg)
    rng = np.random.default_rng(0)
    x = rng.uniform(5.0, 95.0, size=(6, 4, 1))
    u = rng.uniform(size=(6, 4, 1))
    tm = env.get_linear_transition(x, u)
    cm = env.get_quadratic_cost(x, u)
    D, cap = env.downstream, env.max_res_cap
    lo, hi = env.lower_bound, env.upper_bound
    for t in range(len(x)):
        o = u[t] * x[t]
        vap = 0.5 * np.sin(x[t] / cap) * x[t]
        rain = env.rain_shape * env.rain_scale
        assert np.allclose(tm.f[t].sum(), (x[t] + rain - vap).sum() - o[-1, 0])    # mass balance
        fx = (np.eye(4) - np.diag((0.5 * (np.cos(x[t] / cap) * x[t] / cap + np.sin(x[t] / cap)))[:, 0])
              - np.diag(u[t][:, 0]) + D.T @ np.diag(u[t][:, 0]))
        fu = -np.diag(x[t][:, 0]) + D.T @ np.diag(x[t][:, 0])
        assert np.allclose(tm.f_x[t], fx) and np.allclose(tm.f_u[t], fu)
        LP, HP, SP = -env.low_penalty, -env.high_penalty, -env.set_point_penalty
        lx = -LP * (lo > x[t]) + HP * (x[t] > hi) - SP * np.sign((lo + hi) / 2 - x[t])
        assert np.allclose(cm.l_x[t], lx) and not cm.l_u[t].any()
        for hname in ("l_xx", "l_uu", "l_ux", "l_xu"):
            assert not getattr(cm, hname)[t].any()


# --------------------------------------------------------------------- iLQR ---
@pytest.mark.parametrize("beta", [0.0, 5.0])
@pytest.mark.parametrize("bounds", [None, (-1.0, 1.0)])
def test_ilqr_self_consistency(beta, bounds):
    """test_ilqr.py:48-109: shapes; rollouts obey the env exactly."""
    low, high = bounds if bounds else (None, None)
    env = envs_ref.NavigationLQR([[5.5], [-9.0]], beta, low, high)
    s = ilqr_ref.ILQRRef(env)
    T = 10
    x0 = np.zeros((2, 1))
    xs, us, cs = s.start(x0, T, rng=np.random.default_rng(0))
    assert xs.shape == (T + 1, 2, 1) and us.shape == (T, 2, 1) and cs.shape == (T + 1,)
    for t in range(T):
        assert np.array_equal(xs[t + 1], env.transition(xs[t], us[t]))
        assert np.all(us[t] == us[t][0])                      # one scalar per step (Q1)
    models = s.derivatives(xs, us)
    assert all(a.shape[0] == T for a in models[0]) and all(a.shape[0] == T for a in models[1])
    K, k, J, dV1, dV2 = s.backward(T, us, *models)           # default mu = 1.0 (Q5)
    assert K.shape == (T, 2, 2) and k.shape == (T, 2, 1)
    x, u, c, Jn, res = s.forward(xs, us, K, k)
    assert x.shape == xs.shape and u.shape == us.shape and c.shape == (T + 1,)
    for t in range(T):
        assert np.array_equal(x[t + 1], env.transition(x[t], u[t]))
        assert c[t] == env.cost(x[t], u[t])
    assert c[T] == env.final_cost(x[T])


@pytest.mark.parametrize("beta", [0.5, 5.0])
def test_ilqr_equals_lqr_on_linear_navigation(beta):
    """Unbounded NavigationLQR is an LQR problem: iLQR converges to the LQR
    trajectory; costs differ by the dropped constant (T+1)|g|^2
    (envs/__init__.py:27-28)."""
    goal = np.array([5.5, -9.0])
    T = 10
    env = envs_ref.NavigationLQR(goal, beta)
    s = ilqr_ref.ILQRRef(env)
    x, u, c, it = s.solve(np.zeros((2, 1)), T, rng=np.random.default_rng(3))
    F, f, C, cc = lqr_ref.make_lqr_linear_navigation(goal, beta)
    xl, ul, cl, _, _ = lqr_ref.solve(F, f, C, cc, np.zeros(2), T)
    assert it <= 2
    assert np.allclose(x, xl, atol=1e-8) and np.allclose(u, ul, atol=1e-8)
    assert np.allclose(c.sum(), cl.sum() + (T + 1) * goal @ goal)


def test_ilqr_degenerate_backward_on_piecewise_linear_costs(golden):
    """on HVAC / Reservoir V_xx stays 0, K == 0 and k is bang-bang."""
    for name in ("ilqr_hvac6", "ilqr_res4"):
        g = golden(name)
        assert not g["K_mu0"].any()
        assert not g["l_xx"].any() and not g["fl_xx"].any()
        u = g["u_init"]
        k = g["k_mu0"]
        assert np.all(np.isclose(k, 0.0 - u) | np.isclose(k, 1.0 - u))


def test_golden_files_are_reproducible(golden):
    g = golden("ilqr_navlqr")
    env = envs_ref.NavigationLQR([[5.5], [-9.0]], float(g["beta3"]), -1.0, 1.0)
    s = ilqr_ref.ILQRRef(env)
    x, u, c, it = s.solve(g["x03"][:, None], int(g["T3"]), u_init=g["u_init3"][..., None])
    assert it == int(g["sol_iteration3"])
    assert np.array_equal(x, g["sol_states3"]) and np.array_equal(c, g["sol_costs3"])


def test_vectorised_derivatives_equal_the_per_step_loop():
    """oracle/envs_ref.py differentiates all time steps at once (torch.func, as the reference's batch_jacobian does,
    diffenv.py:21-22, 45-72); the per-step torch.autograd.functional loop it replaced stays as `_loop=True`: every
    field of both approximations agrees to rounding on all five envs."""
    import problems
    from oracle import envs_ref
    rng = np.random.default_rng(0)
    nav = problems.NAV_CONFIG
    F, f, C, c, _ = problems.make_lqr_batch_fast(1, 4, 2, seed=1)
    cases = [(envs_ref.HVAC(**problems.hvac_config(8, seed=1)), 8, 8),
             (envs_ref.Reservoir(**problems.reservoir_config(5, seed=1)), 5, 5),
             (envs_ref.Navigation(nav["goal"], nav["deceleration"]["center"], nav["deceleration"]["decay"], nav["low"], nav["high"]), 2, 2),
             (envs_ref.NavigationLQR([[5.5], [-9.0]], 5.0, -1.0, 1.0), 2, 2),
             (envs_ref.LQEnv(F[0], f[0][:, None], C[0], c[0][:, None]), 4, 2)]
    for env, n, m in cases:
        X = [rng.uniform(5, 60, size=(n, 1)) for _ in range(6)]
        U = [rng.uniform(0, 1, size=(m, 1)) for _ in range(6)]
        for name in ("get_linear_transition", "get_quadratic_cost"):
            fast, loop = getattr(env, name)(X, U), getattr(env, name)(X, U, _loop=True)
            for a, b, field in zip(fast, loop, fast._fields):
                assert a.shape == b.shape, (type(env).__name__, name, field)
                assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (type(env).__name__, name, field)


def test_c_oracle_builds_elsewhere_when_its_folder_is_not_writable(tmp_path, monkeypatch):
    """A tree this user may not write to (or a library stamped for another CPU) must not stop the C restatement from
    loading: it is compiled into the next writable folder, stamped there, and found current on the next call."""
    blocked = tmp_path / "file"
    blocked.write_text("")
    spare = tmp_path / "cache"
    monkeypatch.setattr(c_oracle, "_candidates", lambda host: [str(blocked / "_build"), str(spare)])
    so = c_oracle.build()
    assert so == str(spare / "liblqr_oracle.so") and open(so + ".host").read() == c_oracle._host()
    mtime = os.path.getmtime(so)
    assert c_oracle.build() == so and os.path.getmtime(so) == mtime          # current: not compiled again
    with open(so + ".host", "w") as fh:
        fh.write("another cpu")
    assert c_oracle.build() == so and open(so + ".host").read() == c_oracle._host()
